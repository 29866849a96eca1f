"""The disk kernels' own buffers against the independent f64 answers on fuzzed
scenes: tests/disk_truth.py's checks (the model and constants calibrated on the
CPU path, tests/test_disk_truth_cpu.py) with a device renderer, on the first 8
test seeds of every observer family that hold at least 50 compared slots.
geo_render_rows for the disk, shift and emission kernels, geo_render_disk_adaptive
unshaded and with the emission; hits, g and q are read from the buffers armed with
geo_disk_hits_next_render, geo_disk_shift_next_render and
geo_disk_emission_next_render.  64 x 36 holds whole and partial 32 x 8 tiles and
several 16 x 4 waves.  One context per test, the seed's state set on it seed by
seed.  No mutation test here: the reference is the CPU test's."""
import pytest

import disk_truth as DT
import test_disk_cpu as T
import test_gpu_disk_adaptive as GA
import test_gpu_disk_emission as GE

pytestmark = pytest.mark.gpu

PER_FAMILY = 8


class Gpu(GA.Gpu):
    """test_gpu_disk_adaptive's context as disk_truth's checks call a renderer."""
    name = "gpu"

    def _state(self, c, shift=None, em=None):
        self.ctx.set_disk(T.TEX, *c.disk_args)
        self.ctx.clear_disk_emission()
        self.ctx.clear_disk_shift()
        if shift is not None:
            self.ctx.set_disk_shift(*shift)
        if em is not None:
            GE.set_emission(self.ctx, em, c.ramp)

    def _rows(self, c, fields):
        """geo_render_rows of the seed's direct truth scene, the buffers of `fields` armed."""
        b = self.buffers(DT.H, DT.W)
        self.ctx.disk_hits_next_render(b["hits"])
        if "g" in fields:
            self.ctx.disk_shift_next_render(b["g"])
        if "q" in fields:
            self.ctx.disk_emission_next_render(b["q"])
        self.ctx.render_rows(c.frame, c.direct, DT.W, DT.H, 0, DT.H, b["rgba"], b["mask"], b["uv"], b["steps"],
                             b["total"])
        return self.host(b, DT.H, DT.W)

    def disk(self, c):
        self._state(c)
        return self._rows(c, ("hits",))

    def shift(self, c):
        self._state(c, shift=c.shift)
        return self._rows(c, ("hits", "g"))

    def emission(self, c):
        self._state(c, em=c.em)
        return self._rows(c, ("hits", "g", "q"))

    def adaptive(self, c, shaded):
        self._state(c, em=c.em if shaded else None)
        return self.draw(c.frame, c.adaptive, DT.W, DT.H)


@pytest.fixture(scope="module")
def seeds():
    out = DT.gpu_seeds(PER_FAMILY)
    assert len(out) == PER_FAMILY * len(DT.FAMILIES)
    return out


@pytest.mark.parametrize("what", list(DT.WHAT))
def test_against_the_f64_answer(dev, seeds, what):
    gpu = Gpu(dev)
    try:
        s = DT.check(gpu, what, seeds)
    finally:
        gpu.close()
    assert all(n >= 50 for n in s["per_seed"].values()), s["per_seed"]
    assert s["compared"] >= 50 * len(seeds) and s["slot1"] >= 100
    # kCurvedOut and kFlat (tests/test_disk_truth_cpu.py says why not kCurvedIn;
    # tests/test_gpu_disk_step_truth.py holds the kCurvedIn disk kernels to the f64 answer)
    assert s["kinds"] == {0, 2}
