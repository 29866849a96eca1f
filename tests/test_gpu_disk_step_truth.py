"""The disk kernels' own buffers against disk_ref.trace(sub=1): the f64 band on
fuzzed scenes (tests/disk_band_truth.py: the first 6 test seeds with at least 10
in-band hits of each of near_disk, inside_photon_sphere and small_sphere,
unshaded, shifted and with the emission) and the seeds' own steps
(tests/disk_step_truth.py: the first 8 kCurvedIn seeds with at least 50 compared
slots and the six seeds that show the rule's angle clause; disk, shift, emission
and the band).  The checks, bars and per-seed floors are the CPU tests'
(tests/test_disk_band_truth_cpu.py, test_disk_step_truth_cpu.py); no calibration
and no mutations here.  geo_render_rows at 64 x 36; hits, g and q are read from the
buffers armed with geo_disk_hits_next_render, geo_disk_shift_next_render and
geo_disk_emission_next_render; one context per test, the seed's state set on it
seed by seed.  The references are traced in this process (no forked prefetch once
a GPU context exists: disk_truth.trace_all's guard).  profiles/disk_step_truth_gpu.txt
holds a run's printed maxima and counts."""
import pytest

import disk_band_truth as B
import disk_step_truth as ST
import disk_truth as DT
import test_gpu_disk_truth as GT

pytestmark = pytest.mark.gpu

BAND_PER_FAMILY = 6
CURVED_IN = 8


class Gpu(GT.Gpu):
    """test_gpu_disk_truth's context with the f64 band (test_gpu_disk_ring.Gpu's state,
    switched per render: geo_set_disk keeps it)."""

    def ring(self, c, what, on=True):
        self._state(c, shift=c.shift if what == "ring_shift" else None,
                    em=c.em if what == "ring_emission" else None)
        self.ctx.set_disk_ring_f64(bool(on))
        try:
            return self._rows(c, B.WHAT[what][1])
        finally:
            self.ctx.set_disk_ring_f64(False)


@pytest.fixture(scope="module")
def band_seeds():
    out = B.gpu_seeds(BAND_PER_FAMILY)
    assert len(out) == BAND_PER_FAMILY * len(B.BAND_FAMILIES)
    return out


@pytest.fixture(scope="module")
def step_seeds():
    out = ST.gpu_seeds(CURVED_IN)
    assert CURVED_IN <= len(out) <= CURVED_IN + len(ST.ANGLE_CLAUSE_SEEDS)
    return out


@pytest.mark.parametrize("what", list(B.WHAT))
def test_band_against_the_f64_answer(dev, band_seeds, what):
    gpu = Gpu(dev)
    try:
        s = DT.check(gpu, what, band_seeds, layer=B)
    finally:
        gpu.close()
    assert all(n >= 10 for n in s["per_seed"].values()), s["per_seed"]
    assert s["kinds"] == {0}


@pytest.mark.parametrize("what", list(ST.WHAT))
def test_own_step_against_the_f64_answer(dev, step_seeds, what):
    gpu = Gpu(dev)
    try:
        s = DT.check(gpu, what, step_seeds, layer=ST)
    finally:
        gpu.close()
    # the kCurvedIn disk kernels ran: every seed is of that kind
    assert s["kinds"] == {1} and all(ST.case_of(seed).kind == 1 for seed in step_seeds)
    if what != "ring":
        first = step_seeds[:CURVED_IN]
        assert all(s["per_seed"][seed] >= 50 for seed in first), s["per_seed"]


def test_angle_clause_seeds(dev):
    """The kernel's hit buffer on the named seeds: no disagreement off the edges with the
    clause stated, the recorded count without it."""
    gpu = Gpu(dev)
    try:
        for seed, (count, _) in ST.ANGLE_CLAUSE_SEEDS.items():
            c = ST.case_of(seed)
            got = gpu.disk(c)
            assert ST.off_edge_disagreements(c, got) == 0, c.desc
            assert ST.off_edge_disagreements(c, got, "no_angle_clause") == count, c.desc
    finally:
        gpu.close()
