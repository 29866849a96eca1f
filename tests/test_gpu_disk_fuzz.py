"""The disk kernels against the CPU path on seeded random disk scenes
(tests/fuzz_disk_scenes.py), bit for bit: budgets off the group grid (the
probes of the budget tail, under a partial exec mask), steps above pi/4 (lanes
of one wave with different numbers of probes due in a group), edge-on disks.
The CPU path has one lane per "wave"; tests/test_disk_probe_host.py ties it to
a per-step definition of the probes and tests/test_host_disk_fuzz.py runs it on
these seeds.

The one-frame kernels (disk, shift, emission) are compared in every output;
the GEO_FLAG_SS4 kernels in colour and steps against the CPU path's
supersampled frame; the batched kernels (geo_render_disk_batch unshaded and
shaded, geo_render_ss_batch plain, disk and shaded) frame by frame against the
one-frame launch.  Every test asserts that its seeds hold a budget off the grid
and a step above pi/4, and (from the CPU path's hits and the crossings' nodes,
nothing from the device) hits probed in the budget's tail and hits probed
second or third in their group of four steps."""
import math

import numpy as np
import pytest

import test_disk_cpu as T
import test_disk_emission_cpu as XE
import test_disk_probe_host as P
import test_disk_shift_cpu as XS
import test_gpu_disk as G
import test_gpu_disk_batch as DB
import test_gpu_disk_emission as GE
import test_gpu_disk_shift as GS
import test_gpu_ss as SS
import test_gpu_ss_batch as SB
import test_ss_cpu as S
from fuzz_disk_scenes import GROUP_SEEDS, REGRESSION_SEEDS, TAIL_SEEDS, disk_batch, disk_scene, kind_of
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK, GEO_OK

pytestmark = pytest.mark.gpu

VARIANTS = ("plain", "shift", "emission")
# seeds per variant, from the variant's base: 60 whole frames at 64 x 36 and the seeds
# picked for the tail and the group path, 12 frames at 35 x 13 (partial tiles), 24
# supersampled at 49 x 27; tests/test_host_disk_fuzz.py runs the CPU path alone on all of them
BASE = {"plain": 0, "shift": 100, "emission": 200}
PATH_SEEDS = TAIL_SEEDS + GROUP_SEEDS


def seeds_of(variant, w):
    b = BASE[variant]
    if w == 64:
        return list(range(b, b + 60)) + list(PATH_SEEDS) + list(REGRESSION_SEEDS)
    return list(range(b + 60, b + 72))


SIZES = ((64, 36), (35, 13))
SS_SIZE = (49, 27)


def ss_seeds_of(variant):
    b = BASE["plain" if variant == "disk" else variant]
    return list(range(b + 72, b + 84)) + list(TAIL_SEEDS[:6]) + list(GROUP_SEEDS[:6])


BATCH_SEEDS = tuple(range(4)) + TAIL_SEEDS[:4] + GROUP_SEEDS[:4]
# floors of the path counts, no higher than half of what the seeds give (printed by every
# run): seeds of the test with a tail-probed hit / a hit probed second or third in its group
# (measured: bitexact 17..19 / 13..18, ss4 6..9 / 6..7, batches 4 / 5)
PATH_FLOORS = {"bitexact": (8, 6), "ss4": (3, 3), "batches": (2, 2)}
FIELDS = {"plain": ("hits",), "shift": ("hits", "g"), "emission": ("hits", "g", "q")}


@pytest.fixture(scope="module")
def cpu():
    return XE.load_cpu()


@pytest.fixture(scope="module")
def probe():
    return P.load()


class Reach:
    """What a test's seeds held; every test asserts the off-grid budget and the
    step above pi/4, the one-frame tests the three kinds as well."""

    def __init__(self):
        self.n = self.off_grid = self.big_step = self.tail = self.grouped = 0
        self.kinds = set()

    def add(self, scene, probe=None, frame=None, disk_args=None, w=0, h=0, hits=None):
        """hits: the CPU path's (h, w, 3, 2) hit slots of the frame."""
        if hits is not None:
            tail, grouped = P.hit_paths(P.frame_nodes(probe, frame, scene, disk_args, w, h), hits[..., 0] != 0.0,
                                        scene.max_steps)
            self.tail += bool(tail)
            self.grouped += bool(grouped)
        self.n += 1
        self.off_grid += scene.max_steps % 4 != 0
        self.big_step += scene.step > math.pi / 4
        self.kinds.add(kind_of(scene.rs, scene.r_obs, scene.step))  # as make_consts documents

    def check(self, what, kinds=False, third=False):
        print(f"{what}: {self.n} seeds, {self.off_grid} with a budget off the grid, {self.big_step} with a step above "
              f"pi/4, {self.tail} with a tail-probed hit, {self.grouped} with a hit probed second or third in its "
              f"group, kinds {sorted(self.kinds)}")
        tail, grouped = PATH_FLOORS[what.split()[0]]
        assert self.tail >= tail and self.grouped >= grouped, (self.tail, tail, self.grouped, grouped)
        assert self.off_grid >= (max(1, (self.n + 2) // 3) if third else 1), (self.off_grid, self.n)
        assert self.big_step >= 1, self.n
        if kinds:
            assert self.kinds == {0, 1, 2}, self.kinds


def explain(probe, desc, what, g, c, fields, frame, scene, disk_args, w, h):
    """None when g and c agree in every field (floats by their bits), else the
    message: the scene, the first differing pixel's (x, y, slot), both values,
    and that pixel's crossings' nodes and step count by the per-step definition."""
    for f in fields:
        a, b = g[f], c[f]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = a != b
        if not bad.any():
            continue
        i = np.argwhere(bad)[0]
        y, x = int(i[0]), int(i[1])
        px = P.pixel(probe, frame, scene, disk_args, w, h, x, y)
        return (f"{desc}: {what} {f} differs on {int(bad.sum())} elements, first at (x, y, slot...) = "
                f"{(x, y) + tuple(int(v) for v in i[2:])}: gpu {g[f][tuple(i)]!r} cpu {c[f][tuple(i)]!r}; "
                f"jn={px['jn']} steps={px['steps']} (gpu {g['steps'][y, x]}, cpu {c['steps'][y, x]}) kind={px['kind']}")
    if g["total"] != c["total"]:
        return f"{desc}: {what} steps_total gpu {g['total']} cpu {c['total']}"
    return None


def cpu_render(cpu, variant, frame, scene, w, h, disk_args, shift, em, ramp):
    disk = T.make_disk(*disk_args)
    if variant == "plain":
        rc, c = T.render(cpu, frame, scene, T.SKY, w, h, disk, T.TEX)
    elif variant == "shift":
        rc, c = XS.render(cpu, frame, scene, w, h, disk, shift=shift)
    else:
        rc, c = XE.render(cpu, frame, scene, w, h, disk, em=em, ramp=ramp)
    assert rc == GEO_OK
    return c


def set_state(ctx, variant, disk_args, shift, em, ramp):
    """The seed's disk and, by variant, its shading or emission on a context."""
    ctx.set_disk(T.TEX, *disk_args)
    if variant == "shift":
        ctx.set_disk_shift(*shift)
    elif variant == "emission":
        GE.set_emission(ctx, em, ramp)


@pytest.mark.parametrize("variant", VARIANTS)
def test_disk_fuzz_bitexact(dev, cpu, probe, variant):
    """geo_render_rows with every optional output armed against the matching
    CPU entry point."""
    first = disk_scene(BASE[variant], 64, 36)
    gpu = {"plain": G.Gpu, "shift": GS.Gpu, "emission": GE.Gpu}[variant](dev, first[2])
    reach, hit_seeds, pixels = Reach(), 0, 0
    fields = ("rgba", "mask", "steps", "uv") + FIELDS[variant]
    try:
        for w, h in SIZES:
            for seed in seeds_of(variant, w):
                frame, scene, disk_args, shift, (em, ramp), desc = disk_scene(seed, w, h)
                set_state(gpu.ctx, variant, disk_args, shift, em, ramp)
                g = gpu.rows(frame, scene, w, h)
                c = cpu_render(cpu, variant, frame, scene, w, h, disk_args, shift, em, ramp)
                reach.add(scene, probe, frame, disk_args, w, h, c["hits"])
                hit_seeds += bool((c["hits"][..., 0] != 0.0).any())
                msg = explain(probe, desc, variant, g, c, fields, frame, scene, disk_args, w, h)
                assert msg is None, msg
                pixels += w * h
    finally:
        gpu.close()
    reach.check(f"bitexact {variant}", kinds=True, third=True)
    print(f"bitexact {variant}: {hit_seeds} seeds with a disk hit, {pixels} pixels compared")
    assert hit_seeds >= reach.n // 4, (hit_seeds, reach.n)  # real disks (the CPU test counts them per slot)


@pytest.mark.parametrize("variant", ["disk", "shift", "emission"])
def test_disk_fuzz_ss4(dev, cpu, probe, variant):
    """GEO_FLAG_SS4 frames: colour and steps against the CPU path's supersampled frame."""
    w, h = SS_SIZE
    base = BASE["plain" if variant == "disk" else variant]
    gpu = SS.Gpu(dev, "disk", disk_scene(base, w, h)[2])
    reach = Reach()
    try:
        for seed in ss_seeds_of(variant):
            frame, scene, disk_args, shift, (em, ramp), desc = disk_scene(seed, w, h)
            sc = S.ss_scene(scene, "disk")
            disk = T.make_disk(*disk_args)
            # (the paths of the 2w x 2h sample frame, from the CPU path's one-sample render of it)
            rc, one = T.render(cpu, frame, scene, T.SKY, 2 * w, 2 * h, disk, T.TEX)
            assert rc == GEO_OK, desc
            reach.add(scene, probe, frame, disk_args, 2 * w, 2 * h, one["hits"])
            set_state(gpu.ctx, variant, disk_args, shift, em, ramp)
            if variant == "emission":  # as test_gpu_disk_emission.test_ss4 does
                rc, c = XE.render(cpu, frame, sc, w, h, disk, em=em, ramp=ramp, outputs=False)
                want, wtotal = c["rgba"], c["total"]
            else:
                rc, want, wtotal = S.ss_render(cpu, variant, frame, sc, w, h, disk, shift=shift)
            assert rc == GEO_OK, desc
            got, total = gpu.rows(frame, sc, w, h)
            diff = (got != want).any(axis=-1)
            if diff.any():
                y, x = (int(v) for v in np.argwhere(diff)[0])
                raise AssertionError(f"{desc}: ss4 {variant}: {int(diff.sum())} pixels differ, first at (x, y) = "
                                     f"({x}, {y}): gpu {got[y, x]} cpu {want[y, x]}")
            assert total == wtotal, (desc, total, wtotal)
    finally:
        gpu.close()
    reach.check(f"ss4 {variant}")


def test_disk_fuzz_batches(dev, cpu, probe):
    """2..8 frames of one seed's scene (the camera turning, the observer
    drifting: fuzz_disk_scenes.disk_batch) through geo_render_disk_batch,
    unshaded and shaded, and geo_render_ss_batch (plain, disk, shaded): every
    frame is its one-frame geo_render_band_set render, and so are the totals."""
    w, h = 64, 36
    lay = (w, h, 8, 0, 8)  # the whole frame in 8-row bands, the last one clipped
    reach, launched = Reach(), 0
    for i, seed in enumerate(BATCH_SEEDS):
        n = 2 + (5 * i) % 7
        frames, scenes, disk_args, shift, desc = disk_batch(seed, w, h, n)
        rc, one = T.render(cpu, frames[0], scenes[0], T.SKY, w, h, T.make_disk(*disk_args), T.TEX)
        assert rc == GEO_OK, desc
        reach.add(scenes[0], probe, frames[0], disk_args, w, h, one["hits"])
        assert all(s.flags == GEO_FLAG_DISK for s in scenes) and len({s.r_obs for s in scenes}) == n, desc
        for shade in (None, shift):
            ctx = DB.new_ctx(dev, disk=disk_args, shift=shade)
            try:
                got, tot = DB.batch(ctx, dev, frames, scenes, lay)
                ref, ref_tot, _ = DB.singles(ctx, dev, frames, scenes, lay)
            finally:
                ctx.close()
            for f in range(n):
                diff = got[f] != ref[f]
                assert not diff.any(), (desc, "disk batch", "shaded" if shade else "unshaded", f"frame {f}",
                                        f"{int(diff.sum())} bytes, first at pixel {int(np.argwhere(diff)[0][0]) // 4}")
            assert tot == ref_tot, (desc, "disk batch", tot, ref_tot)
            launched += n
        for kind in S.KINDS:
            ss = [S.ss_scene(s, kind) for s in scenes]
            ctx = SB.new_ctx(dev, kind, disk=disk_args)
            try:
                if kind == "shift":
                    ctx.set_disk_shift(*shift)
                got, tot = SB.batch(ctx, dev, frames, ss, lay)
                ref, tots = SB.singles(ctx, dev, frames, ss, lay)
            finally:
                ctx.close()
            for f in range(n):
                diff = got[f] != ref[f]
                assert not diff.any(), (desc, "ss batch", kind, f"frame {f}",
                                        f"{int(diff.sum())} bytes, first at pixel {int(np.argwhere(diff)[0][0]) // 4}")
            assert tot == sum(tots), (desc, "ss batch", kind, tot, tots)
            launched += n
    reach.check("batches")
    print(f"batches: {launched} batched frames compared with their one-frame renders")
