"""The adaptive disk with its capture band in f64 on the device
(geo_render_disk_adaptive_ring, geo.h): the six GEO_MODE_ADAPTIVE
instantiations of geo_render_disk_ring_kernel against the CPU path
(geo_render_cpu_disk_adaptive_ring_f64, the same headers) bit for bit in every
output, the call's three properties on the device's own buffers, the band's
hits, g and q against the independent f64 answer, fuzzed scenes, and the
refusals.  tests/test_disk_adaptive_ring_cpu.py holds the CPU path to the
properties, to the f64 answer on 320 seeds and to the rules.

A wave is 16 x 4 pixels and a tile 32 x 8: 96 x 54 and 100 x 37 leave partial
waves and tiles and hold several workgroups; rows 5..24 start and end inside a
wave's four rows."""
import ctypes

import numpy as np
import pytest

import disk_band_truth as B
import disk_ref as D
import disk_step_truth as ST
import disk_truth as DT
import fuzz_disk_scenes as F
import test_disk_adaptive_cpu as A
import test_disk_adaptive_ring_cpu as AR
import test_disk_cpu as T
import test_disk_emission_cpu as TE
import test_gpu_disk_adaptive as GA
import test_gpu_disk_truth as GT
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4, GEO_MODE_ADAPTIVE,
                                                   GEO_MODE_DIRECT, GEO_MODE_FAN, GEO_OK, lib)

pytestmark = pytest.mark.gpu

W, H = T.W, T.H
VARIANTS = AR.VARIANTS
same, differing = GA.same, GA.differing


@pytest.fixture(scope="module")
def cpu():
    return AR.load_cpu()


class Gpu(GA.Gpu):
    """test_gpu_disk_adaptive's context with geo_set_disk_ring_f64 on, drawing through
    geo_render_disk_adaptive_ring with every output and every armed buffer."""

    def __init__(self, dev, disk_args=None, **kw):
        super().__init__(dev, disk_args, **kw)
        self.ctx.set_disk_ring_f64(True)

    def draw(self, frame, scene, w, h, band_rows=None, row0=0, row_stride=None, nbands=1, total=True, stream=None):
        band_rows = h if band_rows is None else band_rows
        row_stride = band_rows if row_stride is None else row_stride
        nrows = nbands * band_rows
        b = self.buffers(nrows, w)
        self.arm(b)
        self.ctx.render_disk_adaptive_ring(frame, scene, w, h, band_rows, row0, row_stride, nbands, b["rgba"],
                                           b["mask"], b["uv"], b["steps"], b["total"] if total else None,
                                           stream=stream)
        return self.host(b, nrows, w)

    def draw_off(self, frame, scene, w, h):
        """geo_render_disk_adaptive of the same call with the state off."""
        self.ctx.set_disk_ring_f64(False)
        try:
            return GA.Gpu.draw(self, frame, scene, w, h)
        finally:
            self.ctx.set_disk_ring_f64(True)

    def draw_direct(self, frame, scene, w, h):
        """geo_render_band_set of the direct scene with the state on: one band of whole 8-row groups
        that covers the frame (its rows past the frame are clipped), the first h rows returned."""
        rows = (h + 7) // 8 * 8
        b = self.buffers(rows, w)
        self.arm(b)
        self.ctx.render_band_set(frame, scene, w, h, rows, 0, rows, 1, b["rgba"], b["mask"], b["uv"], b["steps"],
                                 b["total"])
        return {k: (v if k == "total" else v[:h]) for k, v in self.host(b, rows, w).items()}

    def draw_plain(self, frame, scene, w, h):
        """geo_render_rows of a scene without the disk: colour, mask, UV, steps and the total."""
        b = self.buffers(h, w)
        self.ctx.render_rows(frame, scene, w, h, 0, h, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
        return self.host(b, h, w)


def cpu_frame(cpu, frame, sc, disk, w=W, h=H, **kw):
    rc, c = AR.render(cpu, frame, sc, disk, 1, w, h, **kw)
    assert rc == GEO_OK
    return c


# ---- 1. the kernels equal the CPU path ----------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["ring", "B"])
def test_kernel_equals_cpu_path(dev, cpu, name, variant):
    frame, scene, disk, disk_args = T.pose(name)
    sc = AR.scenes_of(scene)[0]
    c = cpu_frame(cpu, frame, sc, disk, **VARIANTS[variant])
    gpu = Gpu(dev, disk_args)
    gpu.shade(**VARIANTS[variant])
    g = gpu.draw(frame, sc, W, H)
    off = gpu.draw_off(frame, sc, W, H)
    gpu.close()
    assert same(g, c), (name, variant, differing(g, c))
    assert g["total"] == c["total"]
    assert differing(g, off)  # the band is drawn: not the state-off frame
    if variant == "plain":
        assert (g["g"] == -1.0).all()
    if variant != "emission":
        assert (g["q"] == -1.0).all()


def test_partial_tiles_row_ranges_and_bands(dev, cpu):
    # 100 x 37: no multiple of the tile, partial waves on both edges
    w, h = 100, 37
    frame, scene, disk, disk_args = T.pose("ring", w, h)
    sc = AR.scenes_of(scene)[0]
    gpu = Gpu(dev, disk_args)
    gpu.shade(em=TE.emission())
    c = cpu_frame(cpu, frame, sc, disk, w, h, em=TE.emission())
    rc, off = A.render(cpu, frame, sc, w, h, disk, em=TE.emission())
    assert rc == GEO_OK and (c["steps"] != off["steps"]).sum() >= 500  # band pixels in this frame too
    whole = gpu.draw(frame, sc, w, h)
    assert same(whole, c), differing(whole, c)
    assert whole["total"] == c["total"]
    # rows 5..24: the range starts and ends inside a wave's four rows
    part = gpu.draw(frame, sc, w, h, band_rows=20, row0=5)
    assert same(part, c, slice(None), slice(5, 25))
    assert part["total"] == int(c["steps"][5:25].sum(dtype=np.uint64))
    # a band set of the 96 x 54 frame: 8-row bands at rows 8, 24 and 40
    frame, scene, disk, _ = T.pose("ring")
    sc = AR.scenes_of(scene)[0]
    c = cpu_frame(cpu, frame, sc, disk, em=TE.emission())
    got = gpu.draw(frame, sc, W, H, band_rows=8, row0=8, row_stride=16, nbands=3)
    gpu.close()
    total = 0
    for i in range(3):
        r0 = 8 + 16 * i
        assert same(got, c, slice(8 * i, 8 * i + 8), slice(r0, r0 + 8)), i
        total += int(c["steps"][r0:r0 + 8].sum(dtype=np.uint64))
    assert got["total"] == total


def test_orders_deferred_steps_and_streams(dev, cpu):
    import torch

    frame, scene, disk, disk_args = T.pose("ring")
    sc = AR.scenes_of(scene)[0]
    c = cpu_frame(cpu, frame, sc, disk, em=TE.emission())
    gpu = Gpu(dev, disk_args)
    gpu.shade(em=TE.emission())
    gpu.ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    got = gpu.draw(frame, sc, W, H)
    assert same(got, c) and got["total"] == c["total"]
    # the learned order (period 1): the recording render, and renders after the order was learned
    gpu.ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        got = gpu.draw(frame, sc, W, H)
        torch.cuda.synchronize()
        assert same(got, c) and got["total"] == c["total"], i
    rec, _ = gpu.ctx.dispatch_stats()
    assert rec >= 1
    # the adaptive disk render and the direct ring render between two of them: keys of their own
    gpu.draw_off(frame, sc, W, H)
    gpu.draw_direct(frame, AR.scenes_of(scene)[1], W, H)
    got = gpu.draw(frame, sc, W, H)
    assert same(got, c) and got["total"] == c["total"]
    # GEO_FLAG_DEFER_STEPS with geo_steps_flush
    got = gpu.draw(frame, A.adaptive_of(scene, flags=GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS), W, H, total=False)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    gpu.ctx.steps_flush(tot)
    torch.cuda.synchronize()
    assert same(got, c) and int(tot.item()) == c["total"]
    # a non-default stream
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    got = gpu.draw(frame, sc, W, H, stream=s)
    gpu.close()
    assert same(got, c) and got["total"] == c["total"]


@pytest.mark.parametrize("config", ["budget300", "tol1e30_step0.3"])
@pytest.mark.parametrize("name", ["ring", "B"])
def test_budget_and_tolerance(dev, cpu, name, config):
    frame, scene, disk, disk_args = T.pose(name)
    step, max_steps, tol = AR.CONFIGS[config]
    sc = AR.scenes_of(scene, step=step, max_steps=max_steps, tol=tol)[0]
    c = cpu_frame(cpu, frame, sc, disk, em=TE.emission())
    gpu = Gpu(dev, disk_args)
    gpu.shade(em=TE.emission())
    g = gpu.draw(frame, sc, W, H)
    gpu.close()
    assert same(g, c), (name, config, differing(g, c))
    assert g["total"] == c["total"]


@pytest.mark.parametrize("seed", list(AR.CURVED_IN))
def test_kcurvedin_scenes(dev, cpu, seed):
    """The kCurvedIn kernels: the generator's scenes of tests/test_disk_adaptive_ring_cpu.py, shaded by the seed."""
    c = ST.case_of(seed)
    assert c.kind == 1
    sc = AR.scenes_of(c.direct)[0]
    kw = (dict(), dict(shift=c.shift), dict(em=c.em, ramp=c.ramp))[seed % 3]
    want = cpu_frame(cpu, c.frame, sc, T.make_disk(*c.disk_args), DT.W, DT.H, **kw)
    gpu = Gpu(dev, c.disk_args)
    gpu.shade(**kw)
    g = gpu.draw(c.frame, sc, DT.W, DT.H)
    off = gpu.draw_off(c.frame, sc, DT.W, DT.H)
    gpu.close()
    assert same(g, want), (c.desc, differing(g, want))
    assert g["total"] == want["total"] and differing(g, off)


# ---- 2. the properties on the device's own buffers ------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["ring", "B"])
def test_properties_on_the_device(dev, name, variant):
    frame, scene, _, disk_args = T.pose(name)
    adaptive, direct, plain = AR.scenes_of(scene)
    gpu = Gpu(dev, disk_args)
    gpu.shade(**VARIANTS[variant])
    on = gpu.draw(frame, adaptive, W, H)
    off = gpu.draw_off(frame, adaptive, W, H)
    ring = gpu.draw_direct(frame, direct, W, H)
    sky = gpu.draw_plain(frame, plain, W, H)
    gpu.close()
    r_in, r_out, normal, axis = disk_args
    x = D.trace(frame, scene, W, H, r_in, r_out, normal, axis, sub=1)["x"]
    pixels, hits = AR.check_properties(on, off, ring, sky, x)
    print(name, variant, "band pixels", pixels, "in-band hits", hits)
    assert (pixels >= 2000 and hits >= 100) if name == "ring" else (pixels >= 20 and hits >= 8)


# ---- 3. the band against the f64 answer ------------------------------------------------------
class TruthGpu(GT.Gpu):
    """disk_band_truth's renderer on the device: the case's direct truth scene in GEO_MODE_ADAPTIVE (tol 0)
    through geo_render_disk_adaptive_ring, hits, g and q read from the armed buffers."""

    def ring(self, c, what, on=True):
        self._state(c, shift=c.shift if what == "ring_shift" else None, em=c.em if what == "ring_emission" else None)
        self.ctx.set_disk_ring_f64(bool(on))
        try:
            b = self.buffers(DT.H, DT.W)
            self.arm(b)
            render = self.ctx.render_disk_adaptive_ring if on else self.ctx.render_disk_adaptive
            render(c.frame, AR.scenes_of(c.direct)[0], DT.W, DT.H, DT.H, 0, DT.H, 1, b["rgba"], b["mask"], b["uv"],
                   b["steps"], b["total"])
            return self.host(b, DT.H, DT.W)
        finally:
            self.ctx.set_disk_ring_f64(False)


@pytest.fixture(scope="module")
def band_seeds():
    out = B.gpu_seeds(6)
    assert len(out) == 6 * len(B.BAND_FAMILIES)
    return out


@pytest.mark.parametrize("what", list(B.WHAT))
def test_band_against_the_f64_answer(dev, band_seeds, what):
    """Prints the largest share of each bar (profiles/disk_adaptive_ring_truth_gpu.txt holds a run's lines)."""
    gpu = TruthGpu(dev)
    try:
        s = DT.check(gpu, what, band_seeds, layer=B)
    finally:
        gpu.close()
    assert all(n >= 10 for n in s["per_seed"].values()), s["per_seed"]


# ---- 4. fuzz ---------------------------------------------------------------------------------
FUZZ_SEEDS = tuple(range(1000, 1080))
FUZZ_TOLS = (0.0, 1e-4, 1e-5, 1e-7)


def test_fuzz_kernel_equals_cpu_path(dev, cpu):
    """fuzz_disk_scenes' scenes with rs > 0 at 64 x 36 in the adaptive mode, tol from FUZZ_TOLS, the shading by
    the seed; a scene holds a band pixel when the CPU render differs from the state-off one."""
    gpu = Gpu(dev)
    bad, scenes, band = [], 0, 0
    everywhere = np.ones((DT.H, DT.W), bool)
    for seed in FUZZ_SEEDS:
        frame, scene, disk_args, shift_args, (em, ramp), desc = F.disk_scene(seed, DT.W, DT.H)
        if not scene.rs > 0.0:
            continue
        tol = FUZZ_TOLS[(seed // 3) % len(FUZZ_TOLS)]
        sc = make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, GEO_MODE_ADAPTIVE,
                        GEO_FLAG_DISK, tol)
        kw = (dict(), dict(shift=shift_args), dict(em=em, ramp=ramp))[seed % 3]
        disk = T.make_disk(*disk_args)
        c = cpu_frame(cpu, frame, sc, disk, DT.W, DT.H, **kw)
        rc, off = A.render(cpu, frame, sc, DT.W, DT.H, disk, **kw)
        assert rc == GEO_OK, desc
        scenes += 1
        band += bool(AR.differing(c, off, everywhere))
        gpu.ctx.set_disk(T.TEX, *disk_args)
        gpu.shade(**kw)
        g = gpu.draw(frame, sc, DT.W, DT.H)
        if not same(g, c) or g["total"] != c["total"]:
            bad.append(f"{desc} tol={tol}: {differing(g, c)}")
    gpu.close()
    print(f"{scenes} scenes, {band} with a band pixel")
    assert scenes >= 36 and band >= scenes // 4 + 1, (scenes, band)
    assert not bad, f"{len(bad)} of {scenes} differ; first: {bad[0]}"


# ---- 5. refusals -----------------------------------------------------------------------------
ENTRY = {"ring": lib.geo_render_disk_adaptive_ring, "adaptive": lib.geo_render_disk_adaptive,
         "band_set": lib.geo_render_band_set}


def _raw(gpu, frame, scene, b, call="ring", band_rows=56, nbands=1):
    return ENTRY[call](gpu.ctx._h, ctypes.byref(frame), ctypes.byref(scene), W, H, band_rows, 0, band_rows, nbands,
                       b["rgba"].data_ptr(), None, None, None, None, None)


def test_refusals(dev):
    import torch

    frame, scene, _, disk_args = T.pose("ring")
    adaptive, direct, plain = AR.scenes_of(scene)
    gpu = Gpu(dev, disk_args)
    before = gpu.draw(frame, adaptive, W, H)

    def sc(mode=GEO_MODE_ADAPTIVE, flags=GEO_FLAG_DISK, rs=scene.rs, tol=0.0):
        return make_scene(rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, mode, flags, tol)

    b = gpu.buffers(56, W)
    b["rgba"].fill_(7)
    # GEO_ESTATE with the state off, and nothing written
    gpu.ctx.set_disk_ring_f64(False)
    assert _raw(gpu, frame, adaptive, b) == GEO_ESTATE
    assert _raw(gpu, frame, sc(rs=0.0), b) == GEO_ESTATE
    gpu.ctx.set_disk_ring_f64(True)
    # GEO_EINVAL: the scenes of the older calls, and every flag beside DISK and DEFER_STEPS
    gpu.ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    for bad in (sc(mode=GEO_MODE_DIRECT), sc(mode=GEO_MODE_FAN), sc(flags=0), sc(flags=GEO_FLAG_DISK | GEO_FLAG_SS4),
                sc(flags=GEO_FLAG_DISK | GEO_FLAG_MIPS), sc(flags=GEO_FLAG_DISK | GEO_FLAG_COMPOSITE),
                sc(flags=GEO_FLAG_DISK | GEO_FLAG_RING_F64), sc(flags=GEO_FLAG_RING_F64), sc(tol=-1.0)):
        assert _raw(gpu, frame, bad, b) == GEO_EINVAL, (bad.mode, bad.flags, bad.tol)
    assert _raw(gpu, frame, adaptive, b, band_rows=20, nbands=2) == GEO_EINVAL  # a band set's rows: multiples of 8
    # an armed buffer is consumed by a refused call
    armed = gpu.buffers(56, W)
    gpu.arm(armed)
    assert _raw(gpu, frame, sc(mode=GEO_MODE_DIRECT), armed) == GEO_EINVAL
    assert _raw(gpu, frame, adaptive, armed) == GEO_OK  # a good render: nothing is armed any more
    torch.cuda.synchronize()
    assert (armed["hits"].cpu().numpy() == -1.0).all() and (armed["g"].cpu().numpy() == -1.0).all()
    assert not (armed["rgba"].cpu().numpy()[:H * W * 4] == 0).all()
    # every older entry point's answer for this scene, with the state on, is what it was
    assert _raw(gpu, frame, adaptive, b, "adaptive") == GEO_EINVAL
    assert _raw(gpu, frame, adaptive, b, "band_set") == GEO_EINVAL
    assert lib.geo_render_rows(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(adaptive), W, H, 0, H,
                               b["rgba"].data_ptr(), None, None, None, None, None) == GEO_EINVAL
    for name in ("geo_render_disk_adaptive_batch", "geo_render_disk_ring_batch", "geo_render_disk_batch",
                 "geo_render_emission_batch", "geo_render_ss_batch", "geo_render_band_set_batch"):
        st = getattr(lib, name)(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(adaptive), 1, W, H, 56, 0, 56, 1,
                                b["rgba"].data_ptr(), 56 * W * 4, None, None)
        assert st == GEO_EINVAL, name
    assert lib.geo_render_band_set_frames(gpu.ctx._h, ctypes.byref(frame), 1, ctypes.byref(adaptive), W, H, 56, 0, 56, 1,
                                          b["rgba"].data_ptr(), 56 * W * 4, None, None) == GEO_EINVAL
    torch.cuda.synchronize()
    assert (b["rgba"].cpu().numpy() == 7).all()  # nothing written by any refused call
    # rs = 0 with the state on: geo_render_disk_adaptive, byte for byte
    flat = gpu.draw(frame, sc(rs=0.0), W, H)
    flat_off = gpu.draw_off(frame, sc(rs=0.0), W, H)
    assert same(flat, flat_off) and flat["total"] == flat_off["total"]
    # no disk
    gpu.ctx.clear_disk()  # (clears the ring state too: the missing disk is met first)
    gpu.ctx.set_disk_ring_f64(True)
    assert _raw(gpu, frame, adaptive, b) == GEO_ESTATE
    gpu.ctx.set_disk(T.TEX, *disk_args)
    # after all of them: the same bytes as before
    after = gpu.draw(frame, adaptive, W, H)
    gpu.close()
    assert same(before, after) and before["total"] == after["total"]
