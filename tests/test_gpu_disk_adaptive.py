"""The thin disk in GEO_MODE_ADAPTIVE on the device (geo_render_disk_adaptive,
geo.h): the adaptive disk kernels against the CPU path
(geo_render_cpu_disk_adaptive, the same header csrc/geo_disk.h) bit for bit,
unshaded, shifted and with the emission, on whole frames, partial tiles, row
ranges and bands, at tolerances and budgets that put several crossings into one
step and end rays inside waves, under the context's other features, over fuzzed
scenes, and the call's refusals.  tests/test_disk_adaptive_cpu.py ties the CPU
path to the probe rule's definition, to geometry and to the f64 restatement.

A wave is 16 x 4 pixels and a tile 32 x 8: 96 x 54, 100 x 37 and 64 x 32 leave
partial waves and tiles or hold several."""
import ctypes
import math

import numpy as np
import pytest

import fuzz_disk_scenes as F
import test_disk_adaptive_cpu as A
import test_disk_cpu as T
import test_disk_emission_cpu as TE
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4, GEO_MODE_ADAPTIVE,
                                                   GEO_MODE_DIRECT, GEO_MODE_FAN, GEO_OK, lib)

pytestmark = pytest.mark.gpu

W, H = T.W, T.H
SHIFT = (1, 4, 1.0)
FIELDS = ("rgba", "mask", "steps")
BITS = ("uv", "hits", "g", "q")


@pytest.fixture(scope="module")
def cpu():
    return A.load_cpu()


class Gpu:
    """One context with the test sky and a disk; adaptive disk renders with every output."""

    def __init__(self, dev, disk_args=None, tex=T.TEX, sky=True):
        import schwarzschild_raytracer_wgpu_amd as g

        self.dev = dev
        self.ctx = g.Context(dev.index or 0)
        if sky:
            self.ctx.set_sky(T.SKY)
        if disk_args is not None:
            self.ctx.set_disk(tex, *disk_args)

    def shade(self, shift=None, em=None, ramp=TE.RAMP):
        """The context's shading state: shift = (spin, exponent, gain), em = TE.emission(...)."""
        self.ctx.clear_disk_emission()
        self.ctx.clear_disk_shift()
        if shift is not None:
            self.ctx.set_disk_shift(*shift)
        if em is not None:
            spin, profile, t_ref, t_lo, t_hi, exposure = em
            self.ctx.set_disk_emission(ramp, t_ref, t_lo, t_hi, profile, exposure, spin)

    def buffers(self, nrows, w):
        import torch

        d = self.dev
        return dict(rgba=torch.zeros(nrows * w * 4, dtype=torch.uint8, device=d),
                    mask=torch.zeros(nrows * w, dtype=torch.uint8, device=d),
                    uv=torch.zeros(nrows * w * 2, dtype=torch.float32, device=d),
                    steps=torch.zeros(nrows * w, dtype=torch.int32, device=d),
                    total=torch.zeros(1, dtype=torch.int64, device=d),
                    hits=torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=d),
                    g=torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=d),
                    q=torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=d))

    @staticmethod
    def host(b, nrows, w):
        import torch

        torch.cuda.synchronize()
        return dict(rgba=b["rgba"].cpu().numpy().reshape(nrows, w, 4), mask=b["mask"].cpu().numpy().reshape(nrows, w),
                    uv=b["uv"].cpu().numpy().reshape(nrows, w, 2),
                    steps=b["steps"].cpu().numpy().view(np.uint32).reshape(nrows, w), total=int(b["total"].item()),
                    hits=b["hits"].cpu().numpy().reshape(nrows, w, 3, 2), g=b["g"].cpu().numpy().reshape(nrows, w, 3),
                    q=b["q"].cpu().numpy().reshape(nrows, w, 3))

    def arm(self, b):
        self.ctx.disk_hits_next_render(b["hits"])
        self.ctx.disk_shift_next_render(b["g"])
        self.ctx.disk_emission_next_render(b["q"])

    def draw(self, frame, scene, w, h, band_rows=None, row0=0, row_stride=None, nbands=1, total=True, stream=None):
        """geo_render_disk_adaptive with every output and every armed buffer (the
        whole frame as one band of h rows unless a layout is given)."""
        band_rows = h if band_rows is None else band_rows
        row_stride = band_rows if row_stride is None else row_stride
        nrows = nbands * band_rows
        b = self.buffers(nrows, w)
        self.arm(b)
        self.ctx.render_disk_adaptive(frame, scene, w, h, band_rows, row0, row_stride, nbands, b["rgba"], b["mask"],
                                      b["uv"], b["steps"], b["total"] if total else None, stream=stream)
        return self.host(b, nrows, w)

    def close(self):
        self.ctx.close()


def same(a, b, rows=slice(None), brows=None):
    brows = rows if brows is None else brows
    return (all(np.array_equal(a[f][rows], b[f][brows]) for f in FIELDS) and
            all(np.array_equal(a[f][rows].view(np.uint32), b[f][brows].view(np.uint32)) for f in BITS))


def differing(a, b):
    return [f for f in FIELDS + BITS if not np.array_equal(a[f].view(np.uint32) if f in BITS else a[f],
                                                           b[f].view(np.uint32) if f in BITS else b[f])]


VARIANTS = {"plain": dict(), "shift": dict(shift=SHIFT), "emission": dict(em=TE.emission())}


# ---- 1. the kernel equals the CPU path ----------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", A.POSES4)
def test_kernel_equals_cpu_path(dev, cpu, name, variant):
    frame, scene, disk, disk_args = T.pose(name)
    sc = A.adaptive_of(scene)
    rc, c = A.render(cpu, frame, sc, W, H, disk, **VARIANTS[variant])
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args)
    gpu.shade(**VARIANTS[variant])
    g = gpu.draw(frame, sc, W, H)
    gpu.close()
    assert (c["hits"][..., 0, 0] > 0).sum() > 300  # a real disk on both sides
    assert same(g, c), (name, variant, differing(g, c))
    assert g["total"] == c["total"]
    # what the render does not have stays at its prefill
    if variant == "plain":
        assert (g["g"] == -1.0).all()
    if variant != "emission":
        assert (g["q"] == -1.0).all()


# ---- 2. partial tiles, row ranges and bands -----------------------------------------
def test_partial_tiles_and_bands(dev, cpu):
    # a 100 x 37 frame (no multiple of the 32 x 8 tile), and rows 5..24 of it
    w, h = 100, 37
    frame, scene, disk, disk_args = T.pose("A", w, h)
    sc = A.adaptive_of(scene)
    gpu = Gpu(dev, disk_args)
    gpu.shade(shift=SHIFT)
    whole = gpu.draw(frame, sc, w, h)
    rc, c = A.render(cpu, frame, sc, w, h, disk, shift=SHIFT)
    assert rc == GEO_OK and same(whole, c), differing(whole, c)
    assert whole["total"] == c["total"]
    part = gpu.draw(frame, sc, w, h, band_rows=20, row0=5)
    assert same(part, whole, slice(None), slice(5, 25))
    assert part["total"] == int(whole["steps"][5:25].sum(dtype=np.uint64))
    # 8-row bands 0, 2, 4, 6 of the 96 x 54 frame (band 6 clipped to rows 48..53)
    frame, scene, disk, _ = T.pose("A")
    sc = A.adaptive_of(scene)
    whole = gpu.draw(frame, sc, W, H)
    nb, br = 4, 8
    got = gpu.draw(frame, sc, W, H, band_rows=br, row0=0, row_stride=2 * br, nbands=nb)
    gpu.close()
    total = 0
    for i in range(nb):
        r0 = 2 * i * br
        n = min(br, H - r0)
        assert same(got, whole, slice(i * br, i * br + n), slice(r0, r0 + n)), i
        total += int(whole["steps"][r0:r0 + n].sum(dtype=np.uint64))
    assert got["total"] == total
    # clipped rows are not written: the prefill stays
    clipped = slice(3 * br + (H - 48), None)
    assert (got["hits"][clipped] == -1.0).all() and (got["g"][clipped] == -1.0).all()
    assert (got["rgba"][clipped] == 0).all()


# ---- 3. several crossings per step, and budgets that end inside waves ---------------
@pytest.mark.parametrize("case", ["tol1e-4_step0.3", "tol1e-7_budget12", "tol1e30_step0.8"])
@pytest.mark.parametrize("name", ["A", "B", "flat"])
def test_loose_and_tight_control(dev, cpu, name, case):
    """tol 1e-4 with step 0.3 (hmax = 4.8 > pi), tol 1e-7 with a budget of 12
    attempts (rays run out of attempts inside waves whose other lanes stop), and
    a tolerance that accepts every attempt at step 0.8 (the steps that hold two
    crossings: tests/test_disk_adaptive_cpu.py's docstring)."""
    w, h = 64, 32
    frame, scene, disk, disk_args = T.pose(name, w, h)
    sc = {"tol1e-4_step0.3": A.adaptive_of(scene, tol=1e-4, step=0.3),
          "tol1e-7_budget12": A.adaptive_of(scene, tol=1e-7, max_steps=12),
          "tol1e30_step0.8": A.adaptive_of(scene, tol=1e30, step=0.8)}[case]
    rc, c = A.render(cpu, frame, sc, w, h, disk, em=TE.emission())
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args)
    gpu.shade(em=TE.emission())
    g = gpu.draw(frame, sc, w, h)
    gpu.close()
    assert same(g, c), (name, case, differing(g, c))
    assert g["total"] == c["total"]
    if case == "tol1e-7_budget12":
        spent = c["steps"] == 12
        assert spent.any() and (~spent).any()


# ---- 4. the context's other features ------------------------------------------------
def test_deferred_steps_stream_timing_and_orders(dev):
    import torch

    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    frame, scene, _, disk_args = T.pose("B")
    sc = A.adaptive_of(scene)
    gpu = Gpu(dev, disk_args)
    gpu.shade(em=TE.emission())
    gpu.ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    ref = gpu.draw(frame, sc, W, H)
    # GEO_FLAG_DEFER_STEPS with geo_steps_flush
    got = gpu.draw(frame, A.adaptive_of(scene, flags=GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS), W, H, total=False)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    gpu.ctx.steps_flush(tot)
    torch.cuda.synchronize()
    assert same(got, ref) and int(tot.item()) == ref["total"]
    # a non-default stream
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    got = gpu.draw(frame, sc, W, H, stream=s)
    assert same(got, ref) and got["total"] == ref["total"]
    # geo_time_next_render
    e0, e1 = HipEvent(), HipEvent()
    gpu.ctx.time_next_render(e0, e1)
    got = gpu.draw(frame, sc, W, H)
    ms = e0.elapsed_time(e1)  # raises unless both were recorded
    assert ms > 0.0 and same(got, ref)
    # the learned order (period 1, three renders), then an explicit one: the same bytes
    gpu.ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        got = gpu.draw(frame, sc, W, H)
        assert same(got, ref) and got["total"] == ref["total"], i
    rec, _ = gpu.ctx.dispatch_stats()
    assert rec >= 1
    tx, ty = (W + 31) // 32, (H + 7) // 8
    order = np.array([(y << 16) | x for y in range(ty) for x in range(tx)][::-1], dtype=np.uint32)
    gpu.ctx.set_tile_order(tx, ty, order)
    got = gpu.draw(frame, sc, W, H)
    gpu.close()
    assert same(got, ref) and got["total"] == ref["total"]


# ---- 5. fuzz ------------------------------------------------------------------------
FUZZ_SEEDS = tuple(range(1000, 1200)) + F.TAIL_SEEDS[:6] + F.GROUP_SEEDS[:6]
FUZZ_TOLS = (0.0, 1e-4, 1e-5, 1e-7)


def test_fuzz_kernel_equals_cpu_path(dev, cpu):
    """fuzz_disk_scenes' scenes with the mode switched to adaptive and tol drawn
    from FUZZ_TOLS, at most 64 x 32; the shading state by the seed (none, the
    seed's shift, the seed's emission).  0 differ."""
    gpu = Gpu(dev)
    bad, hit_frames = [], 0
    sizes = ((64, 32), (48, 20), (33, 9))
    for seed in FUZZ_SEEDS:
        w, h = sizes[seed % len(sizes)]
        frame, scene, disk_args, shift_args, (em, ramp), desc = F.disk_scene(seed, w, h)
        tol = FUZZ_TOLS[(seed // 3) % len(FUZZ_TOLS)]
        sc = make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, GEO_MODE_ADAPTIVE,
                        GEO_FLAG_DISK, tol)
        kw = (dict(), dict(shift=shift_args), dict(em=em, ramp=ramp))[seed % 3]
        rc, c = A.render(cpu, frame, sc, w, h, T.make_disk(*disk_args), **kw)
        assert rc == GEO_OK, desc
        gpu.ctx.set_disk(T.TEX, *disk_args)
        gpu.shade(**kw)
        g = gpu.draw(frame, sc, w, h)
        hit_frames += int((c["hits"][..., 0] > 0.0).any())
        if not same(g, c) or g["total"] != c["total"]:
            bad.append(f"{desc} tol={tol} {w}x{h}: {differing(g, c)}")
    gpu.close()
    assert len(FUZZ_SEEDS) >= 200 and hit_frames >= len(FUZZ_SEEDS) // 2, hit_frames
    assert not bad, f"{len(bad)} of {len(FUZZ_SEEDS)} differ; first: {bad[0]}"


# ---- 6. refusals ----------------------------------------------------------------------
def _raw(gpu, frame, scene, b, w=W, h=H, band_rows=None, nbands=1):
    band_rows = h if band_rows is None else band_rows
    return lib.geo_render_disk_adaptive(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(scene), w, h, band_rows, 0,
                                        band_rows, nbands, b["rgba"].data_ptr(), None, None, None, None, None)


def test_refusals(dev):
    import torch

    frame, scene, _, disk_args = T.pose("A")
    sc_ok = A.adaptive_of(scene)
    direct = scene
    plain_adaptive = A.adaptive_of(scene, flags=0)
    gpu = Gpu(dev, disk_args)
    # the frames the older calls draw, before the refusals
    b0 = gpu.buffers(H, W)
    gpu.ctx.render_rows(frame, direct, W, H, 0, H, b0["rgba"], b0["mask"], b0["uv"], b0["steps"], b0["total"])
    direct_before = gpu.host(b0, H, W)
    b0 = gpu.buffers(H, W)
    gpu.ctx.render_rows(frame, plain_adaptive, W, H, 0, H, b0["rgba"], b0["mask"], b0["uv"], b0["steps"], b0["total"])
    plain_before = gpu.host(b0, H, W)
    ok_before = gpu.draw(frame, sc_ok, W, H)
    # mask, uv, steps and the total are the plain adaptive render's
    assert all(np.array_equal(ok_before[f], plain_before[f]) for f in ("mask", "steps"))
    assert np.array_equal(ok_before["uv"].view(np.uint32), plain_before["uv"].view(np.uint32))
    assert ok_before["total"] == plain_before["total"]

    def sc(mode=GEO_MODE_ADAPTIVE, flags=GEO_FLAG_DISK, rs=scene.rs, sphere=scene.sphere_r, r_obs=scene.r_obs, tol=0.0):
        return make_scene(rs, sphere, r_obs, scene.step, scene.max_steps, mode, flags, tol)

    b = gpu.buffers(H, W)
    b["rgba"].fill_(7)
    gpu.ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    refused = [sc(mode=GEO_MODE_DIRECT), sc(mode=GEO_MODE_FAN), sc(flags=0), sc(mode=GEO_MODE_DIRECT, flags=0),
               sc(flags=GEO_FLAG_DISK | GEO_FLAG_MIPS), sc(flags=GEO_FLAG_DISK | GEO_FLAG_COMPOSITE),
               sc(flags=GEO_FLAG_DISK | GEO_FLAG_RING_F64), sc(flags=GEO_FLAG_DISK | GEO_FLAG_SS4),
               sc(tol=-1.0), sc(tol=math.inf), sc(r_obs=0.9), sc(rs=3.5), sc(sphere=8.0), sc(sphere=12.0)]
    for bad in refused:
        assert _raw(gpu, frame, bad, b) == GEO_EINVAL, (bad.mode, bad.flags, bad.tol, bad.rs, bad.sphere_r, bad.r_obs)
    # the layout's rules: a band set's band_rows is a multiple of 8; a row range is any number of rows
    assert _raw(gpu, frame, sc_ok, b, band_rows=20, nbands=2) == GEO_EINVAL
    assert _raw(gpu, frame, sc_ok, b, band_rows=0) == GEO_EINVAL
    # r_in > 1.5 rs with a shift or an emission
    gpu.ctx.set_disk(T.TEX, 3.0, 9.0)
    assert _raw(gpu, frame, sc(rs=2.5), b) == GEO_OK
    torch.cuda.synchronize()
    b["rgba"].fill_(7)
    gpu.shade(shift=SHIFT)
    assert _raw(gpu, frame, sc(rs=2.5), b) == GEO_EINVAL
    gpu.shade(em=TE.emission())
    assert _raw(gpu, frame, sc(rs=2.5), b) == GEO_EINVAL
    gpu.shade()
    gpu.ctx.set_disk(T.TEX, *disk_args)
    # the ring state: refused with a capture orbit to draw, ignored without one
    gpu.ctx.set_disk_ring_f64(True)
    assert _raw(gpu, frame, sc_ok, b) == GEO_EINVAL
    torch.cuda.synchronize()
    assert (b["rgba"].cpu().numpy() == 7).all()  # nothing written by any refused call
    flat = gpu.draw(frame, sc(rs=0.0), W, H)
    gpu.ctx.set_disk_ring_f64(False)
    flat_off = gpu.draw(frame, sc(rs=0.0), W, H)
    assert same(flat, flat_off) and (flat["hits"][..., 0, 0] > 0).sum() > 100
    # armed buffers and the timing pair are consumed by a refused call
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    armed = gpu.buffers(H, W)
    gpu.arm(armed)
    e0, e1 = HipEvent(), HipEvent()
    gpu.ctx.time_next_render(e0, e1)
    assert _raw(gpu, frame, sc(mode=GEO_MODE_DIRECT), armed) == GEO_EINVAL
    assert _raw(gpu, frame, sc_ok, armed) == GEO_OK  # a good render: nothing is armed any more
    torch.cuda.synchronize()
    assert (armed["hits"].cpu().numpy() == -1.0).all() and (armed["g"].cpu().numpy() == -1.0).all()
    with pytest.raises(RuntimeError):
        e0.elapsed_time(e1)  # never recorded
    # no disk, no sky
    gpu.ctx.clear_disk()
    assert _raw(gpu, frame, sc_ok, b) == GEO_ESTATE
    nosky = Gpu(dev, disk_args, sky=False)
    assert _raw(nosky, frame, sc_ok, b) == GEO_ESTATE
    nosky.close()
    # after all of them: the same bytes as before
    gpu.ctx.set_disk(T.TEX, *disk_args)
    b1 = gpu.buffers(H, W)
    gpu.ctx.render_rows(frame, direct, W, H, 0, H, b1["rgba"], b1["mask"], b1["uv"], b1["steps"], b1["total"])
    direct_after = gpu.host(b1, H, W)
    b1 = gpu.buffers(H, W)
    gpu.ctx.render_rows(frame, plain_adaptive, W, H, 0, H, b1["rgba"], b1["mask"], b1["uv"], b1["steps"], b1["total"])
    plain_after = gpu.host(b1, H, W)
    ok_after = gpu.draw(frame, sc_ok, W, H)
    for before, after in ((direct_before, direct_after), (plain_before, plain_after), (ok_before, ok_after)):
        assert same(before, after) and before["total"] == after["total"]
    # the older entry points keep refusing the adaptive disk
    assert lib.geo_render_rows(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(sc_ok), W, H, 0, H,
                               b["rgba"].data_ptr(), None, None, None, None, None) == GEO_EINVAL
    assert lib.geo_render_band_set(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(sc_ok), W, H, 8, 0, 8, 6,
                                   b["rgba"].data_ptr(), None, None, None, None, None) == GEO_EINVAL
    gpu.close()
