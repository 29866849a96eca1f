"""Blackbody emission of the thin disk on the device:
geo_render_disk_frame_kernel and geo_render_ss_disk_frame_kernel (Shade::kDiskEmit) against the CPU path
(geo_render_cpu_disk_emission, the same header csrc/geo_disk.h) bit for bit in
every output and the g and q slots, for each integration kind, partial tiles,
the three one-frame entry points and both dispatch orders; GEO_FLAG_SS4 against
the CPU path and against the device's own double-size frame; and the C-ABI's
state rules and refusals (geo.h).  tests/test_disk_emission_cpu.py ties the
CPU path to the physics."""
import ctypes
import math

import numpy as np
import pytest

import test_disk_cpu as T
import test_disk_emission_cpu as X
import test_disk_shift_cpu as XS
import test_gpu_disk as G
import test_gpu_disk_shift as GS
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import _lib, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_DISK, GEO_FLAG_SS4, GEO_OK, GeoDiskEmission,
                                                   lib)

pytestmark = pytest.mark.gpu
EM = X.emission(X.THIN, exposure=2.0)
EM_POWER = X.emission(X.POWER, exposure=0.5, spin=-1)


@pytest.fixture(scope="module")
def cpu():
    return X.load_cpu()


def set_emission(ctx, em, ramp=X.RAMP):
    spin, profile, t_ref, t_lo, t_hi, exposure = em
    ctx.set_disk_emission(ramp, t_ref, t_lo, t_hi, profile, exposure, spin)


class Gpu(G.Gpu):
    """test_gpu_disk's context with the emission set and the g and q slots armed."""

    def __init__(self, dev, disk_args, em=EM, tex=T.TEX, ramp=X.RAMP):
        super().__init__(dev, disk_args, tex)
        if em is not None:
            set_emission(self.ctx, em, ramp)

    def slots(self, nrows, w):
        import torch

        return torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=self.dev)

    def arm(self, nrows, w, arm_q=True):
        b = self.buffers(nrows, w)
        b["g"], b["q"] = self.slots(nrows, w), self.slots(nrows, w)
        self.ctx.disk_hits_next_render(b["hits"])
        self.ctx.disk_shift_next_render(b["g"])
        if arm_q:
            self.ctx.disk_emission_next_render(b["q"])
        return b

    def host(self, b, nrows, w):
        out = G.Gpu.host(b, nrows, w)
        for f in ("g", "q"):
            out[f] = b[f].cpu().numpy().reshape(nrows, w, 3)
        return out

    def rows(self, frame, scene, w, h, row0=0, nrows=None, arm_q=True):
        nrows = h - row0 if nrows is None else nrows
        b = self.arm(nrows, w, arm_q)
        self.ctx.render_rows(frame, scene, w, h, row0, nrows, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
        return self.host(b, nrows, w)


def same(a, b):
    return G.same(a, b) and all(np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)) for f in ("g", "q"))


def case(name):
    """frame, scene, disk, disk_args, w, h: test_gpu_disk_shift's cases (A, B:
    kCurvedOut; curved_in: kCurvedIn; flat, moving: kFlat), and pose A at 70 x 27."""
    if name == "partial":
        w, h = 70, 27
        frame, scene, disk, args = T.pose("A", w, h)
        return frame, scene, disk, args, w, h
    return GS.case(name)


@pytest.mark.parametrize("name", ["A", "B", "curved_in", "flat", "moving", "partial"])
def test_kernel_equals_cpu_path(dev, cpu, name):
    frame, scene, disk, disk_args, w, h = case(name)
    em = EM_POWER if name in ("B", "moving") else EM
    rc, c = X.render(cpu, frame, scene, w, h, disk, em=em)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args, em)
    g = gpu.rows(frame, scene, w, h)
    gpu.close()
    hit = c["hits"][..., 0] > 0.0
    assert hit[..., 0].sum() > (150 if name == "partial" else 300)  # a real disk on both sides
    assert np.unique(c["q"][hit]).size > 100  # and a real temperature field
    assert same(g, c), name
    assert g["total"] == c["total"]


@pytest.mark.parametrize("ramp_name", ["2", "1024"])
def test_ramp_sizes_and_translucent_texture(dev, cpu, ramp_name):
    ramp = X.ramps()[ramp_name]
    one = np.empty((4, 8, 4), np.uint8)
    one[:] = np.array([10, 200, 30, 200], np.uint8)
    frame, scene, disk, disk_args, w, h = case("A")
    em = X.emission(X.THIN, exposure=40.0)
    rc, c = X.render(cpu, frame, scene, w, h, disk, one, em=em, ramp=ramp)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args, em, one, ramp)
    g = gpu.rows(frame, scene, w, h)
    gpu.close()
    assert same(g, c)


def test_entry_points_and_dispatch_orders(dev, cpu):
    import torch

    frame, scene, disk, disk_args, w, h = case("A")
    rc, c = X.render(cpu, frame, scene, w, h, disk, em=EM)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args)
    fields_eq, fields_bits = ("rgba", "mask", "steps"), ("uv", "hits", "g", "q")
    # geo_render_band_set, 8-row bands at rows 0, 8, ..., 40
    br, nb = 8, 6
    b = gpu.arm(nb * br, w)
    gpu.ctx.render_band_set(frame, scene, w, h, br, 0, 8, nb, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
    got = gpu.host(b, nb * br, w)
    for f in fields_eq:
        assert np.array_equal(got[f], c[f][:nb * br]), f
    for f in fields_bits:
        assert np.array_equal(got[f].view(np.uint32), c[f][:nb * br].view(np.uint32)), f
    # geo_render_bands, the 8-row bands 0, 2, 4, 6 (band 6 clipped to rows 48..53)
    nb = 4
    b = gpu.arm(nb * br, w)
    gpu.ctx.render_bands(frame, scene, w, h, br, 0, 2, nb, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
    got = gpu.host(b, nb * br, w)
    for i in range(nb):
        r0 = 2 * i * br
        n = min(br, h - r0)
        for f in fields_eq:
            assert np.array_equal(got[f][i * br:i * br + n], c[f][r0:r0 + n]), (f, i)
        for f in fields_bits:
            assert np.array_equal(got[f][i * br:i * br + n].view(np.uint32), c[f][r0:r0 + n].view(np.uint32)), (f, i)
    assert (got["q"][3 * br + (h - 48):] == -1.0).all()  # clipped rows are not written
    # both dispatch orders, the learned one rendered until an adopted order has been used
    gpu.ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    assert same(gpu.rows(frame, scene, w, h), c)
    gpu.ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        assert same(gpu.rows(frame, scene, w, h), c), i
        torch.cuda.synchronize()
    rec, _ = gpu.ctx.dispatch_stats()
    gpu.close()
    assert rec >= 1


class SsGpu(G.Gpu):
    def __init__(self, dev, disk_args, em=EM):
        super().__init__(dev, disk_args)
        set_emission(self.ctx, em)

    def colour(self, frame, scene, w, h):
        import torch

        rgba = torch.zeros(h * w * 4, dtype=torch.uint8, device=self.dev)
        total = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.ctx.render_rows(frame, scene, w, h, 0, h, rgba, steps_total=total)
        torch.cuda.synchronize()
        return rgba.cpu().numpy().reshape(h, w, 4), int(total.item())


def ss_of(scene):
    return make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps,
                      flags=GEO_FLAG_DISK | GEO_FLAG_SS4)


@pytest.mark.parametrize("name,size", [("A", (T.W, T.H)), ("curved_in", (T.W, T.H)), ("flat", (35, 13))])
def test_ss4(dev, cpu, name, size):
    """GEO_FLAG_SS4 with the emission: the CPU path's bytes, and the box
    resolve of the device's own one-sample frame of twice the size."""
    w, h = size
    if name == "curved_in":
        frame, scene, disk, disk_args, _, _ = case(name)
        frame2 = default_frame(2 * w, 2 * h, pos=(1.3, 0.0, 0.3), camera=(0.0, -0.3), state=0)
    else:
        frame, scene, disk, disk_args = T.pose(name, w, h)
        frame2 = T.pose(name, 2 * w, 2 * h)[0]
    rc, c = X.render(cpu, frame, ss_of(scene), w, h, disk, em=EM, outputs=False)
    assert rc == GEO_OK
    gpu = SsGpu(dev, disk_args)
    got, total = gpu.colour(frame, ss_of(scene), w, h)
    assert np.array_equal(got, c["rgba"]) and total == c["total"]
    big, total2 = gpu.colour(frame2, scene, 2 * w, 2 * h)
    gpu.close()
    s = big.astype(np.uint32).reshape(h, 2, w, 2, 4)
    assert np.array_equal(got, ((s.sum(axis=(1, 3)) + 2) >> 2).astype(np.uint8))
    assert total == total2


def _raw_rows(gpu, frame, scene, rgba, w=T.W, h=T.H):
    return lib.geo_render_rows(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(scene), w, h, 0, h, rgba.data_ptr(), None,
                               None, None, None, None)


def test_state(dev, cpu):
    """Set, render, clear, render: the shift's bytes again (its state was kept),
    then the unshaded ones; geo_set_disk keeps the emission, geo_clear_disk
    drops it; a refused set leaves the emission in force."""
    frame, scene, disk, disk_args = T.pose("A")
    r_in, r_out, normal, axis = disk_args
    w, h = T.W, T.H
    rc, c = X.render(cpu, frame, scene, w, h, disk, em=EM)
    rcs, s = XS.render(cpu, frame, scene, w, h, disk, shift=GS.SHIFT)
    rcp, p = T.render(cpu, frame, scene, T.SKY, w, h, disk, T.TEX)
    assert rc == GEO_OK and rcs == GEO_OK and rcp == GEO_OK
    gpu = Gpu(dev, disk_args, em=None)
    hd = gpu.ctx._h
    gpu.ctx.set_disk_shift(*GS.SHIFT)
    set_emission(gpu.ctx, EM)
    assert same(gpu.rows(frame, scene, w, h), c)  # the emission, not the shift (g is written all the same)
    # the setter's checks: a refused call leaves the state as it was
    ramp = np.ascontiguousarray(X.RAMP)
    bad = [X.emission(spin=0), X.emission(profile=2), X.emission(t_ref=0.0), X.emission(t_lo=math.nan),
           X.emission(t_hi=math.inf), X.emission(exposure=-1.0), X.emission(t_lo=5000.0, t_hi=5000.0)]
    for em in bad:
        e = GeoDiskEmission(*em)
        assert lib.geo_set_disk_emission(hd, ctypes.byref(e), ramp.ctypes.data, ramp.shape[0]) == GEO_EINVAL, em
    e = GeoDiskEmission(*EM)
    assert lib.geo_set_disk_emission(hd, ctypes.byref(e), None, 64) == GEO_EINVAL
    for n in (0, 1, 1025):
        assert lib.geo_set_disk_emission(hd, ctypes.byref(e), ramp.ctypes.data, n) == GEO_EINVAL
    assert lib.geo_set_disk_emission(None, None, None, 0) == GEO_EINVAL
    assert lib.geo_disk_emission_next_render(hd, None) == GEO_EINVAL
    assert same(gpu.rows(frame, scene, w, h), c)
    # it survives geo_set_disk (a texture swapped under it)
    one = np.empty((4, 8, 4), np.uint8)
    one[:] = np.array([10, 200, 30, 255], np.uint8)
    gpu.ctx.set_disk(one, r_in, r_out, normal, axis)
    rc, c1 = X.render(cpu, frame, scene, w, h, disk, one, em=EM)
    assert rc == GEO_OK and same(gpu.rows(frame, scene, w, h), c1)
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    # cleared: the shift takes effect again, and an armed q buffer is neither written nor left armed
    gpu.ctx.clear_disk_emission()
    u = gpu.rows(frame, scene, w, h)
    assert G.same(u, s) and np.array_equal(u["g"].view(np.uint32), s["g"].view(np.uint32)) and (u["q"] == -1.0).all()
    set_emission(gpu.ctx, EM)
    again = gpu.rows(frame, scene, w, h, arm_q=False)
    assert G.same(again, c) and (again["q"] == -1.0).all()
    # r_in > 1.5 rs at render time
    import torch

    rgba = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    sc = lambda rs: make_scene(rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, flags=GEO_FLAG_DISK)
    gpu.ctx.clear_disk_shift()
    assert _raw_rows(gpu, frame, sc(2.0), rgba) == GEO_EINVAL
    assert _raw_rows(gpu, frame, sc(1.9999), rgba) == GEO_OK
    gpu.ctx.clear_disk_emission()
    assert _raw_rows(gpu, frame, sc(2.0), rgba) == GEO_OK
    set_emission(gpu.ctx, EM)
    # a plain render is untouched by the state
    plain = T.plain_of(scene)
    before = gpu.rows(frame, plain, w, h)
    # geo_clear_disk drops the emission
    gpu.ctx.clear_disk()
    assert _raw_rows(gpu, frame, scene, rgba) == GEO_ESTATE
    after = gpu.rows(frame, plain, w, h)
    assert G.same(before, after, hits=False) and (before["q"] == -1.0).all()
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    u = gpu.rows(frame, scene, w, h)
    assert G.same(u, p) and (u["q"] == -1.0).all() and (u["g"] == -1.0).all()
    torch.cuda.synchronize()
    gpu.close()


def test_refusals(dev):
    import torch

    frame, scene, _, disk_args = T.pose("A")
    w, h = T.W, T.H
    gpu = Gpu(dev, disk_args)
    hd = gpu.ctx._h
    f, s_ = ctypes.byref(frame), ctypes.byref(scene)
    ss = ss_of(scene)
    # both batched entry points: GEO_EINVAL, nothing written
    out = torch.full((w * 48 * 4,), 0x5A, dtype=torch.uint8, device=dev)
    assert lib.geo_render_disk_batch(hd, f, s_, 1, w, h, 8, 0, 8, 6, out.data_ptr(), w * 48 * 4, None,
                                     None) == GEO_EINVAL
    assert lib.geo_render_ss_batch(hd, f, ctypes.byref(ss), 1, w, h, 8, 0, 8, 6, out.data_ptr(), w * 48 * 4, None,
                                   None) == GEO_EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
    # ... and they draw again once the emission is cleared
    gpu.ctx.clear_disk_emission()
    assert lib.geo_render_disk_batch(hd, f, s_, 1, w, h, 8, 0, 8, 6, out.data_ptr(), w * 48 * 4, None, None) == GEO_OK
    assert lib.geo_render_ss_batch(hd, f, ctypes.byref(ss), 1, w, h, 8, 0, 8, 6, out.data_ptr(), w * 48 * 4, None,
                                   None) == GEO_OK
    torch.cuda.synchronize()
    assert not (out.cpu().numpy() == 0x5A).all()
    set_emission(gpu.ctx, EM)
    # an armed q buffer is consumed by a refused call
    rgba = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    qb = gpu.slots(h, w)
    gpu.ctx.disk_emission_next_render(qb)
    bad = make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, _lib.GEO_MODE_ADAPTIVE,
                     GEO_FLAG_DISK)
    assert _raw_rows(gpu, frame, bad, rgba) == GEO_EINVAL
    assert _raw_rows(gpu, frame, scene, rgba) == GEO_OK  # a good emission render: the buffer is no longer armed
    torch.cuda.synchronize()
    assert (qb.cpu().numpy() == -1.0).all()
    # ... by a call refused before the scene is looked at, too
    gpu.ctx.disk_emission_next_render(qb)
    assert lib.geo_render_rows(hd, f, s_, w, h, 0, h + 1, rgba.data_ptr(), None, None, None, None, None) == GEO_EINVAL
    assert _raw_rows(gpu, frame, scene, rgba) == GEO_OK
    torch.cuda.synchronize()
    assert (qb.cpu().numpy() == -1.0).all()
    gpu.ctx.disk_emission_next_render(qb)
    assert _raw_rows(gpu, frame, scene, rgba) == GEO_OK
    torch.cuda.synchronize()
    assert (qb.cpu().numpy() != -1.0).all()
    # SS4 with an armed q buffer is refused (and consumes it); without it, it draws
    qb.fill_(-1.0)
    gpu.ctx.disk_emission_next_render(qb)
    assert _raw_rows(gpu, frame, ss, rgba) == GEO_EINVAL
    assert _raw_rows(gpu, frame, ss, rgba) == GEO_OK
    torch.cuda.synchronize()
    assert (qb.cpu().numpy() == -1.0).all()
    # a batched call with an armed q buffer is refused as with the other buffers
    gpu.ctx.clear_disk_emission()
    gpu.ctx.disk_emission_next_render(qb)
    assert lib.geo_render_disk_batch(hd, f, s_, 1, w, h, 8, 0, 8, 6, out.data_ptr(), w * 48 * 4, None,
                                     None) == GEO_EINVAL
    torch.cuda.synchronize()
    gpu.close()


def test_python_wrappers(dev, cpu):
    import torch

    import schwarzschild_raytracer_wgpu_amd as g

    frame, scene, disk, disk_args = T.pose("B")
    r_in, r_out, normal, axis = disk_args
    w, h = T.W, T.H
    ramp = X.blackbody_ramp(256, 1500.0, 30000.0)
    em = (-1, _lib.GEO_DISK_PROFILE_POWER, 7000.0, 1500.0, 30000.0, 1.5)
    rc, c = X.render(cpu, frame, scene, w, h, disk, em=em, ramp=ramp)
    assert rc == GEO_OK
    ctx = g.Context(dev.index or 0)
    ctx.set_sky(T.SKY)
    ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    ctx.set_disk_emission(ramp, 7000.0, 1500.0, 30000.0, profile=_lib.GEO_DISK_PROFILE_POWER, exposure=1.5, spin=-1)
    rgba = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    q = torch.full((h * w * 3,), -1.0, dtype=torch.float32, device=dev)
    ctx.disk_emission_next_render(q)
    ctx.render_rows(frame, scene, w, h, 0, h, rgba)
    torch.cuda.synchronize()
    assert np.array_equal(rgba.cpu().numpy().reshape(h, w, 4), c["rgba"])
    assert np.array_equal(q.cpu().numpy().reshape(h, w, 3).view(np.uint32), c["q"].view(np.uint32))
    with pytest.raises(ValueError):
        ctx.set_disk_emission(np.zeros((4, 3), np.uint8), 7000.0, 1500.0, 30000.0)
    with pytest.raises(ValueError):
        ctx.disk_emission_next_render(torch.zeros(8, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.GeoError):
        ctx.set_disk_emission(ramp, 7000.0, 30000.0, 1500.0)
    ctx.clear_disk_emission()
    rcp, p = T.render(cpu, frame, scene, T.SKY, w, h, disk, T.TEX)
    ctx.render_rows(frame, scene, w, h, 0, h, rgba)
    torch.cuda.synchronize()
    assert rcp == GEO_OK and np.array_equal(rgba.cpu().numpy().reshape(h, w, 4), p["rgba"])
    ctx.close()


def test_sharded_frame(dev, cpu):
    """dist.ShardedFrame: batch_launch=True names the refusal; batch_launch=False
    draws the emission frame through the one-frame launches."""
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd.dist import ShardedFrame

    frame, scene, disk, disk_args = T.pose("A")
    r_in, r_out, normal, axis = disk_args
    w, h = T.W, T.H
    rc, c = X.render(cpu, frame, scene, w, h, disk, em=EM)
    assert rc == GEO_OK
    ctx = g.Context(dev.index or 0)
    ctx.set_sky(T.SKY)
    ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    set_emission(ctx, EM)
    with pytest.raises(ValueError, match="set_disk_emission"):
        ShardedFrame(ctx, frame, scene, w, h, 8, 0, 1, dev, frames_per_gather=2, batch_launch=True)
    sf = ShardedFrame(ctx, frame, scene, w, h, 8, 0, 1, dev, frames_per_gather=2, batch_launch=False)
    for i in range(3):
        sf.step(i)
    sf.drain()
    torch.cuda.synchronize()
    assert np.array_equal(sf.frame_rgba().cpu().numpy().reshape(h, w, 4), c["rgba"])
    # the emission cleared: the batched object is built again
    ctx.clear_disk_emission()
    assert ShardedFrame(ctx, frame, scene, w, h, 8, 0, 1, dev, frames_per_gather=2, batch_launch=True).batch
    ctx.close()
