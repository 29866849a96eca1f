"""Doppler and redshift shading of the thin disk on the device:
geo_render_disk_frame_kernel (Shade::kDiskShift) against the CPU path (geo_render_cpu_disk_shift,
the same header csrc/geo_disk.h) bit for bit in every output and the g slots,
for each integration kind, a moving observer, partial tiles, a band set and
both dispatch orders, and the C-ABI's state rules (geo.h).
tests/test_disk_shift_cpu.py ties the CPU path to the physics."""
import ctypes
import math

import numpy as np
import pytest

import test_disk_cpu as T
import test_disk_shift_cpu as X
import test_gpu_disk as G
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import _lib, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DISK, GEO_FLAG_MIPS,
                                                   GEO_FLAG_RING_F64, GEO_MODE_ADAPTIVE, GEO_OK, GeoDiskShift, lib)

pytestmark = pytest.mark.gpu
SHIFT = (1, 4, 1.0)


@pytest.fixture(scope="module")
def cpu():
    return X.load_cpu()


class Gpu(G.Gpu):
    """test_gpu_disk's context with the shading set and the g slots armed."""

    def __init__(self, dev, disk_args, shift=SHIFT, tex=T.TEX):
        super().__init__(dev, disk_args, tex)
        if shift is not None:
            self.ctx.set_disk_shift(*shift)

    def g_buffer(self, nrows, w):
        import torch

        return torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=self.dev)

    def rows(self, frame, scene, w, h, row0=0, nrows=None, arm_g=True):
        nrows = h - row0 if nrows is None else nrows
        b = self.buffers(nrows, w)
        gb = self.g_buffer(nrows, w)
        self.ctx.disk_hits_next_render(b["hits"])
        if arm_g:
            self.ctx.disk_shift_next_render(gb)
        self.ctx.render_rows(frame, scene, w, h, row0, nrows, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
        out = self.host(b, nrows, w)
        out["g"] = gb.cpu().numpy().reshape(nrows, w, 3)
        return out


def same(a, b):
    return G.same(a, b) and np.array_equal(a["g"].view(np.uint32), b["g"].view(np.uint32))


def curved_in():
    """An observer at rest between rs and 1.5 rs (kCurvedIn) looking outwards
    at a tilted disk: all three slots are hit."""
    pos = (1.3, 0.0, 0.3)
    frame = default_frame(T.W, T.H, pos=pos, camera=(0.0, -0.3), state=0)
    scene = make_scene(1.0, 50.0, math.sqrt(sum(p * p for p in pos)), T.STEP, 2048, flags=GEO_FLAG_DISK)
    args = (3.0, 9.0, (0.3, -0.2, 1.0), (1.0, 0.0, 0.0))
    return frame, scene, T.make_disk(*args), args, T.W, T.H


def case(name):
    """frame, scene, disk, disk_args, w, h"""
    if name == "curved_in":
        return curved_in()
    if name == "moving":  # movement_to_central is a rotation, k = 0.3; 97 x 55
        w, h = T.W + 1, T.H + 1
        frame, scene, disk = X.moving_frame(0.3, w, h)
        return frame, scene, disk, T.pose("flat")[3], w, h
    w, h = (70, 37) if name == "partial" else (T.W, T.H)
    frame, scene, disk, args = T.pose("A" if name == "partial" else name, w, h)
    return frame, scene, disk, args, w, h


@pytest.mark.parametrize("name", ["A", "B", "curved_in", "flat", "moving", "partial"])
def test_kernel_equals_cpu_path(dev, cpu, name):
    frame, scene, disk, disk_args, w, h = case(name)
    rc, c = X.render(cpu, frame, scene, w, h, disk, shift=SHIFT)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args)
    g = gpu.rows(frame, scene, w, h)
    gpu.close()
    hit = c["hits"][..., 0] > 0.0
    assert hit[..., 0].sum() > 300  # a real disk on both sides
    if name not in ("flat",):
        assert np.unique(c["g"][hit]).size > 100  # and a real shift
    assert same(g, c), name
    assert g["total"] == c["total"]


def test_other_spin_exponent_and_gain(dev, cpu):
    frame, scene, disk, disk_args, w, h = case("B")
    shift = (-1, 3, 0.5)
    rc, c = X.render(cpu, frame, scene, w, h, disk, shift=shift)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args, shift)
    g = gpu.rows(frame, scene, w, h)
    gpu.close()
    assert same(g, c)


def test_band_set_and_dispatch_orders(dev, cpu):
    import torch

    frame, scene, disk, disk_args, w, h = case("A")
    rc, c = X.render(cpu, frame, scene, w, h, disk, shift=SHIFT)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args)
    # geo_render_band_set, 8-row bands at rows 0, 8, ..., 40
    br, nb = 8, 6
    b = gpu.buffers(nb * br, w)
    gb = gpu.g_buffer(nb * br, w)
    gpu.ctx.disk_hits_next_render(b["hits"])
    gpu.ctx.disk_shift_next_render(gb)
    gpu.ctx.render_band_set(frame, scene, w, h, br, 0, 8, nb, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
    got = gpu.host(b, nb * br, w)
    got["g"] = gb.cpu().numpy().reshape(nb * br, w, 3)
    for f in ("rgba", "mask", "steps"):
        assert np.array_equal(got[f], c[f][:nb * br]), f
    for f in ("uv", "hits", "g"):
        assert np.array_equal(got[f].view(np.uint32), c[f][:nb * br].view(np.uint32)), f
    # both dispatch orders
    gpu.ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    assert same(gpu.rows(frame, scene, w, h), c)
    gpu.ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        assert same(gpu.rows(frame, scene, w, h), c), i
    rec, _ = gpu.ctx.dispatch_stats()
    torch.cuda.synchronize()
    gpu.close()
    assert rec >= 1


def test_shifted_then_unshifted(dev, cpu):
    """One context: a shifted render, geo_set_disk_shift(NULL), an unshifted
    one.  The unshifted frame is geo_render_cpu_disk's, and a g buffer armed
    before it is neither written nor left armed."""
    frame, scene, disk, disk_args, w, h = case("A")
    rc, c = X.render(cpu, frame, scene, w, h, disk, shift=SHIFT)
    rcp, p = T.render(cpu, frame, scene, T.SKY, w, h, disk, T.TEX)
    assert rc == GEO_OK and rcp == GEO_OK
    gpu = Gpu(dev, disk_args)
    assert same(gpu.rows(frame, scene, w, h), c)
    assert lib.geo_set_disk_shift(gpu.ctx._h, None) == GEO_OK
    u = gpu.rows(frame, scene, w, h)  # arms the g buffer (prefilled with -1) before the unshifted render
    assert G.same(u, p) and u["total"] == p["total"]
    assert (u["g"] == -1.0).all()
    # shifted again, nothing armed: the earlier arming was consumed, no g is written anywhere
    gpu.ctx.set_disk_shift(*SHIFT)
    again = gpu.rows(frame, scene, w, h, arm_g=False)
    assert G.same(again, c) and (again["g"] == -1.0).all()
    assert not np.array_equal(c["rgba"], p["rgba"])
    gpu.close()


def _raw_rows(gpu, frame, scene, b, w=T.W, h=T.H):
    return lib.geo_render_rows(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(scene), w, h, 0, h, b["rgba"].data_ptr(),
                               None, None, None, None, None)


def test_g_buffer_consumed_by_refused_call(dev):
    import torch

    frame, scene, _, disk_args = T.pose("A")
    gpu = Gpu(dev, disk_args)
    b = gpu.buffers(T.H, T.W)
    gb = gpu.g_buffer(T.H, T.W)
    gpu.ctx.disk_shift_next_render(gb)
    bad = T.make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, GEO_MODE_ADAPTIVE,
                       GEO_FLAG_DISK)
    assert _raw_rows(gpu, frame, bad, b) == GEO_EINVAL
    assert _raw_rows(gpu, frame, scene, b) == GEO_OK  # a good shifted render: the buffer is no longer armed
    torch.cuda.synchronize()
    assert (gb.cpu().numpy() == -1.0).all()
    gpu.ctx.disk_shift_next_render(gb)
    assert _raw_rows(gpu, frame, scene, b) == GEO_OK
    torch.cuda.synchronize()
    assert (gb.cpu().numpy() != -1.0).all()
    assert lib.geo_disk_shift_next_render(gpu.ctx._h, None) == GEO_EINVAL
    gpu.close()


def test_state_rules(dev, cpu):
    import torch

    frame, scene, disk, disk_args = T.pose("A")
    r_in, r_out, normal, axis = disk_args
    rc, c = X.render(cpu, frame, scene, T.W, T.H, disk, shift=SHIFT)
    rcp, p = T.render(cpu, frame, scene, T.SKY, T.W, T.H, disk, T.TEX)
    assert rc == GEO_OK and rcp == GEO_OK
    gpu = Gpu(dev, disk_args, shift=None)
    h = gpu.ctx._h
    # the setter's own checks; a refused call leaves the state as it was
    assert lib.geo_set_disk_shift(h, ctypes.byref(GeoDiskShift(-1, 3, 0.5))) == GEO_OK
    for bad in ((0, 4, 1.0), (2, 4, 1.0), (1, 5, 1.0), (1, 4, 0.0), (1, 4, -2.0), (1, 4, math.inf), (1, 4, math.nan)):
        assert lib.geo_set_disk_shift(h, ctypes.byref(GeoDiskShift(*bad))) == GEO_EINVAL, bad
    rc, other = X.render(cpu, frame, scene, T.W, T.H, disk, shift=(-1, 3, 0.5))
    assert rc == GEO_OK and same(gpu.rows(frame, scene, T.W, T.H), other)
    assert lib.geo_set_disk_shift(None, None) == GEO_EINVAL
    # it survives geo_set_disk (a texture swapped under it) ...
    gpu.ctx.set_disk_shift(*SHIFT)
    one = np.empty((4, 8, 4), np.uint8)
    one[:] = np.array([10, 200, 30, 255], np.uint8)
    gpu.ctx.set_disk(one, r_in, r_out, normal, axis)
    rc, c1 = X.render(cpu, frame, scene, T.W, T.H, disk, one, shift=SHIFT)
    assert rc == GEO_OK and same(gpu.rows(frame, scene, T.W, T.H), c1)
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    assert same(gpu.rows(frame, scene, T.W, T.H), c)
    # ... and geo_clear_disk clears it
    gpu.ctx.clear_disk()
    b = gpu.buffers(T.H, T.W, hits=False)
    assert _raw_rows(gpu, frame, scene, b) == GEO_ESTATE
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    u = gpu.rows(frame, scene, T.W, T.H)
    assert G.same(u, p) and (u["g"] == -1.0).all()
    # r_in > 1.5 rs is asked of a shifted render only, at render time
    def sc(rs, mode=0, flags=GEO_FLAG_DISK):
        return T.make_scene(rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, mode, flags)

    assert _raw_rows(gpu, frame, sc(2.0), b) == GEO_OK
    gpu.ctx.set_disk_shift(*SHIFT)
    assert _raw_rows(gpu, frame, sc(2.0), b) == GEO_EINVAL
    assert _raw_rows(gpu, frame, sc(2.5), b) == GEO_EINVAL
    assert _raw_rows(gpu, frame, sc(1.9999), b) == GEO_OK
    assert _raw_rows(gpu, frame, sc(0.0), b) == GEO_OK
    # what GEO_FLAG_DISK refuses stays refused
    for bad in (sc(1.0, mode=GEO_MODE_ADAPTIVE), sc(1.0, flags=GEO_FLAG_DISK | GEO_FLAG_MIPS),
                sc(1.0, flags=GEO_FLAG_DISK | GEO_FLAG_COMPOSITE), sc(1.0, flags=GEO_FLAG_DISK | GEO_FLAG_RING_F64)):
        assert _raw_rows(gpu, frame, bad, b) == GEO_EINVAL
    ok = sc(1.0)
    assert lib.geo_render_band_set_frames(h, ctypes.byref(frame), 1, ctypes.byref(ok), T.W, T.H, 8, 0, 8, 6,
                                          b["rgba"].data_ptr(), T.W * 48 * 4, None, None) == GEO_EINVAL
    # a plain render is untouched by the state
    plain = T.plain_of(scene)
    before = gpu.rows(frame, plain, T.W, T.H)
    gpu.ctx.clear_disk_shift()
    after = gpu.rows(frame, plain, T.W, T.H)
    assert G.same(before, after, hits=False) and (before["g"] == -1.0).all()
    torch.cuda.synchronize()
    gpu.close()
    assert _lib.GEO_DISK_MAX_CROSSINGS == 3
