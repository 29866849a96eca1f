"""GEO_FLAG_DISK on the device: geo_render_disk_frame_kernel (Shade::kDisk) against the CPU path
(geo_render_cpu_disk, the same header csrc/geo_disk.h) bit for bit, on whole
frames, partial tiles and bands, under the learned dispatch order, and the
C-ABI's rules (geo.h).  tests/test_disk_cpu.py ties the CPU path to geometry
and to the f64 restatement."""
import ctypes
import math

import numpy as np
import pytest

import test_disk_cpu as T
from schwarzschild_raytracer_wgpu_amd import _lib
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DISK, GEO_FLAG_MIPS,
                                                   GEO_FLAG_RING_F64, GEO_MODE_ADAPTIVE, GEO_MODE_FAN, GEO_OK, lib)

pytestmark = pytest.mark.gpu


class Gpu:
    """One context with the test sky and a disk; whole-frame renders with every output."""

    def __init__(self, dev, disk_args=None, tex=T.TEX):
        import schwarzschild_raytracer_wgpu_amd as g

        self.dev = dev
        self.ctx = g.Context(dev.index or 0)
        self.ctx.set_sky(T.SKY)
        if disk_args is not None:
            r_in, r_out, normal, axis = disk_args
            self.ctx.set_disk(tex, r_in, r_out, normal, axis)

    def buffers(self, nrows, w, hits=True):
        import torch

        d = self.dev
        b = dict(rgba=torch.zeros(nrows * w * 4, dtype=torch.uint8, device=d),
                 mask=torch.zeros(nrows * w, dtype=torch.uint8, device=d),
                 uv=torch.zeros(nrows * w * 2, dtype=torch.float32, device=d),
                 steps=torch.zeros(nrows * w, dtype=torch.int32, device=d),
                 total=torch.zeros(1, dtype=torch.int64, device=d))
        if hits:
            b["hits"] = torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=d)
        return b

    @staticmethod
    def host(b, nrows, w):
        import torch

        torch.cuda.synchronize()
        out = dict(rgba=b["rgba"].cpu().numpy().reshape(nrows, w, 4), mask=b["mask"].cpu().numpy().reshape(nrows, w),
                   uv=b["uv"].cpu().numpy().reshape(nrows, w, 2),
                   steps=b["steps"].cpu().numpy().view(np.uint32).reshape(nrows, w), total=int(b["total"].item()))
        if "hits" in b:
            out["hits"] = b["hits"].cpu().numpy().reshape(nrows, w, 3, 2)
        return out

    def rows(self, frame, scene, w, h, row0=0, nrows=None, hits=True):
        nrows = h - row0 if nrows is None else nrows
        b = self.buffers(nrows, w, hits)
        if hits:
            self.ctx.disk_hits_next_render(b["hits"])
        self.ctx.render_rows(frame, scene, w, h, row0, nrows, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
        return self.host(b, nrows, w)

    def close(self):
        self.ctx.close()


def same(a, b, hits=True):
    ok = all(np.array_equal(a[f], b[f]) for f in ("rgba", "mask", "steps"))
    ok = ok and np.array_equal(a["uv"].view(np.uint32), b["uv"].view(np.uint32))
    if hits:
        ok = ok and np.array_equal(a["hits"].view(np.uint32), b["hits"].view(np.uint32))
    return ok


@pytest.fixture(scope="module")
def cpu():
    return T.load_cpu()


@pytest.mark.parametrize("name", ["A", "B", "flat", "tilted"])
def test_kernel_equals_cpu_path(dev, cpu, name):
    frame, scene, disk, disk_args = T.pose(name)
    rc, c = T.render(cpu, frame, scene, T.SKY, T.W, T.H, disk, T.TEX)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args)
    g = gpu.rows(frame, scene, T.W, T.H)
    gpu.close()
    assert (c["hits"][..., 0, 0] > 0).sum() > 300  # a real disk on both sides
    assert same(g, c), name
    assert g["total"] == c["total"]


def test_partial_tiles_and_bands(dev, cpu):
    import torch

    # a 100 x 37 frame (no multiple of the 32 x 8 tile), rows 5..24
    w, h = 100, 37
    frame, scene, disk, disk_args = T.pose("A", w, h)
    gpu = Gpu(dev, disk_args)
    whole = gpu.rows(frame, scene, w, h)
    rc, c = T.render(cpu, frame, scene, T.SKY, w, h, disk, T.TEX)
    assert rc == GEO_OK and same(whole, c)
    part = gpu.rows(frame, scene, w, h, row0=5, nrows=20)
    assert same(part, {f: (whole[f][5:25] if f != "total" else None) for f in whole})
    # 8-row bands 0, 2, 4, 6 of the 96 x 54 frame (band 6 clipped to rows 48..53)
    frame, scene, disk, _ = T.pose("A")
    whole = gpu.rows(frame, scene, T.W, T.H)
    nb, br = 4, 8
    b = gpu.buffers(nb * br, T.W)
    gpu.ctx.disk_hits_next_render(b["hits"])
    gpu.ctx.render_bands(frame, scene, T.W, T.H, br, 0, 2, nb, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
    got = gpu.host(b, nb * br, T.W)
    torch.cuda.synchronize()
    gpu.close()
    for i in range(nb):
        r0 = 2 * i * br
        n = min(br, T.H - r0)
        for f in ("rgba", "mask", "steps"):
            assert np.array_equal(got[f][i * br:i * br + n], whole[f][r0:r0 + n]), (f, i)
        for f in ("uv", "hits"):
            assert np.array_equal(got[f][i * br:i * br + n].view(np.uint32), whole[f][r0:r0 + n].view(np.uint32)), (f, i)
    # clipped rows are not written: the hit slots keep their prefill
    assert (got["hits"][3 * br + (T.H - 48):] == -1.0).all()


def test_learned_dispatch_order(dev):
    frame, scene, _, disk_args = T.pose("B")
    gpu = Gpu(dev, disk_args)
    gpu.ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    ref = gpu.rows(frame, scene, T.W, T.H)
    gpu.ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        assert same(gpu.rows(frame, scene, T.W, T.H), ref), i
    rec, _ = gpu.ctx.dispatch_stats()
    gpu.close()
    assert rec >= 1


def test_steps_total_and_plain_render_unchanged(dev):
    frame, scene, _, disk_args = T.pose("A")
    plain = T.plain_of(scene)
    gpu = Gpu(dev)
    before = gpu.rows(frame, plain, T.W, T.H, hits=False)
    r_in, r_out, normal, axis = disk_args
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    after = gpu.rows(frame, plain, T.W, T.H, hits=False)
    assert same(before, after, hits=False) and before["total"] == after["total"]
    d = gpu.rows(frame, scene, T.W, T.H)
    gpu.close()
    assert d["total"] == before["total"] == int(before["steps"].astype(np.int64).sum())
    assert np.array_equal(d["mask"], before["mask"]) and np.array_equal(d["steps"], before["steps"])
    assert np.array_equal(d["uv"].view(np.uint32), before["uv"].view(np.uint32))
    assert not np.array_equal(d["rgba"], before["rgba"])


def _raw_rows(gpu, frame, scene, b, w=T.W, h=T.H):
    return lib.geo_render_rows(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(scene), w, h, 0, h, b["rgba"].data_ptr(),
                               None, None, None, None, None)


def test_hits_buffer_consumed_by_refused_call(dev):
    import torch

    frame, scene, _, disk_args = T.pose("A")
    gpu = Gpu(dev, disk_args)
    b = gpu.buffers(T.H, T.W)
    gpu.ctx.disk_hits_next_render(b["hits"])
    bad = T.make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, GEO_MODE_ADAPTIVE,
                       GEO_FLAG_DISK)
    assert _raw_rows(gpu, frame, bad, b) == GEO_EINVAL
    assert _raw_rows(gpu, frame, scene, b) == GEO_OK  # a good disk render: the buffer is no longer armed
    torch.cuda.synchronize()
    assert (b["hits"].cpu().numpy() == -1.0).all()
    # armed again, it is written
    gpu.ctx.disk_hits_next_render(b["hits"])
    assert _raw_rows(gpu, frame, scene, b) == GEO_OK
    torch.cuda.synchronize()
    assert (b["hits"].cpu().numpy() != -1.0).all()
    gpu.close()


def test_statuses(dev):
    frame, scene, _, disk_args = T.pose("A")
    gpu = Gpu(dev)
    b = gpu.buffers(T.H, T.W, hits=False)
    assert _raw_rows(gpu, frame, scene, b) == GEO_ESTATE  # no disk set
    r_in, r_out, normal, axis = disk_args
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    assert _raw_rows(gpu, frame, scene, b) == GEO_OK
    gpu.ctx.clear_disk()
    assert _raw_rows(gpu, frame, scene, b) == GEO_ESTATE
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)

    def sc(mode=0, flags=GEO_FLAG_DISK, rs=scene.rs, sphere=scene.sphere_r, r_obs=scene.r_obs):
        return T.make_scene(rs, sphere, r_obs, scene.step, scene.max_steps, mode, flags)

    gpu.ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    for bad in (sc(mode=GEO_MODE_FAN), sc(mode=GEO_MODE_ADAPTIVE), sc(flags=GEO_FLAG_DISK | GEO_FLAG_MIPS),
                sc(flags=GEO_FLAG_DISK | GEO_FLAG_COMPOSITE), sc(flags=GEO_FLAG_DISK | GEO_FLAG_RING_F64),
                sc(r_obs=0.9), sc(rs=3.5), sc(sphere=8.0), sc(sphere=12.0)):
        assert _raw_rows(gpu, frame, bad, b) == GEO_EINVAL
    # the batched entry points
    h = gpu.ctx._h
    ok = sc()
    rgba = b["rgba"].data_ptr()
    assert lib.geo_render_band_set_frames(h, ctypes.byref(frame), 1, ctypes.byref(ok), T.W, T.H, 8, 0, 8, 6, rgba,
                                          T.W * 48 * 4, None, None) == GEO_EINVAL
    assert lib.geo_render_band_set_batch(h, ctypes.byref(frame), ctypes.byref(ok), 1, T.W, T.H, 8, 0, 8, 6, rgba,
                                         T.W * 48 * 4, None, None) == GEO_EINVAL
    # geo_render_band_set accepts it
    assert lib.geo_render_band_set(h, ctypes.byref(frame), ctypes.byref(ok), T.W, T.H, 8, 0, 8, 6, rgba, None, None,
                                   None, None, None) == GEO_OK
    # geo_set_disk's own checks
    tex = np.ascontiguousarray(T.TEX)
    for bad in (T.make_disk(0.0, 9.0), T.make_disk(9.0, 3.0), T.make_disk(3.0, 9.0, normal=(0, 0, 0)),
                T.make_disk(3.0, 9.0, axis=(0, 0, 1.0))):
        assert lib.geo_set_disk(h, ctypes.byref(bad), tex.ctypes.data, tex.shape[1], tex.shape[0]) == GEO_EINVAL
    import torch

    torch.cuda.synchronize()
    gpu.close()
    assert _lib.GEO_FLAG_DISK == 16 and _lib.GEO_DISK_MAX_CROSSINGS == 3 and math.isfinite(T.STEP)
