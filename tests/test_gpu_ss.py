"""GEO_FLAG_SS4 on the device: geo_render_ss_sky_kernel (the plain frame) and
geo_render_ss_disk_frame_kernel (the disk and the shifted disk frame) against the CPU path (tests/test_ss_cpu.py) byte for
byte, against its own definition (the numpy resolve of the GPU's one-sample
render at twice the size), on partial tiles, rows and bands, under the learned
dispatch order, and the C-ABI's rules (geo.h)."""
import ctypes

import numpy as np
import pytest

import test_disk_cpu as T
import test_ss_cpu as S
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4, GEO_MODE_ADAPTIVE,
                                                   GEO_MODE_FAN, GEO_OK, lib)

pytestmark = pytest.mark.gpu
PREFILL = S.PREFILL
GUARD = 3  # rows after the requested ones, which no render may touch


@pytest.fixture(scope="module")
def cpu():
    return S.X.load_cpu()


class Gpu:
    """One context with the test sky and, by kind, the disk and the shift state."""

    def __init__(self, dev, kind="plain", disk_args=None, sky=True):
        import schwarzschild_raytracer_wgpu_amd as g

        self.dev = dev
        self.ctx = g.Context(dev.index or 0)
        if sky:
            self.ctx.set_sky(T.SKY)
        if kind != "plain" and disk_args is not None:
            r_in, r_out, normal, axis = disk_args
            self.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
        if kind == "shift":
            self.ctx.set_disk_shift(*S.SHIFT)

    def out(self, nrows, w):
        import torch

        return (torch.full(((nrows + GUARD) * w * 4,), PREFILL, dtype=torch.uint8, device=self.dev),
                torch.zeros(1, dtype=torch.int64, device=self.dev))

    @staticmethod
    def host(rgba, total, nrows, w):
        """The rows' bytes and steps_total; the guard rows must hold their prefill."""
        import torch

        torch.cuda.synchronize()
        a = rgba.cpu().numpy().reshape(nrows + GUARD, w, 4)
        assert (a[nrows:] == PREFILL).all(), "rows past the requested ones were written"
        return a[:nrows], int(total.item())

    def rows(self, frame, scene, w, h, row0=0, nrows=None):
        nrows = h - row0 if nrows is None else nrows
        rgba, total = self.out(nrows, w)
        self.ctx.render_rows(frame, scene, w, h, row0, nrows, rgba, steps_total=total)
        return self.host(rgba, total, nrows, w)

    def close(self):
        import torch

        torch.cuda.synchronize()
        self.ctx.close()


def case(kind, name, w=T.W, h=T.H):
    """frame, the SS scene, the scene without the flag, disk, disk_args"""
    frame, scene, disk, disk_args = T.pose(name, w, h)
    one = T.plain_of(scene) if kind == "plain" else scene
    return frame, S.ss_scene(scene, kind), one, disk, disk_args


@pytest.mark.parametrize("name", ["A", "B", "flat"])
@pytest.mark.parametrize("kind", S.KINDS)
def test_kernel_equals_cpu_path(dev, cpu, kind, name):
    frame, sc, _, disk, disk_args = case(kind, name)
    rc, want, wtotal = S.ss_render(cpu, kind, frame, sc, T.W, T.H, disk)
    assert rc == GEO_OK
    gpu = Gpu(dev, kind, disk_args)
    got, total = gpu.rows(frame, sc, T.W, T.H)
    gpu.close()
    diff = (got != want).any(axis=-1)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the CPU path"
    assert total == wtotal


@pytest.mark.parametrize("kind", S.KINDS)
def test_kernel_equals_its_definition(dev, kind):
    """Independent of the CPU library: the numpy resolve of the GPU's own
    one-sample render at 192 x 108 with the same uniform."""
    frame, sc, one, _, disk_args = case(kind, "A")
    gpu = Gpu(dev, kind, disk_args)
    got, total = gpu.rows(frame, sc, T.W, T.H)
    samples, stotal = gpu.rows(frame, one, 2 * T.W, 2 * T.H)
    gpu.close()
    assert np.array_equal(got, S.resolve(samples))
    assert total == stotal
    assert not np.array_equal(got, samples[0::2, 0::2])  # and not one of its samples alone


@pytest.mark.parametrize("size", S.SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", S.KINDS)
def test_partial_tiles(dev, cpu, kind, size):
    w, h = size
    frame, sc, _, disk, disk_args = case(kind, "A", w, h)
    rc, want, wtotal = S.ss_render(cpu, kind, frame, sc, w, h, disk)
    assert rc == GEO_OK
    gpu = Gpu(dev, kind, disk_args)
    got, total = gpu.rows(frame, sc, w, h)
    if w == 100:  # rows 5..24
        part, _ = gpu.rows(frame, sc, w, h, row0=5, nrows=20)
        assert np.array_equal(part, got[5:25])
    gpu.close()
    assert np.array_equal(got, want) and total == wtotal


@pytest.mark.parametrize("kind", S.KINDS)
def test_bands(dev, kind):
    """The 8-row bands 0, 2, 4, 6 of the 96 x 54 frame (geo_render_bands; band 6
    clipped to rows 48..53) and a band set; clipped rows keep their prefill."""
    frame, sc, _, _, disk_args = case(kind, "A")
    gpu = Gpu(dev, kind, disk_args)
    whole, _ = gpu.rows(frame, sc, T.W, T.H)
    nb, br = 4, 8
    rgba, total = gpu.out(nb * br, T.W)
    gpu.ctx.render_bands(frame, sc, T.W, T.H, br, 0, 2, nb, rgba, steps_total=total)
    got, _ = gpu.host(rgba, total, nb * br, T.W)
    for i in range(nb):
        r0 = 2 * i * br
        n = min(br, T.H - r0)
        assert np.array_equal(got[i * br:i * br + n], whole[r0:r0 + n]), i
    assert (got[3 * br + (T.H - 48):] == PREFILL).all()
    # geo_render_band_set: 8-row bands at rows 8, 24, 40 (band_rows 8, a stride of 16)
    rgba, total = gpu.out(3 * br, T.W)
    gpu.ctx.render_band_set(frame, sc, T.W, T.H, br, 8, 16, 3, rgba, steps_total=total)
    got, _ = gpu.host(rgba, total, 3 * br, T.W)
    gpu.close()
    for i in range(3):
        assert np.array_equal(got[i * br:(i + 1) * br], whole[8 + 16 * i:16 + 16 * i]), i


def test_dispatch_order(dev):
    frame, sc, one, _, disk_args = case("disk", "B")
    gpu = Gpu(dev, "disk", disk_args)
    gpu.ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    ref, rtotal = gpu.rows(frame, sc, T.W, T.H)
    plain_ref, _ = gpu.rows(frame, one, T.W, T.H)
    gpu.ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    rec0, _ = gpu.ctx.dispatch_stats()
    for i in range(3):
        got, total = gpu.rows(frame, sc, T.W, T.H)
        assert np.array_equal(got, ref) and total == rtotal, i
        if i == 1:  # the one-sample render of the same width x height in between learns an order of its own
            plain, _ = gpu.rows(frame, one, T.W, T.H)
            assert np.array_equal(plain, plain_ref)
    rec, _ = gpu.ctx.dispatch_stats()
    assert rec - rec0 >= 1
    # an explicit order for the sample frame's grid, ceil(192 / 32) x ceil(108 / 8), reversed
    tx, ty = (2 * T.W + 31) // 32, (2 * T.H + 7) // 8
    order = np.array([(y << 16) | x for y in range(ty) for x in range(tx)], np.uint32)[::-1]
    gpu.ctx.set_tile_order(tx, ty, order)
    got, total = gpu.rows(frame, sc, T.W, T.H)
    gpu.close()
    assert np.array_equal(got, ref) and total == rtotal


def _raw_rows(gpu, frame, scene, rgba, w=T.W, h=T.H, mask=None, uv=None, steps=None):
    return lib.geo_render_rows(gpu.ctx._h, ctypes.byref(frame), ctypes.byref(scene), w, h, 0, h, rgba.data_ptr(),
                               mask, uv, steps, None, None)


def test_refusals(dev):
    import torch

    frame, sc, one, _, disk_args = case("disk", "A")
    psc = S.ss_scene(one, "plain")
    # GEO_ESTATE without a sky, and with the disk flag without a disk
    bare = Gpu(dev, sky=False)
    rgba, _ = bare.out(T.H, T.W)
    assert _raw_rows(bare, frame, psc, rgba) == GEO_ESTATE
    bare.ctx.set_sky(T.SKY)
    assert _raw_rows(bare, frame, sc, rgba) == GEO_ESTATE
    torch.cuda.synchronize()
    assert (rgba.cpu().numpy() == PREFILL).all()
    assert _raw_rows(bare, frame, psc, rgba) == GEO_OK
    bare.close()

    gpu = Gpu(dev, "shift", disk_args)
    gpu.ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    rgba, _ = gpu.out(T.H, T.W)
    h = gpu.ctx._h
    for base, scene in ((0, psc), (GEO_FLAG_DISK, sc)):
        fl = base | GEO_FLAG_SS4
        bad = [S.with_flags(scene, fl, GEO_MODE_FAN), S.with_flags(scene, fl, GEO_MODE_ADAPTIVE)]
        bad += [S.with_flags(scene, fl | f) for f in (GEO_FLAG_MIPS, GEO_FLAG_COMPOSITE, GEO_FLAG_RING_F64)]
        for b in bad:
            assert _raw_rows(gpu, frame, b, rgba) == GEO_EINVAL, (b.mode, b.flags)
        assert _raw_rows(gpu, frame, S.with_flags(scene, fl | GEO_FLAG_DEFER_STEPS), rgba) == GEO_OK
        # colour only
        n = T.H * T.W
        mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        uv = torch.zeros(2 * n, dtype=torch.float32, device=dev)
        steps = torch.zeros(n, dtype=torch.int32, device=dev)
        rgba.fill_(PREFILL)
        assert _raw_rows(gpu, frame, scene, rgba, mask=mask.data_ptr()) == GEO_EINVAL
        assert _raw_rows(gpu, frame, scene, rgba, uv=uv.data_ptr()) == GEO_EINVAL
        assert _raw_rows(gpu, frame, scene, rgba, steps=steps.data_ptr()) == GEO_EINVAL
        # the batched entry points
        f, s_, out = ctypes.byref(frame), ctypes.byref(scene), rgba.data_ptr()
        assert lib.geo_render_band_set_frames(h, f, 1, s_, T.W, T.H, 8, 0, 8, 6, out, T.W * 48 * 4, None,
                                              None) == GEO_EINVAL
        assert lib.geo_render_band_set_batch(h, f, s_, 1, T.W, T.H, 8, 0, 8, 6, out, T.W * 48 * 4, None,
                                             None) == GEO_EINVAL
        assert lib.geo_render_disk_batch(h, f, s_, 1, T.W, T.H, 8, 0, 8, 6, out, T.W * 48 * 4, None, None) == GEO_EINVAL
        # twice the size must be a size the entry points take
        assert lib.geo_render_rows(h, f, s_, (1 << 19) + 1, T.H, 0, 1, out, None, None, None, None, None) == GEO_EINVAL
        assert lib.geo_render_rows(h, f, s_, T.W, (1 << 19) + 1, 0, 1, out, None, None, None, None, None) == GEO_EINVAL
        torch.cuda.synchronize()
        assert (rgba.cpu().numpy() == PREFILL).all(), "a refused call wrote its output"
        assert mask.sum().item() == 0 and steps.sum().item() == 0 and uv.abs().sum().item() == 0
    # armed hit and g buffers refuse the call and are consumed: the next one-sample disk render writes neither
    hits = torch.full((T.H * T.W * 6,), -1.0, dtype=torch.float32, device=dev)
    gb = torch.full((T.H * T.W * 3,), -1.0, dtype=torch.float32, device=dev)
    one_disk = S.with_flags(sc, GEO_FLAG_DISK)
    for arm in ("hits", "g"):
        if arm == "hits":
            gpu.ctx.disk_hits_next_render(hits)
        else:
            gpu.ctx.disk_shift_next_render(gb)
        rgba.fill_(PREFILL)
        assert _raw_rows(gpu, frame, sc, rgba) == GEO_EINVAL, arm
        torch.cuda.synchronize()
        assert (rgba.cpu().numpy() == PREFILL).all()
        assert _raw_rows(gpu, frame, one_disk, rgba) == GEO_OK
        torch.cuda.synchronize()
        assert (hits.cpu().numpy() == -1.0).all() and (gb.cpu().numpy() == -1.0).all(), arm
    assert _raw_rows(gpu, frame, sc, rgba) == GEO_OK  # nothing armed: accepted
    gpu.close()


def test_time_next_render(dev):
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    frame, sc, _, _, disk_args = case("plain", "A")
    gpu = Gpu(dev)
    ref, _ = gpu.rows(frame, sc, T.W, T.H)
    a, b = HipEvent(), HipEvent()
    gpu.ctx.time_next_render(a, b)
    got, _ = gpu.rows(frame, sc, T.W, T.H)
    ms = a.elapsed_time(b)
    gpu.close()
    assert np.array_equal(got, ref) and 0.0 < ms < 50.0
