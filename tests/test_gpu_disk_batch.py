"""geo_render_disk_batch: up to GEO_MAX_BATCH_FRAMES thin-disk frames in one
launch (geo_render_disk_batch_kernel<KIND, Shade::kDisk | kDiskShift, false, GEO_MODE_DIRECT>,
the frame in blockIdx.z) draw, frame by
frame, the bytes geo_render_band_set draws for that frame and scene alone,
unshaded and shaded (geo_set_disk_shift), and the bytes of the CPU path
(geo_render_cpu_disk_shift, the same header csrc/geo_disk.h); the C-ABI's
rules (geo.h) and dist.ShardedFrame's routing of disk batches."""
import ctypes
import math

import numpy as np
import pytest

import test_disk_cpu as T
import test_disk_shift_cpu as X
import test_gpu_batch as B
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import _lib, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_MAX_BATCH_FRAMES,
                                                   GEO_MODE_ADAPTIVE, GEO_MODE_FAN, GEO_OK, GeoFrame, GeoScene, lib)

pytestmark = pytest.mark.gpu

DISK = (1.6, 2.2, (0.3, -0.2, 1.0), (1.0, 0.0, 0.0))  # the orbit below is not edge-on to it
# w, h, band_rows, row0, row_stride
PEER = (160, 96, 8, 8, 24)     # a peer's interleaved 8-row bands (N = 3)
RAGGED = (100, 37, 8, 0, 8)    # partial tiles, the last band clipped to rows 32..36
WHOLE = (T.W, T.H, 8, 0, 8)    # the whole 96 x 54 frame (row_stride == band_rows), the last band clipped
FILL = 7


def geo():
    import schwarzschild_raytracer_wgpu_amd as g

    return g


def with_flags(s, flags, mode=0):
    return make_scene(s.rs, s.sphere_r, s.r_obs, s.step, s.max_steps, mode, flags)


def orbit(w, h, n, flags=GEO_FLAG_DISK):
    """test_gpu_batch's orbiting observer ((2.5, 0, 0.1), start_orbit(1.8), rs 1,
    sphere 50, dt 0.05 per frame) with disk scenes."""
    frames, scenes = B._moving(geo(), w, h, n, "orbit")
    return frames, [with_flags(s, flags) for s in scenes]


def pan(name, w, h, n):
    """n frames of pose `name` (rs 0) with the camera turning: one central_to_uv, one scene."""
    pos, cam, fov, rs, state, _, _, _, ms = T.POSES[name]
    frames = [default_frame(w, h, pos=pos, camera=(cam[0] + 0.06 * i, cam[1] - 0.04 * i), rs=rs, fov=fov, state=state)
              for i in range(n)]
    scene = make_scene(rs, 50.0, math.sqrt(sum(p * p for p in pos)), T.STEP, ms, flags=GEO_FLAG_DISK)
    return frames, [scene] * n


def dims(lay):
    w, h, br, row0, stride = lay
    nb = (h - row0 + stride - 1) // stride
    return nb, nb * br, nb * br * w * 4


def new_ctx(dev, disk=DISK, shift=None):
    ctx = geo().Context(dev.index or 0)
    ctx.set_sky(T.SKY)
    if disk is not None:
        ctx.set_disk(T.TEX, *disk)
    if shift is not None:
        ctx.set_disk_shift(*shift)
    return ctx


def batch(ctx, dev, frames, scenes, lay, stride=None, total=True):
    """The batch through Context.render_disk_batch: (bytes per frame slot, steps)."""
    import torch

    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    n = len(frames)
    stride = packed if stride is None else stride
    out = torch.full((n * stride,), FILL, dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev) if total else None
    ctx.render_disk_batch(frames, scenes, w, h, br, row0, rstride, nb, out, frame_stride=stride, steps_total=tot)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, stride), (int(tot.item()) if total else None)


def singles(ctx, dev, frames, scenes, lay, hits=False):
    """Every frame alone through geo_render_band_set: (bytes per frame, steps, hits per frame)."""
    import torch

    w, h, br, row0, rstride = lay
    nb, nrows, packed = dims(lay)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    refs, hs = [], []
    for f, s in zip(frames, scenes):
        ref = torch.full((packed,), FILL, dtype=torch.uint8, device=dev)
        hb = torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=dev)
        if hits:
            ctx.disk_hits_next_render(hb)
        ctx.render_band_set(f, s, w, h, br, row0, rstride, nb, ref, steps_total=tot)
        refs.append(ref)
        hs.append(hb)
    torch.cuda.synchronize()
    return (np.stack([r.cpu().numpy() for r in refs]), int(tot.item()),
            [x.cpu().numpy().reshape(nrows, w, 3, 2) for x in hs])


def raw(ctx, frames, scenes, lay, out, stride=None, n=None):
    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    fa, sa = (GeoFrame * len(frames))(*frames), (GeoScene * len(scenes))(*scenes)
    return lib.geo_render_disk_batch(ctx._h, fa, sa, len(frames) if n is None else n, w, h, br, row0, rstride, nb,
                                     out.data_ptr(), packed if stride is None else stride, None, None)


@pytest.fixture(scope="module")
def cpu():
    return X.load_cpu()


@pytest.fixture(scope="module")
def peer8(dev):
    """The unshaded reference of the 8-frame orbit on the peer layout, rendered once."""
    frames, scenes = orbit(PEER[0], PEER[1], GEO_MAX_BATCH_FRAMES)
    ctx = new_ctx(dev)
    ref, tot, hits = singles(ctx, dev, frames, scenes, PEER, hits=True)
    ctx.close()
    ref.setflags(write=False)
    return frames, scenes, ref, tot, hits


@pytest.mark.parametrize("lay", [PEER, RAGGED], ids=["peer", "ragged"])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_batch_equals_single_frames(dev, lay, n):
    frames, scenes = orbit(lay[0], lay[1], n)
    assert len({s.r_obs for s in scenes}) == n  # every frame its own radius
    _, _, packed = dims(lay)
    ctx = new_ctx(dev)
    got, tot = batch(ctx, dev, frames, scenes, lay)
    ref, ref_tot, hits = singles(ctx, dev, frames, scenes, lay, hits=True)
    plain, _, _ = singles(ctx, dev, frames, [with_flags(s, 0) for s in scenes], lay)
    ctx.close()
    for f in range(n):
        s0, s1 = int((hits[f][..., 0, 0] > 0).sum()), int((hits[f][..., 1, 0] > 0).sum())
        print(f"n={n} frame {f}: slot-0 hits {s0}, slot-1 hits {s1}, differing bytes {int((got[f] != ref[f]).sum())}")
        assert s0 > 300 and s1 > 0, (f, s0, s1)
        assert np.array_equal(got[f], ref[f]), f
        assert not np.array_equal(ref[f], plain[f]), f
        if f:
            assert not np.array_equal(ref[f], ref[f - 1]), f
    assert tot == ref_tot > 0


@pytest.mark.parametrize("shift", [None, (1, 4, 1.0)], ids=["unshaded", "shaded"])
def test_against_the_cpu_path(dev, cpu, shift):
    w, h = WHOLE[:2]
    n = GEO_MAX_BATCH_FRAMES
    frames, scenes = orbit(w, h, n)
    ctx = new_ctx(dev, shift=shift)
    got, _ = batch(ctx, dev, frames, scenes, WHOLE)
    ctx.close()
    for f in (0, n - 1):
        rc, c = X.render(cpu, frames[f], scenes[f], w, h, T.make_disk(*DISK), shift=shift)
        assert rc == GEO_OK and (c["hits"][..., 0, 0] > 0).sum() > 300
        assert np.array_equal(got[f][:h * w * 4].reshape(h, w, 4), c["rgba"]), f
        assert (got[f][h * w * 4:] == FILL).all()  # the clipped rows of the last band


def test_shaded_batches(dev, peer8):
    frames, scenes, unshaded, _, _ = peer8
    outs = []
    for shift in ((1, 4, 1.0), (-1, 3, 2.0)):
        ctx = new_ctx(dev, shift=shift)
        got, tot = batch(ctx, dev, frames, scenes, PEER)
        ref, ref_tot, _ = singles(ctx, dev, frames, scenes, PEER)
        ctx.close()
        assert np.array_equal(got, ref) and tot == ref_tot, shift
        assert not np.array_equal(got, unshaded), shift
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1])
    # and the unshaded batch on a context whose shading was cleared again
    ctx = new_ctx(dev, shift=(1, 4, 1.0))
    ctx.clear_disk_shift()
    got, _ = batch(ctx, dev, frames, scenes, PEER)
    ctx.close()
    assert np.array_equal(got, unshaded)


@pytest.mark.parametrize("name", ["flat", "tilted"])
def test_flat_space_pan(dev, name):
    frames, scenes = pan(name, T.W, T.H, 3)
    disk = T.pose(name)[3]
    ctx = new_ctx(dev, disk=disk)
    got, tot = batch(ctx, dev, frames, scenes[0], WHOLE)  # one GeoScene for every frame
    ref, ref_tot, hits = singles(ctx, dev, frames, scenes, WHOLE, hits=True)
    ctx.close()
    assert (hits[0][..., 0, 0] > 0).sum() > 300
    assert np.array_equal(got, ref) and tot == ref_tot
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2])


def test_frame_stride_and_padding(dev):
    frames, scenes = orbit(RAGGED[0], RAGGED[1], 3)
    w, h = RAGGED[:2]
    _, nrows, packed = dims(RAGGED)
    stride = packed + 4 * 37
    ctx = new_ctx(dev)
    got, _ = batch(ctx, dev, frames, scenes, RAGGED, stride=stride)
    ref, _, _ = singles(ctx, dev, frames, scenes, RAGGED)
    ctx.close()
    assert np.array_equal(got[:, :packed], ref)
    assert (got[:, packed:] == FILL).all()  # the gap keeps its prefill
    assert nrows > h and (got[:, h * w * 4:packed] == FILL).all()  # rows past the frame are not written
    assert not (ref[:, :h * w * 4] == FILL).all()


def test_deferred_steps(dev, peer8):
    import torch

    frames, scenes, ref, ref_tot, _ = peer8
    ctx = new_ctx(dev)
    got, none = batch(ctx, dev, frames, [with_flags(s, GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS) for s in scenes], PEER,
                      total=False)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.steps_flush(tot)
    torch.cuda.synchronize()
    ctx.close()
    assert none is None and np.array_equal(got, ref)
    assert int(tot.item()) == ref_tot


def test_learned_dispatch_order(dev, peer8):
    frames, scenes, ref, ref_tot, _ = peer8
    ctx = new_ctx(dev)
    ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    got, tot = batch(ctx, dev, frames, scenes, PEER)
    assert np.array_equal(got, ref) and tot == ref_tot
    ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        got, tot = batch(ctx, dev, frames, scenes, PEER)
        assert np.array_equal(got, ref) and tot == ref_tot, i
    rec, _ = ctx.dispatch_stats()
    ctx.close()
    assert rec >= 1


def test_time_next_render(dev, peer8):
    import torch

    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    frames, scenes, ref, _, _ = peer8
    ctx = new_ctx(dev)
    e0, e1 = HipEvent(), HipEvent()
    ctx.time_next_render(e0, e1)
    got, _ = batch(ctx, dev, frames, scenes, PEER)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)  # raises unless both were recorded
    ctx.close()
    assert ms > 0.0 and np.array_equal(got, ref)


def test_refusals(dev):
    import torch

    lay = WHOLE
    w, h = lay[:2]
    nb, nrows, packed = dims(lay)
    n = 4
    frames, scenes = orbit(w, h, n)
    ok = scenes[0]
    out = torch.full((GEO_MAX_BATCH_FRAMES * packed + 64,), FILL, dtype=torch.uint8, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == FILL).all())

    def sc(i=0, mode=0, flags=GEO_FLAG_DISK, **kw):
        s = scenes[i]
        f = dict(rs=s.rs, sphere_r=s.sphere_r, r_obs=s.r_obs, step=s.step, max_steps=s.max_steps)
        f.update(kw)
        return make_scene(f["rs"], f["sphere_r"], f["r_obs"], f["step"], f["max_steps"], mode, flags)

    def with_scene(i, s):
        return [s if j == i else scenes[j] for j in range(n)]

    ctx = new_ctx(dev)
    ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    cases = {
        "adaptive": [sc(j, mode=GEO_MODE_ADAPTIVE) for j in range(n)],
        "fan": [sc(j, mode=GEO_MODE_FAN) for j in range(n)],
        "mips": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_MIPS) for j in range(n)],
        "composite": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_COMPOSITE) for j in range(n)],
        "ring": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_RING_F64) for j in range(n)],
        "no disk flag": [sc(j, flags=0) for j in range(n)],
        "one scene without the flag": with_scene(2, sc(2, flags=0)),
        "step differs": with_scene(1, sc(1, step=ok.step * 0.5)),
        "max_steps differs": with_scene(1, sc(1, max_steps=ok.max_steps - 1)),
        "rs differs": with_scene(1, sc(1, rs=0.9)),
        "a later frame inside the horizon": with_scene(3, sc(3, r_obs=0.9)),
        "a later frame on the horizon": with_scene(3, sc(3, r_obs=1.0)),
        "a later frame outside the sphere": with_scene(3, sc(3, r_obs=50.0)),
    }
    for name, bad in cases.items():
        assert raw(ctx, frames, bad, lay, out) == GEO_EINVAL, name
        assert untouched(), name
    assert raw(ctx, frames, scenes, lay, out, n=0) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, n=GEO_MAX_BATCH_FRAMES + 1) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, stride=packed - 4) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, stride=packed + 2) == GEO_EINVAL and untouched()
    # an armed per-pixel buffer: consumed by the refused call
    hb = torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=dev)
    ctx.disk_hits_next_render(hb)
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    one = torch.full((packed,), FILL, dtype=torch.uint8, device=dev)
    ctx.render_band_set(frames[0], scenes[0], w, h, lay[2], lay[3], lay[4], nb, one)
    torch.cuda.synchronize()
    assert bool((hb == -1.0).all()) and not bool((one == FILL).all())
    gb = torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=dev)
    ctx.set_disk_shift(1, 4, 1.0)
    ctx.disk_shift_next_render(gb)
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    # the shading needs circular orbits down to the inner edge
    ctx.set_disk(T.TEX, 1.4, 2.2, DISK[2], DISK[3])
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    ctx.clear_disk_shift()
    assert raw(ctx, frames, scenes, lay, out) == GEO_OK  # unshaded, that disk is drawn
    torch.cuda.synchronize()
    assert not bool((out[:n * packed] == FILL).all())
    out.fill_(FILL)
    ctx.clear_disk()
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    ctx.close()


def test_seeded_family(dev):
    import torch

    rng = np.random.default_rng(20261019)
    sizes = [(64, 40), (100, 37), (96, 54)]
    disks = [(1.6, 2.2), (3.0, 9.0)]
    normals = [(0.0, 0.0, 1.0), (0.3, -0.2, 1.0)]
    shifts = [None, (1, 4, 1.0), (-1, 3, 2.0)]
    ctx = new_ctx(dev, disk=None)
    ran, drawn, differing = 0, 0, 0
    while ran < 12:
        drawn += 1
        assert drawn < 200
        n = int(rng.integers(1, GEO_MAX_BATCH_FRAMES + 1))
        w, h = sizes[int(rng.integers(3))]
        lay = (w, h, 8, 0, 8) if rng.integers(2) else (w, h, 8, 8, 24)
        frames, scenes = orbit(w, h, n) if rng.integers(2) else pan("flat", w, h, n)
        shift = shifts[int(rng.integers(3))]
        r_in, r_out = disks[int(rng.integers(2))]
        ctx.set_disk(T.TEX, r_in, r_out, normals[int(rng.integers(2))], (1.0, 0.0, 0.0))
        if shift is None:
            ctx.clear_disk_shift()
        else:
            ctx.set_disk_shift(*shift)
        _, _, packed = dims(lay)
        probe = torch.full((n * packed,), FILL, dtype=torch.uint8, device=dev)
        rc = raw(ctx, frames, scenes, lay, probe)
        if rc == GEO_EINVAL:  # a draw the rules refuse: drawn again, not skipped
            continue
        assert rc == GEO_OK
        got, tot = batch(ctx, dev, frames, scenes, lay)
        ref, ref_tot, _ = singles(ctx, dev, frames, scenes, lay)
        d = int((got != ref).sum())
        print(f"batch {ran}: n={n} {w}x{h} row0={lay[3]} stride={lay[4]} rs={scenes[0].rs} shift={shift} "
              f"disk={r_in}..{r_out}: {d} bytes differ")
        differing += d
        assert tot == ref_tot
        ran += 1
    ctx.close()
    assert ran == 12 and differing == 0


@pytest.mark.parametrize("shift", [None, (1, 4, 1.0)], ids=["unshaded", "shaded"])
def test_pipeline(dev, shift):
    import torch

    from schwarzschild_raytracer_wgpu_amd.dist import ShardedFrame

    w, h, nsteps = 160, 96, 8
    frames, scenes = orbit(w, h, nsteps)
    ctx = new_ctx(dev, shift=shift)
    sf = ShardedFrame(ctx, frames[0], scenes[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=True)
    assert sf.batch and sf.K == 4
    refs = []
    for f, s in zip(frames, scenes):
        ref = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
        ctx.render_rows(f, s, w, h, 0, h, ref)
        refs.append(ref)
    retired = 0
    for i in range(nsteps):
        sf.step(i, frame=frames[i], scene=scenes[i])
        if i % sf.K == sf.K - 1:
            # the batch just launched, retired: its last frame, and every slot of its buffer
            sf.drain()
            torch.cuda.synchronize()
            assert torch.equal(sf.frame_rgba(), refs[i]), i
            for j in range(i - sf.K + 1, i + 1):
                assert torch.equal(sf.local_view(j)[:h * w * 4], refs[j]), j
                retired += 1
    sf.drain()
    torch.cuda.synchronize()
    ctx.close()
    assert retired == nsteps == sf.frames_done
    assert not torch.equal(refs[0], refs[1])
