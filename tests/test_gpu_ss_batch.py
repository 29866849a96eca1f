"""geo_render_ss_batch: up to GEO_MAX_BATCH_FRAMES GEO_FLAG_SS4 frames in one
launch (geo_render_ss_sky_kernel<KIND, kMaxBatchFrames> and, for disk scenes,
geo_render_disk_batch_kernel<KIND, SHADE, true, GEO_MODE_DIRECT>; the frame in blockIdx.z) draw,
frame by frame, the bytes geo_render_band_set draws for that frame and its SS
scene alone (the plain, the disk and the shifted disk frame), the flag's own
definition (the numpy box resolve of the one-sample render at twice the size)
and the bytes of the CPU path; the C-ABI's rules (geo.h) and
dist.ShardedFrame's routing of supersampled batches.

Which of the nine instantiations runs where (KIND kCurvedOut / kCurvedIn /
kFlat; the plain frame, Shade::kDisk, Shade::kDiskShift): the orbit (rs 1, the
observer outside the horizon) launches the three of kCurvedOut in every test
parametrised by kind; test_flat_space_pan launches the three of kFlat (rs 0);
test_inside_the_horizon launches the plain frame of kCurvedIn.  GEO_FLAG_DISK
refuses an observer at or inside the horizon (r_obs > rs unless rs == 0), so
the two disk instantiations of kCurvedIn run through a step above 1/2:
tests/test_gpu_wave_block_matrix.py, which has a cell for every instantiation."""
import ctypes
import math

import numpy as np
import pytest

import test_disk_cpu as T
import test_gpu_batch as B
import test_ss_cpu as S
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4,
                                                   GEO_MAX_BATCH_FRAMES, GEO_MODE_ADAPTIVE, GEO_MODE_FAN, GEO_OK,
                                                   GeoFrame, GeoScene, lib)

pytestmark = pytest.mark.gpu

DISK = (1.6, 2.2, (0.3, -0.2, 1.0), (1.0, 0.0, 0.0))  # test_gpu_disk_batch's: the orbit is not edge-on to it
# w, h, band_rows, row0, row_stride
PEER = (160, 96, 8, 8, 24)     # a peer's interleaved 8-row bands (N = 3)
RAGGED = (100, 37, 8, 0, 8)    # partial tiles, the last band clipped to rows 32..36
ODD = (33, 19, 8, 0, 8)        # 66 samples a row: a 2-sample column of a third tile; the last band clipped to 3 rows
WHOLE = (T.W, T.H, 8, 0, 8)    # the whole 96 x 54 frame, the last band clipped
LAYS = {"peer": PEER, "ragged": RAGGED, "odd": ODD}
PREFILL = S.PREFILL
GUARD = 64  # bytes after every frame slot, which no launch may touch


def geo():
    import schwarzschild_raytracer_wgpu_amd as g

    return g


def one_sample(scene, kind):
    """The scene of `kind` without GEO_FLAG_SS4."""
    return S.with_flags(scene, 0 if kind == "plain" else GEO_FLAG_DISK)


def orbit(w, h, n, kind, extra=0):
    """test_gpu_batch's orbiting observer ((2.5, 0, 0.1), start_orbit(1.8), rs 1,
    sphere 50) with the SS scenes of `kind`."""
    frames, scenes = B._moving(geo(), w, h, n, "orbit")
    return frames, [S.ss_scene(s, kind, extra) for s in scenes]


def pan(name, w, h, n, kind):
    """n frames of pose `name` (rs 0) with the camera turning: one central_to_uv, one scene."""
    pos, cam, fov, rs, state, _, _, _, ms = T.POSES[name]
    frames = [default_frame(w, h, pos=pos, camera=(cam[0] + 0.06 * i, cam[1] - 0.04 * i), rs=rs, fov=fov, state=state)
              for i in range(n)]
    scene = S.ss_scene(make_scene(rs, 50.0, math.sqrt(sum(p * p for p in pos)), T.STEP, ms), kind)
    return frames, [scene] * n


def dims(lay):
    w, h, br, row0, stride = lay
    nb = (h - row0 + stride - 1) // stride
    return nb, nb * br, nb * br * w * 4


def in_frame_bytes(lay):
    """Per byte of a frame's packed bands: its row lies in the frame."""
    w, h, br, row0, stride = lay
    nb, nrows, _ = dims(lay)
    rows = np.array([row0 + (r // br) * stride + r % br < h for r in range(nrows)])
    return np.repeat(rows, w * 4)


def new_ctx(dev, kind, disk=DISK, sky=True):
    ctx = geo().Context(dev.index or 0)
    if sky:
        ctx.set_sky(T.SKY)
    if kind != "plain" and disk is not None:
        ctx.set_disk(T.TEX, *disk)
    if kind == "shift":
        ctx.set_disk_shift(*S.SHIFT)
    return ctx


def batch(ctx, dev, frames, scenes, lay, stride=None, total=True):
    """The batch through Context.render_ss_batch into prefilled slots of `stride`
    bytes (default: the packed bands and GUARD bytes): (bytes per slot, steps)."""
    import torch

    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    n = len(frames)
    stride = packed + GUARD if stride is None else stride
    out = torch.full((n * stride + GUARD,), PREFILL, dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev) if total else None
    ctx.render_ss_batch(frames, scenes, w, h, br, row0, rstride, nb, out, frame_stride=stride, steps_total=tot)
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a[n * stride:] == PREFILL).all(), "bytes after the last slot were written"
    a = a[:n * stride].reshape(n, stride)
    assert (a[:, packed:] == PREFILL).all(), "bytes between the frames' slots were written"
    return a[:, :packed], (int(tot.item()) if total else None)


def singles(ctx, dev, frames, scenes, lay):
    """Every frame alone through geo_render_band_set: (bytes per frame, steps per frame)."""
    import torch

    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    refs, tots = [], []
    for f, s in zip(frames, scenes):
        ref = torch.full((packed,), PREFILL, dtype=torch.uint8, device=dev)
        tot = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx.render_band_set(f, s, w, h, br, row0, rstride, nb, ref, steps_total=tot)
        refs.append(ref)
        tots.append(tot)
    torch.cuda.synchronize()
    return np.stack([r.cpu().numpy() for r in refs]), [int(t.item()) for t in tots]


def raw(ctx, frames, scenes, lay, out, stride=None, n=None, w=None, h=None):
    ww, hh, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    fa = None if frames is None else (GeoFrame * len(frames))(*frames)
    sa = None if scenes is None else (GeoScene * len(scenes))(*scenes)
    return lib.geo_render_ss_batch(ctx._h, fa, sa, len(frames) if n is None else n, ww if w is None else w,
                                   hh if h is None else h, br, row0, rstride, nb,
                                   None if out is None else out.data_ptr(), packed if stride is None else stride,
                                   None, None)


_REF = {}


def orbit_ref(dev, kind, lay_name):
    """The 8-frame orbit on a layout, every frame rendered alone once (never
    modified): frames, SS scenes, their bytes and steps, and the bytes of the
    same frames without GEO_FLAG_SS4."""
    key = (kind, lay_name)
    if key not in _REF:
        lay = LAYS.get(lay_name, WHOLE)
        frames, scenes = orbit(lay[0], lay[1], GEO_MAX_BATCH_FRAMES, kind)
        ctx = new_ctx(dev, kind)
        ref, tots = singles(ctx, dev, frames, scenes, lay)
        plain, _ = singles(ctx, dev, frames, [one_sample(s, kind) for s in scenes], lay)
        ctx.close()
        ref.setflags(write=False)
        plain.setflags(write=False)
        _REF[key] = (frames, scenes, ref, tuple(tots), plain)
    return _REF[key]


@pytest.fixture(scope="module")
def cpu():
    return S.X.load_cpu()


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("lay_name", ["peer", "ragged", "odd"])
@pytest.mark.parametrize("kind", S.KINDS)
def test_batch_equals_single_frames(dev, kind, lay_name, n):
    lay = LAYS[lay_name]
    frames, scenes, ref, tots, plain = orbit_ref(dev, kind, lay_name)
    frames, scenes = frames[:n], scenes[:n]
    assert len({s.r_obs for s in scenes}) == n  # every frame its own radius
    ctx = new_ctx(dev, kind)
    got, tot = batch(ctx, dev, frames, scenes, lay)
    ctx.close()
    inside = in_frame_bytes(lay)
    for f in range(n):
        print(f"{kind} {lay_name} n={n} frame {f}: differing bytes {int((got[f] != ref[f]).sum())}")
        assert np.array_equal(got[f], ref[f]), f
        assert (got[f][~inside] == PREFILL).all(), f  # rows past the frame are not written
        assert not (got[f][inside] == PREFILL).all(), f
        assert not np.array_equal(ref[f], plain[f]), f  # not the one-sample frame
        if f:
            assert not np.array_equal(ref[f], ref[f - 1]), f
    assert tot == sum(tots[:n]) > 0


@pytest.mark.parametrize("kind", S.KINDS)
def test_batch_equals_the_definition(dev, kind):
    """Independent of the SS kernels: the numpy resolve of the one-sample
    geo_render_rows at 192 x 108 with the same uniform and the scene without the
    flag.  The slots are packed back to back here (frame_stride's default)."""
    import torch

    w, h = WHOLE[:2]
    n = GEO_MAX_BATCH_FRAMES
    nb, _, packed = dims(WHOLE)
    frames, scenes = orbit(w, h, n, kind)
    ctx = new_ctx(dev, kind)
    out = torch.full((n * packed + GUARD,), PREFILL, dtype=torch.uint8, device=dev)
    ctx.render_ss_batch(frames, scenes, w, h, WHOLE[2], WHOLE[3], WHOLE[4], nb, out)
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a[n * packed:] == PREFILL).all()
    got = a[:n * packed].reshape(n, packed)
    for f in (0, n - 1):
        smp = torch.full((2 * h * 2 * w * 4,), PREFILL, dtype=torch.uint8, device=dev)
        ctx.render_rows(frames[f], one_sample(scenes[f], kind), 2 * w, 2 * h, 0, 2 * h, smp)
        torch.cuda.synchronize()
        samples = smp.cpu().numpy().reshape(2 * h, 2 * w, 4)
        mine = got[f][:h * w * 4].reshape(h, w, 4)
        assert np.array_equal(mine, S.resolve(samples)), f
        assert not np.array_equal(mine, samples[0::2, 0::2]), f  # and not one of its samples alone
        assert (got[f][h * w * 4:] == PREFILL).all(), f  # the clipped rows of the last band
    ctx.close()


@pytest.mark.parametrize("kind", S.KINDS)
def test_against_the_cpu_path(dev, cpu, kind):
    w, h = WHOLE[:2]
    n = GEO_MAX_BATCH_FRAMES
    frames, scenes = orbit(w, h, n, kind)
    ctx = new_ctx(dev, kind)
    got, _ = batch(ctx, dev, frames, scenes, WHOLE)
    # the two frames as a batch of their own: its total is the CPU path's two
    _, tot2 = batch(ctx, dev, [frames[0], frames[n - 1]], [scenes[0], scenes[n - 1]], WHOLE)
    ctx.close()
    want_tot = 0
    for f in (0, n - 1):
        rc, c, ctot = S.ss_render(cpu, kind, frames[f], scenes[f], w, h, T.make_disk(*DISK))
        assert rc == GEO_OK and ctot > 0
        diff = (got[f][:h * w * 4].reshape(h, w, 4) != c).any(axis=-1)
        assert not diff.any(), f"frame {f}: {int(diff.sum())} pixels differ from the CPU path"
        want_tot += ctot
    assert tot2 == want_tot


@pytest.mark.parametrize("name", ["flat", "tilted"])
@pytest.mark.parametrize("kind", S.KINDS)
def test_flat_space_pan(dev, kind, name):
    """KIND kFlat: <2, 0>, <2, 1>, <2, 2>."""
    frames, scenes = pan(name, T.W, T.H, 3, kind)
    ctx = new_ctx(dev, kind, disk=T.pose(name)[3])
    got, tot = batch(ctx, dev, frames, scenes[0], WHOLE)  # one GeoScene for every frame
    ref, tots = singles(ctx, dev, frames, scenes, WHOLE)
    plain, _ = singles(ctx, dev, frames, [one_sample(s, kind) for s in scenes], WHOLE)
    ctx.close()
    assert np.array_equal(got, ref) and tot == sum(tots) > 0
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2])
    assert not np.array_equal(ref, plain)


def test_inside_the_horizon(dev, cpu):
    """KIND kCurvedIn, <1, 0>: the plain frame of observers inside the horizon,
    each at its own radius (the one-frame rules allow it for the plain frame
    only; test_gpu_batch's 'fall' stays outside over eight frames, so the
    observers are placed)."""
    w, h = RAGGED[:2]
    pos = [(0.8 - 0.05 * i, 0.0, 0.05) for i in range(4)]
    frames = [default_frame(w, h, pos=p, camera=(math.pi + 0.1 * i, 0.05 * i)) for i, p in enumerate(pos)]
    scenes = [S.ss_scene(make_scene(1.0, 50.0, math.hypot(p[0], p[2]), T.STEP, 1024), "plain") for p in pos]
    assert all(s.r_obs < s.rs for s in scenes) and len({s.r_obs for s in scenes}) == 4
    ctx = new_ctx(dev, "plain")
    got, tot = batch(ctx, dev, frames, scenes, RAGGED)
    ref, tots = singles(ctx, dev, frames, scenes, RAGGED)
    ctx.close()
    assert np.array_equal(got, ref) and tot == sum(tots) > 0
    assert not np.array_equal(ref[0], ref[1])
    rc, c, ctot = S.ss_render(cpu, "plain", frames[3], scenes[3], w, h)
    assert rc == GEO_OK and ctot == tots[3]
    assert np.array_equal(got[3][:h * w * 4].reshape(h, w, 4), c)


@pytest.mark.parametrize("kind", S.KINDS)
def test_frame_stride_and_padding(dev, kind):
    import torch

    frames, scenes, ref, tots, _ = orbit_ref(dev, kind, "ragged")
    frames, scenes = frames[:3], scenes[:3]
    w, h = RAGGED[:2]
    _, nrows, packed = dims(RAGGED)
    stride = packed + 4 * 37
    ctx = new_ctx(dev, kind)
    got, tot = batch(ctx, dev, frames, scenes, RAGGED, stride=stride)  # (asserts that the gaps keep the prefill)
    assert np.array_equal(got, ref[:3]) and tot == sum(tots[:3])
    assert nrows > h and (got[:, h * w * 4:] == PREFILL).all()  # rows past the frame are not written
    out = torch.full((3 * stride,), PREFILL, dtype=torch.uint8, device=dev)
    for bad in (packed - 4, packed + 2):
        assert raw(ctx, frames, scenes, RAGGED, out, stride=bad) == GEO_EINVAL, bad
        torch.cuda.synchronize()
        assert bool((out == PREFILL).all()), bad
    ctx.close()


@pytest.mark.parametrize("kind", S.KINDS)
def test_deferred_steps(dev, kind):
    import torch

    frames, scenes, ref, tots, _ = orbit_ref(dev, kind, "peer")
    ctx = new_ctx(dev, kind)
    got, none = batch(ctx, dev, frames, [S.ss_scene(s, kind, GEO_FLAG_DEFER_STEPS) for s in scenes], PEER, total=False)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.steps_flush(tot)
    torch.cuda.synchronize()
    ctx.close()
    assert none is None and np.array_equal(got, ref)
    assert int(tot.item()) == sum(tots)


@pytest.mark.parametrize("kind", S.KINDS)
def test_dispatch_order(dev, kind):
    frames, scenes, ref, tots, _ = orbit_ref(dev, kind, "peer")
    ctx = new_ctx(dev, kind)
    ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    got, tot = batch(ctx, dev, frames, scenes, PEER)
    assert np.array_equal(got, ref) and tot == sum(tots)
    ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        got, tot = batch(ctx, dev, frames, scenes, PEER)
        assert np.array_equal(got, ref) and tot == sum(tots), i
    rec, _ = ctx.dispatch_stats()
    assert rec >= 1
    # an explicit order for the sample frame's grid, ceil(2 w / 32) x ceil(2 nrows / 8), reversed
    _, nrows, _ = dims(PEER)
    tx, ty = (2 * PEER[0] + 31) // 32, (2 * nrows + 7) // 8
    order = np.array([(y << 16) | x for y in range(ty) for x in range(tx)], np.uint32)[::-1]
    ctx.set_tile_order(tx, ty, np.ascontiguousarray(order))
    got, tot = batch(ctx, dev, frames, scenes, PEER)
    ctx.close()
    assert np.array_equal(got, ref) and tot == sum(tots)


def test_time_next_render(dev):
    import torch

    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    frames, scenes, ref, _, _ = orbit_ref(dev, "disk", "peer")
    ctx = new_ctx(dev, "disk")
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
    FL = GEO_FLAG_SS4 | GEO_FLAG_DISK
    frames, scenes = orbit(w, h, n, "disk")
    ok = scenes[0]
    out = torch.full((GEO_MAX_BATCH_FRAMES * packed + 64,), PREFILL, dtype=torch.uint8, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == PREFILL).all())

    def sc(i=0, mode=0, flags=FL, **kw):
        s = scenes[i]
        f = dict(rs=s.rs, sphere_r=s.sphere_r, r_obs=s.r_obs, step=s.step, max_steps=s.max_steps)
        f.update(kw)
        return make_scene(f["rs"], f["sphere_r"], f["r_obs"], f["step"], f["max_steps"], mode, flags)

    def with_scene(i, s):
        return [s if j == i else scenes[j] for j in range(n)]

    # GEO_ESTATE without a sky, and with the disk flag without a disk
    bare = new_ctx(dev, "plain", sky=False)
    plain = [sc(j, flags=GEO_FLAG_SS4) for j in range(n)]
    assert raw(bare, frames, plain, lay, out) == GEO_ESTATE and untouched()
    bare.set_sky(T.SKY)
    assert raw(bare, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    assert raw(bare, frames, plain, lay, out) == GEO_OK
    torch.cuda.synchronize()
    assert not bool((out[:n * packed] == PREFILL).all())
    out.fill_(PREFILL)
    bare.close()

    ctx = new_ctx(dev, "disk")
    ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    cases = {
        "no SS4 flag, disk": [sc(j, flags=GEO_FLAG_DISK) for j in range(n)],
        "no SS4 flag, plain": [sc(j, flags=0) for j in range(n)],
        "one scene without the flag": with_scene(2, sc(2, flags=GEO_FLAG_DISK)),
        "the first scene without the flag": with_scene(0, sc(0, flags=GEO_FLAG_DISK)),
        "step differs": with_scene(1, sc(1, step=ok.step * 0.5)),
        "max_steps differs": with_scene(1, sc(1, max_steps=ok.max_steps - 1)),
        "rs differs": with_scene(1, sc(1, rs=0.9)),
        "a later frame inside the horizon": with_scene(3, sc(3, r_obs=0.9)),
        "a later frame on the horizon": with_scene(3, sc(3, r_obs=1.0)),
        "a later frame outside the sphere": with_scene(3, sc(3, r_obs=50.0)),
    }
    for base in (GEO_FLAG_SS4, FL):
        cases.update({
            f"adaptive {base}": [sc(j, mode=GEO_MODE_ADAPTIVE, flags=base) for j in range(n)],
            f"fan {base}": [sc(j, mode=GEO_MODE_FAN, flags=base) for j in range(n)],
            f"mips {base}": [sc(j, flags=base | GEO_FLAG_MIPS) for j in range(n)],
            f"composite {base}": [sc(j, flags=base | GEO_FLAG_COMPOSITE) for j in range(n)],
            f"ring {base}": [sc(j, flags=base | GEO_FLAG_RING_F64) for j in range(n)],
        })
    for name, bad in cases.items():
        assert raw(ctx, frames, bad, lay, out) == GEO_EINVAL, name
        assert untouched(), name
    assert raw(ctx, frames, scenes, lay, out, n=0) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, n=GEO_MAX_BATCH_FRAMES + 1) == GEO_EINVAL and untouched()
    assert raw(ctx, None, scenes, lay, out, n=n) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, None, lay, out) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, None) == GEO_EINVAL and untouched()
    # twice the size must be a size the entry points take (one frame: no stride rule comes first)
    assert raw(ctx, frames[:1], scenes[:1], lay, out, w=(1 << 19) + 1) == GEO_EINVAL and untouched()
    assert raw(ctx, frames[:1], scenes[:1], lay, out, h=(1 << 19) + 1) == GEO_EINVAL and untouched()
    # the three older batched calls keep refusing the flag
    fa, sa = (GeoFrame * n)(*frames), (GeoScene * n)(*scenes)
    for fn in (lib.geo_render_band_set_batch, lib.geo_render_disk_batch):
        assert fn(ctx._h, fa, sa, n, w, h, lay[2], lay[3], lay[4], nb, out.data_ptr(), packed, None,
                  None) == GEO_EINVAL and untouched()
    assert lib.geo_render_band_set_frames(ctx._h, fa, n, ctypes.byref(ok), w, h, lay[2], lay[3], lay[4], nb,
                                          out.data_ptr(), packed, None, None) == GEO_EINVAL and untouched()
    # an armed per-pixel buffer: consumed by the refused call; the next one-frame render must not write it
    one = torch.full((packed,), PREFILL, dtype=torch.uint8, device=dev)
    one_disk = one_sample(scenes[0], "disk")
    hb = torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=dev)
    ctx.disk_hits_next_render(hb)
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    ctx.render_band_set(frames[0], one_disk, w, h, lay[2], lay[3], lay[4], nb, one)
    torch.cuda.synchronize()
    assert bool((hb == -1.0).all()) and not bool((one == PREFILL).all())
    gb = torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=dev)
    ctx.set_disk_shift(*S.SHIFT)
    ctx.disk_shift_next_render(gb)
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    ctx.render_band_set(frames[0], one_disk, w, h, lay[2], lay[3], lay[4], nb, one)
    torch.cuda.synchronize()
    assert bool((gb == -1.0).all()) and bool((hb == -1.0).all())
    # the shading needs circular orbits down to the inner edge
    ctx.set_disk(T.TEX, 1.4, 2.2, DISK[2], DISK[3])
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    ctx.clear_disk_shift()
    assert raw(ctx, frames, scenes, lay, out) == GEO_OK  # unshaded, that disk is drawn
    torch.cuda.synchronize()
    assert not bool((out[:n * packed] == PREFILL).all()) and bool((out[n * packed:] == PREFILL).all())
    out.fill_(PREFILL)
    ctx.clear_disk()
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    ctx.close()


def test_seeded_family(dev):
    import torch

    rng = np.random.default_rng(20261020)
    sizes = [(64, 40), (100, 37), (33, 19)]
    disks = [(1.6, 2.2), (3.0, 9.0)]
    normals = [(0.0, 0.0, 1.0), (0.3, -0.2, 1.0)]
    ctx = new_ctx(dev, "disk", disk=None)
    ran, drawn, differing = 0, 0, 0
    while ran < 12:
        drawn += 1
        assert drawn < 200
        n = int(rng.integers(1, GEO_MAX_BATCH_FRAMES + 1))
        w, h = sizes[int(rng.integers(3))]
        lay = (w, h, 8, 0, 8) if rng.integers(2) else (w, h, 8, 8, 24)
        kind = S.KINDS[int(rng.integers(3))]
        frames, scenes = orbit(w, h, n, kind) if rng.integers(2) else pan("flat", w, h, n, kind)
        r_in, r_out = disks[int(rng.integers(2))]
        ctx.set_disk(T.TEX, r_in, r_out, normals[int(rng.integers(2))], (1.0, 0.0, 0.0))
        if kind == "shift":
            ctx.set_disk_shift(*S.SHIFT)
        else:
            ctx.clear_disk_shift()
        _, _, packed = dims(lay)
        probe = torch.full((n * packed,), PREFILL, dtype=torch.uint8, device=dev)
        rc = raw(ctx, frames, scenes, lay, probe)
        if rc == GEO_EINVAL:  # a draw the rules refuse: drawn again, not skipped
            continue
        assert rc == GEO_OK
        got, tot = batch(ctx, dev, frames, scenes, lay)
        ref, tots = singles(ctx, dev, frames, scenes, lay)
        d = int((got != ref).sum())
        print(f"batch {ran}: n={n} {w}x{h} row0={lay[3]} stride={lay[4]} rs={scenes[0].rs} {kind} "
              f"disk={r_in}..{r_out}: {d} bytes differ")
        differing += d
        assert tot == sum(tots) > 0
        ran += 1
    ctx.close()
    assert ran == 12 and differing == 0


@pytest.mark.parametrize("kind", ["plain", "shift"])
def test_pipeline(dev, kind):
    import torch

    from schwarzschild_raytracer_wgpu_amd.dist import ShardedFrame

    w, h, nsteps = 160, 96, 8
    frames, scenes = orbit(w, h, nsteps, kind)
    ctx = new_ctx(dev, kind)
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
