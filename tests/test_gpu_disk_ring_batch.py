"""geo_render_disk_ring_batch: up to GEO_MAX_BATCH_FRAMES thin-disk frames with
the capture band's pixels in f64 (geo_set_disk_ring_f64) in one render launch
(geo_render_disk_ring_batch_kernel<KIND, SHADE, SS>, SS with
GEO_FLAG_SS4; the frame in blockIdx.z, its band constants from the context's
device table) draw, frame by frame, the bytes geo_render_band_set draws for
that frame and scene alone with the state on, and the bytes of the CPU path
(geo_render_cpu_disk_ring_f64 / _shift_ring_f64); a supersampled frame is the
box resolve of the one-sample ring render of twice the size; the C-ABI's rules
(geo.h) and dist.ShardedFrame's disk_ring_batch routing.

The batch that exercises the band is the ring walk: pose "ring" of
tests/test_disk_cpu.py (the camera on the photon ring's upper edge, fov 0.004)
with the observer stepping outwards, so every frame has its own r_obs and its
own band constants.  The tests count, per frame, the band's pixels with a disk
hit and the pixels whose colour the state changes: a batch that never reached
the f64 arm cannot pass.  test_gpu_disk_batch's orbit has few such pixels and
serves the layouts and the plumbing.

Which instantiation runs where (KIND kCurvedOut / kCurvedIn; SHADE plain / shift
/ emit; SS false / true):
  geo_render_disk_ring_batch_kernel<Out, plain|shift|emit, false>  test_batch_equals_single_frames, test_against_the_cpu_path
  geo_render_disk_ring_batch_kernel<In, plain|emit, false>         test_batch_equals_single_frames[curved_in-*]
  geo_render_disk_ring_batch_kernel<In, shift, false>              test_fuzzed_batches (seeds with a step outside kCurvedOut's)
  geo_render_disk_ring_batch_kernel<Out, plain|shift|emit, true>   test_ss4_is_the_resolve
  geo_render_disk_ring_batch_kernel<In, plain|shift|emit, true>    test_ss4_curved_in
test_fuzzed_batches prints the (kind, variant, SS4) triples its seeds draw."""
import math

import numpy as np
import pytest

import oracle as O
import test_disk_cpu as T
import test_disk_emission_cpu as X
import test_disk_ring_cpu as RC
import test_gpu_disk_batch as DB
from fuzz_disk_scenes import disk_batch, disk_scene, kind_of
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4,
                                                   GEO_MAX_BATCH_FRAMES, GEO_MODE_ADAPTIVE, GEO_MODE_FAN, GEO_OK,
                                                   GeoFrame, GeoScene, lib)
from test_gpu_disk_batch import FILL, PEER, RAGGED, WHOLE, dims, orbit, pan
from test_gpu_disk_emission import EM, set_emission, ss_of
from test_gpu_disk_fuzz import BATCH_SEEDS

pytestmark = pytest.mark.gpu

N = GEO_MAX_BATCH_FRAMES
SHIFT = (1, 4, 1.0)
VARIANTS = ("plain", "shift", "emission")
RING_DISK = T.POSES["ring"][5] + T.POSES["ring"][6:8]  # (3, 9), normal z, axis x
# the floors of the issue's table (measured on the CPU path: at least 64 and 22 on these layouts)
MIN_BAND_HITS, MIN_CHANGED = 50, 15


def walk(w, h, n, curved_in=False, dx=0.05, x0=14.0):
    """Pose "ring" with the observer at (x0 + dx i, 0, 5.1) in frame i, at
    rest, the camera kept on the photon ring's upper edge (its angular radius
    falls as 1 / r_obs).  curved_in: step 0.75 and 256 steps (kCurvedIn)."""
    _, _, fov, rs, state, _, _, _, ms = T.POSES["ring"]
    frames, scenes = [], []
    for i in range(n):
        x, z = x0 + dx * i, 5.1
        theta = -math.atan2(z, x) + 0.1695 * math.hypot(14.0, 5.1) / math.hypot(x, z)
        frames.append(default_frame(w, h, pos=(x, 0.0, z), camera=(math.pi, theta), rs=rs, fov=fov, state=state))
        if curved_in:
            scenes.append(make_scene(rs, 50.0, math.hypot(x, z), 0.75, 256, flags=GEO_FLAG_DISK))
        else:
            scenes.append(make_scene(rs, 50.0, math.hypot(x, z), math.pi / 100, ms, flags=GEO_FLAG_DISK))
    kind = 1 if curved_in else 0
    assert all(kind_of(s.rs, s.r_obs, s.step) == kind for s in scenes) and len({s.r_obs for s in scenes}) == n
    return frames, scenes


def state_of(variant):
    """(shift, em) for the CPU path's render."""
    return dict(shift=SHIFT if variant == "shift" else None, em=EM if variant == "emission" else None)


def new_ctx(dev, variant="plain", disk=RING_DISK, ring=True, em=EM, ramp=X.RAMP, shift=SHIFT):
    ctx = DB.new_ctx(dev, disk=disk, shift=shift if variant == "shift" else None)
    if variant == "emission":
        set_emission(ctx, em, ramp)
    ctx.set_disk_ring_f64(ring)
    return ctx


def ss_all(scenes, ss):
    return [ss_of(s) for s in scenes] if ss else list(scenes)


def batch(ctx, dev, frames, scenes, lay, stride=None, total=True):
    """The batch through Context.render_disk_ring_batch: (bytes per frame slot, steps)."""
    import torch

    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    n = len(frames)
    stride = packed if stride is None else stride
    out = torch.full((n * stride,), FILL, dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev) if total else None
    ctx.render_disk_ring_batch(frames, scenes, w, h, br, row0, rstride, nb, out, frame_stride=stride, steps_total=tot)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, stride), (int(tot.item()) if total else None)


def singles(ctx, dev, frames, scenes, lay, hits=False):
    """Every frame alone through geo_render_band_set: (bytes per frame, steps per frame, hits per frame)."""
    refs, tots, hs = [], [], []
    for f, s in zip(frames, scenes):
        ref, tot, hb = DB.singles(ctx, dev, [f], [s], lay, hits=hits)
        refs.append(ref[0])
        tots.append(tot)
        hs.append(hb[0])
    return np.stack(refs), tots, hs


def raw(ctx, frames, scenes, lay, out, stride=None, n=None, fn=None):
    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    fa, sa = (GeoFrame * len(frames))(*frames), (GeoScene * len(scenes))(*scenes)
    fn = lib.geo_render_disk_ring_batch if fn is None else fn
    return fn(ctx._h, fa, sa, len(frames) if n is None else n, w, h, br, row0, rstride, nb, out.data_ptr(),
              packed if stride is None else stride, None, None)


def in_band(frame, scene, w, h):
    """The band's pixels as the kernels decide them (on the f32 ray)."""
    return O.ring_band(frame, RC.ring_scene(scene), w, h) == 1


def resolve(rgba):
    """GEO_FLAG_SS4's box resolve of a (2h, 2w, 4) frame."""
    s = rgba.astype(np.uint32)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def packed_whole(rgba):
    """A whole (h, w, 4) frame as layout WHOLE packs it: the rows past the frame keep the prefill."""
    _, _, packed = dims(WHOLE)
    out = np.full(packed, FILL, np.uint8)
    out[:rgba.size] = rgba.reshape(-1)
    return out


@pytest.fixture(scope="module")
def cpu():
    return RC.load_cpu()


class Refs:
    """The one-frame renders of a walk, rendered once per (layout, variant,
    kind) and shared: with the state on (bytes, steps, hit buffers) and off."""

    def __init__(self, dev):
        self.dev, self.cache = dev, {}

    def get(self, lay, variant, curved_in=False):
        key = (lay, variant, curved_in)
        if key not in self.cache:
            frames, scenes = walk(lay[0], lay[1], N, curved_in)
            ctx = new_ctx(self.dev, variant)
            on, tots, hits = singles(ctx, self.dev, frames, scenes, lay, hits=True)
            ctx.set_disk_ring_f64(False)
            off, _, _ = singles(ctx, self.dev, frames, scenes, lay)
            ctx.close()
            on.setflags(write=False)
            off.setflags(write=False)
            self.cache[key] = (frames, scenes, on, tots, hits, off)
        return self.cache[key]


@pytest.fixture(scope="module")
def refs(dev):
    return Refs(dev)


def band_evidence(lay, frames, scenes, on, off, hits, what):
    """Every frame has band pixels with a disk hit, and the state changes its colours."""
    w, h = lay[:2]
    for f in range(len(frames)):
        band = in_band(frames[f], scenes[f], w, h)
        hit = (hits[f][:h, :, :, 0] > 0.0).any(axis=-1)
        changed = (on[f][:h * w * 4].reshape(h, w, 4) != off[f][:h * w * 4].reshape(h, w, 4)).any(axis=-1)
        nb, nc = int((band & hit).sum()), int(changed.sum())
        print(f"{what} frame {f}: r_obs {scenes[f].r_obs:.4f}, band pixels with a hit {nb}, colours changed by the state {nc}")
        assert nb >= MIN_BAND_HITS and nc >= MIN_CHANGED, (what, f, nb, nc)


CASES = [(lay, v, False) for lay in (WHOLE, RAGGED) for v in VARIANTS] + [(WHOLE, "plain", True),
                                                                         (WHOLE, "emission", True)]
CASE_IDS = [f"{'whole' if lay is WHOLE else 'ragged'}-{'curved_in-' if ci else ''}{v}" for lay, v, ci in CASES]


@pytest.mark.parametrize("lay,variant,curved_in", CASES, ids=CASE_IDS)
def test_batch_equals_single_frames(dev, refs, lay, variant, curved_in):
    frames, scenes, on, tots, hits, off = refs.get(lay, variant, curved_in)
    band_evidence(lay, frames, scenes, on, off, hits, f"{variant} {lay[0]}x{lay[1]}")
    ctx = new_ctx(dev, variant)
    for n in (1, 2, N):
        got, tot = batch(ctx, dev, frames[:n], scenes[:n], lay)
        for f in range(n):
            print(f"n={n} frame {f}: differing bytes {int((got[f] != on[f]).sum())}")
            assert np.array_equal(got[f], on[f]), (n, f)
            if f:
                assert not np.array_equal(on[f], on[f - 1]), f
        assert tot == sum(tots[:n]) > 0, (n, tot, tots[:n])
    ctx.close()


def test_orbit_on_the_peer_layout(dev):
    """A peer's interleaved bands (row_stride > band_rows, row0 > 0), every variant."""
    frames, scenes = orbit(PEER[0], PEER[1], N)
    for variant in VARIANTS:
        ctx = new_ctx(dev, variant, disk=DB.DISK)
        got, tot = batch(ctx, dev, frames, scenes, PEER)
        ref, tots, _ = singles(ctx, dev, frames, scenes, PEER)
        ctx.close()
        assert np.array_equal(got, ref) and tot == sum(tots) > 0, variant
        assert not np.array_equal(got[0], got[N - 1])


@pytest.mark.parametrize("variant", VARIANTS)
def test_against_the_cpu_path(dev, cpu, refs, variant):
    w, h = WHOLE[:2]
    frames, scenes, on, tots, _, _ = refs.get(WHOLE, variant)
    ctx = new_ctx(dev, variant)
    got, _ = batch(ctx, dev, frames, scenes, WHOLE)
    ctx.close()
    for f in (0, N - 1):
        rc, c = RC.render(cpu, frames[f], scenes[f], T.make_disk(*RING_DISK), 1, **state_of(variant))
        assert rc == GEO_OK
        assert np.array_equal(got[f][:h * w * 4].reshape(h, w, 4), c["rgba"]), f
        assert (got[f][h * w * 4:] == FILL).all()  # the clipped rows of the last band
        assert tots[f] == c["total"], f
    assert not np.array_equal(got[0], got[N - 1])


def ss_refs(dev, cpu, variant, curved_in=False, cpu_frames=range(N)):
    """Per walk frame: the resolve of the device's one-frame ring render at
    192 x 108 packed as WHOLE packs it, that render's steps, the CPU path's
    resolve, and the state-off supersampled batch frame."""
    import torch

    w, h = WHOLE[:2]
    frames, scenes = walk(w, h, N, curved_in)
    ctx = new_ctx(dev, variant)
    want, tots, hit_counts, cpu_want = [], [], [], {}
    for f in range(N):
        out = torch.zeros(4 * w * h * 4, dtype=torch.uint8, device=dev)
        tot = torch.zeros(1, dtype=torch.int64, device=dev)
        hb = torch.full((4 * w * h * 6,), -1.0, dtype=torch.float32, device=dev)
        ctx.disk_hits_next_render(hb)
        ctx.render_rows(frames[f], scenes[f], 2 * w, 2 * h, 0, 2 * h, out, steps_total=tot)
        torch.cuda.synchronize()
        one = out.cpu().numpy().reshape(2 * h, 2 * w, 4)
        want.append(packed_whole(resolve(one)))
        tots.append(int(tot.item()))
        hit = (hb.cpu().numpy().reshape(2 * h, 2 * w, 3, 2)[..., 0] > 0.0).any(axis=-1)
        hit_counts.append(int((in_band(frames[f], scenes[f], 2 * w, 2 * h) & hit).sum()))
        if f in cpu_frames:
            rc, c = RC.render(cpu, frames[f], scenes[f], T.make_disk(*RING_DISK), 1, w=2 * w, h=2 * h,
                              **state_of(variant))
            assert rc == GEO_OK
            assert np.array_equal(c["rgba"], one) and c["total"] == tots[f], f
            cpu_want[f] = packed_whole(resolve(c["rgba"]))
    # the same scenes supersampled with the state off: the older batches' frames
    ctx.set_disk_ring_f64(False)
    nb, _, packed = dims(WHOLE)
    off = torch.full((N * packed,), FILL, dtype=torch.uint8, device=dev)
    older = ctx.render_emission_batch if variant == "emission" else ctx.render_ss_batch
    older(frames, ss_all(scenes, True), w, h, WHOLE[2], WHOLE[3], WHOLE[4], nb, off)
    torch.cuda.synchronize()
    ctx.close()
    return frames, scenes, want, tots, hit_counts, cpu_want, off.cpu().numpy().reshape(N, packed)


@pytest.mark.parametrize("variant", VARIANTS)
def test_ss4_is_the_resolve(dev, cpu, variant):
    w, h = WHOLE[:2]
    frames, scenes, want, tots, hit_counts, cpu_want, off = ss_refs(dev, cpu, variant)
    ss = ss_all(scenes, True)
    ctx = new_ctx(dev, variant)
    for n in (1, N):
        got, tot = batch(ctx, dev, frames[:n], ss[:n], WHOLE)
        for f in range(n):
            changed = int((got[f].reshape(-1, 4) != off[f].reshape(-1, 4)).any(axis=-1).sum())
            print(f"ss4 {variant} n={n} frame {f}: band samples with a hit {hit_counts[f]}, output pixels changed "
                  f"by the state {changed}, differing bytes {int((got[f] != want[f]).sum())}")
            assert hit_counts[f] >= MIN_BAND_HITS and changed >= MIN_CHANGED, (f, hit_counts[f], changed)
            assert np.array_equal(got[f], want[f]), (n, f)
            assert np.array_equal(got[f], cpu_want[f]), (n, f)
        assert tot == sum(tots[:n]) > 0, (n, tot)
    ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_ss4_curved_in(dev, cpu, variant):
    frames, scenes, want, tots, hit_counts, cpu_want, off = ss_refs(dev, cpu, variant, curved_in=True,
                                                                    cpu_frames=(0, N - 1))
    ctx = new_ctx(dev, variant)
    got, tot = batch(ctx, dev, frames, ss_all(scenes, True), WHOLE)
    ctx.close()
    assert min(hit_counts) >= MIN_BAND_HITS
    assert np.array_equal(got, np.stack(want)) and tot == sum(tots)
    for f, c in cpu_want.items():
        assert np.array_equal(got[f], c), f
    assert all(not np.array_equal(got[f], off[f]) for f in range(N))


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_frame_stride_and_padding(dev, ss):
    frames, scenes = walk(RAGGED[0], RAGGED[1], 3)
    w, h = RAGGED[:2]
    _, nrows, packed = dims(RAGGED)
    stride = packed + 4 * 37
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev, "shift")
    got, _ = batch(ctx, dev, frames, sc, RAGGED, stride=stride)
    tight, _ = batch(ctx, dev, frames, sc, RAGGED)
    if not ss:
        ref, _, _ = singles(ctx, dev, frames, scenes, RAGGED)
        assert np.array_equal(tight, ref)
    ctx.close()
    assert np.array_equal(got[:, :packed], tight)
    assert (got[:, packed:] == FILL).all()  # the gap keeps its prefill
    assert nrows > h and (got[:, h * w * 4:packed] == FILL).all()  # rows past the frame are not written
    assert not (tight[:, :h * w * 4] == FILL).all()


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_deferred_steps_orders_and_timing(dev, ss):
    """GEO_FLAG_DEFER_STEPS, the row-major, learned (period 1) and explicit
    orders, and geo_time_next_render: the same frames and steps every way."""
    import torch

    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    lay = WHOLE
    frames, scenes = walk(lay[0], lay[1], N)
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev, "emission")
    ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    ref, ref_tot = batch(ctx, dev, frames, sc, lay)
    if not ss:
        one, tots, _ = singles(ctx, dev, frames, scenes, lay)
        assert np.array_equal(ref, one) and ref_tot == sum(tots)
    flags = GEO_FLAG_DISK | (GEO_FLAG_SS4 if ss else 0) | GEO_FLAG_DEFER_STEPS
    deferred = [make_scene(s.rs, s.sphere_r, s.r_obs, s.step, s.max_steps, 0, flags) for s in scenes]
    got, none = batch(ctx, dev, frames, deferred, lay, total=False)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.steps_flush(tot)
    torch.cuda.synchronize()
    assert none is None and np.array_equal(got, ref) and int(tot.item()) == ref_tot
    ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        got, tot = batch(ctx, dev, frames, sc, lay)
        assert np.array_equal(got, ref) and tot == ref_tot, i
    rec, _ = ctx.dispatch_stats()
    assert rec >= 1
    # an explicit order: the grid's tiles (the sample frame's under SS4) back to front
    f = 2 if ss else 1
    tx, ty = (f * lay[0] + 31) // 32, (f * dims(lay)[1] + 7) // 8
    order = np.array([(y << 16) | x for y in range(ty) for x in range(tx)][::-1], dtype=np.uint32)
    ctx.set_tile_order(tx, ty, order)
    got, tot = batch(ctx, dev, frames, sc, lay)
    assert np.array_equal(got, ref) and tot == ref_tot
    e0, e1 = HipEvent(), HipEvent()
    ctx.time_next_render(e0, e1)
    got, _ = batch(ctx, dev, frames, sc, lay)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)  # raises unless both were recorded
    ctx.close()
    assert ms > 0.0 and np.array_equal(got, ref)


def test_two_streams_in_flight(dev, refs):
    """Two batches of one context on two streams, issued back to back with no
    wait between them, each with its own walk: a table of band constants per
    render-stream slot, so neither reads the other's."""
    import torch

    lay = WHOLE
    fa, sa, on_a, tots_a, _, _ = refs.get(lay, "plain")
    fb, sb = walk(lay[0], lay[1], N, dx=-0.04, x0=13.9)
    ctx = new_ctx(dev, "plain")
    on_b, tots_b, _ = singles(ctx, dev, fb, sb, lay)
    assert not np.array_equal(on_a, on_b)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    nb, _, packed = dims(lay)
    # (the outputs filled before anything is issued: the streams do not order against the fills)
    outs = [[(torch.full((N * packed,), FILL, dtype=torch.uint8, device=dev),
              torch.zeros(1, dtype=torch.int64, device=dev)) for _ in range(2)] for _ in range(2)]
    torch.cuda.synchronize()
    for pair in outs:  # twice: each slot's table is written again behind its stream's earlier render
        for (o, t), fr, sc, st in zip(pair, (fa, fb), (sa, sb), (s1, s2)):
            ctx.render_disk_ring_batch(fr, sc, lay[0], lay[1], lay[2], lay[3], lay[4], nb, o, steps_total=t,
                                       stream=st)
    torch.cuda.synchronize()
    ctx.close()
    for (oa, ta), (ob, tb) in outs:
        assert np.array_equal(oa.cpu().numpy().reshape(N, packed), on_a) and int(ta.item()) == sum(tots_a)
        assert np.array_equal(ob.cpu().numpy().reshape(N, packed), on_b) and int(tb.item()) == sum(tots_b)


def test_rules(dev):
    import torch

    lay = WHOLE
    w, h = lay[:2]
    nb, nrows, packed = dims(lay)
    n = 4
    frames, scenes = walk(w, h, n)
    ok = scenes[0]
    out = torch.full((N * packed + 64,), 0x5A, dtype=torch.uint8, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 0x5A).all())

    def sc(i=0, mode=0, flags=GEO_FLAG_DISK, **kw):
        s = scenes[i]
        f = dict(rs=s.rs, sphere_r=s.sphere_r, r_obs=s.r_obs, step=s.step, max_steps=s.max_steps)
        f.update(kw)
        return make_scene(f["rs"], f["sphere_r"], f["r_obs"], f["step"], f["max_steps"], mode, flags)

    def with_scene(i, s):
        return [s if j == i else scenes[j] for j in range(n)]

    # the state off, then no disk
    ctx = new_ctx(dev, "plain", ring=False)
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    assert raw(ctx, frames, ss_all(scenes, True), lay, out) == GEO_ESTATE and untouched()
    ctx.set_disk_ring_f64(True)
    ctx.clear_disk()  # (drops the state with the disk)
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    ctx.close()

    ctx = new_ctx(dev, "emission")
    ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    ss = GEO_FLAG_DISK | GEO_FLAG_SS4
    cases = {
        "adaptive": [sc(j, mode=GEO_MODE_ADAPTIVE) for j in range(n)],
        "fan": [sc(j, mode=GEO_MODE_FAN) for j in range(n)],
        "mips": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_MIPS) for j in range(n)],
        "composite": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_COMPOSITE) for j in range(n)],
        "disk | ring_f64": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_RING_F64) for j in range(n)],
        "ss4 mips": [sc(j, flags=ss | GEO_FLAG_MIPS) for j in range(n)],
        "no disk flag": [sc(j, flags=0) for j in range(n)],
        "ss4 without the disk flag": [sc(j, flags=GEO_FLAG_SS4) for j in range(n)],
        "one scene without the flag": with_scene(2, sc(2, flags=0)),
        "ss4 on one frame only": with_scene(2, sc(2, flags=ss)),
        "ss4 on all frames but one": [sc(j, flags=ss if j != 1 else GEO_FLAG_DISK) for j in range(n)],
        "step differs": with_scene(1, sc(1, step=ok.step * 0.5)),
        "max_steps differs": with_scene(1, sc(1, max_steps=ok.max_steps - 1)),
        "rs differs": with_scene(1, sc(1, rs=0.9)),
        "sphere_r differs": with_scene(1, sc(1, sphere_r=49.0)),
        "a later frame inside the horizon": with_scene(3, sc(3, r_obs=0.9)),
        "a later frame outside the sphere": with_scene(3, sc(3, r_obs=50.0)),
    }
    for name, bad in cases.items():
        assert raw(ctx, frames, bad, lay, out) == GEO_EINVAL, name
        assert untouched(), name
    assert raw(ctx, frames, scenes, lay, out, n=0) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, n=N + 1) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, stride=packed - 4) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, stride=packed + 2) == GEO_EINVAL and untouched()
    # each of the three armed per-pixel buffers: consumed by the refused call, plain and SS4
    one = torch.full((packed,), FILL, dtype=torch.uint8, device=dev)
    hb = torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=dev)
    gb = torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=dev)
    qb = torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=dev)
    arms = ((ctx.disk_hits_next_render, hb), (ctx.disk_shift_next_render, gb), (ctx.disk_emission_next_render, qb))
    for s4 in (False, True):
        for arm, buf in arms:
            arm(buf)
            assert raw(ctx, frames, ss_all(scenes, s4), lay, out) == GEO_EINVAL and untouched()
            one.fill_(FILL)
            ctx.render_band_set(frames[0], scenes[0], w, h, lay[2], lay[3], lay[4], nb, one)
            torch.cuda.synchronize()
            assert bool((buf == -1.0).all()) and not bool((one == FILL).all())
    # the shading needs circular orbits down to the inner edge: r_in > 1.5 rs
    ctx.set_disk(T.TEX, 1.5, 9.0, RING_DISK[2], RING_DISK[3])
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    ctx.set_disk(T.TEX, *RING_DISK)
    # a good call draws; the older calls and the one-frame SS4 render keep refusing while the state is on
    assert raw(ctx, frames, scenes, lay, out) == GEO_OK
    torch.cuda.synchronize()
    assert not bool((out[:n * packed] == 0x5A).all())
    out.fill_(0x5A)
    s4 = ss_all(scenes, True)
    assert raw(ctx, frames, scenes, lay, out, fn=lib.geo_render_emission_batch) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, s4, lay, out, fn=lib.geo_render_emission_batch) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, fn=lib.geo_render_disk_batch) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, s4, lay, out, fn=lib.geo_render_ss_batch) == GEO_EINVAL and untouched()
    fa, sa = (GeoFrame * 1)(frames[0]), (GeoScene * 1)(s4[0])
    assert lib.geo_render_band_set(ctx._h, fa, sa, w, h, lay[2], lay[3], lay[4], nb, out.data_ptr(), None, None, None,
                                   None, None) == GEO_EINVAL and untouched()
    ctx.close()


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_no_capture_orbit(dev, ss):
    """rs = 0: the state is ignored and the frames are the older batches'."""
    import torch

    lay = RAGGED
    w, h = lay[:2]
    nb, _, packed = dims(lay)
    frames, scenes = pan("flat", w, h, 5)
    sc = ss_all(scenes, ss)
    for variant in VARIANTS:
        ctx = new_ctx(dev, variant)
        got, tot = batch(ctx, dev, frames, sc, lay)
        ctx.set_disk_ring_f64(False)
        older = (ctx.render_emission_batch if variant == "emission" else
                 ctx.render_ss_batch if ss else ctx.render_disk_batch)
        ref = torch.full((5 * packed,), FILL, dtype=torch.uint8, device=dev)
        rtot = torch.zeros(1, dtype=torch.int64, device=dev)
        older(frames, sc, w, h, lay[2], lay[3], lay[4], nb, ref, steps_total=rtot)
        torch.cuda.synchronize()
        ctx.close()
        assert np.array_equal(got, ref.cpu().numpy().reshape(5, packed)) and tot == int(rtot.item()) > 0, variant
        assert not (got[:, :h * w * 4] == FILL).all()


def test_fuzzed_batches(dev):
    """fuzz_disk_scenes.disk_batch's seeds with a capture orbit (rs > 0, the
    observer outside 1.5 rs), the variant by seed % 3, GEO_FLAG_SS4 on the odd
    seeds: every one-sample frame is its one-frame ring render; every
    supersampled one the resolve of its one-frame ring render of twice the size."""
    import torch

    w, h = 64, 36
    lay = (w, h, 8, 0, 8)
    _, _, packed = dims(lay)
    launched, kinds = 0, set()
    for i, seed in enumerate(BATCH_SEEDS):
        n = 2 + (5 * i) % 7
        frames, scenes, disk_args, shift, desc = disk_batch(seed, w, h, n)
        if not (scenes[0].rs > 0.0 and all(s.r_obs > 1.5 * s.rs for s in scenes)):
            continue
        variant = VARIANTS[seed % 3]
        if variant != "plain" and not disk_args[0] > 1.5 * scenes[0].rs:
            variant = "plain"  # (the shading's r_in > 1.5 rs rule)
        em, ramp = disk_scene(seed, w, h)[4]
        ss = bool(seed % 2)
        ctx = new_ctx(dev, variant, disk=disk_args, em=em, ramp=ramp, shift=shift)
        try:
            got, tot = batch(ctx, dev, frames, ss_all(scenes, ss), lay)
            if not ss:
                ref, tots, _ = singles(ctx, dev, frames, scenes, lay)
            else:
                ref, tots = [], []
                for f in range(n):
                    one = torch.zeros(4 * w * h * 4, dtype=torch.uint8, device=dev)
                    t = torch.zeros(1, dtype=torch.int64, device=dev)
                    ctx.render_rows(frames[f], scenes[f], 2 * w, 2 * h, 0, 2 * h, one, steps_total=t)
                    torch.cuda.synchronize()
                    r = np.full(packed, FILL, np.uint8)
                    r[:h * w * 4] = resolve(one.cpu().numpy().reshape(2 * h, 2 * w, 4)).reshape(-1)
                    ref.append(r)
                    tots.append(int(t.item()))
        finally:
            ctx.close()
        for f in range(n):
            diff = got[f] != ref[f]
            assert not diff.any(), (desc, variant, "ss4" if ss else "one sample", f"frame {f}",
                                    f"{int(diff.sum())} bytes, first at pixel {int(np.argwhere(diff)[0][0]) // 4}")
        assert tot == sum(tots), (desc, variant, ss, tot, tots)
        launched += n
        kinds.add((kind_of(scenes[0].rs, scenes[0].r_obs, scenes[0].step), variant, ss))
    print(f"fuzzed ring batches: {launched} batched frames compared; (kind, variant, ss4) drawn: {sorted(kinds)}")
    assert launched >= 8


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_pipeline(dev, ss):
    import torch

    from schwarzschild_raytracer_wgpu_amd.dist import ShardedFrame

    w, h, nsteps = T.W, 56, 8  # (whole 8-row bands: the frame's rows are the rank's packed rows)
    frames, scenes = walk(w, h, nsteps)
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev, "emission")
    with pytest.raises(ValueError, match="set_disk_ring_f64"):
        ShardedFrame(ctx, frames[0], sc[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=True)
    with pytest.raises(ValueError, match="set_disk_ring_f64"):
        ShardedFrame(ctx, frames[0], sc[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=True,
                     emission_batch=True)
    sf = ShardedFrame(ctx, frames[0], sc[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=True,
                      disk_ring_batch=True)
    assert sf.batch and sf.K == 4
    # the one-frame ring frames: the render itself, or (SS4) the resolve of the render of twice the size
    refs = []
    for f, s in zip(frames, scenes):
        k = 2 if ss else 1
        one = torch.zeros(k * k * h * w * 4, dtype=torch.uint8, device=dev)
        ctx.render_rows(f, s, k * w, k * h, 0, k * h, one)
        torch.cuda.synchronize()
        img = one.cpu().numpy().reshape(k * h, k * w, 4)
        refs.append((resolve(img) if ss else img).reshape(-1))
    retired = 0
    for i in range(nsteps):
        sf.step(i, frame=frames[i], scene=sc[i])
        if i % sf.K == sf.K - 1:
            sf.drain()
            torch.cuda.synchronize()
            assert np.array_equal(sf.frame_rgba().cpu().numpy().reshape(-1), refs[i]), i
            for j in range(i - sf.K + 1, i + 1):
                assert np.array_equal(sf.local_view(j)[:h * w * 4].cpu().numpy(), refs[j]), j
                retired += 1
    sf.drain()
    torch.cuda.synchronize()
    ctx.close()
    assert retired == nsteps == sf.frames_done
    assert not np.array_equal(refs[0], refs[1])
