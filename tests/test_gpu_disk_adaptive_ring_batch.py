"""geo_render_disk_adaptive_ring_batch: up to GEO_MAX_BATCH_FRAMES
GEO_MODE_ADAPTIVE thin-disk frames with the capture band's pixels in f64
(geo_set_disk_ring_f64) in one render launch
(geo_render_disk_ring_batch_kernel<KIND, SHADE, SS, GEO_MODE_ADAPTIVE>).  A
one-sample frame is its one-frame geo_render_disk_adaptive_ring render byte for
byte, and so the CPU path's (geo_render_cpu_disk_adaptive_ring_f64); a
GEO_FLAG_SS4 frame is the box resolve of that render at twice the size, which
no one-frame call draws.  Then the band's evidence against the state-off
adaptive batch, the call's mechanics, the C-ABI's refusals (geo.h), fuzzed
batches and dist.ShardedFrame's disk_ring_any_mode route.  All comparisons are
bit for bit.

Frames are 96 x 54 (a wave is 16 x 4 pixels, a tile 32 x 8: partial waves and
tiles, several workgroups), 48 x 27 output under SS4 (the same 96 x 54
samples); the walk, its layouts and the band's test come from
tests/test_gpu_disk_ring_batch.py, the walk's parameters from
tests/test_disk_adaptive_ring_batch_host.py, which holds every frame drawn here
to the conditions that make these tests meaningful, on the CPU path: an in-band
pixel with a slot-2 hit, a hit outside the band, a wave block with lanes of
both kinds."""
import numpy as np
import pytest

import fuzz_disk_scenes as F
import test_disk_adaptive_cpu as A
import test_disk_adaptive_ring_batch_host as HB
import test_disk_adaptive_ring_cpu as AR
import test_disk_cpu as T
import test_gpu_disk_batch as DB
import test_gpu_disk_ring_batch as RB
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4,
                                                   GEO_MAX_BATCH_FRAMES, GEO_MODE_ADAPTIVE, GEO_MODE_DIRECT,
                                                   GEO_MODE_FAN, GEO_OK, GeoFrame, GeoScene, lib)
from test_gpu_disk_ring_batch import PEER, RAGGED, WHOLE, in_band, new_ctx, resolve, state_of
from test_gpu_disk_batch import FILL, dims

pytestmark = pytest.mark.gpu

N = GEO_MAX_BATCH_FRAMES
VARIANTS = RB.VARIANTS
SS_OUT = (48, 27, 8, 0, 8)  # the SS4 tests' output layout: its samples are the 96 x 54 frame's
walk, direct_of = HB.walk, HB.direct_of
FUZZ_SEEDS = range(40, 80)


def ss_all(scenes, ss=True):
    return [make_scene(s.rs, s.sphere_r, s.r_obs, s.step, s.max_steps, s.mode,
                       s.flags | (GEO_FLAG_SS4 if ss else 0), s.tol) for s in scenes]


def batch(ctx, dev, frames, scenes, lay, stride=None, total=True, call=None):
    """The batch through Context.render_disk_adaptive_ring_batch: (bytes per frame slot, steps)."""
    import torch

    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    n = len(frames)
    stride = packed if stride is None else stride
    out = torch.full((n * stride,), FILL, dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev) if total else None
    call = ctx.render_disk_adaptive_ring_batch if call is None else call
    call(frames, scenes, w, h, br, row0, rstride, nb, out, frame_stride=stride, steps_total=tot)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, stride), (int(tot.item()) if total else None)


def singles(ctx, dev, frames, scenes, lay, k=1):
    """Every frame alone through geo_render_disk_adaptive_ring on the layout times k (k = 2: the sample
    frame of a GEO_FLAG_SS4 render; `scenes` without the flag): (bytes per frame as (nrows k, w k, 4), the
    steps per frame).  The unwritten rows of a clipped band keep FILL (and so does their resolve)."""
    import torch

    w, h, br, row0, rstride = (k * v for v in lay)
    nb, nrows, packed = dims((w, h, br, row0, rstride))
    refs, tots = [], []
    for f, s in zip(frames, scenes):
        ref = torch.full((packed,), FILL, dtype=torch.uint8, device=dev)
        tot = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx.render_disk_adaptive_ring(f, s, w, h, br, row0, rstride, nb, ref, steps_total=tot)
        refs.append(ref)
        tots.append(tot)
    torch.cuda.synchronize()
    return np.stack([r.cpu().numpy().reshape(nrows, w, 4) for r in refs]), [int(t.item()) for t in tots]


def flat(imgs):
    return np.stack([i.reshape(-1) for i in imgs])


def raw(ctx, frames, scenes, lay, out, stride=None, n=None, fn=None):
    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    fa, sa = (GeoFrame * len(frames))(*frames), (GeoScene * len(scenes))(*scenes)
    fn = lib.geo_render_disk_adaptive_ring_batch if fn is None else fn
    return fn(ctx._h, fa, sa, len(frames) if n is None else n, w, h, br, row0, rstride, nb, out.data_ptr(),
              packed if stride is None else stride, None, None)


@pytest.fixture(scope="module")
def cpu():
    return AR.load_cpu()


class Refs:
    """The one-frame geo_render_disk_adaptive_ring renders of a walk, rendered once per (layout, variant,
    kind, k) and shared, read-only: (frames, scenes, bytes per frame, steps per frame)."""

    def __init__(self, dev):
        self.dev, self.cache = dev, {}

    def get(self, lay, variant, curved_in=False, k=1):
        key = (lay, variant, curved_in, k)
        if key not in self.cache:
            frames, scenes = walk(lay[0], lay[1], N, curved_in)
            ctx = new_ctx(self.dev, variant)
            on, tots = singles(ctx, self.dev, frames, scenes, lay, k)
            ctx.close()
            on = flat([resolve(b) for b in on]) if k == 2 else flat(on)
            on.setflags(write=False)
            self.cache[key] = (frames, scenes, on, tots)
        return self.cache[key]


@pytest.fixture(scope="module")
def refs(dev):
    return Refs(dev)


# ---- 1. the batch equals the one-frame renders ------------------------------------------------------
CASES = [(lay, v, False) for lay in (WHOLE, RAGGED) for v in VARIANTS] + [(WHOLE, "shift", True)]
CASE_IDS = [f"{'whole' if lay is WHOLE else 'ragged'}-{'curved_in-' if ci else ''}{v}" for lay, v, ci in CASES]


@pytest.mark.parametrize("lay,variant,curved_in", CASES, ids=CASE_IDS)
def test_batch_equals_single_frames(dev, refs, lay, variant, curved_in):
    frames, scenes, on, tots = refs.get(lay, variant, curved_in)
    assert all(s.mode == GEO_MODE_ADAPTIVE and s.flags == GEO_FLAG_DISK for s in scenes)
    assert F.kind_of(scenes[0].rs, scenes[0].r_obs, scenes[0].step) == (1 if curved_in else 0)
    ctx = new_ctx(dev, variant)
    for n in (1, 3, N):
        got, tot = batch(ctx, dev, frames[:n], scenes[:n], lay)
        for f in range(n):
            print(f"n={n} frame {f}: differing bytes {int((got[f] != on[f]).sum())}")
            assert np.array_equal(got[f], on[f]), (n, f)
            if f:
                assert not np.array_equal(on[f], on[f - 1]), f
        assert tot == sum(tots[:n]) > 0, (n, tot, tots[:n])
    ctx.close()


def test_orbit_on_the_peer_layout(dev):
    """A moving observer on a peer's interleaved bands (row_stride > band_rows, row0 > 0), every variant."""
    frames, scenes = DB.orbit(PEER[0], PEER[1], N)
    scenes = [A.adaptive_of(s) for s in scenes]
    for variant in VARIANTS:
        ctx = new_ctx(dev, variant, disk=DB.DISK)
        got, tot = batch(ctx, dev, frames, scenes, PEER)
        ref, tots = singles(ctx, dev, frames, scenes, PEER)
        ctx.close()
        assert np.array_equal(got, flat(ref)) and tot == sum(tots) > 0, variant
        assert not np.array_equal(got[0], got[N - 1])


# ---- 2. against the CPU path ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_against_the_cpu_path(dev, cpu, refs, variant):
    w, h = WHOLE[:2]
    frames, scenes, on, tots = refs.get(WHOLE, variant)
    ctx = new_ctx(dev, variant)
    got, _ = batch(ctx, dev, frames, scenes, WHOLE)
    ctx.close()
    for f in (0, 3, N - 1):
        rc, c = AR.render(cpu, frames[f], scenes[f], T.make_disk(*RB.RING_DISK), 1, w, h, **state_of(variant))
        assert rc == GEO_OK
        assert np.array_equal(got[f][:h * w * 4].reshape(h, w, 4), c["rgba"]), f
        assert (got[f][h * w * 4:] == FILL).all()  # the clipped rows of the last band
        assert tots[f] == c["total"], f
    assert not np.array_equal(got[0], got[N - 1])


# ---- 3. the band's evidence -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_band_pixels_differ_from_the_state_off_batch_and_no_others(dev, refs, variant):
    """With the state off the same frames through geo_render_disk_adaptive_batch: equal outside the band
    bit for bit, different inside it.  A kernel that ignored MODE (the direct integrator outside the band)
    or the band (the adaptive one inside it) could not pass both."""
    w, h = WHOLE[:2]
    frames, scenes, on, _ = refs.get(WHOLE, variant)
    ctx = new_ctx(dev, variant)
    got, tot = batch(ctx, dev, frames, scenes, WHOLE)
    ctx.set_disk_ring_f64(False)
    off, off_tot = batch(ctx, dev, frames, scenes, WHOLE, call=ctx.render_disk_adaptive_batch)
    direct, _ = batch(ctx, dev, frames, [direct_of(s) for s in scenes], WHOLE, call=ctx.render_disk_batch
                      if variant != "emission" else ctx.render_emission_batch)
    ctx.close()
    assert tot != off_tot
    for f in range(N):
        band = in_band(frames[f], direct_of(scenes[f]), w, h)
        a, b = got[f][:h * w * 4].reshape(h, w, 4), off[f][:h * w * 4].reshape(h, w, 4)
        differ = (a != b).any(axis=-1)
        d = direct[f][:h * w * 4].reshape(h, w, 4)
        print(f"{variant} frame {f}: band pixels {int(band.sum())}, in-band pixels that differ {int((differ & band).sum())}, "
              f"others {int((differ & ~band).sum())}; non-band pixels that differ from the direct disk batch's "
              f"{int(((a != d).any(axis=-1) & ~band).sum())}")
        assert (differ & band).sum() >= 1, f
        assert not (differ & ~band).any(), f


# ---- 4. SS4 is the resolve -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_ss4_is_the_resolve(dev, cpu, refs, variant):
    w, h = SS_OUT[:2]
    frames, scenes, want, tots = refs.get(SS_OUT, variant, k=2)
    ctx = new_ctx(dev, variant)
    one, _ = batch(ctx, dev, frames, scenes, SS_OUT)
    for n in (1, N):
        got, tot = batch(ctx, dev, frames[:n], ss_all(scenes[:n]), SS_OUT)
        for f in range(n):
            print(f"ss4 {variant} n={n} frame {f}: differing bytes {int((got[f] != want[f]).sum())}")
            assert np.array_equal(got[f], want[f]), (n, f)
            assert not np.array_equal(got[f], one[f]), f  # not the one-sample 48 x 27 frame
        assert tot == sum(tots[:n]) > 0, (n, tot)
    ctx.close()
    for f in (0, N - 1):
        rc, c = AR.render(cpu, frames[f], scenes[f], T.make_disk(*RB.RING_DISK), 1, 2 * w, 2 * h, **state_of(variant))
        assert rc == GEO_OK and c["total"] == tots[f]
        assert np.array_equal(got[f][:h * w * 4].reshape(h, w, 4), resolve(c["rgba"])), f
        assert (got[f][h * w * 4:] == FILL).all()


def test_ss4_curved_in(dev, cpu, refs):
    w, h = SS_OUT[:2]
    frames, scenes, want, tots = refs.get(SS_OUT, "emission", True, k=2)
    assert F.kind_of(scenes[0].rs, scenes[0].r_obs, scenes[0].step) == 1
    ctx = new_ctx(dev, "emission")
    got, tot = batch(ctx, dev, frames, ss_all(scenes), SS_OUT)
    ctx.close()
    assert np.array_equal(got, want) and tot == sum(tots) > 0
    rc, c = AR.render(cpu, frames[0], scenes[0], T.make_disk(*RB.RING_DISK), 1, 2 * w, 2 * h, **state_of("emission"))
    assert rc == GEO_OK and np.array_equal(got[0][:h * w * 4].reshape(h, w, 4), resolve(c["rgba"]))


# ---- 5. call mechanics ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", [False, True], ids=["one-sample", "ss4"])
def test_frame_stride_and_padding(dev, ss):
    frames, scenes = walk(RAGGED[0], RAGGED[1], 3)
    w, h = RAGGED[:2]
    _, nrows, packed = dims(RAGGED)
    stride = packed + 4 * 37
    ctx = new_ctx(dev, "shift")
    got, _ = batch(ctx, dev, frames, ss_all(scenes, ss), RAGGED, stride=stride)
    big, _ = singles(ctx, dev, frames, scenes, RAGGED, k=2 if ss else 1)
    ctx.close()
    ref = flat([resolve(b) for b in big]) if ss else flat(big)
    assert np.array_equal(got[:, :packed], ref)
    assert (got[:, packed:] == FILL).all()  # the bytes between frames are untouched
    assert nrows > h and (got[:, h * w * 4:packed] == FILL).all()  # rows past the frame are not written
    assert not (ref[:, :h * w * 4] == FILL).all()


@pytest.mark.parametrize("ss", [False, True], ids=["one-sample", "ss4"])
def test_deferred_steps_orders_and_timing(dev, refs, ss):
    """GEO_FLAG_DEFER_STEPS, the row-major, learned (period 1) and explicit orders, and
    geo_time_next_render: the same frames and steps every way."""
    import torch

    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    lay = SS_OUT if ss else WHOLE
    frames, scenes, ref, tots = refs.get(lay, "emission", k=2 if ss else 1)
    ref_tot = sum(tots)
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev, "emission")
    ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    got, tot = batch(ctx, dev, frames, sc, lay)
    assert np.array_equal(got, ref) and tot == ref_tot
    deferred = [make_scene(s.rs, s.sphere_r, s.r_obs, s.step, s.max_steps, s.mode, s.flags | GEO_FLAG_DEFER_STEPS,
                           s.tol) for s in sc]
    got, none = batch(ctx, dev, frames, deferred, lay, total=False)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.steps_flush(tot)
    torch.cuda.synchronize()
    assert none is None and np.array_equal(got, ref) and int(tot.item()) == ref_tot
    ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    rec0, _ = ctx.dispatch_stats()
    for i in range(3):
        got, tot = batch(ctx, dev, frames, sc, lay)
        assert np.array_equal(got, ref) and tot == ref_tot, i
    rec, _ = ctx.dispatch_stats()
    assert rec > rec0
    # an explicit order: the grid's tiles (the sample frame's under SS4) back to front
    k = 2 if ss else 1
    tx, ty = (k * lay[0] + 31) // 32, (k * dims(lay)[1] + 7) // 8
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
    """Two batches of one context on two streams, issued back to back with no wait between them, each
    with its own walk: a table of band constants per render-stream slot, so neither reads the other's."""
    import torch

    lay = WHOLE
    fa, sa, on_a, tots_a = refs.get(lay, "plain")
    fb, sb = walk(lay[0], lay[1], N, **HB.WALK_B)
    ctx = new_ctx(dev, "plain")
    on_b, tots_b = singles(ctx, dev, fb, sb, lay)
    on_b = flat(on_b)
    assert not np.array_equal(on_a, on_b)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    nb, _, packed = dims(lay)
    # (the outputs filled before anything is issued: the streams do not order against the fills)
    outs = [[(torch.full((N * packed,), FILL, dtype=torch.uint8, device=dev),
              torch.zeros(1, dtype=torch.int64, device=dev)) for _ in range(2)] for _ in range(2)]
    torch.cuda.synchronize()
    for pair in outs:  # twice: each slot's table is written again behind its stream's earlier render
        for (o, t), fr, sc, st in zip(pair, (fa, fb), (sa, sb), (s1, s2)):
            ctx.render_disk_adaptive_ring_batch(fr, sc, lay[0], lay[1], lay[2], lay[3], lay[4], nb, o, steps_total=t,
                                                stream=st)
    torch.cuda.synchronize()
    ctx.close()
    for (oa, ta), (ob, tb) in outs:
        assert np.array_equal(oa.cpu().numpy().reshape(N, packed), on_a) and int(ta.item()) == sum(tots_a)
        assert np.array_equal(ob.cpu().numpy().reshape(N, packed), on_b) and int(tb.item()) == sum(tots_b)


# ---- 6. no capture orbit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", [False, True], ids=["one-sample", "ss4"])
def test_no_capture_orbit(dev, ss):
    """rs = 0: the state is ignored and the frames are geo_render_disk_adaptive_batch's, with the state on
    here and off there."""
    frames, scenes = DB.pan("flat", T.W, T.H, 3)
    sc = ss_all([A.adaptive_of(s) for s in scenes], ss)
    for variant in VARIANTS:
        ctx = new_ctx(dev, variant, disk=T.pose("flat")[3])
        on, on_tot = batch(ctx, dev, frames, sc, WHOLE)
        ctx.set_disk_ring_f64(False)
        off, off_tot = batch(ctx, dev, frames, sc, WHOLE, call=ctx.render_disk_adaptive_batch)
        ctx.close()
        assert np.array_equal(on, off) and on_tot == off_tot > 0, variant
        assert not (off[:, :T.W * T.H * 4] == FILL).all()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_refusals(dev):
    import torch

    lay = WHOLE
    w, h = lay[:2]
    nb, nrows, packed = dims(lay)
    n = 4
    frames, scenes = walk(w, h, n)
    ok = scenes[0]
    out = torch.full((N * packed + 64,), 0x5A, dtype=torch.uint8, device=dev)
    A_, D_ = GEO_MODE_ADAPTIVE, GEO_FLAG_DISK

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 0x5A).all())

    def sc(i=0, mode=A_, flags=D_, tol=0.0, **kw):
        s = scenes[i]
        f = dict(rs=s.rs, sphere_r=s.sphere_r, r_obs=s.r_obs, step=s.step, max_steps=s.max_steps)
        f.update(kw)
        return make_scene(f["rs"], f["sphere_r"], f["r_obs"], f["step"], f["max_steps"], mode, flags, tol)

    def with_scene(i, s):
        return [s if j == i else scenes[j] for j in range(n)]

    # the state off; no disk (clear_disk drops the state with it: set again); no sky
    ctx = new_ctx(dev, "plain", ring=False)
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    assert raw(ctx, frames, ss_all(scenes), lay, out) == GEO_ESTATE and untouched()
    ctx.set_disk_ring_f64(True)
    assert raw(ctx, frames, scenes, lay, out) == GEO_OK
    torch.cuda.synchronize()
    out.fill_(0x5A)
    ctx.clear_disk()
    ctx.set_disk_ring_f64(True)
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    ctx.close()
    import schwarzschild_raytracer_wgpu_amd as g

    ctx = g.Context(dev.index or 0)  # no sky
    ctx.set_disk(T.TEX, *RB.RING_DISK)
    ctx.set_disk_ring_f64(True)
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    ctx.close()

    ctx = new_ctx(dev, "emission")
    ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    ss = D_ | GEO_FLAG_SS4
    cases = {
        "direct": [sc(j, mode=GEO_MODE_DIRECT) for j in range(n)],
        "fan": [sc(j, mode=GEO_MODE_FAN) for j in range(n)],
        "one direct scene": with_scene(2, sc(2, mode=GEO_MODE_DIRECT)),
        "disk | ring_f64": [sc(j, flags=D_ | GEO_FLAG_RING_F64) for j in range(n)],
        "mips": [sc(j, flags=D_ | GEO_FLAG_MIPS) for j in range(n)],
        "composite": [sc(j, flags=D_ | GEO_FLAG_COMPOSITE) for j in range(n)],
        "ss4 mips": [sc(j, flags=ss | GEO_FLAG_MIPS) for j in range(n)],
        "no disk flag": [sc(j, flags=0) for j in range(n)],
        "ss4 on one frame only": with_scene(2, sc(2, flags=ss)),
        "ss4 on all frames but one": [sc(j, flags=ss if j != 1 else D_) for j in range(n)],
        "tol differs": with_scene(1, sc(1, tol=1e-5)),
        "step differs": with_scene(1, sc(1, step=ok.step * 0.5)),
        "max_steps differs": with_scene(1, sc(1, max_steps=ok.max_steps - 1)),
        "rs differs": with_scene(1, sc(1, rs=0.9)),
        "a later frame inside the horizon": with_scene(3, sc(3, r_obs=0.9)),
        "tol negative": [sc(j, tol=-1e-6) for j in range(n)],
    }
    for name, bad in cases.items():
        assert raw(ctx, frames, bad, lay, out) == GEO_EINVAL, name
        assert untouched(), name
    assert raw(ctx, frames, scenes, lay, out, n=0) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, n=N + 1) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, stride=packed - 4) == GEO_EINVAL and untouched()
    # each of the three armed per-pixel buffers: consumed by the refused call, one sample and SS4: the
    # one-frame render that follows, which would write an armed buffer, leaves them alone
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
            ctx.render_disk_adaptive_ring(frames[0], scenes[0], w, h, lay[2], lay[3], lay[4], nb, one)
            torch.cuda.synchronize()
            assert bool((buf == -1.0).all()) and not bool((one == FILL).all())
    # a valid call follows the refusals and draws
    assert raw(ctx, frames, scenes, lay, out) == GEO_OK
    torch.cuda.synchronize()
    assert not bool((out[:n * packed] == 0x5A).all()) and bool((out[n * packed:] == 0x5A).all())
    out.fill_(0x5A)
    # the older calls keep their refusals while the state is on
    s4 = ss_all(scenes)
    direct = [direct_of(s) for s in scenes]
    for fn, scs in ((lib.geo_render_disk_adaptive_batch, scenes), (lib.geo_render_disk_adaptive_batch, s4),
                    (lib.geo_render_disk_ring_batch, scenes), (lib.geo_render_disk_ring_batch, s4),
                    (lib.geo_render_emission_batch, scenes), (lib.geo_render_disk_batch, scenes),
                    (lib.geo_render_emission_batch, direct), (lib.geo_render_disk_batch, direct)):
        assert raw(ctx, frames, scs, lay, out, fn=fn) == GEO_EINVAL and untouched(), fn.__name__
    fa, sa = (GeoFrame * 1)(frames[0]), (GeoScene * 1)(s4[0])
    assert lib.geo_render_disk_adaptive_ring(ctx._h, fa, sa, w, h, lay[2], lay[3], lay[4], nb, out.data_ptr(), None,
                                             None, None, None, None) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, direct, lay, out, fn=lib.geo_render_disk_ring_batch) == GEO_OK  # (and draws the direct ones)
    torch.cuda.synchronize()
    ctx.close()


# ---- 8. fuzz -------------------------------------------------------------------------------------------------------------
def test_fuzzed_batches(dev):
    """fuzz_disk_scenes.disk_batch's seeds 40..79 forced to the adaptive mode with the state on, the
    variant by seed % 3, one sample and GEO_FLAG_SS4 each: every frame is its one-frame
    geo_render_disk_adaptive_ring render, or the resolve of that render at twice the size.  Ten of the
    forty seeds hold no band pixel in any frame (counted on the CPU when the range was picked: the flat
    observers' eight, rs = 0, the state ignored, and seeds 43 and 73); at most half may."""
    w, h = 64, 36
    lay = (w, h, 8, 0, 8)
    launched, band_free, kinds = 0, 0, set()
    for i, seed in enumerate(FUZZ_SEEDS):
        n = 2 + (5 * i) % 7
        frames, scenes, disk_args, shift, desc = F.disk_batch(seed, w, h, n)
        band = sum(int(in_band(frames[f], scenes[f], w, h).sum()) for f in range(n)) if scenes[0].rs > 0.0 else 0
        band_free += band == 0
        scenes = [A.adaptive_of(s) for s in scenes]
        variant = VARIANTS[seed % 3]
        em, ramp = F.disk_scene(seed, w, h)[4]
        ctx = new_ctx(dev, variant, disk=disk_args, em=em, ramp=ramp, shift=shift)
        try:
            got, tot = batch(ctx, dev, frames, scenes, lay)
            ref, tots = singles(ctx, dev, frames, scenes, lay)
            got4, tot4 = batch(ctx, dev, frames, ss_all(scenes), lay)
            big, tots4 = singles(ctx, dev, frames, scenes, lay, k=2)
        finally:
            ctx.close()
        ref, ref4 = flat(ref), flat([resolve(b) for b in big])
        for f in range(n):
            for what, g_, r_ in (("one sample", got, ref), ("ss4", got4, ref4)):
                diff = g_[f] != r_[f]
                assert not diff.any(), (desc, variant, what, f"frame {f}", f"{int(diff.sum())} bytes, first at pixel "
                                        f"{int(np.argwhere(diff)[0][0]) // 4}")
        assert tot == sum(tots) and tot4 == sum(tots4), (desc, variant, tot, tots, tot4, tots4)
        launched += 2 * n
        kinds.add((F.kind_of(scenes[0].rs, scenes[0].r_obs, scenes[0].step), variant))
    print(f"fuzzed adaptive ring batches: {launched} batched frames compared; seeds without a band pixel: {band_free} "
          f"of {len(FUZZ_SEEDS)}; (kind, variant) drawn: {sorted(kinds)}")
    assert len(FUZZ_SEEDS) == 40 and band_free <= len(FUZZ_SEEDS) // 2


# ---- 9. the pipeline --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", [False, True], ids=["one-sample", "ss4"])
@pytest.mark.parametrize("batch_launch", [True, False], ids=["batched", "per-frame"])
def test_pipeline(dev, batch_launch, ss):
    import torch

    from schwarzschild_raytracer_wgpu_amd.dist import ShardedFrame

    w, h, nsteps = T.W, 56, 8  # (whole 8-row bands: the frame's rows are the rank's packed rows)
    frames, scenes = walk(w, h, nsteps)
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev, "emission")
    with pytest.raises(ValueError, match="disk_ring_any_mode=True"):
        ShardedFrame(ctx, frames[0], sc[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=batch_launch)
    with pytest.raises(ValueError, match="set_disk_ring_f64"):
        ShardedFrame(ctx, frames[0], sc[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=batch_launch,
                     disk_ring_batch=True, emission_batch=True)
    sf = ShardedFrame(ctx, frames[0], sc[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=batch_launch,
                      disk_ring_any_mode=True)
    assert sf.batch == batch_launch and sf.K == (4 if batch_launch else 1)
    # the one-frame ring frames: the render itself, or (SS4) the resolve of the render of twice the size
    k = 2 if ss else 1
    refs = []
    for f, s in zip(frames, scenes):
        one = torch.zeros(k * k * h * w * 4, dtype=torch.uint8, device=dev)
        ctx.render_disk_adaptive_ring(f, s, k * w, k * h, k * h, 0, k * h, 1, one)
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
