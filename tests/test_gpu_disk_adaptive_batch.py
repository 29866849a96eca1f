"""geo_render_disk_adaptive_batch: up to GEO_MAX_BATCH_FRAMES thin-disk frames in
GEO_MODE_ADAPTIVE in one launch (geo_render_disk_batch_kernel's GEO_MODE_ADAPTIVE
instantiations, plain, shifted and emission, one sample and SS4: wave_block_body
with the adaptive integrator on DiskBatchFrame, the frame in blockIdx.z).  A one-sample frame is
its one-frame geo_render_disk_adaptive render bit for bit, and so the CPU
path's (geo_render_cpu_disk_adaptive); a GEO_FLAG_SS4 frame is the box resolve
(numpy, below) of the one-frame render at twice the size, which no one-frame
call draws.  Then the step control, the layout, the step counters and the
dispatch, the C-ABI's rules (geo.h), fuzzed scenes and dist.ShardedFrame's
routing.

Layouts (test_gpu_disk_batch.py's): PEER 160 x 96 in 8-row bands 24 apart from
row 8, RAGGED 100 x 37 (partial tiles, a clipped last band), WHOLE 96 x 54.  A
wave is 16 x 4 pixels and a tile 32 x 8.

What the floors below stand on, checked on the CPU path
(geo_render_cpu_disk_adaptive) when the tests were written (the tests print
the counts they see): over the three layouts the 8 orbit frames hold 983 to 1460 slot-0
hits and 28 to 72 slot-1 hits; an unshaded SS4 frame differs from its
one-sample frame in 1585 to 2029 pixels (a shaded one on PEER and RAGGED in
1509 or more); the step-control cases hold 900 or more slot-0 hits each, the
budget-12 case no slot-1 hit by construction, and each differs from the
default-tol frame in 262 or more pixels; the 12 fuzz seeds are all accepted in
the adaptive mode with and without the shift, reach all three integration kinds
and hold 30 790 slot-0, 622 slot-1 and 28 slot-2 hits in total."""
import numpy as np
import pytest

import fuzz_disk_scenes as F
import test_disk_adaptive_cpu as A
import test_disk_cpu as T
import test_disk_emission_cpu as TE
import test_gpu_disk_batch as DB
import test_gpu_disk_fuzz as GF
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4,
                                                   GEO_MAX_BATCH_FRAMES, GEO_MODE_ADAPTIVE, GEO_MODE_DIRECT,
                                                   GEO_MODE_FAN, GEO_OK, GeoFrame, GeoScene, lib)

pytestmark = pytest.mark.gpu

PEER, RAGGED, WHOLE, DISK, FILL = DB.PEER, DB.RAGGED, DB.WHOLE, DB.DISK, DB.FILL
N = GEO_MAX_BATCH_FRAMES
SHADES = {"plain": dict(), "shift": dict(shift=(1, 4, 1.0)), "emission": dict(em=TE.emission())}
dims = DB.dims


def new_ctx(dev, disk=DISK, shift=None, em=None, ramp=TE.RAMP, sky=True):
    ctx = DB.geo().Context(dev.index or 0)
    if sky:
        ctx.set_sky(T.SKY)
    if disk is not None:
        ctx.set_disk(T.TEX, *disk)
    if shift is not None:
        ctx.set_disk_shift(*shift)
    if em is not None:
        spin, profile, t_ref, t_lo, t_hi, exposure = em
        ctx.set_disk_emission(ramp, t_ref, t_lo, t_hi, profile, exposure, spin)
    return ctx


def ad(scenes, ss=False, flags=0, **kw):
    """The scenes in the adaptive mode (test_disk_adaptive_cpu.adaptive_of), with GEO_FLAG_SS4 or without."""
    return [A.adaptive_of(s, flags=GEO_FLAG_DISK | (GEO_FLAG_SS4 if ss else 0) | flags, **kw) for s in scenes]


def orbit(w, h, n, ss=False, **kw):
    frames, scenes = DB.orbit(w, h, n)
    return frames, ad(scenes, ss, **kw)


def resolve(img):
    """GEO_FLAG_SS4's definition on a (2h, 2w, 4) uint8 frame: (s00 + s01 + s10 + s11 + 2) >> 2 per channel."""
    s = img.astype(np.uint16)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def batch(ctx, dev, frames, scenes, lay, stride=None, total=True):
    """The batch through Context.render_disk_adaptive_batch: (bytes per frame slot, steps)."""
    import torch

    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    n = len(frames)
    stride = packed if stride is None else stride
    out = torch.full((n * stride,), FILL, dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev) if total else None
    ctx.render_disk_adaptive_batch(frames, scenes, w, h, br, row0, rstride, nb, out, frame_stride=stride,
                                   steps_total=tot)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, stride), (int(tot.item()) if total else None)


def singles(ctx, dev, frames, scenes, lay, hits=False, k=1):
    """Every frame alone through geo_render_disk_adaptive on the layout times k
    (k = 2: the sample frame of a GEO_FLAG_SS4 render; `scenes` without the
    flag): (bytes per frame as (nrows k, w k, 4), steps, hits per frame).  The
    unwritten rows of a clipped band keep FILL (and so does their resolve)."""
    import torch

    w, h, br, row0, rstride = (k * v for v in lay)
    nb, nrows, packed = dims((w, h, br, row0, rstride))
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    refs, hs = [], []
    for f, s in zip(frames, scenes):
        ref = torch.full((packed,), FILL, dtype=torch.uint8, device=dev)
        hb = torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=dev)
        if hits:
            ctx.disk_hits_next_render(hb)
        ctx.render_disk_adaptive(f, s, w, h, br, row0, rstride, nb, ref, steps_total=tot)
        refs.append(ref)
        hs.append(hb)
    torch.cuda.synchronize()
    return (np.stack([r.cpu().numpy().reshape(nrows, w, 4) for r in refs]), int(tot.item()),
            [x.cpu().numpy().reshape(nrows, w, 3, 2) for x in hs])


def flat(imgs):
    return np.stack([i.reshape(-1) for i in imgs])


def ss_refs(ctx, dev, frames, scenes, lay):
    """The SS4 batch's definition: each frame's one-frame render at 2W x 2H (layout doubled), resolved."""
    big, tot, _ = singles(ctx, dev, frames, scenes, lay, k=2)
    return flat([resolve(b) for b in big]), tot


def raw(ctx, frames, scenes, lay, out, stride=None, n=None, fn=None):
    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    fa, sa = (GeoFrame * len(frames))(*frames), (GeoScene * len(scenes))(*scenes)
    fn = lib.geo_render_disk_adaptive_batch if fn is None else fn
    return fn(ctx._h, fa, sa, len(frames) if n is None else n, w, h, br, row0, rstride, nb, out.data_ptr(),
              packed if stride is None else stride, None, None)


def never_recorded(e0, e1):
    """A timing pair that no render carried: hipEventElapsedTime refuses it.  The error stays
    behind as the thread's last HIP error, where the next kernel launch of anybody's would
    find it: it is taken off again here."""
    from schwarzschild_raytracer_wgpu_amd import timing

    with pytest.raises(RuntimeError):
        e0.elapsed_time(e1)
    timing._hip.hipGetLastError()


@pytest.fixture(scope="module")
def cpu():
    return A.load_cpu()


# ---- 1, 2. the batch equals the one-frame renders, one sample and SS4 ------------------
@pytest.mark.parametrize("lay", [PEER, RAGGED], ids=["peer", "ragged"])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_batch_equals_single_frames(dev, lay, n):
    frames, scenes = orbit(lay[0], lay[1], n)
    assert len({s.r_obs for s in scenes}) == n  # every frame its own radius
    assert all(s.mode == GEO_MODE_ADAPTIVE and s.flags == GEO_FLAG_DISK for s in scenes)
    outs = {}
    for name, shade in SHADES.items():
        ctx = new_ctx(dev, **shade)
        got, tot = batch(ctx, dev, frames, scenes, lay)
        ref, ref_tot, hits = singles(ctx, dev, frames, scenes, lay, hits=True)
        ctx.close()
        ref = flat(ref)
        for f in range(n):
            s0, s1 = int((hits[f][..., 0, 0] > 0).sum()), int((hits[f][..., 1, 0] > 0).sum())
            print(f"{name} n={n} frame {f}: slot-0 hits {s0}, slot-1 hits {s1}, differing bytes "
                  f"{int((got[f] != ref[f]).sum())}")
            assert s0 > 300 and s1 > 0, (name, f, s0, s1)
            assert np.array_equal(got[f], ref[f]), (name, f)
            if f:
                assert not np.array_equal(ref[f], ref[f - 1]), (name, f)
        print(f"{name} n={n}: attempts batch {tot}, one-frame renders {ref_tot}")
        assert tot == ref_tot > 0, name
        outs[name] = got
    for f in range(n):
        assert not np.array_equal(outs["emission"][f], outs["shift"][f]), f
        assert not np.array_equal(outs["shift"][f], outs["plain"][f]), f


@pytest.mark.parametrize("lay", [PEER, RAGGED], ids=["peer", "ragged"])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_ss4_is_the_resolve(dev, lay, n):
    frames, scenes = orbit(lay[0], lay[1], n)
    ss = ad(scenes, True)
    for name, shade in SHADES.items():
        ctx = new_ctx(dev, **shade)
        got, tot = batch(ctx, dev, frames, ss, lay)
        ref, ref_tot = ss_refs(ctx, dev, frames, scenes, lay)
        one, _ = batch(ctx, dev, frames, scenes, lay)
        ctx.close()
        for f in range(n):
            px = int((got[f].reshape(-1, 4) != one[f].reshape(-1, 4)).any(axis=1).sum())
            print(f"{name} n={n} frame {f}: differing bytes {int((got[f] != ref[f]).sum())}; {px} pixels differ from "
                  f"the one-sample frame")
            assert np.array_equal(got[f], ref[f]), (name, f)
            assert px > 0, (name, f)
        print(f"{name} n={n}: attempts batch {tot}, 2W x 2H renders {ref_tot}")
        assert tot == ref_tot > 0, name


# ---- 3. against the CPU path -----------------------------------------------------------
@pytest.mark.parametrize("name", list(SHADES))
def test_against_the_cpu_path(dev, cpu, name):
    w, h = WHOLE[:2]
    frames, scenes = orbit(w, h, N)
    shade = SHADES[name]
    ctx = new_ctx(dev, **shade)
    got, tot = batch(ctx, dev, frames, scenes, WHOLE)
    got4, tot4 = batch(ctx, dev, frames, ad(scenes, True), WHOLE)
    ctx.close()
    disk = T.make_disk(*DISK)
    want, want4 = 0, 0
    for f in range(N):
        rc, c = A.render(cpu, frames[f], scenes[f], w, h, disk, **shade)
        assert rc == GEO_OK and (c["hits"][..., 0, 0] > 0).sum() > 300
        assert np.array_equal(got[f][:h * w * 4].reshape(h, w, 4), c["rgba"]), f
        assert (got[f][h * w * 4:] == FILL).all()  # the clipped rows of the last band
        want += c["total"]
        rc, c2 = A.render(cpu, frames[f], scenes[f], 2 * w, 2 * h, disk, **shade)
        assert rc == GEO_OK
        assert np.array_equal(got4[f][:h * w * 4].reshape(h, w, 4), resolve(c2["rgba"])), f
        assert (got4[f][h * w * 4:] == FILL).all()
        want4 += c2["total"]
    assert tot == want and tot4 == want4


# ---- 4. step control ---------------------------------------------------------------------
STEP_CASES = {"tol 1e-4, step 0.3": dict(tol=1e-4, step=0.3), "tol 1e-7, budget 12": dict(tol=1e-7, max_steps=12),
              "tol 1e30, step 0.8 (kCurvedIn)": dict(tol=1e30, step=0.8)}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_control(dev, case):
    lay = RAGGED
    frames, scenes = orbit(lay[0], lay[1], N, **STEP_CASES[case])
    _, default = orbit(lay[0], lay[1], N)
    if "kCurvedIn" in case:
        assert F.kind_of(scenes[0].rs, scenes[0].r_obs, scenes[0].step) == 1
    ctx = new_ctx(dev, shift=(1, 4, 1.0))
    got, tot = batch(ctx, dev, frames, scenes, lay)
    ref, ref_tot, hits = singles(ctx, dev, frames, scenes, lay, hits=True)
    base, _ = batch(ctx, dev, frames, default, lay)
    ctx.close()
    ref = flat(ref)
    for f in range(N):
        s0 = int((hits[f][..., 0, 0] > 0).sum())
        print(f"{case} frame {f}: slot-0 hits {s0}, slot-1 hits {int((hits[f][..., 1, 0] > 0).sum())}")
        assert s0 > 300, (f, s0)
        assert np.array_equal(got[f], ref[f]), f
        assert not np.array_equal(got[f], base[f]), f
    assert tot == ref_tot > 0


def test_flat_space_pan(dev):
    frames, scenes = DB.pan("flat", T.W, T.H, 3)
    scenes = ad(scenes)
    assert F.kind_of(scenes[0].rs, scenes[0].r_obs, scenes[0].step) == 2  # kFlat
    for shade in SHADES.values():
        ctx = new_ctx(dev, disk=T.pose("flat")[3], **shade)
        got, tot = batch(ctx, dev, frames, scenes[0], WHOLE)  # one GeoScene for every frame
        ref, ref_tot, hits = singles(ctx, dev, frames, scenes, WHOLE, hits=True)
        got4, tot4 = batch(ctx, dev, frames, ad(scenes, True), WHOLE)
        ref4, ref_tot4 = ss_refs(ctx, dev, frames, scenes, WHOLE)
        ctx.close()
        assert all((hh[..., 0, 0] > 0).sum() > 300 for hh in hits)
        assert np.array_equal(got, flat(ref)) and tot == ref_tot > 0
        assert np.array_equal(got4, ref4) and tot4 == ref_tot4 > 0
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


# ---- 5. frame stride and padding ------------------------------------------------------------
@pytest.mark.parametrize("ss", [False, True], ids=["one-sample", "ss4"])
def test_frame_stride_and_padding(dev, ss):
    frames, scenes = orbit(RAGGED[0], RAGGED[1], 3)
    w, h = RAGGED[:2]
    _, nrows, packed = dims(RAGGED)
    stride = packed + 4 * 37
    ctx = new_ctx(dev)
    got, _ = batch(ctx, dev, frames, ad(scenes, ss), RAGGED, stride=stride)
    ref = ss_refs(ctx, dev, frames, scenes, RAGGED)[0] if ss else flat(singles(ctx, dev, frames, scenes, RAGGED)[0])
    ctx.close()
    assert np.array_equal(got[:, :packed], ref)
    assert (got[:, packed:] == FILL).all()  # the gap keeps its prefill
    assert nrows > h and (got[:, h * w * 4:packed] == FILL).all()  # rows past the frame are not written
    assert not (ref[:, :h * w * 4] == FILL).all()


# ---- 6. steps and dispatch --------------------------------------------------------------------
@pytest.mark.parametrize("ss", [False, True], ids=["one-sample", "ss4"])
def test_deferred_steps_orders_and_timing(dev, ss):
    import torch

    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    lay = PEER
    frames, scenes = orbit(lay[0], lay[1], N)
    sc = ad(scenes, ss)
    ctx = new_ctx(dev, em=TE.emission())
    ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    ref, ref_tot = ss_refs(ctx, dev, frames, scenes, lay) if ss else singles(ctx, dev, frames, scenes, lay)[:2]
    ref = ref if ss else flat(ref)
    got, tot = batch(ctx, dev, frames, sc, lay)
    assert np.array_equal(got, ref) and tot == ref_tot > 0
    # GEO_FLAG_DEFER_STEPS and geo_steps_flush; steps_total NULL without it
    got, none = batch(ctx, dev, frames, ad(scenes, ss, flags=GEO_FLAG_DEFER_STEPS), lay, total=False)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.steps_flush(tot)
    torch.cuda.synchronize()
    assert none is None and np.array_equal(got, ref) and int(tot.item()) == ref_tot
    got, none = batch(ctx, dev, frames, sc, lay, total=False)
    assert none is None and np.array_equal(got, ref)
    # the learned order, period 1: the same bytes while the statistics advance
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


# ---- 7. refusals ------------------------------------------------------------------------------------
def test_refusals(dev):
    import torch

    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    lay = WHOLE
    w, h = lay[:2]
    nb, nrows, packed = dims(lay)
    n = 4
    frames, scenes = orbit(w, h, n)
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

    def one_frame(ctx, scene, f=0):
        """Frame f alone: the one-frame adaptive disk render, or (another mode) geo_render_band_set."""
        o = torch.full((packed,), FILL, dtype=torch.uint8, device=dev)
        if scene.mode == A_ and scene.flags & D_:
            ctx.render_disk_adaptive(frames[f], scene, w, h, lay[2], lay[3], lay[4], nb, o)
        else:
            ctx.render_band_set(frames[f], scene, w, h, lay[2], lay[3], lay[4], nb, o)
        torch.cuda.synchronize()
        return o.cpu().numpy()

    # no sky, no disk
    for kw in (dict(sky=False), dict(disk=None)):
        ctx = new_ctx(dev, **kw)
        assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched(), kw
        assert raw(ctx, frames, ad(scenes, True), lay, out) == GEO_ESTATE and untouched(), kw
        ctx.close()

    ctx = new_ctx(dev, em=TE.emission())
    ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    direct_disk, plain_adaptive = sc(mode=GEO_MODE_DIRECT), sc(flags=0)
    before = [one_frame(ctx, s) for s in (direct_disk, plain_adaptive, ok)]
    ss = D_ | GEO_FLAG_SS4
    cases = {
        "direct": [sc(j, mode=GEO_MODE_DIRECT) for j in range(n)],
        "fan": [sc(j, mode=GEO_MODE_FAN) for j in range(n)],
        "one direct scene": with_scene(2, sc(2, mode=GEO_MODE_DIRECT)),
        "no disk flag": [sc(j, flags=0) for j in range(n)],
        "ss4 without the disk flag": [sc(j, flags=GEO_FLAG_SS4) for j in range(n)],
        "one scene without the flag": with_scene(2, sc(2, flags=0)),
        "mips": [sc(j, flags=D_ | GEO_FLAG_MIPS) for j in range(n)],
        "composite": [sc(j, flags=D_ | GEO_FLAG_COMPOSITE) for j in range(n)],
        "disk | ring_f64": [sc(j, flags=D_ | GEO_FLAG_RING_F64) for j in range(n)],
        "ss4 mips": [sc(j, flags=ss | GEO_FLAG_MIPS) for j in range(n)],
        "ss4 on one frame only": with_scene(2, sc(2, flags=ss)),
        "ss4 on all frames but one": [sc(j, flags=ss if j != 1 else D_) for j in range(n)],
        "tol differs": with_scene(1, sc(1, tol=1e-5)),
        "step differs": with_scene(1, sc(1, step=ok.step * 0.5)),
        "max_steps differs": with_scene(1, sc(1, max_steps=ok.max_steps - 1)),
        "rs differs": with_scene(1, sc(1, rs=0.9)),
        "sphere_r differs": with_scene(1, sc(1, sphere_r=49.0)),
        "mixed kinds: a later frame inside the horizon": with_scene(3, sc(3, r_obs=0.9)),
        "a later frame outside the sphere": with_scene(3, sc(3, r_obs=50.0)),
        "tol negative": [sc(j, tol=-1e-6) for j in range(n)],
        "tol infinite": [sc(j, tol=float("inf")) for j in range(n)],
        "tol nan": [sc(j, tol=float("nan")) for j in range(n)],
    }
    for name, bad in cases.items():
        assert raw(ctx, frames, bad, lay, out) == GEO_EINVAL, name
        assert untouched(), name
    assert raw(ctx, frames, scenes, lay, out, n=0) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, n=N + 1) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, stride=packed - 4) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, scenes, lay, out, stride=packed + 2) == GEO_EINVAL and untouched()
    # each of the three armed per-pixel buffers: consumed by the refused call, one sample and
    # SS4; the next good call writes nothing to them.  The refused timing pair is dropped too.
    one = torch.full((packed,), FILL, dtype=torch.uint8, device=dev)
    hb = torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=dev)
    gb = torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=dev)
    qb = torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=dev)
    arms = ((ctx.disk_hits_next_render, hb), (ctx.disk_shift_next_render, gb), (ctx.disk_emission_next_render, qb))
    for s4 in (False, True):
        for arm, buf in arms:
            arm(buf)
            e0, e1 = HipEvent(), HipEvent()
            ctx.time_next_render(e0, e1)
            assert raw(ctx, frames, ad(scenes, s4), lay, out) == GEO_EINVAL and untouched()
            one.fill_(FILL)
            ctx.render_disk_adaptive(frames[0], scenes[0], w, h, lay[2], lay[3], lay[4], nb, one)
            torch.cuda.synchronize()
            assert bool((buf == -1.0).all()) and not bool((one == FILL).all())
            never_recorded(e0, e1)
    # the shading needs circular orbits down to the inner edge: r_in > 1.5 rs, emission or shift
    ctx.set_disk(T.TEX, 1.5, 2.2, DISK[2], DISK[3])
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    ctx.clear_disk_emission()
    ctx.set_disk_shift(1, 4, 1.0)
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    ctx.clear_disk_shift()
    assert raw(ctx, frames, scenes, lay, out) == GEO_OK  # unshaded, that disk is drawn
    torch.cuda.synchronize()
    assert not bool((out[:n * packed] == 0x5A).all())
    out.fill_(0x5A)
    ctx.set_disk(T.TEX, *DISK)
    spin, profile, t_ref, t_lo, t_hi, exposure = TE.emission()
    ctx.set_disk_emission(TE.RAMP, t_ref, t_lo, t_hi, profile, exposure, spin)
    # the ring state on with rs > 0: refused, one sample and SS4
    ctx.set_disk_ring_f64(True)
    assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, ad(scenes, True), lay, out) == GEO_EINVAL and untouched()
    ctx.set_disk_ring_f64(False)
    # the older calls still refuse the adaptive disk scene, and geo_render_disk_adaptive SS4
    s4 = ad(scenes, True)
    for fn, scs in ((lib.geo_render_disk_batch, scenes), (lib.geo_render_ss_batch, s4),
                    (lib.geo_render_emission_batch, scenes), (lib.geo_render_emission_batch, s4),
                    (lib.geo_render_disk_ring_batch, scenes), (lib.geo_render_disk_ring_batch, s4),
                    (lib.geo_render_band_set_batch, scenes), (lib.geo_render_band_set_batch, s4)):
        assert raw(ctx, frames, scs, lay, out, fn=fn) == GEO_EINVAL and untouched(), fn.__name__
    fa, sa = (GeoFrame * 1)(frames[0]), (GeoScene * 1)(s4[0])
    assert lib.geo_render_disk_adaptive(ctx._h, fa, sa, w, h, lay[2], lay[3], lay[4], nb, out.data_ptr(), None, None,
                                        None, None, None) == GEO_EINVAL and untouched()
    # what was drawn before the refusals is drawn again, byte for byte
    after = [one_frame(ctx, s) for s in (direct_disk, plain_adaptive, ok)]
    for a, b in zip(before, after):
        assert np.array_equal(a, b) and not (a == FILL).all()
    assert not np.array_equal(before[0], before[2]) and not np.array_equal(before[1], before[2])
    ctx.close()


@pytest.mark.parametrize("ss", [False, True], ids=["one-sample", "ss4"])
def test_ring_state_is_ignored_without_a_capture_orbit(dev, ss):
    """rs == 0: GEO_OK with geo_set_disk_ring_f64 on, and the bytes of the state off."""
    frames, scenes = DB.pan("flat", T.W, T.H, 3)
    sc = ad(scenes, ss)
    ctx = new_ctx(dev, disk=T.pose("flat")[3], shift=(1, 4, 1.0))
    off, off_tot = batch(ctx, dev, frames, sc, WHOLE)
    ctx.set_disk_ring_f64(True)
    on, on_tot = batch(ctx, dev, frames, sc, WHOLE)  # (raises unless GEO_OK)
    ctx.close()
    assert np.array_equal(on, off) and on_tot == off_tot > 0
    assert not (off[:, :T.W * T.H * 4] == FILL).all()


# ---- 8. fuzz ----------------------------------------------------------------------------------------------
def test_fuzzed_batches(dev):
    """test_gpu_disk_fuzz.py's BATCH_SEEDS through fuzz_disk_scenes.disk_batch
    with the mode switched to adaptive: unshaded, the seed's shift and
    TE.emission(), one sample and SS4; every frame against its one-frame render
    (SS4: the resolve), and the totals."""
    w, h = 64, 36
    lay = (w, h, 8, 0, 8)
    TOLS = (0.0, 1e-4, 1e-5, 1e-7)
    kinds, launched, slot0, slot1 = set(), 0, 0, 0
    for i, seed in enumerate(GF.BATCH_SEEDS):
        n = 2 + (5 * i) % 7
        frames, scenes, disk_args, shift, desc = F.disk_batch(seed, w, h, n)
        scenes = ad(scenes, tol=TOLS[i % 4])
        desc += f" adaptive tol={TOLS[i % 4]}"
        kinds.add(F.kind_of(scenes[0].rs, scenes[0].r_obs, scenes[0].step))
        for name, shade in (("plain", dict()), ("shift", dict(shift=shift)), ("emission", dict(em=TE.emission()))):
            ctx = new_ctx(dev, disk=disk_args, **shade)
            try:
                got, tot = batch(ctx, dev, frames, scenes, lay)
                ref, ref_tot, hits = singles(ctx, dev, frames, scenes, lay, hits=name == "plain")
                got4, tot4 = batch(ctx, dev, frames, ad(scenes, True, tol=TOLS[i % 4]), lay)
                ref4, ref_tot4 = ss_refs(ctx, dev, frames, scenes, lay)
            finally:
                ctx.close()
            ref = flat(ref)
            for f in range(n):
                for what, g_, r_ in (("one sample", got, ref), ("ss4", got4, ref4)):
                    diff = g_[f] != r_[f]
                    assert not diff.any(), (desc, name, what, f"frame {f}", f"{int(diff.sum())} bytes, first at pixel "
                                            f"{int(np.argwhere(diff)[0][0]) // 4}")
            assert tot == ref_tot and tot4 == ref_tot4, (desc, name, tot, ref_tot, tot4, ref_tot4)
            launched += 2 * n
            if name == "plain":
                slot0 += sum(int((hh[..., 0, 0] > 0).sum()) for hh in hits)
                slot1 += sum(int((hh[..., 1, 0] > 0).sum()) for hh in hits)
    print(f"fuzzed adaptive batches: {launched} batched frames compared, kinds {sorted(kinds)}, slot-0 hits {slot0}, "
          f"slot-1 hits {slot1}")
    assert kinds == {0, 1, 2}
    assert slot0 > 20_000 and slot1 > 400, (slot0, slot1)


# ---- 9. the pipeline ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", [False, True], ids=["one-sample", "ss4"])
@pytest.mark.parametrize("batch_launch", [True, False], ids=["batched", "per-frame"])
@pytest.mark.parametrize("name", ["plain", "emission"])
def test_pipeline(dev, name, batch_launch, ss):
    import torch

    from schwarzschild_raytracer_wgpu_amd.dist import ShardedFrame

    w, h, nsteps = 160, 96, 8
    frames, scenes = orbit(w, h, nsteps)
    sc = ad(scenes, ss)
    ctx = new_ctx(dev, **SHADES[name])
    sf = ShardedFrame(ctx, frames[0], sc[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=batch_launch)
    assert sf.batch == batch_launch and sf.K == (4 if batch_launch else 1)
    # render_disk_adaptive's frames: the render itself, or (SS4) the resolve of the render of twice the size
    k = 2 if ss else 1
    refs = []
    for f, s in zip(frames, scenes):
        one = torch.zeros(k * k * h * w * 4, dtype=torch.uint8, device=dev)
        ctx.render_disk_adaptive(f, s, k * w, k * h, k * h, 0, k * h, 1, one)
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
    assert retired == nsteps == sf.frames_done
    assert not np.array_equal(refs[0], refs[1])
    # while the ring state is on such a scene is refused by name, by a new object and by this one
    ctx.set_disk_ring_f64(True)
    with pytest.raises(ValueError, match="set_disk_ring_f64"):
        ShardedFrame(ctx, frames[0], sc[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=batch_launch)
    with pytest.raises(ValueError, match="set_disk_ring_f64"):
        for i in range(sf.K):  # (a batch renders at its K-th frame)
            sf.step(i, frame=frames[i], scene=sc[i])
    ctx.close()
