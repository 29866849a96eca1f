"""geo_render_emission_batch: up to GEO_MAX_BATCH_FRAMES frames of the
blackbody disk (geo_set_disk_emission) in one launch
(geo_render_disk_batch_kernel with Shade::kDiskEmit, one sample or
GEO_FLAG_SS4; the frame in blockIdx.z) draw, frame by frame, the bytes
geo_render_band_set draws for that frame and scene alone, and the bytes of the
CPU path (geo_render_cpu_disk_emission, the same header csrc/geo_disk.h); the
C-ABI's rules (geo.h) and dist.ShardedFrame's emission_batch routing.  The
scenes, layouts and helpers are tests/test_gpu_disk_batch.py's."""
import numpy as np
import pytest

import test_disk_cpu as T
import test_disk_emission_cpu as X
import test_gpu_disk_batch as DB
from fuzz_disk_scenes import disk_batch, disk_scene
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_ESTATE, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4,
                                                   GEO_MAX_BATCH_FRAMES, GEO_MODE_ADAPTIVE, GEO_MODE_FAN, GEO_OK,
                                                   GeoFrame, GeoScene, lib)
from test_gpu_disk_batch import DISK, FILL, PEER, RAGGED, WHOLE, dims, orbit, pan, singles
from test_gpu_disk_emission import EM, set_emission, ss_of
from test_gpu_disk_fuzz import BATCH_SEEDS

pytestmark = pytest.mark.gpu

SHIFT = (1, 4, 1.0)
EM_POWER = X.emission(X.POWER, exposure=0.5)
EM_BACK = X.emission(X.THIN, exposure=2.0, spin=-1)  # EM with the disk turning the other way


def flags_of(ss):
    return GEO_FLAG_DISK | (GEO_FLAG_SS4 if ss else 0)


def ss_all(scenes, ss):
    return [ss_of(s) for s in scenes] if ss else list(scenes)


def new_ctx(dev, disk=DISK, em=EM, ramp=X.RAMP, shift=None):
    ctx = DB.new_ctx(dev, disk=disk, shift=shift)
    if em is not None:
        set_emission(ctx, em, ramp)
    return ctx


def batch(ctx, dev, frames, scenes, lay, stride=None, total=True):
    """The batch through Context.render_emission_batch: (bytes per frame slot, steps)."""
    import torch

    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    n = len(frames)
    stride = packed if stride is None else stride
    out = torch.full((n * stride,), FILL, dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev) if total else None
    ctx.render_emission_batch(frames, scenes, w, h, br, row0, rstride, nb, out, frame_stride=stride, steps_total=tot)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, stride), (int(tot.item()) if total else None)


def raw(ctx, frames, scenes, lay, out, stride=None, n=None, fn=None):
    w, h, br, row0, rstride = lay
    nb, _, packed = dims(lay)
    fa, sa = (GeoFrame * len(frames))(*frames), (GeoScene * len(scenes))(*scenes)
    fn = lib.geo_render_emission_batch if fn is None else fn
    return fn(ctx._h, fa, sa, len(frames) if n is None else n, w, h, br, row0, rstride, nb, out.data_ptr(),
              packed if stride is None else stride, None, None)


@pytest.fixture(scope="module")
def cpu():
    return X.load_cpu()


@pytest.fixture(scope="module")
def peer8(dev):
    """The 8-frame orbit on the peer layout, every frame alone, rendered once:
    the emission frames (plain and SS4) and their steps."""
    frames, scenes = orbit(PEER[0], PEER[1], GEO_MAX_BATCH_FRAMES)
    ctx = new_ctx(dev)
    out = {}
    for ss in (False, True):
        ref, tot, _ = singles(ctx, dev, frames, ss_all(scenes, ss), PEER)
        ref.setflags(write=False)
        out[ss] = (ref, tot)
    ctx.close()
    return frames, scenes, out


@pytest.fixture(scope="module")
def others(dev):
    """What the emission frames must differ from: the same orbit frames
    unshaded and shaded (geo_set_disk_shift), every frame alone."""
    out = {}
    for lay in (PEER, RAGGED):
        frames, scenes = orbit(lay[0], lay[1], GEO_MAX_BATCH_FRAMES)
        for ss in (False, True):
            sc = ss_all(scenes, ss)
            ctx = new_ctx(dev, em=None)
            plain, _, _ = singles(ctx, dev, frames, sc, lay)
            ctx.set_disk_shift(*SHIFT)
            shaded, _, _ = singles(ctx, dev, frames, sc, lay)
            ctx.close()
            out[lay, ss] = (plain, shaded)
    return out


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
@pytest.mark.parametrize("lay", [PEER, RAGGED], ids=["peer", "ragged"])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_batch_equals_single_frames(dev, others, lay, n, ss):
    frames, scenes = orbit(lay[0], lay[1], n)
    assert len({s.r_obs for s in scenes}) == n  # every frame its own radius
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev)
    got, tot = batch(ctx, dev, frames, sc, lay)
    ref, ref_tot, _ = singles(ctx, dev, frames, sc, lay)
    # the hits of the one-frame emission render (one sample per pixel: SS4 draws colour only)
    _, _, hits = singles(ctx, dev, frames, scenes, lay, hits=True)
    ctx.close()
    plain, shaded = others[lay, ss]
    for f in range(n):
        s0, s1 = int((hits[f][..., 0, 0] > 0).sum()), int((hits[f][..., 1, 0] > 0).sum())
        print(f"n={n} ss={ss} frame {f}: slot-0 hits {s0}, slot-1 hits {s1}, "
              f"differing bytes {int((got[f] != ref[f]).sum())}")
        assert s0 > 300 and s1 > 0, (f, s0, s1)
        assert np.array_equal(got[f], ref[f]), f
        # (the orbit's first n frames are the same for every n)
        assert not np.array_equal(ref[f], plain[f]) and not np.array_equal(ref[f], shaded[f]), f
        if f:
            assert not np.array_equal(ref[f], ref[f - 1]), f
    assert tot == ref_tot > 0


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_against_the_cpu_path(dev, cpu, ss):
    w, h = WHOLE[:2]
    n = GEO_MAX_BATCH_FRAMES
    frames, scenes = orbit(w, h, n)
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev)
    got, _ = batch(ctx, dev, frames, sc, WHOLE)
    ctx.close()
    for f in (0, n - 1):
        rc, c = X.render(cpu, frames[f], sc[f], w, h, T.make_disk(*DISK), em=EM, outputs=not ss)
        assert rc == GEO_OK
        assert np.array_equal(got[f][:h * w * 4].reshape(h, w, 4), c["rgba"]), f
        assert (got[f][h * w * 4:] == FILL).all()  # the clipped rows of the last band
    assert not np.array_equal(got[0], got[n - 1])


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_profiles_and_ramp_sizes(dev, peer8, ss):
    """Both profiles, and ramps of 2, 256 and 1024 entries (n - 2 = 0 is the
    edge of the entry clamp)."""
    frames, scenes, refs = peer8
    frames, sc = frames[:3], ss_all(scenes[:3], ss)
    ramps = {"2": X.ramps()["2"], "256": X.blackbody_ramp(256, X.T_LO, X.T_HI), "1024": X.ramps()["1024"]}
    outs = {}
    for em_name, em in (("thin", EM), ("power", EM_POWER)):
        for ramp_name, ramp in ramps.items():
            ctx = new_ctx(dev, em=em, ramp=ramp)
            got, tot = batch(ctx, dev, frames, sc, PEER)
            ref, ref_tot, _ = singles(ctx, dev, frames, sc, PEER)
            ctx.close()
            assert np.array_equal(got, ref) and tot == ref_tot, (em_name, ramp_name)
            outs[em_name, ramp_name] = got
    keys = list(outs)
    for i, a in enumerate(keys):
        assert not np.array_equal(outs[a], refs[ss][0][:3]), a  # (peer8's ramp has 64 entries)
        for b in keys[i + 1:]:
            assert not np.array_equal(outs[a], outs[b]), (a, b)


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_spin_is_the_emissions(dev, peer8, ss):
    """While geo_set_disk_shift is set too, the emission takes its place, spin
    included: the shift turns one way, the emission the other."""
    frames, scenes, refs = peer8
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev, em=EM_BACK, shift=(1, 4, 1.0))
    got, tot = batch(ctx, dev, frames, sc, PEER)
    ref, ref_tot, _ = singles(ctx, dev, frames, sc, PEER)
    ctx.close()
    assert np.array_equal(got, ref) and tot == ref_tot
    # the spin +1 emission batch, with the same shift under it: peer8's frames, and not these
    ctx = new_ctx(dev, em=EM, shift=(1, 4, 1.0))
    fwd, _ = batch(ctx, dev, frames, sc, PEER)
    ctx.close()
    assert np.array_equal(fwd, refs[ss][0])
    assert not np.array_equal(got, fwd)


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_frame_stride_and_padding(dev, ss):
    frames, scenes = orbit(RAGGED[0], RAGGED[1], 3)
    sc = ss_all(scenes, ss)
    w, h = RAGGED[:2]
    _, nrows, packed = dims(RAGGED)
    stride = packed + 4 * 37
    ctx = new_ctx(dev)
    got, _ = batch(ctx, dev, frames, sc, RAGGED, stride=stride)
    ref, _, _ = singles(ctx, dev, frames, sc, RAGGED)
    ctx.close()
    assert np.array_equal(got[:, :packed], ref)
    assert (got[:, packed:] == FILL).all()  # the gap keeps its prefill
    assert nrows > h and (got[:, h * w * 4:packed] == FILL).all()  # rows past the frame are not written
    assert not (ref[:, :h * w * 4] == FILL).all()


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_deferred_steps(dev, peer8, ss):
    import torch

    frames, scenes, refs = peer8
    ref, ref_tot = refs[ss]
    ctx = new_ctx(dev)
    deferred = [make_scene(s.rs, s.sphere_r, s.r_obs, s.step, s.max_steps, 0, flags_of(ss) | GEO_FLAG_DEFER_STEPS)
                for s in scenes]
    got, none = batch(ctx, dev, frames, deferred, PEER, total=False)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.steps_flush(tot)
    torch.cuda.synchronize()
    ctx.close()
    assert none is None and np.array_equal(got, ref)
    assert int(tot.item()) == ref_tot


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_learned_dispatch_order(dev, peer8, ss):
    frames, scenes, refs = peer8
    ref, ref_tot = refs[ss]
    sc = ss_all(scenes, ss)
    ctx = new_ctx(dev)
    ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    got, tot = batch(ctx, dev, frames, sc, PEER)
    assert np.array_equal(got, ref) and tot == ref_tot
    ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        got, tot = batch(ctx, dev, frames, sc, PEER)
        assert np.array_equal(got, ref) and tot == ref_tot, i
    rec, _ = ctx.dispatch_stats()
    ctx.close()
    assert rec >= 1


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_time_next_render(dev, peer8, ss):
    import torch

    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    frames, scenes, refs = peer8
    ctx = new_ctx(dev)
    e0, e1 = HipEvent(), HipEvent()
    ctx.time_next_render(e0, e1)
    got, _ = batch(ctx, dev, frames, ss_all(scenes, ss), PEER)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)  # raises unless both were recorded
    ctx.close()
    assert ms > 0.0 and np.array_equal(got, refs[ss][0])


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

    # no emission set, then no disk
    ctx = new_ctx(dev, em=None)
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    assert raw(ctx, frames, ss_all(scenes, True), lay, out) == GEO_ESTATE and untouched()
    set_emission(ctx, EM)
    ctx.clear_disk()  # (drops the emission with the disk)
    assert raw(ctx, frames, scenes, lay, out) == GEO_ESTATE and untouched()
    ctx.close()

    ctx = new_ctx(dev)
    ctx.set_fan(np.linspace(1.0, -1.0, 16, dtype=np.float32))
    cases = {
        "adaptive": [sc(j, mode=GEO_MODE_ADAPTIVE) for j in range(n)],
        "fan": [sc(j, mode=GEO_MODE_FAN) for j in range(n)],
        "mips": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_MIPS) for j in range(n)],
        "composite": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_COMPOSITE) for j in range(n)],
        "ring": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_RING_F64) for j in range(n)],
        "ss4 mips": [sc(j, flags=GEO_FLAG_DISK | GEO_FLAG_SS4 | GEO_FLAG_MIPS) for j in range(n)],
        "no disk flag": [sc(j, flags=0) for j in range(n)],
        "ss4 without the disk flag": [sc(j, flags=GEO_FLAG_SS4) for j in range(n)],
        "one scene without the flag": with_scene(2, sc(2, flags=0)),
        "ss4 on one frame only": with_scene(2, sc(2, flags=GEO_FLAG_DISK | GEO_FLAG_SS4)),
        "ss4 on all frames but one": [sc(j, flags=flags_of(j != 1)) for j in range(n)],
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
    # each of the three armed per-pixel buffers: consumed by the refused call, plain and SS4
    one = torch.full((packed,), FILL, dtype=torch.uint8, device=dev)
    hb = torch.full((nrows * w * 6,), -1.0, dtype=torch.float32, device=dev)
    gb = torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=dev)
    qb = torch.full((nrows * w * 3,), -1.0, dtype=torch.float32, device=dev)
    arms = ((ctx.disk_hits_next_render, hb), (ctx.disk_shift_next_render, gb), (ctx.disk_emission_next_render, qb))
    for ss in (False, True):
        for arm, buf in arms:
            arm(buf)
            assert raw(ctx, frames, ss_all(scenes, ss), lay, out) == GEO_EINVAL and untouched()
            one.fill_(FILL)
            ctx.render_band_set(frames[0], scenes[0], w, h, lay[2], lay[3], lay[4], nb, one)
            torch.cuda.synchronize()
            assert bool((buf == -1.0).all()) and not bool((one == FILL).all())
    # the emission needs circular orbits down to the inner edge: r_in > 1.5 rs
    for r_in in (1.4, 1.5):
        ctx.set_disk(T.TEX, r_in, 2.2, DISK[2], DISK[3])
        assert raw(ctx, frames, scenes, lay, out) == GEO_EINVAL and untouched(), r_in
    ctx.set_disk(T.TEX, *DISK)
    # a good call draws; the older batched calls keep refusing while the emission is set
    assert raw(ctx, frames, scenes, lay, out) == GEO_OK
    torch.cuda.synchronize()
    assert not bool((out[:n * packed] == FILL).all())
    out.fill_(FILL)
    assert raw(ctx, frames, scenes, lay, out, fn=lib.geo_render_disk_batch) == GEO_EINVAL and untouched()
    assert raw(ctx, frames, ss_all(scenes, True), lay, out, fn=lib.geo_render_ss_batch) == GEO_EINVAL and untouched()
    ctx.close()


def test_seeded_family(dev):
    import torch

    rng = np.random.default_rng(20261020)
    sizes = [(64, 40), (100, 37), (96, 54)]
    disks = [(1.6, 2.2), (3.0, 9.0)]
    normals = [(0.0, 0.0, 1.0), (0.3, -0.2, 1.0)]
    profiles = [EM, EM_POWER]
    ctx = new_ctx(dev, disk=None, em=None)
    ran, drawn, differing = 0, 0, 0
    while ran < 12:
        drawn += 1
        assert drawn < 200
        n = int(rng.integers(1, GEO_MAX_BATCH_FRAMES + 1))
        w, h = sizes[int(rng.integers(3))]
        lay = (w, h, 8, 0, 8) if rng.integers(2) else (w, h, 8, 8, 24)
        frames, scenes = orbit(w, h, n) if rng.integers(2) else pan("flat", w, h, n)
        r_in, r_out = disks[int(rng.integers(2))]
        ctx.set_disk(T.TEX, r_in, r_out, normals[int(rng.integers(2))], (1.0, 0.0, 0.0))
        em = profiles[int(rng.integers(2))]
        set_emission(ctx, em)
        ss = bool(rng.integers(2))
        sc = ss_all(scenes, ss)
        _, _, packed = dims(lay)
        probe = torch.full((n * packed,), FILL, dtype=torch.uint8, device=dev)
        rc = raw(ctx, frames, sc, lay, probe)
        if rc == GEO_EINVAL:  # a draw the rules refuse: drawn again, not skipped
            continue
        assert rc == GEO_OK
        got, tot = batch(ctx, dev, frames, sc, lay)
        ref, ref_tot, _ = singles(ctx, dev, frames, sc, lay)
        d = int((got != ref).sum())
        print(f"batch {ran}: n={n} {w}x{h} row0={lay[3]} stride={lay[4]} rs={scenes[0].rs} ss4={ss} "
              f"profile={em[1]} disk={r_in}..{r_out}: {d} bytes differ")
        differing += d
        assert tot == ref_tot
        ran += 1
    ctx.close()
    assert ran == 12 and differing == 0


def test_fuzzed_batches(dev):
    """fuzz_disk_scenes.disk_batch's seeds (2..8 frames, the camera turning,
    the observer drifting) with the seed's own emission and ramp, plain and
    SS4: every frame is its one-frame render."""
    w, h = 64, 36
    lay = (w, h, 8, 0, 8)
    launched = 0
    for i, seed in enumerate(BATCH_SEEDS):
        n = 2 + (5 * i) % 7
        frames, scenes, disk_args, _, desc = disk_batch(seed, w, h, n)
        em, ramp = disk_scene(seed, w, h)[4]
        ctx = new_ctx(dev, disk=disk_args, em=em, ramp=ramp)
        try:
            for ss in (False, True):
                sc = ss_all(scenes, ss)
                got, tot = batch(ctx, dev, frames, sc, lay)
                ref, ref_tot, _ = singles(ctx, dev, frames, sc, lay)
                for f in range(n):
                    diff = got[f] != ref[f]
                    assert not diff.any(), (desc, "ss4" if ss else "plain", f"frame {f}",
                                            f"{int(diff.sum())} bytes, first at pixel {int(np.argwhere(diff)[0][0]) // 4}")
                assert tot == ref_tot, (desc, ss, tot, ref_tot)
                launched += n
        finally:
            ctx.close()
    print(f"fuzzed emission batches: {launched} batched frames compared with their one-frame renders")


@pytest.mark.parametrize("ss", [False, True], ids=["plain", "ss4"])
def test_pipeline(dev, ss):
    import torch

    from schwarzschild_raytracer_wgpu_amd.dist import ShardedFrame

    w, h, nsteps = 160, 96, 8
    frames, scenes = orbit(w, h, nsteps)
    scenes = ss_all(scenes, ss)
    ctx = new_ctx(dev)
    with pytest.raises(ValueError, match="set_disk_emission.*emission_batch"):
        ShardedFrame(ctx, frames[0], scenes[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=True)
    sf = ShardedFrame(ctx, frames[0], scenes[0], w, h, 8, 0, 1, dev, frames_per_gather=4, batch_launch=True,
                      emission_batch=True)
    assert sf.batch and sf.K == 4

    def one_frame_refs():
        refs = []
        for f, s in zip(frames, scenes):
            ref = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
            ctx.render_rows(f, s, w, h, 0, h, ref)
            refs.append(ref)
        return refs

    def run(first, refs):
        retired = 0
        for i in range(nsteps):
            sf.step(first + i, frame=frames[i], scene=scenes[i])
            if i % sf.K == sf.K - 1:
                # the batch just launched, retired: its last frame, and every slot of its buffer
                sf.drain()
                torch.cuda.synchronize()
                assert torch.equal(sf.frame_rgba(), refs[i]), i
                for j in range(i - sf.K + 1, i + 1):
                    assert torch.equal(sf.local_view(first + j)[:h * w * 4], refs[j]), j
                    retired += 1
        sf.drain()
        torch.cuda.synchronize()
        return retired

    emission = one_frame_refs()
    assert run(0, emission) == nsteps == sf.frames_done
    assert not torch.equal(emission[0], emission[1])
    # the same object with the emission cleared still draws the disk batch (the SS4 batch) without it
    ctx.clear_disk_emission()
    plain = one_frame_refs()
    assert not torch.equal(plain[0], emission[0])
    assert run(nsteps, plain) == nsteps and sf.frames_done == 2 * nsteps
    ctx.close()
