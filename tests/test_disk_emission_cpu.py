"""Blackbody emission of the thin disk on the CPU path
(geo_render_cpu_disk_emission, include/geo/geo_cpu.h; csrc/geo_disk.h):
q = T_obs / t_ref against closed forms in flat space, against the f64
restatement tests/disk_emission_ref.py in curved space, the colour step against
a numpy restatement, beaming as a colour difference, scenes.blackbody_ramp
against its known chromaticities, GEO_FLAG_SS4 and the argument rules.
tests/test_gpu_disk_emission.py ties the kernels to this path bit for bit."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import disk_emission_ref as E
import disk_ref as D
import test_disk_cpu as T
import test_disk_shift_cpu as TS
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import _lib, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_EINVAL, GEO_FLAG_COMPOSITE, GEO_FLAG_DISK, GEO_FLAG_MIPS,
                                                   GEO_FLAG_RING_F64, GEO_FLAG_SS4, GEO_MODE_ADAPTIVE, GEO_MODE_FAN,
                                                   GEO_OK, GeoDiskEmission)
from schwarzschild_raytracer_wgpu_amd.scenes import blackbody_ramp, blackbody_xyz

W, H = T.W, T.H
POWER, THIN = E.POWER, E.THIN
T_REF, T_LO, T_HI = 6000.0, 1500.0, 24000.0
RAMP = blackbody_ramp(64, T_LO, T_HI)
WHITE = np.full((2, 4, 4), 255, np.uint8)


def load_cpu():
    lib = TS.load_cpu()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.geo_render_cpu_disk_emission.restype = ctypes.c_int
    lib.geo_render_cpu_disk_emission.argtypes = [vp, vp, vp, u32, u32, vp, u32, u32, u32, u32, u32, u32, ctypes.c_int,
                                                 vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, u32, vp, vp]
    return lib


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


def emission(profile=THIN, t_ref=T_REF, t_lo=T_LO, t_hi=T_HI, exposure=1.0, spin=1):
    return (spin, profile, t_ref, t_lo, t_hi, exposure)


def render(lib, frame, scene, w, h, disk, tex=T.TEX, em=emission(), ramp=RAMP, sky=T.SKY, threads=4, outputs=True):
    """geo_render_cpu_disk_emission over the whole frame; em = (spin, profile,
    t_ref, t_lo, t_hi, exposure) or None (the unshaded disk: out_g and out_q
    stay at their prefill -1).  outputs=False: colour only (GEO_FLAG_SS4)."""
    sky = np.ascontiguousarray(sky, dtype=np.uint8)
    tex = np.ascontiguousarray(tex, dtype=np.uint8)
    rgba = np.zeros((h, w, 4), np.uint8)
    mask = np.empty((h, w), np.uint8)
    uv = np.empty((h, w, 2), np.float32)
    steps = np.empty((h, w), np.uint32)
    total = ctypes.c_ulonglong()
    hits = np.full((h, w, 3, 2), -1.0, np.float32)
    g = np.full((h, w, 3), -1.0, np.float32)
    q = np.full((h, w, 3), -1.0, np.float32)
    e = None if em is None else GeoDiskEmission(*em)
    rmp = None if ramp is None else np.ascontiguousarray(ramp, dtype=np.uint8)
    p = (lambda a: a.ctypes.data) if outputs else (lambda a: None)
    rc = lib.geo_render_cpu_disk_emission(
        ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1], sky.shape[0], None, 0, w, h, 0,
        h, 1, threads, rgba.ctypes.data, p(mask), p(uv), p(steps), ctypes.addressof(total), ctypes.addressof(disk),
        tex.ctypes.data, tex.shape[1], tex.shape[0], p(hits), None if e is None else ctypes.addressof(e),
        None if rmp is None else rmp.ctypes.data, 0 if rmp is None else rmp.shape[0], p(g), p(q))
    return rc, dict(rgba=rgba, mask=mask, uv=uv, steps=steps, total=total.value, hits=hits, g=g, q=q)


def test_announced():
    hdr = open(os.path.join(T.ROOT, "include", "geo", "geo.h")).read()
    assert re.search(r"^#define GEO_HAS_DISK_EMISSION 1$", hdr, re.M)
    assert re.search(r"^#define GEO_ABI_VERSION 8\b", hdr, re.M)
    assert _lib.GEO_HAS_DISK_EMISSION == 1
    assert (_lib.GEO_DISK_PROFILE_POWER, _lib.GEO_DISK_PROFILE_THIN, _lib.GEO_DISK_RAMP_MAX) == (0, 1, 1024)
    assert ctypes.sizeof(GeoDiskEmission) == 24
    # both symbols are exported (no GPU needed to look them up)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.geo_set_disk_emission and lib.geo_disk_emission_next_render
    assert _lib.lib.geo_abi_version() == 8


@pytest.mark.parametrize("name", ["A", "flat"])
def test_off_state(cpu, name):
    frame, scene, disk, _ = T.pose(name)
    rc, want = T.render(cpu, frame, scene, T.SKY, W, H, disk, T.TEX)
    assert rc == GEO_OK
    rc, a = render(cpu, frame, scene, W, H, disk, em=None, ramp=None)
    assert rc == GEO_OK and TS.same_frame(a, want)
    assert (a["hits"][..., 0] > 0.0).sum() > 500
    assert (a["g"] == -1.0).all() and (a["q"] == -1.0).all()


def test_argument_checks(cpu):
    frame, scene, disk, _ = T.pose("A")
    w, h = 16, 9
    frame = default_frame(w, h, pos=T.POSES["A"][0], camera=T.POSES["A"][1], fov=T.POSES["A"][2])

    def rc_of(sc, em=emission(), dk=disk, ramp=RAMP):
        return render(cpu, frame, sc, w, h, dk, em=em, ramp=ramp)[0]

    def sc(rs=1.0, mode=0, flags=GEO_FLAG_DISK):
        return make_scene(rs, 50.0, scene.r_obs, T.STEP, 256, mode, flags)

    assert rc_of(sc()) == GEO_OK
    for good in (emission(POWER, spin=-1), emission(exposure=3.0e38), emission(t_ref=1e-3)):
        assert rc_of(sc(), good) == GEO_OK
    inf, nan = math.inf, math.nan
    bad = [emission(spin=s) for s in (0, 2, -2)] + [emission(profile=2), emission(profile=0xFFFFFFFF)]
    for v in (0.0, -1.0, inf, nan):
        bad += [emission(t_ref=v), emission(t_lo=v), emission(t_hi=v), emission(exposure=v)]
    bad += [emission(t_lo=3000.0, t_hi=3000.0), emission(t_lo=3000.0, t_hi=2000.0)]
    for em in bad:
        assert rc_of(sc(), em) == GEO_EINVAL, em
    assert rc_of(sc(), ramp=None) == GEO_EINVAL
    for n in (1, 1025):
        assert rc_of(sc(), ramp=np.zeros((n, 4), np.uint8)) == GEO_EINVAL
    for n in (2, 1024):
        assert rc_of(sc(), ramp=np.zeros((n, 4), np.uint8)) == GEO_OK
    # circular orbits down to the inner edge: r_in > 1.5 rs at render time
    for r_in, rs in ((3.0, 2.0), (3.0, 2.5)):
        assert rc_of(sc(rs=rs), dk=T.make_disk(r_in, 9.0)) == GEO_EINVAL
        assert rc_of(sc(rs=rs), None, dk=T.make_disk(r_in, 9.0)) == GEO_OK
    assert rc_of(sc(rs=1.9999), dk=T.make_disk(3.0, 9.0)) == GEO_OK
    assert rc_of(sc(rs=0.0)) == GEO_OK
    # what the unshaded disk refuses stays refused
    assert rc_of(sc(flags=0)) == GEO_EINVAL
    for mode in (GEO_MODE_FAN, GEO_MODE_ADAPTIVE):
        assert rc_of(sc(mode=mode)) == GEO_EINVAL
    for fl in (GEO_FLAG_MIPS, GEO_FLAG_COMPOSITE, GEO_FLAG_RING_F64):
        assert rc_of(sc(flags=GEO_FLAG_DISK | fl)) == GEO_EINVAL
    # GEO_FLAG_SS4 is colour only
    assert rc_of(sc(flags=GEO_FLAG_DISK | GEO_FLAG_SS4)) == GEO_EINVAL
    assert render(cpu, frame, sc(flags=GEO_FLAG_DISK | GEO_FLAG_SS4), w, h, disk, outputs=False)[0] == GEO_OK


def test_flat_space_power(cpu):
    """g = 1 (flat space, a static observer): q = (r_in/r)^(3/4) against the f64 trace's radius."""
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose("flat")
    assert scene.rs == 0.0 and frame.psi_factor_and_position[0] == 0.0
    ref = D.trace(frame, scene, W, H, r_in, r_out, normal, axis)
    for spin in (1, -1):
        rc, a = render(cpu, frame, scene, W, H, disk, em=emission(POWER, spin=spin))
        assert rc == GEO_OK
        both = (a["hits"][..., 0, 0] > 0.0) & ref["hit"][..., 0]
        assert both.sum() > 1000
        assert (a["g"][a["hits"][..., 0] > 0.0] == np.float32(1.0)).all()
        want = (r_in / ref["r"][..., 0][both]) ** 0.75
        err = np.abs(a["q"][..., 0][both] / want - 1.0).max()
        print("flat POWER: hits", int(both.sum()), "max rel q", err)
        assert err <= E.TOL_Q_POWER
        assert np.array_equal(a["q"] != 0.0, a["hits"][..., 0] != 0.0)


def test_flat_space_thin(cpu):
    """g = 1: q = tau.  0 at the inner edge, at most 1, and its maximum at r = 49/36 r_in."""
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose("flat")
    rc, a = render(cpu, frame, scene, W, H, disk, em=emission(THIN))
    assert rc == GEO_OK
    hit = a["hits"][..., 0, 0] > 0.0
    r = a["hits"][..., 0, 0][hit].astype(np.float64)
    q = a["q"][..., 0][hit].astype(np.float64)
    assert hit.sum() > 1000
    assert q.max() <= 1.0 + E.TOL_Q_THIN and q.min() >= 0.0
    # the inner edge: tau rises from 0 with an infinite slope, so the innermost hit (0.08 % outside r_in) already
    # reads 0.29; it is tau of its own radius, and tau(r_in) = 0
    i0 = int(np.argmin(r))
    assert r[i0] < r_in * 1.002
    assert abs(q[i0] - E.tau(THIN, r_in, r[i0])) <= E.TOL_Q_THIN
    assert float(E.tau(THIN, r_in, r_in)) == 0.0
    # one pixel's radial extent at the maximum: the largest radius step between
    # horizontally or vertically neighbouring hits near r = 49/36 r_in
    rr = np.where(hit, a["hits"][..., 0, 0].astype(np.float64), np.nan)
    r_pk = 49.0 / 36.0 * r_in
    with np.errstate(invalid="ignore"):
        dx = np.abs(np.diff(rr, axis=1))
        dy = np.abs(np.diff(rr, axis=0))
        near = np.abs(rr - r_pk) < 0.1 * r_in  # both neighbours near the peak: no step across the disk's hole
        near_x = near[:, 1:] & near[:, :-1]
        near_y = near[1:, :] & near[:-1, :]
        extent = max(np.nanmax(np.where(near_x, dx, np.nan)), np.nanmax(np.where(near_y, dy, np.nan)))
    r_max = r[int(np.argmax(q))]
    print("flat THIN: hits", int(hit.sum()), "q max", q.max(), "at r", r_max, "peak", r_pk, "pixel extent", extent,
          "least q", q.min(), "at r", r[i0])
    assert abs(r_max - r_pk) <= extent
    # against the trace's radius, as the curved poses are compared
    ref = D.trace(frame, scene, W, H, r_in, r_out, normal, axis)
    s = E.compare(a["q"], a["hits"], ref, E.q_ref(frame, scene, W, H, ref, r_in, normal, axis, 1, THIN), THIN, r_in)
    print(s)
    assert s["max_err_q"] <= E.TOL_Q_THIN and s["strip_share"] < 0.05


STRIP_CAP = 0.05  # the inner-edge strip's share of the compared hits (the strip is 0.2 % and 1 % of the annuli)


@pytest.mark.parametrize("name", list(T.CURVED))
def test_against_f64_restatement(cpu, name):
    """q of every slot against disk_emission_ref (g by the photon's local
    direction, tau by powers), both spins, both profiles."""
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose(name)
    ref = D.trace(frame, scene, W, H, r_in, r_out, normal, axis)
    for profile, tol in ((POWER, E.TOL_Q_POWER), (THIN, E.TOL_Q_THIN)):
        for spin in (1, -1):
            rc, a = render(cpu, frame, scene, W, H, disk, em=emission(profile, spin=spin))
            assert rc == GEO_OK
            s = E.compare(a["q"], a["hits"], ref, E.q_ref(frame, scene, W, H, ref, r_in, normal, axis, spin, profile),
                          profile, r_in)
            left_out = D.compare(a["hits"], ref, r_in, r_out)["excluded_share"]
            print(name, "profile", profile, "spin", spin, s, "compare's excluded share of the frame", left_out)
            assert s["compared"][0] >= 0.9 * TS.F64_MIN[name][0] and s["compared"][1] >= 0.9 * TS.F64_MIN[name][1]
            assert s["band_share_of_hits"] < left_out
            assert s["strip_share"] < STRIP_CAP
            assert s["max_err_q"] <= tol


def calibration(cpu):
    """The measured maxima behind TOL_Q_POWER and TOL_Q_THIN (disk_emission_ref's docstring)."""
    worst = {POWER: 0.0, THIN: 0.0}
    for pos, r_in, r_out, normal in D.CAL_DISKS:
        r_obs = math.sqrt(sum(p * p for p in pos))
        phi0 = math.atan2(-pos[1], -pos[0])
        th0 = -math.atan2(pos[2], math.hypot(pos[0], pos[1]))
        for dphi, dth in D.CAL_CAMS:
            frame = default_frame(W, H, pos=pos, camera=(phi0 + dphi, th0 + dth))
            scene = make_scene(1.0, 50.0, r_obs, T.STEP, 2048, flags=GEO_FLAG_DISK)
            ref = D.trace(frame, scene, W, H, r_in, r_out, normal)
            for profile in (POWER, THIN):
                rc, a = render(cpu, frame, scene, W, H, T.make_disk(r_in, r_out, normal), em=emission(profile))
                assert rc == GEO_OK
                s = E.compare(a["q"], a["hits"], ref, E.q_ref(frame, scene, W, H, ref, r_in, normal, profile=profile),
                              profile, r_in)
                assert sum(s["compared"]) > 100
                worst[profile] = max(worst[profile], s["max_err_q"])
    return worst


def test_calibration_record(cpu):
    assert E.TOL_Q_POWER == D.tol_rule(E.CAL_Q_POWER)
    assert E.TOL_Q_THIN == D.tol_rule(E.CAL_Q_THIN)
    worst = calibration(cpu)
    print("calibration: max rel q (POWER)", worst[POWER], "max abs q (THIN)", worst[THIN])
    assert worst[POWER] <= E.CAL_Q_POWER
    assert worst[THIN] <= E.CAL_Q_THIN


def ramps():
    two = np.array([[255, 40, 0, 255], [30, 90, 255, 255]], np.uint8)
    seven = np.array([[250 - 40 * i, (37 * i * i) % 256, 10 + 40 * i, 255] for i in range(7)], np.uint8)
    return {"2": two, "7": seven, "1024": blackbody_ramp(1024, T_LO, T_HI)}


@pytest.mark.parametrize("ramp_name", ["2", "7", "1024"])
def test_colour_step(cpu, ramp_name):
    """The path's own q and hits through disk_emission_ref.colour_np and
    composite_np give the rendered bytes exactly."""
    ramp = ramps()[ramp_name]
    frame, scene, disk, _ = T.pose("A")
    plain = T.render(cpu, frame, T.plain_of(scene), T.SKY, W, H)[1]["rgba"]
    one = np.empty((4, 8, 4), np.uint8)
    one[:] = np.array([10, 200, 30, 200], np.uint8)  # one colour, translucent: every sample is that texel
    saturated = unsaturated = False
    for tex in (one, WHITE):
        rc, base = T.render(cpu, frame, scene, T.SKY, W, H, disk, tex)
        assert rc == GEO_OK
        for profile in (POWER, THIN):
            for exposure in (0.5, 4.0, 40.0):
                em = emission(profile, exposure=exposure)
                rc, a = render(cpu, frame, scene, W, H, disk, tex, em=em, ramp=ramp)
                assert rc == GEO_OK
                want = plain.copy()
                for k in (2, 1, 0):
                    hk = a["hits"][..., k, 0] > 0.0
                    src = E.colour_np(np.broadcast_to(tex[0, 0], want[hk].shape), a["q"][..., k][hk], ramp, T_REF, T_LO,
                                      T_HI, exposure)
                    want[hk] = T.composite_np(src, want[hk])
                    if k == 0:
                        saturated = saturated or bool((src[..., :3] == 255).any())
                        unsaturated = unsaturated or bool((src[..., :3].max(axis=-1) < 255).any())
                assert np.array_equal(a["rgba"], want), (profile, exposure)
                assert np.array_equal(a["rgba"][..., 3], base["rgba"][..., 3])
                assert not np.array_equal(a["rgba"], base["rgba"])
    assert saturated and unsaturated
    assert (a["hits"][..., 1, 0] > 0.0).sum() >= 10  # more than one slot was blended


def test_white_texture_draws_the_ramp(cpu):
    """m = 1 (exposure 1, q = 1) on a white opaque texture is the ramp colour itself."""
    ramp = ramps()["7"]
    q = np.array([1.0], np.float32)
    out = E.colour_np(np.full((1, 4), 255, np.uint8), q, ramp, T_REF, T_LO, T_HI, 1.0)
    pos = 6.0 * (1 / T_LO - 1 / T_REF) / (1 / T_LO - 1 / T_HI)
    i, w = int(pos), int((pos - int(pos)) * 256)
    want = (ramp[i].astype(int) * (256 - w) + ramp[i + 1].astype(int) * w + 128) >> 8
    assert np.array_equal(out[0, :3], want[:3])


def test_beaming_is_colour(cpu):
    """Pose A's mirror pairs under a ramp whose R falls and B rises: the
    approaching hit's ramp colour has B - R no smaller than the receding
    one's, for either spin.  POWER: a pair's two hits share r, hence tau, and
    q differs by g alone.  The ramp colour is the path's own q through
    disk_emission_ref.ramp_np, which test_colour_step holds to the rendered
    bytes (the bytes themselves carry the brightness factor m as well, which
    scales a negative B - R the other way)."""
    n = 256
    ramp = np.zeros((n, 4), np.uint8)
    ramp[:, 0] = np.arange(n)[::-1]
    ramp[:, 1] = 128
    ramp[:, 2] = np.arange(n)
    ramp[:, 3] = 255
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose(TS.SIGN_POSE)
    for spin in (1, -1):
        rc, a = render(cpu, frame, scene, W, H, disk, WHITE, em=emission(POWER, spin=spin), ramp=ramp)
        assert rc == GEO_OK
        ia, ir = TS.mirror_pairs(a["hits"], frame, scene, normal, axis, spin)
        assert ia.size >= 100
        col = E.ramp_np(a["q"][..., 0].ravel(), ramp, T_REF, T_LO, T_HI)
        bmr = col[:, 2] - col[:, 0]
        bad = int((bmr[ia] < bmr[ir]).sum())
        strict = int((bmr[ia] > bmr[ir]).sum())
        print(f"spin {spin:+d}: {ia.size} pairs, {bad} with B - R smaller on the approaching side, {strict} strictly "
              f"bluer; B - R from {bmr[ia].min()} to {bmr[ia].max()} (approaching), {bmr[ir].min()} to {bmr[ir].max()}")
        assert bad == 0
        assert strict >= 0.9 * ia.size


KNOWN = {2856.0: (0.4464, 0.4085, (255, 180, 100)), 6500.0: (0.3135, 0.3237, (255, 249, 254)),
         10000.0: (0.2807, 0.2883, (205, 217, 255))}


def test_blackbody_ramp():
    for t, (x, y, rgb) in KNOWN.items():
        X = blackbody_xyz(t)
        assert abs(X[0] / X.sum() - x) <= 0.003 and abs(X[1] / X.sum() - y) <= 0.003, t
        # the ramp's end entries are those temperatures' colours
        assert tuple(blackbody_ramp(2, t, 2.0 * t)[0, :3]) == rgb
        assert tuple(blackbody_ramp(2, 0.5 * t, t)[1, :3]) == rgb
    X = blackbody_xyz(2856.0)
    assert abs(X[0] / X.sum() - 0.4476) < 0.003 and abs(X[1] / X.sum() - 0.4074) < 0.003  # CIE illuminant A
    for n in (2, 7, 1024):
        r = blackbody_ramp(n, 1000.0, 40000.0)
        assert r.shape == (n, 4) and r.dtype == np.uint8 and (r[:, 3] == 255).all()
        assert (r[:, :3].max(axis=1) == 255).all()
        ratio = r[:, 0].astype(np.float64) / np.maximum(r[:, 2], 1)  # R/B, non-increasing with temperature
        assert (np.diff(ratio) <= 0.0).all()
        # entry i sits at 1/T = 1/t_lo - i/(n-1) (1/t_lo - 1/t_hi)
        i = n // 2
        t_i = 1.0 / (1.0 / 1000.0 - i / (n - 1) * (1.0 / 1000.0 - 1.0 / 40000.0))
        assert np.array_equal(r[i], blackbody_ramp(2, t_i, 2.0 * t_i)[0])
    for bad in ((1, 1000.0, 2000.0), (1025, 1000.0, 2000.0), (8, 2000.0, 2000.0), (8, 0.0, 2000.0)):
        with pytest.raises(ValueError):
            blackbody_ramp(*bad)


@pytest.mark.parametrize("name", ["A", "flat"])
def test_ss4_is_the_box_resolve(cpu, name):
    frame, scene, disk, _ = T.pose(name)
    em = emission(THIN, exposure=2.0)
    ss_scene = make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps,
                          flags=GEO_FLAG_DISK | GEO_FLAG_SS4)
    rc, a = render(cpu, frame, ss_scene, W, H, disk, em=em, outputs=False)
    assert rc == GEO_OK
    frame2, scene2, disk2, _ = T.pose(name, 2 * W, 2 * H)
    rc, b = render(cpu, frame2, scene2, 2 * W, 2 * H, disk2, em=em)
    assert rc == GEO_OK
    s = b["rgba"].astype(np.uint32).reshape(H, 2, W, 2, 4)
    box = ((s.sum(axis=(1, 3)) + 2) >> 2).astype(np.uint8)
    assert np.array_equal(a["rgba"], box)
    assert a["total"] == b["total"]
    rc, plain = render(cpu, frame, ss_scene, W, H, disk, em=None, ramp=None, outputs=False)
    assert rc == GEO_OK and not np.array_equal(plain["rgba"], a["rgba"])


GOLDEN_EMISSION = (1, THIN, 9000.0, 1500.0, 30000.0, 1.0)  # render_frame.py --disk-emission 9000 1500 30000 1


def test_golden_frame(cpu):
    """tests/golden/frame_disk_emission.png (the README's disk pose with the
    emission on: `tools/render_frame.py tests/golden/frame_disk_emission.png
    --disk 1.6 2.2 --disk-emission 9000 1500 30000 1 --cpu --width 480 --height
    270`) is what the CPU path draws, byte for byte."""
    from schwarzschild_raytracer_wgpu_amd import imageio
    from schwarzschild_raytracer_wgpu_amd.scenes import make_disk_texture, make_sky

    w, h = 480, 270
    frame, scene, disk, _ = T.pose("B", w, h)
    rc, a = render(cpu, frame, scene, w, h, disk, make_disk_texture((1024, 128)), em=GOLDEN_EMISSION,
                   ramp=blackbody_ramp(256, GOLDEN_EMISSION[3], GOLDEN_EMISSION[4]),
                   sky=make_sky("equirect", (2048, 1024)))
    assert rc == GEO_OK
    gold = imageio.load_texture(os.path.join(T.ROOT, "tests", "golden", "frame_disk_emission.png"))
    assert gold.shape == (h, w, 4)
    diff = (a["rgba"] != gold).any(axis=-1)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the golden frame"
    plain = imageio.load_texture(os.path.join(T.ROOT, "tests", "golden", "frame_disk.png"))
    assert (gold != plain).any(axis=-1).sum() > 1000
