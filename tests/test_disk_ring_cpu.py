"""The disk's capture band in f64 on the CPU path
(geo_render_cpu_disk_ring_f64, include/geo/geo_cpu.h; csrc/geo_band.h
band_lambda_disk with csrc/geo_disk.h): the third image's radii against the
f64 restatement tests/disk_ref.py at the scene's own step, that nothing
outside the band changes, that the sky side is the plain GEO_FLAG_RING_F64
render's, the shaded and emission renders inside the band, and the rules.
tests/test_gpu_disk_ring.py ties the kernels to this path bit for bit.
The flat bar disk_ring_ref.TOL_R_BAND holds on the three poses used here; on
fuzzed scenes (tests/disk_band_truth.py, test_disk_band_truth_cpu.py) the band's
radius carries a 1/H term, which that layer's model has."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import disk_emission_ref as E
import disk_ref as D
import disk_ring_ref as R
import disk_shift_ref as S
import test_disk_cpu as T
import test_disk_emission_cpu as X
import test_disk_shift_cpu as TS
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import _lib, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_EINVAL, GEO_FLAG_DISK, GEO_FLAG_RING_F64, GEO_FLAG_SS4, GEO_OK,
                                                   GeoDiskEmission, GeoDiskShift)

W, H = T.W, T.H


def load_cpu():
    lib = X.load_cpu()
    lib.geo_render_cpu_disk_ring_f64.restype = ctypes.c_int
    lib.geo_render_cpu_disk_ring_f64.argtypes = lib.geo_render_cpu_disk_emission.argtypes + [ctypes.c_int]
    lib.geo_render_cpu_disk_shift_ring_f64.restype = ctypes.c_int
    lib.geo_render_cpu_disk_shift_ring_f64.argtypes = lib.geo_render_cpu_disk_shift.argtypes + [ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


def render(lib, frame, scene, disk, ring=1, w=W, h=H, tex=T.TEX, em=None, ramp=X.RAMP, shift=None, sky=T.SKY, row0=0,
           nrows=None, threads=4, outputs=True):
    """geo_render_cpu_disk_ring_f64 (em = (spin, profile, t_ref, t_lo, t_hi,
    exposure) or None: the unshaded disk), or with shift = (spin, exponent,
    gain) geo_render_cpu_disk_shift_ring_f64; rows row0 .. row0 + nrows - 1.
    Outputs a render does not write keep their prefill -1."""
    nrows = h - row0 if nrows is None else nrows
    sky = np.ascontiguousarray(sky, dtype=np.uint8)
    tex = np.ascontiguousarray(tex, dtype=np.uint8)
    rgba = np.zeros((nrows, w, 4), np.uint8)
    mask = np.empty((nrows, w), np.uint8)
    uv = np.empty((nrows, w, 2), np.float32)
    steps = np.empty((nrows, w), np.uint32)
    total = ctypes.c_ulonglong()
    hits = np.full((nrows, w, 3, 2), -1.0, np.float32)
    g = np.full((nrows, w, 3), -1.0, np.float32)
    q = np.full((nrows, w, 3), -1.0, np.float32)
    p = (lambda a: a.ctypes.data) if outputs else (lambda a: None)
    head = [ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1], sky.shape[0], None, 0, w, h,
            row0, nrows, 1, threads, rgba.ctypes.data, p(mask), p(uv), p(steps), ctypes.addressof(total),
            ctypes.addressof(disk), tex.ctypes.data, tex.shape[1], tex.shape[0], p(hits)]
    if shift is not None:
        sh = GeoDiskShift(*shift)
        rc = lib.geo_render_cpu_disk_shift_ring_f64(*head, ctypes.addressof(sh), p(g), ring)
    else:
        e = None if em is None else GeoDiskEmission(*em)
        rmp = None if em is None else np.ascontiguousarray(ramp, dtype=np.uint8)
        rc = lib.geo_render_cpu_disk_ring_f64(*head, None if e is None else ctypes.addressof(e),
                                              None if rmp is None else rmp.ctypes.data,
                                              0 if rmp is None else rmp.shape[0], p(g), p(q), ring)
    return rc, dict(rgba=rgba, mask=mask, uv=uv, steps=steps, total=total.value, hits=hits, g=g, q=q)


def ring_scene(scene):
    """The same scene with GEO_FLAG_RING_F64 in place of GEO_FLAG_DISK."""
    return make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, flags=GEO_FLAG_RING_F64)


@pytest.fixture(scope="module")
def frames(cpu):
    """Per pose: the state on, the state off, the reference's trace at the
    scene's own step (sub=1: the state's definition) and the disk's radii."""
    out = {}
    for name in ("ring", "B", "A"):
        frame, scene, disk, (r_in, r_out, normal, axis) = T.pose(name)
        rc, on = render(cpu, frame, scene, disk, 1)
        assert rc == GEO_OK
        rc, off = render(cpu, frame, scene, disk, 0)
        assert rc == GEO_OK
        out[name] = (on, off, D.trace(frame, scene, W, H, r_in, r_out, normal, axis, sub=1), r_in, r_out)
    return out


def test_announced():
    hdr = open(os.path.join(T.ROOT, "include", "geo", "geo.h")).read()
    assert re.search(r"^#define GEO_HAS_DISK_RING_F64 1$", hdr, re.M)
    assert re.search(r"^#define GEO_ABI_VERSION 8\b", hdr, re.M)
    assert _lib.GEO_HAS_DISK_RING_F64 == 1
    assert ctypes.CDLL(_lib.LIB_PATH).geo_set_disk_ring_f64  # exported (no GPU needed to look it up)
    assert _lib.lib.geo_abi_version() == 8


def test_off_is_the_emission_entry(cpu):
    """ring_f64 = 0 is geo_render_cpu_disk_emission (and geo_render_cpu_disk_shift)."""
    frame, scene, disk, _ = T.pose("ring")
    for em in (None, X.emission()):
        rc, a = render(cpu, frame, scene, disk, 0, em=em)
        rcw, want = X.render(cpu, frame, scene, W, H, disk, em=em, ramp=X.RAMP if em else None)
        assert rc == GEO_OK and rcw == GEO_OK and TS.same_frame(a, want)
        assert np.array_equal(a["g"], want["g"]) and np.array_equal(a["q"], want["q"])
    rc, a = render(cpu, frame, scene, disk, 0, shift=(1, 4, 1.0))
    rcw, want = TS.render(cpu, frame, scene, W, H, disk)
    assert rc == GEO_OK and rcw == GEO_OK and TS.same_frame(a, want) and np.array_equal(a["g"], want["g"])


def test_third_image_radii(frames):
    """Pose "ring": all slot-2 hits (every one inside the band) against
    disk_ref.trace(sub=1), no pixel left out.  With the state on the radii
    hold the disk's bar TOL_R = 2^-13 (measured 2.11e-6) and the band's own
    bar disk_ring_ref.TOL_R_BAND; with it off they miss TOL_R (1.25e-3), which
    records the gain."""
    on, off, ref, r_in, r_out = frames["ring"]
    s = D.compare(on["hits"], ref, r_in, r_out, slots=(2,), use_band=False)
    print("ring, on", s)
    assert s["hits2"] >= 100 and s["ref_hits2"] >= 100
    assert s["disagree_off_edge"] == 0
    assert s["max_rel_r"] <= D.TOL_R
    b = R.band_compare(on["hits"], ref, r_in, r_out)
    print("ring, on, in-band", b)
    assert b["both2"] >= 100 and b["disagree_off_edge"] == 0 and b["max_rel_r"] <= R.TOL_R_BAND
    s0 = D.compare(off["hits"], ref, r_in, r_out, slots=(2,), use_band=False)
    print("ring, off", s0)
    assert s0["hits2"] >= 100 and s0["max_rel_r"] > D.TOL_R


def test_pose_b_band_hits(frames):
    """Pose B: every hit inside the band within TOL_R and TOL_AZ (and the
    band's own bar), at least 8 slot-0 and 4 slot-1 hits, none disputed."""
    on, _, ref, r_in, r_out = frames["B"]
    b = R.band_compare(on["hits"], ref, r_in, r_out)
    print("B, on, in-band", b)
    assert b["both0"] >= 8 and b["both1"] >= 4
    assert b["disagree_off_edge"] == 0
    assert b["max_rel_r"] <= D.TOL_R and b["max_az"] <= D.TOL_AZ
    assert b["max_rel_r"] <= R.TOL_R_BAND


def calibration(cpu):
    """The measured maximum behind TOL_R_BAND (disk_ring_ref's docstring) and the hits it was measured on."""
    worst, n = 0.0, 0
    cams = []
    for i, (pos, r_in, r_out, normal) in enumerate(D.CAL_DISKS):
        phi0 = math.atan2(-pos[1], -pos[0])
        th0 = -math.atan2(pos[2], math.hypot(pos[0], pos[1]))
        cams += [(pos, r_in, r_out, normal, dict(camera=(phi0 + dphi, th0 + dth))) for dphi, dth in D.CAL_CAMS]
        if i == 0:
            cams.append((pos, r_in, r_out, normal, dict(camera=R.cal_ring_camera(pos), fov=R.CAL_RING_FOV, state=0)))
    for pos, r_in, r_out, normal, kw in cams:
        r_obs = math.sqrt(sum(p * p for p in pos))
        frame = default_frame(W, H, pos=pos, **kw)
        scene = make_scene(1.0, 50.0, r_obs, T.STEP, 2048, flags=GEO_FLAG_DISK)
        rc, a = render(cpu, frame, scene, T.make_disk(r_in, r_out, normal), 1)
        assert rc == GEO_OK
        b = R.band_compare(a["hits"], D.trace(frame, scene, W, H, r_in, r_out, normal, sub=1), r_in, r_out)
        assert b["disagree_off_edge"] == 0
        worst = max(worst, b["max_rel_r"])
        n += b["both0"] + b["both1"] + b["both2"]
    return worst, n


def test_calibration_record(cpu):
    assert R.TOL_R_BAND == D.tol_rule(R.CAL_R_BAND)
    worst, n = calibration(cpu)
    print("calibration: max rel r of", n, "in-band hits", worst)
    assert n >= 250  # (290 when recorded)
    assert worst <= R.CAL_R_BAND


@pytest.mark.parametrize("name", ["ring", "B", "A"])
def test_nothing_leaks(frames, name):
    """Outside the band (|b/b_c - 1| >= GEO_RING_X by the f64 reference, less
    a guard zone of 1e-5 around the edge: the band test is on the f32 ray)
    every output equals the state-off render's bit for bit.  Pose A has no
    band pixel: its whole frame is equal, steps_total too."""
    on, off, ref, _, _ = frames[name]
    out = ref["x"] >= R.BAND + R.GUARD
    assert out.sum() >= 0.4 * W * H
    if name == "A":
        assert out.all() and on["total"] == off["total"]
    else:
        assert (ref["x"] < R.BAND - R.GUARD).sum() >= 20
    for f in ("rgba", "mask", "steps"):
        assert np.array_equal(on[f][out], off[f][out]), f
    for f in ("hits", "uv"):
        assert np.array_equal(on[f].view(np.uint32)[out], off[f].view(np.uint32)[out]), f


@pytest.mark.parametrize("name", ["ring", "B", "A"])
def test_sky_side_is_the_ring_render(cpu, frames, name):
    """mask, UV, steps and steps_total are the plain GEO_FLAG_RING_F64
    render's on every pixel, and a pixel with no hit has that render's colour."""
    on = frames[name][0]
    frame, scene, _, _ = T.pose(name)
    rc, p = T.render(cpu, frame, ring_scene(scene), T.SKY, W, H)
    assert rc == GEO_OK
    assert np.array_equal(on["mask"], p["mask"]) and np.array_equal(on["steps"], p["steps"])
    assert np.array_equal(on["uv"].view(np.uint32), p["uv"].view(np.uint32))
    assert on["total"] == p["total"]
    nohit = ~(on["hits"][..., 0] > 0.0).any(axis=-1)
    assert nohit.any() and np.array_equal(on["rgba"][nohit], p["rgba"][nohit])


@pytest.mark.parametrize("name", ["ring", "B"])
def test_shift_and_emission_in_the_band(cpu, frames, name):
    """g and q with the state on, against disk_shift_ref and
    disk_emission_ref on the trace at the scene's own step.  Judged on the
    pixels those modules compare, |b/b_c - 1| >= BAND_G = 0.002, which now
    takes in the band's outer part 0.002 <= x < 0.005 (its pixels run through
    the f64 path), with the modules' own bars; and, beyond what they compare,
    on every hit inside the band (x < 0.005 less the guard, down to the
    capture orbit: the third image), with the same bars (for THIN outside the
    inner-edge strip, as disk_emission_ref.compare)."""
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose(name)
    ref = frames[name][2]
    inb = ref["x"] < R.BAND - R.GUARD
    gref = S.shift(frame, scene, W, H, ref, normal, axis, 1)
    rc, a = render(cpu, frame, scene, disk, 1, shift=(1, 4, 1.0))
    assert rc == GEO_OK
    s = S.compare(a["g"], a["hits"], ref, gref)
    print(name, "g, the module's pixels", s)
    assert sum(s["compared"]) >= 30 and s["max_rel_g"] <= S.TOL_G
    worst, n = 0.0, 0
    for k in range(3):
        both = (a["hits"][..., k, 0] > 0.0) & ref["hit"][..., k] & inb
        if both.any():
            worst = max(worst, float(np.abs(a["g"][..., k][both].astype(np.float64) / gref[..., k][both] - 1.0).max()))
        n += int(both.sum())
    print(name, "g, in-band hits", n, worst)
    assert n >= 12 and worst <= S.TOL_G
    for profile, tol in ((E.POWER, E.TOL_Q_POWER), (E.THIN, E.TOL_Q_THIN)):
        rc, a = render(cpu, frame, scene, disk, 1, em=X.emission(profile))
        assert rc == GEO_OK
        qr = E.q_ref(frame, scene, W, H, ref, r_in, normal, axis, 1, profile)
        s = E.compare(a["q"], a["hits"], ref, qr, profile, r_in)
        print(name, "q, profile", profile, "the module's pixels", s)
        assert sum(s["compared"]) >= 30 and s["max_err_q"] <= tol
        worst, n = 0.0, 0
        for k in range(3):
            both = (a["hits"][..., k, 0] > 0.0) & ref["hit"][..., k] & inb
            if profile == E.THIN:
                with np.errstate(invalid="ignore"):
                    both &= ~(ref["r"][..., k] - r_in < r_in * E.STRIP)
            if both.any():
                got, want = a["q"][..., k][both].astype(np.float64), qr[..., k][both]
                err = np.abs(got / want - 1.0) if profile == E.POWER else np.abs(got - want)
                worst = max(worst, float(err.max()))
            n += int(both.sum())
        print(name, "q, profile", profile, "in-band hits", n, worst)
        assert n >= 12 and worst <= tol


@pytest.mark.parametrize("name", ["ring", "B"])
def test_white_texture_draws_the_ramp_in_the_band(cpu, frames, name):
    """A white opaque texture: every in-band pixel with a hit shows
    disk_emission_ref.colour_np at the q of its nearest hit, byte for byte."""
    frame, scene, disk, _ = T.pose(name)
    ref = frames[name][2]
    rc, a = render(cpu, frame, scene, disk, 1, tex=X.WHITE, em=X.emission())
    assert rc == GEO_OK
    inb = ref["x"] < R.BAND - R.GUARD
    hit = a["hits"][..., 0] > 0.0
    px = inb & hit.any(axis=-1)
    assert px.sum() >= 12
    near = np.argmax(hit, axis=-1)  # the lowest slot that hit: the nearest, drawn last
    q = np.take_along_axis(a["q"], near[..., None], axis=-1)[..., 0][px]
    want = E.colour_np(np.full((int(px.sum()), 4), 255, np.uint8), q, X.RAMP, X.T_REF, X.T_LO, X.T_HI, 1.0)
    assert np.array_equal(a["rgba"][px], want)


def test_rules(cpu):
    # rs = 0: no capture orbit, the state is ignored
    frame, scene, disk, _ = T.pose("flat")
    rc, a = render(cpu, frame, scene, disk, 1)
    rcw, want = T.render(cpu, frame, scene, T.SKY, W, H, disk, T.TEX)
    assert rc == GEO_OK and rcw == GEO_OK and TS.same_frame(a, want)
    # colour-only renders are refused while it is on, and the flag pair stays refused
    frame, scene, disk, _ = T.pose("B")

    def sc(flags):
        return make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, flags=flags)

    ss = sc(GEO_FLAG_DISK | GEO_FLAG_SS4)
    assert render(cpu, frame, ss, disk, 0, outputs=False)[0] == GEO_OK
    assert render(cpu, frame, ss, disk, 1, outputs=False)[0] == GEO_EINVAL
    assert render(cpu, frame, ss, disk, 1, outputs=False, shift=(1, 4, 1.0))[0] == GEO_EINVAL
    for ring in (0, 1):
        assert render(cpu, frame, sc(GEO_FLAG_DISK | GEO_FLAG_RING_F64), disk, ring)[0] == GEO_EINVAL
        assert render(cpu, frame, sc(GEO_FLAG_RING_F64), disk, ring)[0] == GEO_EINVAL
    # rows: a part of the frame is that part of the whole frame
    rc, whole = render(cpu, frame, scene, disk, 1)
    rc2, part = render(cpu, frame, scene, disk, 1, row0=11, nrows=20)
    assert rc == GEO_OK and rc2 == GEO_OK
    assert np.array_equal(part["rgba"], whole["rgba"][11:31]) and np.array_equal(
        part["hits"].view(np.uint32), whole["hits"].view(np.uint32)[11:31])
