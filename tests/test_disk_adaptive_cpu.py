"""The thin disk in GEO_MODE_ADAPTIVE on the CPU path
(geo_render_cpu_disk_adaptive, include/geo/geo_cpu.h; csrc/geo_disk.h,
geodesic_angle_adaptive_disk).  tests/test_gpu_disk_adaptive.py ties the
kernels to this path bit for bit.

The probe rule against its definition (tests/native/disk_adaptive_host.cpp, a
host build of the product header): one scalar ray, a per-ray break, dp5_step
called directly, no cursor, no ballots.  Per lane, exactly: the traveled angle
and the attempts of geodesic_angle_adaptive_disk are geodesic_angle_adaptive's
and the definition's, every U_k has the definition's bits, and disk_hit's
verdict is the rule's (probed, a_k < the angle, u_lo <= U <= u_hi).  The sweep
is SCENES x STEPS x TOLS x BUDGETS x NORMALS x 48 x 8 rays = 1 327 104 lanes.
TOLS holds 0 (the default), 1e-4 and 1e-7, and 1e30 beside them: with the first
three no accepted step of the sweep holds two crossings (measured 0: the error
control keeps a step that long from being accepted while the ray still
integrates), and a tolerance that accepts every attempt is what lets h grow
past pi (all 360 such steps come from it).  Measured on the definition's side,
with the floor asserted beside each:

    probes compared                                            239 514   (100 000)
    ... in the lane's stopping attempt                          82 734    (40 000)
    accepted steps holding two or more crossings                   360       (150)
    probes of a crossing a rejected attempt's span held first   27 592    (12 000)
    lanes that exhaust the budget                              464 064   (200 000)
    lanes with no crossing                                      27 648    (13 000)
    probes that are hits                                       113 442    (50 000)
    lanes of kind kCurvedOut / kCurvedIn / kFlat   663 552 / 221 184 / 442 368
                                                  (300 000 / 100 000 / 200 000)
    mismatches                                                       0

What a host build cannot see: it has one lane per wave, so `live` is all or
nothing; the GPU tests run the kernels' waves against this path.

Then the renders: the plain outputs against geo_render_cpu's adaptive render,
the hits against the independent f64 answer tests/disk_ref.py on poses A and B
(the direct mode's bars TOL_R and TOL_AZ were shown to hold at the default tol
on those two poses only; next to the capture orbit, 0.02 <= |b/b_c - 1| < 0.05,
fuzzed scenes reach 1.95e-4 in radius, which tests/disk_truth.py's model of the
adaptive mode carries and include/geo/geo.h documents) and against
straight lines in flat space, the shading against disk_shift_ref and
disk_emission_ref on the returned radii, and the argument rules.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import disk_emission_ref as E
import disk_ref as D
import disk_shift_ref as S
import oracle as O
import test_disk_cpu as T
import test_disk_emission_cpu as TE
import test_disk_probe_host as P
import test_disk_shift_cpu as TS
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import _lib, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_EINVAL, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4, GEO_MODE_ADAPTIVE,
                                                   GEO_MODE_DIRECT, GEO_MODE_FAN, GEO_OK, GeoDiskEmission,
                                                   GeoDiskShift)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "disk_adaptive_host.cpp")
SO = os.path.join(HERE, "native", "libdisk_adaptive_host.so")
W, H = T.W, T.H
POSES4 = ("A", "B", "flat", "tilted")

# ---- 1. the definition --------------------------------------------------------
SCENES = P.SCENES
STEPS = (math.pi / 100, 0.093, 0.3, 0.8)
TOLS = (0.0, 1e-4, 1e-7, 1e30)
BUDGETS = (1, 2, 5, 12, 47, 1000)
NORMALS = P.NORMALS
N_THETA, N_PHI = P.N_THETA, P.N_PHI
NAMES = ("lanes", "mismatch", "first", "what", "compared", "at_stop", "multi", "after_rej", "exhausted", "no_crossing",
         "accepted", "stopped", "curved_out", "curved_in", "flat")
WHAT = ((1, "angle != geodesic_angle_adaptive"), (2, "steps != geodesic_angle_adaptive"),
        (4, "angle or steps != the definition"), (8, "Uk != the definition"), (16, "hit verdict differs"))
# floors: round numbers no higher than half of the measured counts (docstring)
FLOORS = {"compared": 100_000, "at_stop": 40_000, "multi": 150, "after_rej": 12_000, "exhausted": 200_000,
          "no_crossing": 13_000, "accepted": 50_000, "curved_out": 300_000, "curved_in": 100_000, "flat": 200_000}


def load_host():
    deps = [SRC] + [os.path.join(HERE, "..", "schwarzschild_raytracer_wgpu_amd", "csrc", h)
                    for h in ("geo_disk.h", "geo_pixel.h", "geo_math.h", "geo_band.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-mfma",
                        "-msse4.1", "-o", SO, SRC], check=True)
    so = ctypes.CDLL(SO)
    so.disk_adaptive_counters.restype = ctypes.c_uint32
    so.disk_adaptive_sweep.argtypes = [ctypes.c_void_p, ctypes.c_uint32] * 5 + [ctypes.c_uint32] * 3 + [ctypes.c_void_p]
    so.disk_adaptive_sweep.restype = ctypes.c_int
    so.disk_adaptive_lane.argtypes = [ctypes.c_float] * 4 + [ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p] + \
        [ctypes.c_uint32] * 4 + [ctypes.c_void_p]
    so.disk_adaptive_lane.restype = ctypes.c_int
    assert so.disk_adaptive_counters() == len(NAMES)
    return so


@pytest.fixture(scope="module")
def host():
    return load_host()


def sweep(so, scenes, steps, tols, budgets, normals):
    sc = np.ascontiguousarray(scenes, dtype=np.float32)
    st = np.ascontiguousarray(steps, dtype=np.float32)
    to = np.ascontiguousarray(tols, dtype=np.float32)
    bu = np.ascontiguousarray(budgets, dtype=np.uint32)
    no = np.ascontiguousarray(normals, dtype=np.float32)
    out = np.zeros(len(NAMES), dtype=np.uint64)
    rc = so.disk_adaptive_sweep(sc.ctypes.data, len(sc), st.ctypes.data, len(st), to.ctypes.data, len(to),
                                bu.ctypes.data, len(bu), no.ctypes.data, len(no), N_THETA, N_PHI,
                                min(16, os.cpu_count() or 1), out.ctypes.data)
    assert rc == 0, rc
    return {n: int(v) for n, v in zip(NAMES, out)}


def describe(so, c, scenes, steps, tols, budgets, normals):
    """The first differing lane of a sweep: its frame, ray and both sides' values."""
    q, ray = divmod(c["first"], N_THETA * N_PHI)
    q, i_n = divmod(q, len(normals))
    q, i_b = divmod(q, len(budgets))
    q, i_t = divmod(q, len(tols))
    i_s, i_h = divmod(q, len(steps))
    i, jp = divmod(ray, N_PHI)
    out = np.zeros(12, dtype=np.uint32)
    nv = np.ascontiguousarray(normals[i_n], dtype=np.float32)
    so.disk_adaptive_lane(*scenes[i_s], steps[i_h], budgets[i_b], tols[i_t], nv.ctypes.data, i, N_THETA, jp, N_PHI,
                          out.ctypes.data)
    return (f"{c['mismatch']} lanes differ; first: scene={scenes[i_s]} step={steps[i_h]:.5f} tol={tols[i_t]} "
            f"max_steps={budgets[i_b]} normal={normals[i_n]} theta#{i} phi#{jp} kind={out[10]}: "
            f"{', '.join(t for b, t in WHAT if c['what'] & b)}; angle={hex(out[0])} definition's={hex(out[1])} "
            f"steps={out[2]} definition's={out[3]} plain loop's={out[11]} Uk={[hex(x) for x in out[4:7]]} "
            f"definition's={[hex(x) for x in out[7:10]]}")


def test_probes_equal_the_definition(host):
    c = sweep(host, SCENES, STEPS, TOLS, BUDGETS, NORMALS)
    print("adaptive disk probe sweep:", {n: c[n] for n in NAMES if n not in ("first", "what")})
    assert c["lanes"] == len(SCENES) * len(STEPS) * len(TOLS) * len(BUDGETS) * len(NORMALS) * N_THETA * N_PHI
    # the reach conditions: a sweep that stops visiting a path fails here
    for name, floor in FLOORS.items():
        assert c[name] >= floor, (name, c[name], floor)
    assert c["mismatch"] == 0, describe(host, c, SCENES, STEPS, TOLS, BUDGETS, NORMALS)


# ---- the CPU path ---------------------------------------------------------------
def load_cpu():
    lib = TE.load_cpu()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.geo_render_cpu_disk_adaptive.restype = ctypes.c_int
    lib.geo_render_cpu_disk_adaptive.argtypes = [vp, vp, vp, u32, u32, vp, u32, u32, u32, u32, u32, u32, ctypes.c_int,
                                                 vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, u32, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


def adaptive_of(scene, tol=0.0, max_steps=None, step=None, flags=GEO_FLAG_DISK):
    return make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step if step is None else step,
                      scene.max_steps if max_steps is None else max_steps, GEO_MODE_ADAPTIVE, flags, tol)


def render(lib, frame, scene, w, h, disk, tex=T.TEX, shift=None, em=None, ramp=TE.RAMP, sky=T.SKY, row0=0,
           nrows=None, threads=4):
    """geo_render_cpu_disk_adaptive; shift = (spin, exponent, gain) or None,
    em = (spin, profile, t_ref, t_lo, t_hi, exposure) or None.  hits, g and q
    are prefilled with -1."""
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
    e = None if em is None else GeoDiskEmission(*em)
    s = None if shift is None else GeoDiskShift(*shift)
    rmp = None if (ramp is None or em is None) else np.ascontiguousarray(ramp, dtype=np.uint8)
    rc = lib.geo_render_cpu_disk_adaptive(
        ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1], sky.shape[0], None, 0, w, h,
        row0, nrows, 1, threads, rgba.ctypes.data, mask.ctypes.data, uv.ctypes.data, steps.ctypes.data,
        ctypes.addressof(total), None if disk is None else ctypes.addressof(disk), tex.ctypes.data, tex.shape[1],
        tex.shape[0], hits.ctypes.data, None if e is None else ctypes.addressof(e),
        None if rmp is None else rmp.ctypes.data, 0 if rmp is None else rmp.shape[0], g.ctypes.data, q.ctypes.data,
        None if s is None else ctypes.addressof(s))
    return rc, dict(rgba=rgba, mask=mask, uv=uv, steps=steps, total=total.value, hits=hits, g=g, q=q)


def test_announced():
    hdr = open(os.path.join(T.ROOT, "include", "geo", "geo.h")).read()
    assert re.search(r"^#define GEO_HAS_DISK_ADAPTIVE 1$", hdr, re.M)
    assert re.search(r"^#define GEO_ABI_VERSION 8\b", hdr, re.M)
    assert _lib.GEO_HAS_DISK_ADAPTIVE == 1
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.geo_render_disk_adaptive  # exported (no GPU needed to look it up)
    assert _lib.lib.geo_abi_version() == 8


# ---- 2. the plain outputs -------------------------------------------------------
@pytest.fixture(scope="module")
def frames(cpu):
    """The four poses' adaptive disk frames and plain adaptive frames, rendered once."""
    out = {}
    for name in POSES4:
        frame, scene, disk, _ = T.pose(name)
        sc = adaptive_of(scene)
        rc, a = render(cpu, frame, sc, W, H, disk)
        assert rc == GEO_OK
        rcp, p = T.render(cpu, frame, adaptive_of(scene, flags=0), T.SKY, W, H)
        assert rcp == GEO_OK
        out[name] = (a, p)
    return out


@pytest.mark.parametrize("name", POSES4)
def test_plain_outputs(frames, name):
    a, p = frames[name]
    hit = (a["hits"][..., 0] > 0.0).any(axis=-1)
    assert hit.sum() > 300 and (~hit).sum() > 300
    assert np.array_equal(a["rgba"][~hit], p["rgba"][~hit])
    assert np.array_equal(a["mask"], p["mask"]) and np.array_equal(a["steps"], p["steps"])
    assert np.array_equal(a["uv"].view(np.uint32), p["uv"].view(np.uint32))
    assert a["total"] == p["total"]
    # unshaded: g and q are not written
    assert (a["g"] == -1.0).all() and (a["q"] == -1.0).all()


# ---- 3. against the independent f64 answer --------------------------------------
REF_STEPS = 1000  # with step pi/100: neither disk_ref's angle budget nor the attempt budget binds off the band
REF_TOL = 0.0     # the tolerance the curved poses are run at (the default; see the test's docstring)


@pytest.fixture(scope="module")
def curved(cpu):
    out = {}
    for name in T.CURVED:
        frame, scene, disk, (r_in, r_out, normal, axis) = T.pose(name)
        sc = adaptive_of(scene, tol=REF_TOL, max_steps=REF_STEPS)
        rc, a = render(cpu, frame, sc, W, H, disk)
        assert rc == GEO_OK
        rcp, p = T.render(cpu, frame, adaptive_of(sc, tol=REF_TOL, flags=0), T.SKY, W, H)
        assert rcp == GEO_OK
        ref = D.trace(frame, sc, W, H, r_in, r_out, normal, axis)
        out[name] = (a, p, ref, r_in, r_out, frame, sc, normal, axis)
    return out


@pytest.mark.parametrize("name", list(T.CURVED))
def test_curved_space_against_disk_ref(curved, name):
    """The direct mode's committed bars TOL_R and TOL_AZ, its band BAND_X and
    its cap on the excluded share, at the adaptive mode's default tol, on poses
    A and B (the fuzzed scenes and their wider bar next to the band:
    tests/test_disk_truth_cpu.py)."""
    a, p, ref, r_in, r_out = curved[name][:5]
    s = D.compare(a["hits"], ref, r_in, r_out)
    shadow = p["mask"] == 1
    covered = int((shadow & (a["hits"][..., 0, 0] > 0.0)).sum())
    print(name, s, "shadow pixels", int(shadow.sum()), "covered at k=0", covered)
    n0, n1 = T.CURVED[name]
    assert s["excluded_share"] <= 0.02
    assert s["total0"] >= n0 and s["total1"] >= n1 and s["ref_total0"] >= n0 and s["ref_total1"] >= n1
    assert covered > 0
    assert s["disagree_off_edge"] == 0
    assert s["max_rel_r"] <= D.TOL_R and s["max_az"] <= D.TOL_AZ


# ---- 4. flat space --------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat", "tilted"])
def test_flat_space_against_straight_lines(frames, name):
    """rs = 0: the expected hit is where the segment from the observer to the
    pixel's sky point meets the disk plane inside the annulus (no ODE on the
    reference side), as test_disk_cpu's test of the direct mode."""
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose(name)
    a, _ = frames[name]
    ref = O.render_f64(frame, T.plain_of(scene), W, H, threads=4)
    U, V = ref["uv"][..., 0].astype(np.float64), ref["uv"][..., 1].astype(np.float64)
    sky_pt = 50.0 * np.stack([np.sin(math.pi * V) * np.cos(2 * math.pi * U), np.sin(math.pi * V) * np.sin(2 * math.pi * U),
                              np.cos(math.pi * V)], axis=-1)
    obs = D.observer_world(frame, scene.r_obs)
    n, ex, ey = D.disk_basis(normal, axis)
    d0 = obs.dot(n)
    d1 = sky_pt @ n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = d0 / (d0 - d1)
    X = obs[None, None, :] + t[..., None] * (sky_pt - obs[None, None, :])
    r = np.linalg.norm(X, axis=-1)
    want = (ref["mask"] == 0) & (t > 0.0) & (t < 1.0) & (r >= r_in) & (r <= r_out)
    az = np.mod(np.arctan2(X @ ey, X @ ex) / (2 * math.pi), 1.0)
    got = a["hits"][..., 0, 0] > 0.0
    print(name, "slot-0 hits", int(got.sum()), "expected", int(want.sum()))
    near_edge = (np.abs(r / r_in - 1.0) <= D.TOL_R) | (np.abs(r / r_out - 1.0) <= D.TOL_R)
    assert not ((got != want) & ~near_edge).any()
    both = got & want
    assert both.sum() > 1000
    er = np.abs(a["hits"][..., 0, 0][both] / r[both] - 1.0).max()
    ea = D.az_err(a["hits"][..., 0, 1][both], az[both]).max()
    print(name, "max rel r", er, "max az", ea)
    assert er <= D.TOL_R and ea <= D.TOL_AZ
    # a straight line meets the plane once
    assert not (a["hits"][..., 1:, 0] > 0.0).any()


# ---- 5. shading -----------------------------------------------------------------
def ref_at_returned_radii(ref, hits):
    """disk_ref.trace's dict with the CPU path's own hits and radii in place of
    the trace's: the shading refs then restate g and q on the returned radii."""
    out = dict(ref)
    hit = hits[..., 0] > 0.0
    out["hit"] = hit
    out["r"] = np.where(hit, hits[..., 0].astype(np.float64), np.nan)
    return out


@pytest.mark.parametrize("name", list(T.CURVED))
def test_shading_on_the_returned_radii(cpu, curved, name):
    a0, _, ref, r_in, r_out, frame, sc, normal, axis = curved[name]
    disk = T.make_disk(r_in, r_out, normal, axis)
    for spin in (1, -1):
        rc, a = render(cpu, frame, sc, W, H, disk, shift=(spin, 4, 1.0))
        assert rc == GEO_OK
        assert np.array_equal(a["hits"].view(np.uint32), a0["hits"].view(np.uint32))
        assert (a["q"] == -1.0).all()
        assert np.array_equal(a["g"] != 0.0, a["hits"][..., 0] != 0.0)
        own = ref_at_returned_radii(ref, a["hits"])
        s = S.compare(a["g"], a["hits"], own, S.shift(frame, sc, W, H, own, normal, axis, spin))
        print(name, "shift spin", spin, s)
        assert s["compared"][0] >= 0.9 * TS.F64_MIN[name][0] and s["compared"][1] >= 0.9 * TS.F64_MIN[name][1]
        assert s["max_rel_g"] <= S.TOL_G
        for profile, tol in ((E.POWER, E.TOL_Q_POWER), (E.THIN, E.TOL_Q_THIN)):
            rc, b = render(cpu, frame, sc, W, H, disk, em=TE.emission(profile, spin=spin))
            assert rc == GEO_OK
            assert np.array_equal(b["hits"].view(np.uint32), a0["hits"].view(np.uint32))
            # the emission's g is the shift's (its own spin)
            assert np.array_equal(b["g"].view(np.uint32), a["g"].view(np.uint32))
            s = E.compare(b["q"], b["hits"], own, E.q_ref(frame, sc, W, H, own, r_in, normal, axis, spin, profile),
                          profile, r_in)
            print(name, "emission profile", profile, "spin", spin, s)
            assert s["compared"][0] >= 0.9 * TS.F64_MIN[name][0] and s["max_err_q"] <= tol


@pytest.mark.parametrize("name", POSES4)
def test_identity_shift_is_the_unshaded_render(cpu, frames, name):
    frame, scene, disk, _ = T.pose(name)
    rc, a = render(cpu, frame, adaptive_of(scene), W, H, disk, shift=(1, 0, 1.0))
    assert rc == GEO_OK
    assert TS.same_frame(a, frames[name][0])
    assert np.array_equal(a["g"] != 0.0, a["hits"][..., 0] != 0.0)


def test_emission_takes_the_shifts_place(cpu):
    frame, scene, disk, _ = T.pose("A")
    sc = adaptive_of(scene)
    rc, a = render(cpu, frame, sc, W, H, disk, em=TE.emission())
    rc2, b = render(cpu, frame, sc, W, H, disk, em=TE.emission(), shift=(-1, 2, 3.0))
    assert rc == GEO_OK and rc2 == GEO_OK
    assert TS.same_frame(a, b) and np.array_equal(a["q"], b["q"]) and np.array_equal(a["g"], b["g"])
    assert (a["q"][a["hits"][..., 0] > 0.0] > 0.0).all()


def test_row_range_and_threads(cpu, frames):
    frame, scene, disk, _ = T.pose("B")
    rc, a = render(cpu, frame, adaptive_of(scene), W, H, disk, row0=5, nrows=20, threads=1)
    assert rc == GEO_OK
    full = frames["B"][0]
    for f in ("rgba", "mask", "steps", "hits", "uv"):
        assert np.array_equal(a[f], full[f][5:25]), f
    assert a["total"] == int(full["steps"][5:25].sum(dtype=np.uint64))


# ---- 6. the argument rules ------------------------------------------------------
def test_argument_checks(cpu):
    frame, scene, disk, _ = T.pose("A")
    w, h = 16, 9
    frame = default_frame(w, h, pos=T.POSES["A"][0], camera=T.POSES["A"][1], fov=T.POSES["A"][2])

    def rc_of(sc, dk=disk, **kw):
        return render(cpu, frame, sc, w, h, dk, **kw)[0]

    def sc(rs=1.0, sphere=50.0, r_obs=scene.r_obs, mode=GEO_MODE_ADAPTIVE, flags=GEO_FLAG_DISK, tol=0.0):
        return make_scene(rs, sphere, r_obs, T.STEP, 256, mode, flags, tol)

    assert rc_of(sc()) == GEO_OK
    assert rc_of(sc(flags=GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS)) == GEO_OK
    assert rc_of(sc(rs=0.0)) == GEO_OK
    assert rc_of(sc(tol=1e-4)) == GEO_OK
    # the direct and fan scenes are the older functions'
    for mode in (GEO_MODE_DIRECT, GEO_MODE_FAN):
        assert rc_of(sc(mode=mode)) == GEO_EINVAL
    # the function needs the flag and a disk, and takes DEFER_STEPS at most beside it
    assert rc_of(sc(flags=0)) == GEO_EINVAL
    assert rc_of(sc(), dk=None) == GEO_EINVAL
    for fl in (GEO_FLAG_MIPS, GEO_FLAG_COMPOSITE, GEO_FLAG_RING_F64, GEO_FLAG_SS4):
        assert rc_of(sc(flags=GEO_FLAG_DISK | fl)) == GEO_EINVAL
    # tol under the adaptive mode's rules
    for tol in (-1.0, math.inf, math.nan):
        assert rc_of(sc(tol=tol)) == GEO_EINVAL
    # GEO_FLAG_DISK's rules
    assert rc_of(sc(r_obs=0.9)) == GEO_EINVAL            # observer inside the horizon
    assert rc_of(sc(rs=3.5)) == GEO_EINVAL               # rs >= r_in
    assert rc_of(sc(sphere=8.0)) == GEO_EINVAL           # r_out >= sphere_r
    assert rc_of(sc(sphere=12.0)) == GEO_EINVAL          # r_obs >= sphere_r
    for bad in (T.make_disk(0.0, 9.0), T.make_disk(9.0, 3.0), T.make_disk(3.0, 3.0),
                T.make_disk(3.0, 9.0, normal=(0, 0, 0)), T.make_disk(3.0, 9.0, axis=(0, 0, 2.0))):
        assert rc_of(sc(), dk=bad) == GEO_EINVAL
    # the shift's and the emission's rules, and r_in > 1.5 rs with either
    assert rc_of(sc(), shift=(1, 4, 1.0)) == GEO_OK and rc_of(sc(), em=TE.emission()) == GEO_OK
    for shift in ((0, 4, 1.0), (1, 5, 1.0), (1, 4, 0.0), (1, 4, math.inf)):
        assert rc_of(sc(), shift=shift) == GEO_EINVAL
    for em in (TE.emission(spin=0), TE.emission(profile=2), TE.emission(t_ref=0.0), TE.emission(t_lo=3000.0, t_hi=2000.0)):
        assert rc_of(sc(), em=em) == GEO_EINVAL
    assert rc_of(sc(), em=TE.emission(), ramp=np.zeros((1, 4), np.uint8)) == GEO_EINVAL
    for r_in, rs in ((3.0, 2.0), (3.0, 2.5)):
        dk = T.make_disk(r_in, 9.0)
        assert rc_of(sc(rs=rs), dk=dk) == GEO_OK
        assert rc_of(sc(rs=rs), dk=dk, shift=(1, 4, 1.0)) == GEO_EINVAL
        assert rc_of(sc(rs=rs), dk=dk, em=TE.emission()) == GEO_EINVAL
    # an invalid shift is not read while an emission is given
    assert rc_of(sc(), em=TE.emission(), shift=(0, 9, -1.0)) == GEO_OK


def test_older_cpu_functions_keep_refusing_the_adaptive_mode(cpu):
    frame, scene, disk, _ = T.pose("A")
    w, h = 16, 9
    frame = default_frame(w, h, pos=T.POSES["A"][0], camera=T.POSES["A"][1], fov=T.POSES["A"][2])
    sc = make_scene(1.0, 50.0, scene.r_obs, T.STEP, 256, GEO_MODE_ADAPTIVE, GEO_FLAG_DISK)
    assert T.render(cpu, frame, sc, T.SKY, w, h, disk, T.TEX, want_hits=False)[0] == GEO_EINVAL
    assert T.render(cpu, frame, sc, T.SKY, w, h)[0] == GEO_EINVAL  # geo_render_cpu: the flag
    assert TS.render(cpu, frame, sc, w, h, disk)[0] == GEO_EINVAL
    assert TE.render(cpu, frame, sc, w, h, disk)[0] == GEO_EINVAL
    # and the plain adaptive render is drawn as before
    assert T.render(cpu, frame, adaptive_of(sc, flags=0), T.SKY, w, h)[0] == GEO_OK
