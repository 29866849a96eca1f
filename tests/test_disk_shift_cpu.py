"""Doppler and redshift shading of the thin disk on the CPU path
(geo_render_cpu_disk_shift, include/geo/geo_cpu.h; csrc/geo_disk.h): the
frequency ratio g against closed forms (flat space, a face-on disk, a moving
observer), against the f64 restatement tests/disk_shift_ref.py, its sign by the
approaching and the receding side of the disk, the colour step against a numpy
restatement, and the argument rules.  tests/test_gpu_disk_shift.py ties the
kernel to this path bit for bit."""
import ctypes
import math
import os

import numpy as np
import pytest

import disk_ref as D
import disk_shift_ref as S
import test_disk_cpu as T
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_EINVAL, GEO_FLAG_COMPOSITE, GEO_FLAG_DISK, GEO_FLAG_MIPS,
                                                   GEO_FLAG_RING_F64, GEO_MODE_ADAPTIVE, GEO_MODE_FAN, GEO_OK,
                                                   GeoDiskShift)

W, H = T.W, T.H
G_MAX = 16.0  # GEO_DISK_G_MAX


def load_cpu():
    lib = T.load_cpu()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.geo_render_cpu_disk_shift.restype = ctypes.c_int
    lib.geo_render_cpu_disk_shift.argtypes = [vp, vp, vp, u32, u32, vp, u32, u32, u32, u32, u32, u32, ctypes.c_int, vp,
                                              vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


def render(lib, frame, scene, w, h, disk, tex=T.TEX, shift=(1, 4, 1.0), sky=T.SKY, threads=4):
    """geo_render_cpu_disk_shift over the whole frame; shift = (spin, exponent,
    gain) or None (the unshaded disk: out_g stays at its prefill -1)."""
    sky = np.ascontiguousarray(sky, dtype=np.uint8)
    tex = np.ascontiguousarray(tex, dtype=np.uint8)
    rgba = np.zeros((h, w, 4), np.uint8)
    mask = np.empty((h, w), np.uint8)
    uv = np.empty((h, w, 2), np.float32)
    steps = np.empty((h, w), np.uint32)
    total = ctypes.c_ulonglong()
    hits = np.full((h, w, 3, 2), -1.0, np.float32)
    g = np.full((h, w, 3), -1.0, np.float32)
    sh = None if shift is None else GeoDiskShift(*shift)
    rc = lib.geo_render_cpu_disk_shift(ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1],
                                       sky.shape[0], None, 0, w, h, 0, h, 1, threads, rgba.ctypes.data, mask.ctypes.data,
                                       uv.ctypes.data, steps.ctypes.data, ctypes.addressof(total),
                                       ctypes.addressof(disk), tex.ctypes.data, tex.shape[1], tex.shape[0],
                                       hits.ctypes.data, None if sh is None else ctypes.addressof(sh), g.ctypes.data)
    return rc, dict(rgba=rgba, mask=mask, uv=uv, steps=steps, total=total.value, hits=hits, g=g)


def same_frame(a, b):
    return (all(np.array_equal(a[f], b[f]) for f in ("rgba", "mask", "steps")) and a["total"] == b["total"]
            and np.array_equal(a["uv"].view(np.uint32), b["uv"].view(np.uint32))
            and np.array_equal(a["hits"].view(np.uint32), b["hits"].view(np.uint32)))


@pytest.fixture(scope="module")
def unshifted(cpu):
    """geo_render_cpu_disk's frames of the poses, rendered once."""
    out = {}
    for name in T.POSES:
        frame, scene, disk, _ = T.pose(name)
        rc, a = T.render(cpu, frame, scene, T.SKY, W, H, disk, T.TEX)
        assert rc == GEO_OK
        out[name] = a
    return out


@pytest.mark.parametrize("name", ["A", "flat"])
def test_identity(cpu, unshifted, name):
    frame, scene, disk, _ = T.pose(name)
    rc, a = render(cpu, frame, scene, W, H, disk, shift=(1, 0, 1.0))
    assert rc == GEO_OK
    assert same_frame(a, unshifted[name])
    assert (a["hits"][..., 0] > 0.0).sum() > 500
    assert np.array_equal(a["g"] != 0.0, a["hits"][..., 0] != 0.0)
    # no shift given: the unshaded frame, and out_g is not written
    rc, b = render(cpu, frame, scene, W, H, disk, shift=None)
    assert rc == GEO_OK and same_frame(b, unshifted[name]) and (b["g"] == -1.0).all()


@pytest.mark.parametrize("name", ["flat", "tilted"])
def test_flat_space_unmoving(cpu, unshifted, name):
    frame, scene, disk, _ = T.pose(name)
    assert scene.rs == 0.0 and frame.psi_factor_and_position[0] == 0.0
    for exponent in (1, 2, 3, 4):
        for spin in (1, -1):
            rc, a = render(cpu, frame, scene, W, H, disk, shift=(spin, exponent, 1.0))
            assert rc == GEO_OK
            hit = a["hits"][..., 0] > 0.0
            assert hit.sum() > 1000
            assert (a["g"][hit] == np.float32(1.0)).all() and (a["g"][~hit] == 0.0).all()
            assert same_frame(a, unshifted[name])


def face_on():
    """Pose A's observer at rest, the disk's normal along its position: w = 0."""
    pos, cam, fov, rs, _, (r_in, r_out), _, _, ms = T.POSES["A"]
    frame = default_frame(W, H, pos=pos, camera=cam, rs=rs, fov=fov, state=0)
    r_obs = math.sqrt(sum(p * p for p in pos))
    scene = make_scene(rs, 50.0, r_obs, T.STEP, ms, flags=GEO_FLAG_DISK)
    return frame, scene, T.make_disk(r_in, r_out, pos, (0.0, 1.0, 0.0))


def test_face_on(cpu):
    frame, scene, disk = face_on()
    for spin in (1, -1):
        rc, a = render(cpu, frame, scene, W, H, disk, shift=(spin, 4, 1.0))
        assert rc == GEO_OK
        h0 = a["hits"][..., 0, 0] > 0.0
        assert h0.sum() > 300
        r = a["hits"][..., 0, 0][h0].astype(np.float64)
        want = np.sqrt(1.0 - 1.5 * scene.rs / r) / math.sqrt(1.0 - scene.rs / scene.r_obs)
        err = np.abs(a["g"][..., 0][h0] / want - 1.0).max()
        print("face-on: slot-0 hits", int(h0.sum()), "max rel g", err)
        assert err <= S.TOL_G


SIGN_POSE = "A"
PAIR_AZ = 0.004  # turns: a pair's azimuths mirror each other this closely (about one pixel of the image)


def mirror_pairs(hits, frame, scene, normal, axis, spin):
    """Slot-0 hits paired across the image of the disk axis: (ia, ir) flat
    pixel indices, ia on the side whose matter approaches the observer.  The
    hit point and the matter's direction spin * (n x x_hat) are formed in the
    sky frame from (r, U) and the disk basis; the mirror is the plane through
    the disk axis and the observer."""
    n, ex, ey = D.disk_basis(normal, axis)
    obs = D.observer_world(frame, scene.r_obs)
    r = hits[..., 0, 0].astype(np.float64).ravel()
    az = hits[..., 0, 1].astype(np.float64).ravel()
    idx = np.nonzero(r > 0.0)[0]
    r, az = r[idx], az[idx]
    ang = 2.0 * math.pi * az
    xh = np.cos(ang)[:, None] * ex[None, :] + np.sin(ang)[:, None] * ey[None, :]
    vel = spin * np.cross(np.broadcast_to(n, xh.shape), xh)
    towards = ((obs[None, :] - r[:, None] * xh) * vel).sum(axis=-1)
    az_obs = math.atan2(obs.dot(ey), obs.dot(ex)) / (2.0 * math.pi)
    ia, ir = [], []
    rec = np.nonzero(towards < 0.0)[0]
    for i in np.nonzero(towards > 0.0)[0]:
        cand = rec[np.abs(r[rec] / r[i] - 1.0) < 0.01]
        if cand.size == 0:
            continue
        d = D.az_err(az[cand], np.mod(2.0 * az_obs - az[i], 1.0))
        j = cand[int(np.argmin(d))]
        if d.min() <= PAIR_AZ:
            ia.append(idx[i])
            ir.append(idx[j])
    return np.array(ia), np.array(ir)


def test_sign(cpu):
    """The side of the disk whose matter moves towards the observer is the
    brighter one.  Pose A (inclined, curved, the observer falling radially: its
    own Doppler factor is the same on both pixels of a mirror pair)."""
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose(SIGN_POSE)
    ref = D.trace(frame, scene, W, H, r_in, r_out, normal, axis)
    for spin in (1, -1):
        rc, a = render(cpu, frame, scene, W, H, disk, shift=(spin, 4, 1.0))
        assert rc == GEO_OK
        ia, ir = mirror_pairs(a["hits"], frame, scene, normal, axis, spin)
        assert ia.size >= 100
        g = a["g"][..., 0].ravel()
        bad = int((~(g[ia] > g[ir])).sum())
        # the f64 restatement alone, on the same pairs (where it hits both)
        gr = S.shift(frame, scene, W, H, ref, normal, axis, spin)[..., 0].ravel()
        both = ref["hit"][..., 0].ravel()[ia] & ref["hit"][..., 0].ravel()[ir]
        ref_bad = int((~(gr[ia][both] > gr[ir][both])).sum())
        print(f"spin {spin:+d}: {ia.size} pairs, {bad} with g(approaching) <= g(receding); f64 restatement: {ref_bad} "
              f"of {int(both.sum())}")
        assert ref_bad == 0
        assert bad <= 0.01 * ia.size
        # the other spin on the same pixels: the inequality swaps
        rc, o = render(cpu, frame, scene, W, H, disk, shift=(-spin, 4, 1.0))
        assert rc == GEO_OK
        go = o["g"][..., 0].ravel()
        assert int((~(go[ia] < go[ir])).sum()) <= 0.01 * ia.size


# the least hits compared in slots 0 and 1 (pose A: 920 and 34, pose B: 406 and 28)
F64_MIN = {"A": (900, 30), "B": (400, 25)}


@pytest.mark.parametrize("name", list(T.CURVED))
def test_against_f64_restatement(cpu, name):
    """g of slots 0 and 1 against disk_shift_ref (the photon's local direction
    at the hit, no conserved angular momentum), outside the band
    disk_shift_ref.BAND_G of the capture orbit.  The band's share of the hit
    pixels is below the share of the frame disk_ref.compare leaves out on the
    same pose.  With compare's own band, disk_ref.BAND_X, that cannot hold on
    these poses (0.4 % against 0.15 % on pose A, 15 % against 1.8 % on pose B:
    the secondary images lie along the capture orbit), hence the narrower one
    (disk_shift_ref's docstring).  No slot-2 hit of these poses lies outside it."""
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose(name)
    ref = D.trace(frame, scene, W, H, r_in, r_out, normal, axis)
    for spin in (1, -1):
        rc, a = render(cpu, frame, scene, W, H, disk, shift=(spin, 4, 1.0))
        assert rc == GEO_OK
        s = S.compare(a["g"], a["hits"], ref, S.shift(frame, scene, W, H, ref, normal, axis, spin))
        left_out = D.compare(a["hits"], ref, r_in, r_out)["excluded_share"]
        print(name, spin, s, "compare's excluded share of the frame", left_out)
        assert s["compared"][0] >= F64_MIN[name][0] and s["compared"][1] >= F64_MIN[name][1]
        assert s["band_share_of_hits"] < left_out
        assert s["max_rel_g"] <= S.TOL_G


def calibration(cpu):
    """The measured maximum behind TOL_G (disk_shift_ref's docstring)."""
    worst = 0.0
    for pos, r_in, r_out, normal in D.CAL_DISKS:
        r_obs = math.sqrt(sum(p * p for p in pos))
        phi0 = math.atan2(-pos[1], -pos[0])
        th0 = -math.atan2(pos[2], math.hypot(pos[0], pos[1]))
        for dphi, dth in D.CAL_CAMS:
            frame = default_frame(W, H, pos=pos, camera=(phi0 + dphi, th0 + dth))
            scene = make_scene(1.0, 50.0, r_obs, T.STEP, 2048, flags=GEO_FLAG_DISK)
            rc, a = render(cpu, frame, scene, W, H, T.make_disk(r_in, r_out, normal))
            assert rc == GEO_OK
            ref = D.trace(frame, scene, W, H, r_in, r_out, normal)
            s = S.compare(a["g"], a["hits"], ref, S.shift(frame, scene, W, H, ref, normal))
            assert sum(s["compared"]) > 100
            worst = max(worst, s["max_rel_g"])
    return worst


def test_calibration_record(cpu):
    assert S.TOL_G == D.tol_rule(S.CAL_G)
    worst = calibration(cpu)
    print("calibration: max rel g", worst)
    assert worst <= S.CAL_G


def moving_frame(k, w, h):
    """Flat space, the "flat" pose's observer and disk; the camera looks along
    the motion axis (display_to_movement a diagonal rotation, so the centre
    pixel's ray is +z of the moving frame) and movement_to_central turns that
    axis onto the disk point (5, 0, 0); psi_factor_and_position[0] = k."""
    frame, scene, disk, (r_in, r_out, normal, axis) = T.pose("flat", w, h)
    m0 = frame.display_to_movement
    sz = 1.0 if m0[14] > 0.0 else -1.0  # d = M0 (-ny M0[12], -nx M0[13], M0[14])
    rot0 = np.diag([1.0, sz, sz])
    for c in range(3):
        for r in range(3):
            m0[4 * c + r] = rot0[r, c]
    m2, _ = D._m3(frame.central_to_uv)
    obs = D.observer_world(frame, scene.r_obs)
    t = np.array([5.0, 0.0, 0.0]) - obs
    t = m2.T @ (t / np.linalg.norm(t))   # the traced ray's direction of travel, central frame
    c2 = np.array([t[0], t[1], -t[2]])   # the pixel direction that travels along t (geo_disk.h's conventions)
    c2 /= np.linalg.norm(c2)             # (central_to_uv is orthogonal to f32 precision only)
    u = np.cross(c2, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    rot1 = np.stack([u, np.cross(c2, u), c2], axis=1)  # a rotation taking +z to c2
    assert abs(np.linalg.det(rot1) - 1.0) < 1e-12
    for c in range(3):
        for r in range(3):
            frame.movement_to_central[4 * c + r] = rot1[r, c]
    frame.psi_factor_and_position[0] = k
    return frame, scene, disk


@pytest.mark.parametrize("k", [0.3, -0.5])
def test_moving_observer(cpu, k):
    w, h = W + 1, H + 1  # odd: the centre pixel's ray is the camera axis
    frame, scene, disk = moving_frame(k, w, h)
    rc, a = render(cpu, frame, scene, w, h, disk, shift=(1, 4, 1.0))
    assert rc == GEO_OK
    want = S.observer_doppler(frame, w, h)
    hit = a["hits"][..., 0] > 0.0
    assert hit.sum() > 500 and not hit[..., 1:].any()
    kf = float(frame.psi_factor_and_position[0])
    err = np.abs(a["g"][..., 0][hit[..., 0]] / want[hit[..., 0]] - 1.0).max()
    cy, cx = h // 2, w // 2
    centre = math.sqrt((1.0 + kf) / (1.0 - kf))
    print("k", k, "hits", int(hit.sum()), "max rel g", err, "centre g", a["g"][cy, cx, 0], "closed form", centre,
          "centre r", a["hits"][cy, cx, 0, 0])
    assert err <= S.TOL_G
    assert abs(a["hits"][cy, cx, 0, 0] / 5.0 - 1.0) < 1e-3  # the camera axis meets the disk where it was aimed
    assert abs(a["g"][cy, cx, 0] / centre - 1.0) <= S.TOL_G


def scale_np(sample, g, exponent, gain):
    """geo_disk.h's colour step on (..., 4) uint8 samples and f32 g."""
    g = g.astype(np.float32)
    gp = np.ones_like(g)
    for _ in range(exponent):
        gp = (gp * g).astype(np.float32)
    m = np.minimum((np.float32(gain) * gp).astype(np.float32), np.float32(65536.0)).astype(np.float64)
    # fma(c, m, 0.5) in f32: the product is exact in f64, and so is the sum for every m that matters
    v = np.floor((sample[..., :3].astype(np.float64) * m[..., None] + 0.5).astype(np.float32)).astype(np.int64)
    out = sample.copy()
    out[..., :3] = np.minimum(v, 255).astype(np.uint8)
    return out


def test_colour_step(cpu, unshifted):
    frame, scene, disk, _ = T.pose("A")
    plain = T.render(cpu, frame, T.plain_of(scene), T.SKY, W, H)[1]["rgba"]
    one = np.empty((4, 8, 4), np.uint8)
    one[:] = np.array([10, 200, 30, 200], np.uint8)  # one colour, translucent: every sample is that texel
    rc, base = T.render(cpu, frame, scene, T.SKY, W, H, disk, one)
    assert rc == GEO_OK
    saturated = False
    for exponent in (1, 2, 3, 4):
        for gain in (0.25, 1.0, 3.0):
            rc, a = render(cpu, frame, scene, W, H, disk, one, shift=(1, exponent, gain))
            assert rc == GEO_OK
            want = plain.copy()
            for k in (2, 1, 0):
                hk = a["hits"][..., k, 0] > 0.0
                src = scale_np(np.broadcast_to(one[0, 0], want[hk].shape), a["g"][..., k][hk], exponent, gain)
                want[hk] = T.composite_np(src, want[hk])
                if k == 0:
                    saturated = saturated or bool((src[..., :3] == 255).any())
            assert np.array_equal(a["rgba"], want), (exponent, gain)
            assert np.array_equal(a["rgba"][..., 3], base["rgba"][..., 3])
            assert not np.array_equal(a["rgba"], base["rgba"])
    assert saturated
    assert (a["hits"][..., 1, 0] > 0.0).sum() >= 10  # more than one slot was blended


def test_argument_checks(cpu):
    frame, scene, disk, _ = T.pose("A")
    w, h = 16, 9
    frame = default_frame(w, h, pos=T.POSES["A"][0], camera=T.POSES["A"][1], fov=T.POSES["A"][2])

    def rc_of(sc, shift=(1, 4, 1.0), dk=disk):
        return render(cpu, frame, sc, w, h, dk, shift=shift)[0]

    def sc(rs=1.0, mode=0, flags=GEO_FLAG_DISK):
        return make_scene(rs, 50.0, scene.r_obs, T.STEP, 256, mode, flags)

    assert rc_of(sc()) == GEO_OK
    for good in ((-1, 0, 1e-3), (1, 4, 3.0e38)):
        assert rc_of(sc(), good) == GEO_OK
    for bad in ((0, 4, 1.0), (2, 4, 1.0), (-2, 4, 1.0), (1, 5, 1.0), (1, 4, 0.0), (1, 4, -1.0), (1, 4, math.inf),
                (1, 4, math.nan)):
        assert rc_of(sc(), bad) == GEO_EINVAL, bad
    # circular orbits down to the inner edge: r_in > 1.5 rs when shaded
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
    assert rc_of(sc(rs=3.5)) == GEO_EINVAL


def test_g_is_clamped(cpu):
    """An observer at rest 0.2 % outside the horizon, looking outwards through
    its escape cone: the static observer's potential alone is
    1 / sqrt(1 - rs/r_obs) = 22.4, times sqrt(1 - 1.5 rs/r) >= 0.7 on the disk:
    g is GEO_DISK_G_MAX wherever the Doppler factor does not pull it below."""
    w, h = 32, 18
    frame = default_frame(w, h, pos=(1.002, 0.0, 0.0), camera=(0.0, 0.0), fov=0.25, state=0)
    scene = make_scene(1.0, 50.0, 1.002, T.STEP, 2048, flags=GEO_FLAG_DISK)
    rc, a = render(cpu, frame, scene, w, h, T.make_disk(3.0, 9.0, (1.0, 0.0, 1.0)), shift=(1, 4, 1.0))
    assert rc == GEO_OK
    hit = a["hits"][..., 0] > 0.0
    g = a["g"][hit]
    print("clamp: hits", int(hit.sum()), "at the clamp", int((g == G_MAX).sum()), "least g", g.min())
    assert hit.sum() >= 20 and (g == np.float32(G_MAX)).sum() >= 10 and (g <= G_MAX).all() and (g > 10.0).all()


def test_golden_frame(cpu):
    """tests/golden/frame_disk_shift.png (the README's disk pose with the
    shading on: `tools/render_frame.py tests/golden/frame_disk_shift.png --disk
    1.6 2.2 --disk-shift 1 4 1 --cpu --width 480 --height 270`) is what the CPU
    path draws, byte for byte."""
    from schwarzschild_raytracer_wgpu_amd import imageio
    from schwarzschild_raytracer_wgpu_amd.scenes import make_disk_texture, make_sky

    w, h = 480, 270
    frame, scene, disk, _ = T.pose("B", w, h)
    rc, a = render(cpu, frame, scene, w, h, disk, make_disk_texture((1024, 128)), shift=(1, 4, 1.0),
                   sky=make_sky("equirect", (2048, 1024)))
    assert rc == GEO_OK
    gold = imageio.load_texture(os.path.join(T.ROOT, "tests", "golden", "frame_disk_shift.png"))
    assert gold.shape == (h, w, 4)
    diff = (a["rgba"] != gold).any(axis=-1)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the golden frame"
    plain = imageio.load_texture(os.path.join(T.ROOT, "tests", "golden", "frame_disk.png"))
    assert (gold != plain).any(axis=-1).sum() > 1000
