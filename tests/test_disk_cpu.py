"""GEO_FLAG_DISK on the CPU path (geo_render_cpu_disk, include/geo/geo_cpu.h):
the thin accretion disk through the kernel's own header (csrc/geo_disk.h),
checked against straight-line geometry in flat space, against the f64
restatement tests/disk_ref.py in curved space (primary, secondary and third
image), and for its compositing and argument rules.  tests/test_gpu_disk.py
ties the kernel to this path bit for bit."""
import ctypes
import math
import os

import numpy as np
import pytest

import disk_ref as D
import oracle as O
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_EINVAL, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_MODE_ADAPTIVE, GEO_MODE_FAN,
                                                   GEO_OK, GeoDisk)
from schwarzschild_raytracer_wgpu_amd.scenes import make_disk_texture, make_sky

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "schwarzschild_raytracer_wgpu_amd", "libgeo_cpu.so")
W, H = 96, 54
STEP = math.pi / 100


def load_cpu():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    base = [vp, vp, vp, u32, u32, vp, u32, u32, u32, u32, u32, u32, ctypes.c_int, vp, vp, vp, vp, vp]
    lib.geo_render_cpu.restype = ctypes.c_int
    lib.geo_render_cpu.argtypes = base
    lib.geo_render_cpu_disk.restype = ctypes.c_int
    lib.geo_render_cpu_disk.argtypes = base + [vp, vp, u32, u32, vp]
    return lib


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


def make_disk(r_in, r_out, normal=(0.0, 0.0, 1.0), axis=(1.0, 0.0, 0.0)):
    return GeoDisk(r_in, r_out, (ctypes.c_float * 3)(*normal), (ctypes.c_float * 3)(*axis))


def render(lib, frame, scene, sky, w, h, disk=None, tex=None, row0=0, nrows=None, threads=4, want_hits=True):
    """geo_render_cpu_disk (disk given) or geo_render_cpu."""
    nrows = h - row0 if nrows is None else nrows
    sky = np.ascontiguousarray(sky, dtype=np.uint8)
    rgba = np.zeros((nrows, w, 4), np.uint8)
    mask = np.empty((nrows, w), np.uint8)
    uv = np.empty((nrows, w, 2), np.float32)
    steps = np.empty((nrows, w), np.uint32)
    total = ctypes.c_ulonglong()
    args = [ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1], sky.shape[0], None, 0, w,
            h, row0, nrows, 1, threads, rgba.ctypes.data, mask.ctypes.data, uv.ctypes.data, steps.ctypes.data,
            ctypes.addressof(total)]
    hits = None
    if disk is None:
        rc = lib.geo_render_cpu(*args)
    else:
        tex = np.ascontiguousarray(tex, dtype=np.uint8)
        hits = np.full((nrows, w, 3, 2), -1.0, np.float32) if want_hits else None
        rc = lib.geo_render_cpu_disk(*args, ctypes.addressof(disk), tex.ctypes.data, tex.shape[1], tex.shape[0],
                                     None if hits is None else hits.ctypes.data)
    return rc, dict(rgba=rgba, mask=mask, uv=uv, steps=steps, total=total.value, hits=hits)


# name: (pos, camera, fov, rs, state, (r_in, r_out), normal, axis, max_steps)
POSES = {
    "A": ((14.0, 0.0, 5.1), (math.pi, -0.35), math.pi / 3, 1.0, 1, (3.0, 9.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), 2048),
    "B": ((2.4, 0.0, 0.7), (math.pi, -0.28), math.pi / 2, 1.0, 1, (1.6, 2.2), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), 2048),
    "flat": ((10.0, 3.0, 4.0), (math.pi + 0.2, -0.3), math.pi / 2, 0.0, 0, (3.0, 9.0), (0.0, 0.0, 1.0),
             (1.0, 0.0, 0.0), 512),
    "tilted": ((10.0, 3.0, 4.0), (math.pi + 0.2, -0.3), math.pi / 2, 0.0, 0, (3.0, 9.0), (0.3, -0.2, 1.0),
               (1.0, 0.0, 0.0), 512),
    # the third image: pose A's observer at rest, the camera raised from the
    # direction to the centre by 0.1695 rad onto the photon ring's upper edge
    # (its angular radius there is 0.1692), fov 0.004: pixels of 4e-5 rad
    "ring": ((14.0, 0.0, 5.1), (math.pi, -math.atan2(5.1, 14.0) + 0.1695), 0.004, 1.0, 0, (3.0, 9.0), (0.0, 0.0, 1.0),
             (1.0, 0.0, 0.0), 2048),
}
RING_SLOT2 = 8  # the floor the test asserts; disk_ref finds 148 (test_third_image)


def pose(name, w=W, h=H):
    pos, cam, fov, rs, state, (r_in, r_out), normal, axis, ms = POSES[name]
    frame = default_frame(w, h, pos=pos, camera=cam, rs=rs, fov=fov, state=state)
    r_obs = math.sqrt(sum(p * p for p in pos))
    scene = make_scene(rs, 50.0, r_obs, STEP, ms, flags=GEO_FLAG_DISK)
    return frame, scene, make_disk(r_in, r_out, normal, axis), (r_in, r_out, normal, axis)


SKY = make_sky("equirect", (128, 64))
TEX = make_disk_texture((64, 16))


def plain_of(scene):
    return make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps)


def test_camera_restatement_matches_oracle():
    for name in ("A", "B", "flat"):
        frame, scene, _, _ = pose(name)
        ref = O.render_f64(frame, plain_of(scene), W, H, threads=4)
        c2 = D.camera(frame, W, H)
        theta = np.arctan2(c2[..., 2], np.hypot(c2[..., 0], c2[..., 1]))
        assert np.abs(theta - ref["theta"]).max() < 1e-12, name


def test_observer_position_is_central_to_uv_z():
    for name in ("A", "B", "flat"):
        frame, scene, _, _ = pose(name)
        p = D.observer_world(frame, scene.r_obs)
        assert np.allclose(p, [frame.psi_factor_and_position[i] for i in (1, 2, 3)], rtol=0, atol=2e-6 * scene.r_obs)


@pytest.mark.parametrize("name", ["flat", "tilted"])
def test_flat_space_against_straight_lines(cpu, name):
    """rs = 0: the expected hit is where the segment from the observer to the
    pixel's sky point (50 s(U, V), (U, V) from the f64 oracle) meets the disk
    plane inside the annulus; no ODE on the reference side."""
    frame, scene, disk, (r_in, r_out, normal, axis) = pose(name)
    rc, a = render(cpu, frame, scene, SKY, W, H, disk, TEX)
    assert rc == GEO_OK
    ref = O.render_f64(frame, plain_of(scene), W, H, threads=4)
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
    if name == "flat":
        assert int(want.sum()) == 1662  # the issue's prototype count
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


CURVED = {"A": (500, 20), "B": (300, 20)}


@pytest.fixture(scope="module")
def curved(cpu):
    out = {}
    for name in CURVED:
        frame, scene, disk, (r_in, r_out, normal, axis) = pose(name)
        rc, a = render(cpu, frame, scene, SKY, W, H, disk, TEX)
        assert rc == GEO_OK
        rcp, p = render(cpu, frame, plain_of(scene), SKY, W, H)
        assert rcp == GEO_OK
        ref = D.trace(frame, scene, W, H, r_in, r_out, normal, axis)
        out[name] = (a, p, ref, r_in, r_out)
    return out


@pytest.mark.parametrize("name", list(CURVED))
def test_curved_space_against_disk_ref(curved, name):
    a, p, ref, r_in, r_out = curved[name]
    s = D.compare(a["hits"], ref, r_in, r_out)
    shadow = p["mask"] == 1
    covered = int((shadow & (a["hits"][..., 0, 0] > 0.0)).sum())
    print(name, s, "shadow pixels", int(shadow.sum()), "covered at k=0", covered)
    n0, n1 = CURVED[name]
    assert s["excluded_share"] <= 0.02
    assert s["total0"] >= n0 and s["total1"] >= n1 and s["ref_total0"] >= n0 and s["ref_total1"] >= n1
    assert covered > 0
    assert s["disagree_off_edge"] == 0
    assert s["max_rel_r"] <= D.TOL_R and s["max_az"] <= D.TOL_AZ


def test_third_image(cpu):
    """Pose "ring" (POSES): pose A's observer at rest, the camera on the photon
    ring's upper edge, fov 0.004.  disk_ref finds 148 slot-2 hits there, an
    arc two pixels thick next to the shadow (the test asserts at least
    RING_SLOT2 = 8); the CPU path must report slot 2 on the same pixels up to
    the edge rule.  Every pixel counts: the third image lies inside the 0.02
    band, so radii are not compared (they differ by up to 1.3e-3 relative)."""
    frame, scene, disk, (r_in, r_out, normal, axis) = pose("ring")
    rc, a = render(cpu, frame, scene, SKY, W, H, disk, TEX)
    assert rc == GEO_OK
    ref = D.trace(frame, scene, W, H, r_in, r_out, normal, axis)
    s = D.compare(a["hits"], ref, r_in, r_out, slots=(2,), use_band=False)
    print("ring", s)
    assert s["ref_hits2"] >= RING_SLOT2
    assert s["hits2"] >= RING_SLOT2
    assert s["disagree_off_edge"] == 0


def composite_np(s, d):
    """geo_pixel.h composite_ on (..., 4) uint8 arrays."""
    s = s.astype(np.uint32)
    d = d.astype(np.uint32)
    a = s[..., 3:4]
    ia = 255 - a

    def div255(v):
        p = v + 128
        return (p + (p >> 8)) >> 8

    rgb = div255(s[..., :3] * a + d[..., :3] * ia)
    al = div255(a * 255 + d[..., 3:4] * ia)
    return np.concatenate([rgb, al], axis=-1).astype(np.uint8)


def test_compositing(cpu, curved):
    """(One colour for every slot cannot see the order of the images:
    tests/test_sampler_cpu.py::test_disk and its `disk_order_reversed` mutation do.)"""
    a, p, _, _, _ = curved["A"]
    nohit = ~(a["hits"][..., 0] > 0.0).any(axis=-1)
    assert nohit.any() and (~nohit).any()
    assert np.array_equal(a["rgba"][nohit], p["rgba"][nohit])
    assert np.array_equal(a["mask"], p["mask"]) and np.array_equal(a["steps"], p["steps"])
    assert np.array_equal(a["uv"].view(np.uint32), p["uv"].view(np.uint32))
    assert a["total"] == p["total"]
    frame, scene, disk, _ = pose("A")
    # an opaque one-colour texture: every slot-0 hit is that colour
    colour = np.array([10, 200, 30, 255], np.uint8)
    one = np.empty((4, 8, 4), np.uint8)
    one[:] = colour
    rc, b = render(cpu, frame, scene, SKY, W, H, disk, one)
    assert rc == GEO_OK
    h0 = b["hits"][..., 0, 0] > 0.0
    assert np.array_equal(b["hits"], a["hits"])  # the geometry does not depend on the texture
    assert h0.sum() > 500 and (b["rgba"][h0] == colour).all()
    # half alpha: slots 0 and 1 both hit = composite_ applied twice over the plain frame
    half = one.copy()
    half[..., 3] = 128
    rc, c = render(cpu, frame, scene, SKY, W, H, disk, half)
    assert rc == GEO_OK
    h = c["hits"][..., 0] > 0.0
    two = h[..., 0] & h[..., 1] & ~h[..., 2]
    assert two.sum() >= 10
    src = np.broadcast_to(half[0, 0], p["rgba"][two].shape)
    want = composite_np(src, composite_np(src, p["rgba"][two]))
    assert np.array_equal(c["rgba"][two], want)
    only0 = h[..., 0] & ~h[..., 1] & ~h[..., 2]
    src = np.broadcast_to(half[0, 0], p["rgba"][only0].shape)
    assert np.array_equal(c["rgba"][only0], composite_np(src, p["rgba"][only0]))


def test_argument_checks(cpu):
    frame, scene, disk, _ = pose("A")
    w, h = 16, 9
    frame = default_frame(w, h, pos=POSES["A"][0], camera=POSES["A"][1], fov=POSES["A"][2])

    def rc_of(sc, dk=disk, tex=TEX):
        return render(cpu, frame, sc, SKY, w, h, dk, tex, want_hits=False)[0]

    def sc(rs=1.0, sphere=50.0, r_obs=scene.r_obs, mode=0, flags=GEO_FLAG_DISK):
        return make_scene(rs, sphere, r_obs, STEP, 256, mode, flags)

    assert rc_of(sc()) == GEO_OK
    assert rc_of(sc(flags=GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS)) == GEO_OK
    assert rc_of(sc(rs=0.0)) == GEO_OK
    # geo_render_cpu itself keeps rejecting the flag
    assert render(cpu, frame, sc(), SKY, w, h)[0] == GEO_EINVAL
    # the disk entry point needs the flag
    assert rc_of(sc(flags=0)) == GEO_EINVAL
    for mode in (GEO_MODE_FAN, GEO_MODE_ADAPTIVE):
        assert rc_of(sc(mode=mode)) == GEO_EINVAL
    for fl in (GEO_FLAG_MIPS, GEO_FLAG_COMPOSITE, GEO_FLAG_RING_F64):
        assert rc_of(sc(flags=GEO_FLAG_DISK | fl)) == GEO_EINVAL
    assert rc_of(sc(r_obs=0.9)) == GEO_EINVAL            # observer inside the horizon
    assert rc_of(sc(rs=3.5)) == GEO_EINVAL               # rs >= r_in
    assert rc_of(sc(sphere=8.0)) == GEO_EINVAL           # r_out >= sphere_r
    assert rc_of(sc(sphere=12.0)) == GEO_EINVAL          # r_obs >= sphere_r
    for bad in (make_disk(0.0, 9.0), make_disk(9.0, 3.0), make_disk(3.0, 3.0), make_disk(3.0, 9.0, normal=(0, 0, 0)),
                make_disk(3.0, 9.0, axis=(0, 0, 2.0)), make_disk(3.0, 9.0, axis=(0, 0, 0))):
        assert rc_of(sc(), dk=bad) == GEO_EINVAL


def calibration(cpu):
    """The measured maxima behind TOL_R and TOL_AZ (disk_ref's docstring)."""
    worst_r = worst_az = 0.0
    for pos, r_in, r_out, normal in D.CAL_DISKS:
        r_obs = math.sqrt(sum(p * p for p in pos))
        phi0 = math.atan2(-pos[1], -pos[0])
        th0 = -math.atan2(pos[2], math.hypot(pos[0], pos[1]))
        for dphi, dth in D.CAL_CAMS:
            frame = default_frame(W, H, pos=pos, camera=(phi0 + dphi, th0 + dth))
            scene = make_scene(1.0, 50.0, r_obs, STEP, 2048, flags=GEO_FLAG_DISK)
            rc, a = render(cpu, frame, scene, SKY, W, H, make_disk(r_in, r_out, normal), TEX)
            assert rc == GEO_OK
            ref = D.trace(frame, scene, W, H, r_in, r_out, normal)
            s = D.compare(a["hits"], ref, r_in, r_out)
            assert s["hits0"] > 100
            worst_r = max(worst_r, s["max_rel_r"])
            worst_az = max(worst_az, s["max_az"])
    return worst_r, worst_az


def test_calibration_record(cpu):
    """TOL_R and TOL_AZ follow the rule (4 x the calibration maximum, rounded
    up to a power of two) for the recorded maxima, and the calibration set
    still measures no more than what is recorded."""
    assert D.TOL_R == D.tol_rule(D.CAL_R) and D.TOL_AZ == D.tol_rule(D.CAL_AZ)
    worst_r, worst_az = calibration(cpu)
    print("calibration: max rel r", worst_r, "max az", worst_az)
    assert worst_r <= D.CAL_R and worst_az <= D.CAL_AZ


def test_golden_frame(cpu):
    """tests/golden/frame_disk.png (the frame the README shows: pose B's
    observer and disk, 480 x 270, `tools/render_frame.py tests/golden/frame_disk.png
    --disk 1.6 2.2 --cpu --width 480 --height 270`) is what the CPU path draws,
    byte for byte: the f32 path is fixed (explicit fma, no contraction), so
    any change of the disk's arithmetic or compositing shows here."""
    from schwarzschild_raytracer_wgpu_amd import imageio

    w, h = 480, 270
    frame, scene, disk, _ = pose("B", w, h)
    sky = make_sky("equirect", (2048, 1024))
    rc, a = render(cpu, frame, scene, sky, w, h, disk, make_disk_texture((1024, 128)), want_hits=False)
    assert rc == GEO_OK
    gold = imageio.load_texture(os.path.join(ROOT, "tests", "golden", "frame_disk.png"))
    assert gold.shape == (h, w, 4)
    diff = (a["rgba"] != gold).any(axis=-1)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the golden frame"
