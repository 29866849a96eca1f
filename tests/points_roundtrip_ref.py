"""The reference side of the point path's round trip.

The sphere render says which place each pixel sees; the point path
(geo_rays_* / geo_points_* / geo_draw_points, the reference's RayConnector and
its point shader vs_main) says at which pixel each place is seen.  This module
turns the independent f64 answers for the first half into world points whose
source pixel is known, in numpy and f64, with no code shared with csrc/:

* sky_points:   oracle.render_f64's sky point of every pixel;
* plane_points: disk_ref.trace's crossings of a plane through the centre;
* far_is_physical: whether the connector's own discrete problem (48 nodes,
  Newton from the linear guess, 5 iterations) has a positive converged
  solution -- a property of the reference's algorithm, not of this port: where
  it has none, the reference draws the far-side point elsewhere too;
* exact_angle:  the incoming angle of the two-point problem by f64 shooting.

Feeding those places to the point path must give back the pixel they came from
(tests/test_points_roundtrip_cpu.py on the oracle's mirror, which the HIP
kernels equal bit for bit; tests/test_gpu_points_roundtrip.py on the kernels).

POSES holds the observers.  All at rs = 1, sphere_r = 50, step pi/100, 2048
steps, 240 x 135.  MEASURED holds what the CPU test measured on the mirror
(`libm=False`) for each pose, and the test asserts the counts it can; see
test_points_roundtrip_cpu.py's docstring for the angle maxima.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import disk_ref as D
import oracle as O

RS, SPHERE_R, STEP, MAX_STEPS = 1.0, 50.0, math.pi / 100, 2048
W, H = 240, 135
NR_NODES = 48
ANGLE_TOL = 5e-4          # the reference's bar (tests.rs:26)
ANGLE_RADII = (25.0, 7.0, 2.5, 1.6, 1.2)
R_IN, R_OUT = 1.01 * RS, 0.999 * SPHERE_R   # the annulus wide open

UNMOVING, FALLING, ORBITING = 0, 1, 2
TILT = (0.2, 0.1, 1.0)
FLAT = (0.0, 0.0, 1.0)

# name: pos, state, energy, camera, fov, plane normal (None: sky points only,
# disk_ref.trace needs r_obs > 1.5 rs)
POSES = {
    "r25_rest":        ((25.0, 0.0, 1.0), UNMOVING, 1.0, (math.pi, 0.0), math.pi / 2, FLAT),
    "r25_rest_narrow": ((25.0, 0.0, 1.0), UNMOVING, 1.0, (math.pi + 0.05, 0.0), math.pi / 32, FLAT),
    "r9_fall":         ((9.0, 2.0, 4.0), FALLING, 1.3, (math.pi + 0.2, -0.4), math.pi / 2, TILT),
    "r9_fall_narrow":  ((9.0, 2.0, 4.0), FALLING, 1.3, (math.pi + 0.25, -0.5), math.pi / 32, TILT),
    "r3_fall":         ((3.1, 0.4, 0.9), FALLING, 1.0, (math.pi + 0.1, -0.3), math.pi / 2, TILT),
    "r3_fall_narrow":  ((3.1, 0.4, 0.9), FALLING, 1.0, (math.pi + 0.5, -0.1), math.pi / 32, TILT),
    "r2p5_fall_hole":  ((2.5, 0.0, 0.1), FALLING, 1.0, (math.pi, 0.0), math.pi / 2, FLAT),
    "r2p5_rest_hole":  ((2.5, 0.0, 0.1), UNMOVING, 1.0, (math.pi, 0.0), math.pi / 2, FLAT),
    "r2p5_fall_away":  ((2.5, 0.0, 0.1), FALLING, 1.0, (0.3, 0.2), math.pi / 2, FLAT),
    "r2p5_rest_away":  ((2.5, 0.0, 0.1), UNMOVING, 1.0, (0.3, 0.2), math.pi / 2, FLAT),
    "r1p2_fall":       ((1.2, 0.0, 0.05), FALLING, 1.0, (0.0, 0.0), math.pi / 2, None),
    "r1p2_rest":       ((1.2, 0.0, 0.05), UNMOVING, 1.0, (0.4, 0.3), math.pi / 2, None),
    "r0p8_fall":       ((0.8, 0.0, 0.05), FALLING, 1.0, (0.0, 0.0), math.pi / 2, None),
    # Observer.start_orbit(3.2) from (2.5, 0, 0.1), then 60 update_position(1/60).
    # The camera is one under which no pixel sees the observer's antipode to
    # within 1e-4 rad (MEASURED's ring_margin; under (pi, 0) and (pi + 0.3, 0.1)
    # one pixel does, to 1e-5, and no f32 position can carry that point's
    # azimuth: test_points_roundtrip_cpu.py's docstring)
    "orbit":           ((2.5, 0.0, 0.1), ORBITING, 3.2, (math.pi + 0.2, -0.1), math.pi / 2, FLAT),
    # the resolution test's poses: the three narrow ones at the fov chosen below
    "r25_rest_fine":   ((25.0, 0.0, 1.0), UNMOVING, 1.0, (math.pi + 0.05, 0.0), math.pi / 48, FLAT),
    "r9_fall_fine":    ((9.0, 2.0, 4.0), FALLING, 1.3, (math.pi + 0.25, -0.5), math.pi / 96, TILT),
    "r3_fall_fine":    ((3.1, 0.4, 0.9), FALLING, 1.0, (math.pi + 0.5, -0.1), math.pi / 64, TILT),
}
RESOLUTION_POSES = ("r25_rest_fine", "r9_fall_fine", "r3_fall_fine")
RESOLUTION_OFFSET = 5e-4   # rad, added to and taken from the vertices' w
RESOLUTION_SHARE = 0.9
ORBIT_UPDATES, ORBIT_DT = 60, 1.0 / 60.0


@functools.lru_cache(maxsize=None)
def frame_of(name, w=W, h=H):
    """(frame, scene, observer position f32 (3,)) of a pose, through the
    library's host observer (tests/test_observer_orbit.py ties it to the
    oracle's)."""
    from schwarzschild_raytracer_wgpu_amd import Observer, make_scene

    pos, state, energy, cam, fov, _ = POSES[name]
    o = Observer(RS, fov, w, h)
    o.set_position(*pos)
    o.set_camera(*cam)
    if state == ORBITING:
        assert o.start_orbit(energy)
        for _ in range(ORBIT_UPDATES):
            o.update_position((0.0, 0.0, 0.0), ORBIT_DT)
    else:
        o.set_energy(energy)
        if state == UNMOVING:
            o.start_unmoving()
        else:
            o.start_frozen_fall()
    frame = o.calc_transformation_pipeline()
    p = np.array(o.get_position(), np.float64)
    scene = make_scene(RS, SPHERE_R, float(np.linalg.norm(p)), STEP, MAX_STEPS)
    return frame, scene, p.astype(np.float32)


def _pixels(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32)


def sky_points(frame, scene, w, h):
    """The sky point each pixel sees, from oracle.render_f64: P = sphere_r
    (cos lat cos lon, cos lat sin lon, sin lat), lon = 2 pi U, lat = pi (1/2 -
    V); the ray's sweep is pi/2 - lam.  Near for sweep < pi, far for pi < sweep
    < 2 pi; a ray of neither connector is left out.  Returns dict: P (n, 3)
    f64, pix (n, 2) int32, sweep (n,), far (n,) bool, r (n,)."""
    ref = O.render_f64(frame, scene, w, h, threads=8)
    sky = (ref["mask"] == 0).ravel()
    uv = ref["uv"].astype(np.float64).reshape(-1, 2)
    lon, lat = 2.0 * math.pi * uv[:, 0], math.pi * (0.5 - uv[:, 1])
    R = float(scene.sphere_r)
    P = R * np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], -1)
    sweep = math.pi / 2 - ref["lam"].ravel()
    near = sky & (sweep < math.pi)
    far = sky & (sweep > math.pi) & (sweep < 2.0 * math.pi)
    keep = near | far
    return dict(P=P[keep], pix=_pixels(w, h)[keep], sweep=sweep[keep], far=far[keep], r=np.full(int(keep.sum()), R))


def plane_points(frame, scene, w, h, normal, axis=(1.0, 0.0, 0.0)):
    """Where each pixel's ray crosses the plane through the centre, from
    disk_ref.trace with the annulus wide open: crossing k at (r, az) is the
    world point r (cos 2 pi az ex + sin 2 pi az ey) of disk_basis.  Crossing 0
    is a near point, crossing 1 a far point (sweep: the angle at the centre
    between the point and the observer, or 2 pi minus it); crossing 2 is
    dropped.  Same dict as sky_points."""
    t = D.trace(frame, scene, w, h, R_IN, R_OUT, normal=normal, axis=axis)
    _, ex, ey = D.disk_basis(normal, axis)
    obs = D.observer_world(frame, float(scene.r_obs))
    pix = _pixels(w, h)
    out = dict(P=[], pix=[], sweep=[], far=[], r=[])
    for k in (0, 1):
        hit = t["hit"][..., k].ravel()
        r = t["r"][..., k].ravel()[hit]
        az = 2.0 * math.pi * t["az"][..., k].ravel()[hit]
        P = r[:, None] * (np.cos(az)[:, None] * ex + np.sin(az)[:, None] * ey)
        d = np.arccos(np.clip(P @ obs / (r * np.linalg.norm(obs)), -1.0, 1.0))
        out["P"].append(P)
        out["pix"].append(pix[hit])
        out["sweep"].append(d if k == 0 else 2.0 * math.pi - d)
        out["far"].append(np.full(r.size, k == 1))
        out["r"].append(r)
    return {f: np.concatenate(v) for f, v in out.items()}


def _fd_residual(u, s, rs):
    return s[:, None] * (-u[:, :-2] + 2.0 * u[:, 1:-1] - u[:, 2:]) - u[:, 1:-1] + 1.5 * rs * u[:, 1:-1] ** 2


def far_is_physical(rs, r_obs, r_point, sweep):
    """f64 Newton on the connector's own finite-difference problem -- 48 nodes
    of u = 1/r equally spaced over `sweep`, residual (-u[i-1] + 2 u[i] -
    u[i+1]) / h^2 - u[i] + 1.5 rs u[i]^2 -- from the linear guess, 5
    iterations.  True where every node is > 0 and the largest residual is
    < 1e-6.  Elementwise over r_point and sweep."""
    r1, phi = np.broadcast_arrays(np.asarray(r_point, np.float64), np.asarray(sweep, np.float64))
    shape = r1.shape
    r1, phi = r1.ravel(), phi.ravel()
    wgt = np.linspace(0.0, 1.0, NR_NODES)
    u = (1.0 / r_obs) * (1.0 - wgt)[None, :] + (1.0 / r1)[:, None] * wgt[None, :]
    s = (float(NR_NODES - 1) / phi) ** 2
    n = NR_NODES - 2
    with np.errstate(all="ignore"):
        for _ in range(5):
            res = _fd_residual(u, s, rs)
            diag = 2.0 * s[:, None] - 1.0 + 3.0 * rs * u[:, 1:-1]
            c = np.empty_like(res)
            d = np.empty_like(res)
            c[:, 0] = -s / diag[:, 0]
            d[:, 0] = res[:, 0] / diag[:, 0]
            for i in range(1, n):   # the tridiagonal Jacobian, by elimination
                m = diag[:, i] + s * c[:, i - 1]
                c[:, i] = -s / m
                d[:, i] = (res[:, i] + s * d[:, i - 1]) / m
            for i in range(n - 2, -1, -1):
                d[:, i] -= c[:, i] * d[:, i + 1]
            u[:, 1:-1] -= d
        res = _fd_residual(u, s, rs)
        ok = (u.min(axis=1) > 0.0) & (np.abs(res).max(axis=1) < 1e-6)
    return ok.reshape(shape)


def ray_angle(rs, r, u_bar, near=True):
    """calc_ray_angle's formula (ray_connector.rs:141-157) in f64: the angle
    between the incoming ray and the direction to the centre, from the slope
    u_bar = du/dphi at the observer (radius r); negated for the far side."""
    u_bar, r = np.broadcast_arrays(np.asarray(u_bar, np.float64), np.asarray(r, np.float64))
    with np.errstate(all="ignore"):
        q = r * r * u_bar * u_bar / (1.0 - rs / r)
        outside = np.sign(u_bar) * np.arccos(np.sqrt(1.0 / (1.0 + q)))
        inside = np.where(-q - 1.0 > 0.0, -math.pi / 2 + np.arctan(np.sqrt(1.0 / (-q - 1.0))), 0.0)
    theta = np.where(r > rs, outside, inside)
    return (math.pi / 2 - theta) * (1.0 if near else -1.0)


def _shoot(u0, p, phi, rs, steps):
    """u(phi) of u'' = -u + 1.5 rs u^2, u(0) = u0, u'(0) = p: RK4, `steps`
    steps.  Returns (u, escaped, captured): a ray that reached u <= 0 (left to
    infinity) or else u > 1/rs (passed the horizon) on the way is no path to
    the point; the flags say on which side of the wanted slope it lies."""
    h = phi / steps
    c = 1.5 * rs
    cap = 1.0 / rs if rs > 0.0 else math.inf
    u = u0 + 0.0 * p
    v = p.copy()
    escaped = np.zeros(p.shape, bool)
    captured = np.zeros(p.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            k1u, k1v = v, -u + c * u * u
            a = u + 0.5 * h * k1u
            k2u, k2v = v + 0.5 * h * k1v, -a + c * a * a
            a = u + 0.5 * h * k2u
            k3u, k3v = v + 0.5 * h * k2v, -a + c * a * a
            a = u + h * k3u
            k4u, k4v = v + h * k3v, -a + c * a * a
            u = u + h / 6.0 * (k1u + 2.0 * k2u + 2.0 * k3u + k4u)
            v = v + h / 6.0 * (k1v + 2.0 * k2v + 2.0 * k3v + k4v)
            escaped |= (u <= 0.0) & ~captured      # whichever comes first
            captured |= ~(u <= cap) & ~escaped
    return u, escaped, captured


def exact_angle(rs, r_obs, r_point, sweep, near=True, steps=2000, tol=1e-14):
    """The incoming angle of the ray from an observer at radius r_obs > rs to
    a point at radius r_point, `sweep` radians around the centre: the
    boundary-value problem u'' = -u + 1.5 rs u^2, u(0) = 1/r_obs, u(sweep) =
    1/r_point by f64 shooting (RK4, `steps` steps).  The slope u'(0) comes
    from a bracketed root search that starts at the straight chord's slope and
    grows the bracket outwards; a slope whose ray escapes before `sweep` counts
    as too low and one that is captured as too high, so the miss is monotone in
    the slope and the root found is the ray that stays outside the horizon.
    Then Illinois false position (bisection while an end is such a ray).
    Returns (angle, converged), elementwise; r_obs may be an array too."""
    r0, r1, phi = np.broadcast_arrays(np.asarray(r_obs, np.float64), np.asarray(r_point, np.float64),
                                      np.asarray(sweep, np.float64))
    shape = phi.shape
    r0, r1, phi = r0.ravel(), r1.ravel(), phi.ravel()
    u0, u1 = 1.0 / r0, 1.0 / r1

    def F(p, idx):
        u, esc, cap = _shoot(u0[idx], p, phi[idx], rs, steps)
        return np.where(cap, np.inf, np.where(esc, -np.inf, u - u1[idx]))

    n = phi.size
    every = np.arange(n)
    # the straight line through both ends: u = u0 cos(phi) + p sin(phi)
    p0 = (u1 - u0 * np.cos(phi)) / np.sin(phi)
    f0 = F(p0, every)
    a, b, fa, fb = p0.copy(), p0.copy(), f0.copy(), f0.copy()
    below, above, f_below, f_above = p0.copy(), p0.copy(), f0.copy(), f0.copy()
    delta = 1e-3 * (np.abs(p0) + u0)
    bracketed = f0 == 0.0
    for _ in range(40):
        i = np.flatnonzero(~bracketed)
        if i.size == 0:
            break
        nb, na = below[i] - delta[i], above[i] + delta[i]
        fnb, fna = F(nb, i), F(na, i)
        up = np.sign(fna) != np.sign(f0[i])
        down = ~up & (np.sign(fnb) != np.sign(f0[i]))
        # the bracket is the last step on the side that changed sign
        a[i] = np.where(up, above[i], np.where(down, nb, a[i]))
        fa[i] = np.where(up, f_above[i], np.where(down, fnb, fa[i]))
        b[i] = np.where(up, na, np.where(down, below[i], b[i]))
        fb[i] = np.where(up, fna, np.where(down, f_below[i], fb[i]))
        bracketed[i] = up | down
        below[i], above[i], f_below[i], f_above[i] = nb, na, fnb, fna
        delta[i] = 4.0 * delta[i]
    p, fp = a.copy(), fa.copy()
    side = np.zeros(n, np.int8)
    active = bracketed & (fa != 0.0)
    for _ in range(200):
        i = np.flatnonzero(active)
        if i.size == 0:
            break
        ai, bi, fai, fbi = a[i], b[i], fa[i], fb[i]
        with np.errstate(all="ignore"):
            pi = (ai * fbi - bi * fai) / (fbi - fai)
        pi = np.where(np.isfinite(pi) & (pi > ai) & (pi < bi), pi, 0.5 * (ai + bi))
        fpi = F(pi, i)
        p[i], fp[i] = pi, fpi
        left = np.sign(fpi) == np.sign(fai)   # the root lies in [p, b]
        # Illinois: an end kept twice in a row has its value halved
        fbi = np.where(left & (side[i] == -1), 0.5 * fbi, fbi)
        fai = np.where(~left & (side[i] == 1), 0.5 * fai, fai)
        a[i], fa[i] = np.where(left, pi, ai), np.where(left, fpi, fai)
        b[i], fb[i] = np.where(left, bi, pi), np.where(left, fbi, fpi)
        side[i] = np.where(left, -1, 1)
        active[i] = np.abs(fpi) >= tol
    ok = bracketed & (np.abs(fp) < tol)
    return ray_angle(rs, r0, p, near).reshape(shape), ok.reshape(shape)


def angle_cases():
    """The angle test's points: 400 of the accretion disk's (r in 16..26) per
    observer radius of ANGLE_RADII, the observer just off the x axis.  Returns
    (pos (5, 400, 3) f32, obs (5, 3) f32)."""
    from test_points import accretion_disk

    pos = np.stack([accretion_disk(400, seed=int(10 * r)) for r in ANGLE_RADII])
    obs = np.array([[r * math.cos(0.012), 0.0, r * math.sin(0.012)] for r in ANGLE_RADII], np.float32)
    return pos, obs


@functools.lru_cache(maxsize=None)
def angle_reference():
    """(exact near-side angle (5, 400), converged (5, 400)) of angle_cases()."""
    pos, obs = angle_cases()
    p, o = pos.astype(np.float64), obs.astype(np.float64)
    r0 = np.linalg.norm(o, axis=1)[:, None]
    r1 = np.linalg.norm(p, axis=2)
    sweep = np.arccos(np.clip(np.einsum("ijk,ik->ij", p, o) / (r0 * r1), -1.0, 1.0))
    return exact_angle(RS, r0, r1, sweep)


def _physical(scene, pts):
    phys = np.ones(pts["far"].shape, bool)
    f = pts["far"]
    phys[f] = far_is_physical(float(scene.rs), float(scene.r_obs), pts["r"][f], pts["sweep"][f])
    return phys


@functools.lru_cache(maxsize=None)
def pose_points(name, w=W, h=H):
    """Every reference point of a pose, sky points first, then plane points
    (where the pose has a plane): dict P (n, 3) f32, pix (n, 2), far (n,),
    physical (n,) (far_is_physical; True for every near point), plane (n,)."""
    frame, scene, _ = frame_of(name, w, h)
    parts = [sky_points(frame, scene, w, h)]
    normal = POSES[name][5]
    if normal is not None:
        parts.append(plane_points(frame, scene, w, h, normal))
    out = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
    out["plane"] = np.concatenate([np.full(p["far"].size, i == 1) for i, p in enumerate(parts)])
    out["physical"] = _physical(scene, out)
    out["P"] = out["P"].astype(np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


def connectors(pts):
    """Which connectors of a near + far batch over pts["P"] (near side first)
    the landing check reads: every near point's near connector and every
    physical far point's far connector.  Returns (index into the 2n
    connectors, source pixel of each)."""
    n = pts["far"].size
    near = np.flatnonzero(~pts["far"])
    far = np.flatnonzero(pts["far"] & pts["physical"])
    return np.concatenate([near, n + far]), np.concatenate([pts["pix"][near], pts["pix"][far]])


# What tests/test_points_roundtrip_cpu.py measured on the mirror per pose: k is
# the frame's aberration factor; every near point and every far point that
# far_is_physical keeps landed on its own pixel (near_exact == near, far_exact
# == far_physical); 1 - far_physical / far is the share of far-side points the
# reference's connector (and this port) draws elsewhere; ring_margin is the
# smallest |sin(sweep)| among the points with sweep > pi/2 (the test's docstring
# says why it matters).
MEASURED = {
    "r25_rest":        dict(k=0.000, near=47802, far=1238, far_physical=258, ring_margin=6.0e-4),
    "r25_rest_narrow": dict(k=0.000, near=14863, far=10031, far_physical=484, ring_margin=3.2e-3),
    "r9_fall":         dict(k=0.683, near=47231, far=569, far_physical=118, ring_margin=4.1e-4),
    "r9_fall_narrow":  dict(k=0.683, near=32400, far=31960, far_physical=8144, ring_margin=3.7e-4),
    "r3_fall":         dict(k=0.554, near=50733, far=4157, far_physical=2654, ring_margin=1.2e-4),
    "r3_fall_narrow":  dict(k=0.554, near=32197, far=20831, far_physical=3347, ring_margin=2.1e-3),
    "r2p5_fall_hole":  dict(k=0.632, near=43102, far=5958, far_physical=4856, ring_margin=1.5e-4),
    "r2p5_rest_hole":  dict(k=0.000, near=23396, far=16038, far_physical=9672, ring_margin=9.4e-4),
    "r2p5_fall_away":  dict(k=0.632, near=44720, far=0, far_physical=0, ring_margin=1.0),
    "r2p5_rest_away":  dict(k=0.000, near=45551, far=0, far_physical=0, ring_margin=0.92),
    "r1p2_fall":       dict(k=0.912, near=32400, far=0, far_physical=0, ring_margin=1.0),
    "r1p2_rest":       dict(k=0.000, near=19749, far=2440, far_physical=2440, ring_margin=7.2e-5),
    "r0p8_fall":       dict(k=0.895, near=32400, far=0, far_physical=0, ring_margin=1.0),
    "orbit":           dict(k=0.786, near=32820, far=12222, far_physical=9821, ring_margin=1.3e-4),
    "r25_rest_fine":   dict(k=0.000, near=9365, far=5044, far_physical=228, ring_margin=7.9e-4),
    "r9_fall_fine":    dict(k=0.683, near=32400, far=14525, far_physical=11699, ring_margin=2.7e-4),
    "r3_fall_fine":    dict(k=0.554, near=32400, far=24988, far_physical=5313, ring_margin=6.4e-4),
}
# The resolution test: share of near points that leave their pixel when w is
# shifted by (+5e-4, -5e-4) rad, at fov pi/32 and at the fov chosen (the widest
# of pi/32, /40, /48, /64, /96, /128 at which both shares reach 90 % and the
# unshifted landing stays exact, which it does at every one of them).
MOVED_AT_PI_32 = {"r25_rest_narrow": (0.999, 0.877), "r9_fall_narrow": (0.0, 0.0), "r3_fall_narrow": (0.0, 0.0)}
MOVED = {"r25_rest_fine": (1.0, 1.0), "r9_fall_fine": (1.0, 1.0), "r3_fall_fine": (1.0, 1.0)}
