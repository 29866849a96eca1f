"""Round trip, reference -> point path, on the oracle's mirror (CPU only).

The world point that a pixel sees (tests/points_roundtrip_ref.py: the f64
render's sky point, disk_ref.trace's plane crossings) goes through the mirror
of the point path, `O.Rays(..., sides=3, libm=False).update(obs, reset=True)`
and `O.draw_points`, which the HIP kernels equal bit for bit
(tests/test_gpu_points.py), and must land on the pixel it came from.  The
mirror and the kernels share one reading of the reference; the places and
pixels here come from code that shares none of it, so a sign in the inverted
aberration, the far side's + pi or calc_ray_angle's convention would show.

Measured here (rs = 1, 240 x 135; points_roundtrip_ref.MEASURED has the counts
per pose):

* Landing: every near point of every pose lands on its own pixel (573 529
  points, none at distance 1), unmoving, falling (k up to 0.91), orbiting
  (k = 0.79), outside and inside the photon sphere and the horizon.  Every far
  point that far_is_physical keeps lands exactly too.
* Angle, near side, 400 disk points per observer radius, against f64 shooting:
  max |error| 8.8e-5, 6.2e-5, 6.2e-5, 6.5e-5 and 3.9e-4 rad at r_obs = 25, 7,
  2.5, 1.6 and 1.2 (the reference's bar: 5e-4).  Points closer than
  SMALLEST_ANGLE are in; without them r_obs = 25 gives 4.6e-5.
* Resolution: shifting w by +5e-4 / -5e-4 rad moves 100 % / 100 % of the near
  points off their pixel at the fovs chosen in the helper (pi/48, pi/96,
  pi/64).  At fov pi/32 the shares are 99.9 % / 87.7 % (r = 25, unmoving), 0 %
  (k = 0.68) and 0 % (k = 0.55): the aberration shrinks the view, and at
  r = 25 the connector's own error (a fifth of a pixel there) points one way.
* The antipode: a sky point within ~1e-5 rad of sweep pi (the Einstein ring)
  has its azimuth about the observer's axis carried by R sin(sweep) = 5e-4 of
  its position, against 1e-5 of f32 UV granularity in the reference itself.
  The orbiting observer, whose aberration spreads the ring over four times as
  many pixels, met one such pixel under the cameras (pi, 0) (sweep pi - 9e-6,
  near, one pixel off) and (pi + 0.3, 0.1) (sweep pi + 4e-6, far, one pixel
  off); moving that point by 3e-6 moves its pixel by two.  The orbit pose's
  camera (pi + 0.2, -0.1) keeps |sin(sweep)| >= 1.3e-4 for every point; the
  other poses have 7.2e-5 or more, and all land exactly.
"""
import math

import numpy as np
import pytest

import oracle as O
import points_roundtrip_ref as R

MIN_NEAR, MIN_FAR_PHYSICAL = 1000, 100
_cache = {}


def mirror(name):
    """(vertices (2n, 4) of the near + far batch, frame) of a pose's points."""
    if name not in _cache:
        frame, _, obs = R.frame_of(name)
        pts = R.pose_points(name)
        v = O.Rays(R.RS, pts["P"], sides=3, libm=False).update(obs, reset=True)
        v.setflags(write=False)
        _cache[name] = v
    return _cache[name], R.frame_of(name)[0]


@pytest.mark.parametrize("name", list(R.POSES))
def test_landing(name):
    pts = R.pose_points(name)
    v, frame = mirror(name)
    _, xy = O.draw_points(frame, v, R.W, R.H)
    idx, pix = R.connectors(pts)
    n_near = int((~pts["far"]).sum())
    n_far = int(pts["far"].sum())
    n_phys = idx.size - n_near
    d = np.abs(xy[idx] - pix).max(axis=1)
    print(f"{name}: near {n_near} exact {(d[:n_near] == 0).sum()}; far {n_far} physical {n_phys} "
          f"exact {(d[n_near:] == 0).sum()}")
    assert n_near >= MIN_NEAR, (name, n_near)
    if n_far:
        assert n_phys >= MIN_FAR_PHYSICAL, (name, n_far, n_phys)
    bad = np.flatnonzero(d[:n_near] > 0)
    assert bad.size == 0, f"{name}: {bad.size} of {n_near} near points off their pixel, first {pix[bad[:3]]} -> " \
                          f"{xy[idx[bad[:3]]]}"
    bad = n_near + np.flatnonzero(d[n_near:] > 0)
    assert bad.size == 0, f"{name}: {bad.size} of {n_phys} physical far points off their pixel ({n_far - n_phys} " \
                          f"of {n_far} far points left out by far_is_physical), first {pix[bad[:3]]} -> " \
                          f"{xy[idx[bad[:3]]]}"


def test_measured_counts_are_current():
    """MEASURED is what the assertions above saw (libm differences may move a
    count by a pixel or two: 1 %)."""
    for name, m in R.MEASURED.items():
        pts = R.pose_points(name)
        got = (int((~pts["far"]).sum()), int(pts["far"].sum()), int((pts["far"] & pts["physical"]).sum()))
        for g, want in zip(got, (m["near"], m["far"], m["far_physical"])):
            assert abs(g - want) <= 0.01 * want + 2, (name, got, m)


def test_angle_near_side():
    pos, obs = R.angle_cases()
    want, ok = R.angle_reference()
    assert ok.all(), f"shooting did not converge for {(~ok).sum()} points"
    for i, r in enumerate(R.ANGLE_RADII):
        out = O.Rays(R.RS, pos[i], sides=1, libm=False).update(obs[i], reset=True)
        err = np.abs(out[:, 3].astype(np.float64) - want[i])
        print(f"r_obs = {r}: max |angle error| {err.max():.2e} rad")
        assert err.max() < R.ANGLE_TOL, (r, err.max())


@pytest.mark.parametrize("name", R.RESOLUTION_POSES)
def test_resolution(name):
    """The landing check sees an angle error of 5e-4 rad, of either sign."""
    pts = R.pose_points(name)
    v, frame = mirror(name)
    near = np.flatnonzero(~pts["far"])
    for sign in (1.0, -1.0):
        vv = v[near].copy()
        vv[:, 3] += np.float32(sign * R.RESOLUTION_OFFSET)
        _, xy = O.draw_points(frame, vv, R.W, R.H)
        moved = float((np.abs(xy - pts["pix"][near]).max(axis=1) > 0).mean())
        print(f"{name}: w {sign * R.RESOLUTION_OFFSET:+.0e}: {100 * moved:.1f} % of {near.size} near points moved")
        assert moved >= R.RESOLUTION_SHARE, (name, sign, moved)


def test_far_is_physical_against_dense_newton():
    """The helper's batched elimination against a dense solve of the same
    Newton step, on both verdicts."""
    rng = np.random.default_rng(3)
    r_obs = 2.5
    r1 = rng.uniform(2.0, 50.0, 60)
    sweep = rng.uniform(math.pi + 0.05, 2 * math.pi - 0.05, 60)
    got = R.far_is_physical(R.RS, r_obs, r1, sweep)
    want = []
    for a, phi in zip(r1, sweep):
        u = np.linspace(1 / r_obs, 1 / a, R.NR_NODES)
        s = (47 / phi) ** 2
        with np.errstate(all="ignore"):
            for _ in range(5):
                res = s * (-u[:-2] + 2 * u[1:-1] - u[2:]) - u[1:-1] + 1.5 * R.RS * u[1:-1] ** 2
                J = np.diag(2 * s - 1 + 3 * R.RS * u[1:-1]) - s * (np.eye(46, k=1) + np.eye(46, k=-1))
                u[1:-1] -= np.linalg.solve(J, res)
            res = s * (-u[:-2] + 2 * u[1:-1] - u[2:]) - u[1:-1] + 1.5 * R.RS * u[1:-1] ** 2
        want.append(bool(u.min() > 0 and np.abs(res).max() < 1e-6))
    want = np.array(want)
    assert 5 < want.sum() < 55  # both verdicts occur
    assert np.array_equal(got, want)


def test_exact_angle_in_flat_space():
    """rs = 0: the shooting's answer is the Euclidean angle at the observer."""
    rng = np.random.default_rng(4)
    r0 = 7.0
    r1 = rng.uniform(1.0, 30.0, 50)
    sweep = rng.uniform(0.01, math.pi - 0.01, 50)
    got, ok = R.exact_angle(0.0, r0, r1, sweep)
    # the triangle centre - observer - point: the angle at the observer
    want = np.arctan2(r1 * np.sin(sweep), r0 - r1 * np.cos(sweep))
    assert ok.all()
    assert np.abs(got - want).max() < 1e-9
