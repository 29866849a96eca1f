"""An independent f64 answer for GEO_FLAG_DISK (the thin accretion disk).

numpy, f64, no code shared with csrc/geo_disk.h:

* the camera of shader.wgsl:60-75 restated (pixel centre NDC, FOV column,
  display_to_movement, the aberration sin(l') = (s - k)/(1 - s k) as the
  boost along z, movement_to_central); its angle to the black hole equals
  oracle.render_f64's `theta` to ~4e-15 (test_disk_cpu checks 1e-12);
* the ray in its plane: u0 = 1/r, u0' = (E/r) tan(theta), E = sqrt(1 - rs/r);
* RK4 of the Binet equation u'' = -u + (3 rs/2) u^2 at step/8, with a partial
  RK4 step from the fine node below each crossing angle a_k = a_0 + k pi;
* the hit rule of include/geo/geo.h: crossing k (k < 3) is a hit when a_k lies
  within the angle the main loop integrates (before the ray leaves the sky
  sphere, u <= 1/sphere_r; before the horizon, u > 1/rs with u' > 0; before
  the budget max_steps * step) and r_in <= 1/u(a_k) <= r_out.

At step/8 (sub=8, the truth of the pi/100 layers) "within the angle the loop
integrates" is left to u(a_k) itself: a ray that left the sphere inside the fine
step before a_k shows u(a_k) < 1/sphere_r, outside the annulus.  That holds in
the continuum and at a fine step.  At the scene's own step (sub=1, the same
discrete map in f64: it measures the rounding of the path, not truncation, and
so is an answer at every step and budget) it does not, and trace states the
rule's remaining clauses as geo.h has them, in f64 and from the reference's own
text (sphere_ray_tracer.rs:60-191 restated: _ended_before_the_loop, the loop's
exit tests with `bound`, _newton):

* crossing k counts only while its node floor(a_k / step) lies below the step
  count (the loop executed the step that starts there);
* crossing k counts only while a_k lies below the traveled angle the loop
  returns: node * step + Newton's step length (three iterations from the steeper
  end) where the stopping step crosses the sphere, NO_VALUE = 15 > a_2 otherwise;
* a ray that the reference's pre-filters or radial cases end before the loop
  draws nothing.

The second clause is not implied by u(a_k): for step > 2.28 three Newton
iterations on an RK4 step of that length do not converge and can return a
negative length (-0.2 step to -1271 steps where it matters), so the returned
angle lies below a crossing the loop has already probed with u(a_k) inside the
annulus.  On tests/fuzz_disk_scenes.py's seeds 0..399 that happens on 244 slots
of six seeds (tests/disk_step_truth.py's ANGLE_CLAUSE_SEEDS), every one of them
"u(a_k) in the annulus, a_k >= angle"; with the clause stated the CPU path and
this trace disagree on no slot off the annulus' edges, and the pre-filters and
the node clause change none (the observers inside the photon sphere included).
The constants below, TOL_R_BAND and disk_truth.py's were all measured with sub=8
or at step pi/100, where Newton's length lies inside its step: none of them moves
(tests/test_disk_step_truth_cpu.py::test_the_clauses_change_nothing_at_the_truth_step).

The sub=8 trace holds for every observer between the horizon and the sky sphere (or
rs = 0) as long as the disk lies outside the photon sphere, r_in > 1.5 rs,
which GEO_FLAG_DISK's scenes in tests/fuzz_disk_scenes.py keep.  Inside the
photon sphere the reference's pre-filters (sphere_ray_tracer.rs:106-119) end
some rays before the loop: those that start inwards (they fall into the
horizon: the potential has no barrier below 1.5 rs) and those that start
outwards with b > b_c (they turn back below the photon sphere).  Either kind
stays at r < 1.5 rs < r_in, so no crossing of it is a hit on either side: the
filters cannot change a hit, and the trace needs none of them.
tests/disk_truth.py runs the trace over the fuzzed observers (inside the
photon sphere, under a small sky sphere, tilted and edge-on disks) and counts
no hit/no-hit disagreement off the annulus' edges.

trace also returns `cond` = hypot(A, B) of a_0 = atan2(-B, A), the length of
the disk normal's projection onto the ray's plane: a_0, and with it every
crossing's radius and azimuth, is conditioned like 1/cond (cond -> 0 where the
ray's plane nearly contains the disk's plane).

Tolerances (the scheme of f64_bar.py's K_AMP and A_DIR): the CPU path
(geo_render_cpu_disk, bit-equal to the kernel) was measured against this
module on a calibration set that is none of the test poses -- the disk 3..9
(normal (0.2, 0.1, 1)) seen from (9, 2, 4) and the disk 1.6..2.2 seen from
(3.1, 0.4, 0.9), each under five cameras (phi, theta) offsets (0, 0),
(0.25, 0.1), (-0.3, 0.05), (0.1, -0.2), (-0.15, 0.15) from the direction to
the centre, 96 x 54, fov pi/2, every pixel with |b/b_c - 1| >= 0.02, every
slot hit on both sides:

    max relative radius error   2.46e-5  (CAL_R)
    max azimuth error (turns)   1.45e-7  (CAL_AZ)

each multiplied by 4 (a finite calibration set) and rounded up to a power of
two.  tests/test_disk_cpu.py::test_calibration_record re-measures them and
checks the constants against the rule.
"""
from __future__ import annotations

import math

import numpy as np

CAL_R = 2.5e-5    # measured maximum 2.46e-5, relative radius (calibration set above)
CAL_AZ = 1.5e-7   # measured maximum 1.45e-7, azimuth in turns
TOL_R = 2.0 ** -13   # 1.22e-4: 4 * CAL_R = 1.0e-4 rounded up to a power of two
TOL_AZ = 2.0 ** -20  # 9.5e-7: 4 * CAL_AZ = 6.0e-7 rounded up to a power of two
BAND_X = 0.02     # |b/b_c - 1| below which a pixel is left to the bit-equality tests
MAX_CROSSINGS = 3
NO_VALUE = 15.0   # the traveled angle of a ray that never crosses the sky sphere (sphere_ray_tracer.rs:22)
NEWTON_STEP_MAX = 0.5  # the step up to which Newton's length lies inside its step (trace, sub=1)

CAL_DISKS = [((9.0, 2.0, 4.0), 3.0, 9.0, (0.2, 0.1, 1.0)), ((3.1, 0.4, 0.9), 1.6, 2.2, (0.2, 0.1, 1.0))]
CAL_CAMS = [(0.0, 0.0), (0.25, 0.1), (-0.3, 0.05), (0.1, -0.2), (-0.15, 0.15)]


def tol_rule(measured: float) -> float:
    """4 x the measured maximum, rounded up to a power of two."""
    return 2.0 ** math.ceil(math.log2(4.0 * measured))


def _m3(m16):
    """3 x 3 part of a column-major 4 x 4 (f32 values, f64 arithmetic)."""
    a = np.array([float(v) for v in m16], dtype=np.float64).reshape(4, 4).T
    return a[:3, :3], a


def camera(frame, width, height, k=None):
    """Per pixel, in f64: the unit direction c2 (h, w, 3) in the black-hole-
    central frame (shader.wgsl:60-75).  k: the frame's own aberration factor
    unless given (trace's mutation)."""
    m0_3, m0 = _m3(frame.display_to_movement)
    m1_3, _ = _m3(frame.movement_to_central)
    k = float(frame.psi_factor_and_position[0]) if k is None else k
    px = np.arange(width, dtype=np.float64)[None, :]
    py = np.arange(height, dtype=np.float64)[:, None]
    nx = (2.0 * px + 1.0 - width) / width + 0.0 * py
    ny = (height - 2.0 * py - 1.0) / height + 0.0 * px
    # column 3 of display_to_movement carries the FOV scale (observer.rs:253-254)
    v = np.stack([-ny * m0[0, 3], -nx * m0[1, 3], np.full_like(nx, m0[2, 3])], axis=-1)
    d = v @ m0_3.T
    L = np.linalg.norm(d, axis=-1)
    den = L - k * d[..., 2]
    e = np.stack([d[..., 0] * math.sqrt(1.0 - k * k) / den, d[..., 1] * math.sqrt(1.0 - k * k) / den,
                  (d[..., 2] - k * L) / den], axis=-1)
    return e @ m1_3.T


def observer_world(frame, r_obs):
    m2, _ = _m3(frame.central_to_uv)
    return r_obs * (m2 @ np.array([0.0, 0.0, 1.0]))


def disk_basis(normal, axis):
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    a = np.asarray(axis, dtype=np.float64)
    ex = a - a.dot(n) * n
    ex = ex / np.linalg.norm(ex)
    return n, ex, np.cross(n, ex)


def _f(u, c):
    return -u + c * u * u


def _rk4(u, v, h, c):
    """One RK4 step of (u, v)' = (v, f(u)), elementwise step h."""
    k1u, k1v = v, _f(u, c)
    k2u, k2v = v + 0.5 * h * k1v, _f(u + 0.5 * h * k1u, c)
    k3u, k3v = v + 0.5 * h * k2v, _f(u + 0.5 * h * k2u, c)
    k4u, k4v = v + h * k3v, _f(u + h * k3u, c)
    return u + h / 6.0 * (k1u + 2 * k2u + 2 * k3u + k4u), v + h / 6.0 * (k1v + 2 * k2v + 2 * k3v + k4v)


def _ended_before_the_loop(rs, R, r0, E, st, ct):
    """The rays the reference's radial cases and pre-filters end before the RK4 loop
    (sphere_ray_tracer.rs:60-119, restated for r0 > rs): they integrate nothing and draw
    no disk.  st, ct: sin and cos of the ray's angle to the black hole."""
    rotation = r0 * ct
    falling = st > 0.0
    inside_sphere, sphere_outside = r0 < R, R > rs
    with np.errstate(divide="ignore"):
        inv_b2 = (E / rotation) ** 2
    barrier = (rs > 0.0) & (inv_b2 < 4.0 / (27.0 * rs * rs)) if rs > 0.0 else np.zeros(st.shape, dtype=bool)
    r3_2 = 1.5 * rs
    different_sides = ((r0 < r3_2) != (R < r3_2)) and abs(r0 - r3_2) > 1e-10
    return ((rotation < 1e-10) | (inside_sphere and not sphere_outside) | (barrier & different_sides) |
            ((r0 < r3_2 and inside_sphere) & falling) | ((r0 > r3_2 and not inside_sphere) & ~falling))


def _newton(u, v, nu, nv, su, h, c):
    """The reference's three Newton iterations on the step length from the steeper end
    (sphere_ray_tracer.rs:150-181): the length at which the RK4 map from (u, v) meets su."""
    first = np.abs(v) > np.abs(nv)
    ns = np.where(first, 0.0, h)
    wu, wv = np.where(first, u, nu), np.where(first, v, nv)
    for _ in range(3):
        with np.errstate(divide="ignore", invalid="ignore"):
            ns = ns - (wu - su) / wv
            wu, wv = _rk4(u, v, ns, c)
    return ns


# wrong traces for tests/disk_truth.py's mutation test: the aberration dropped (k = 0),
# E = 1 in the initial slope, flat geodesics in a curved scene (c = 0), the azimuth's sense
# flipped, the slots shifted by one (slot k holds crossing k + 1), and the budget ignored
# (in the crossing condition and in t_end)
RULES = ("full", "no_angle_clause", "u_only")
MUTATIONS = ("no_aberration", "slope_e1", "flat_c", "az_flipped", "slot_shift", "budget_ignored")


def trace(frame, scene, width, height, r_in, r_out, normal=(0.0, 0.0, 1.0), axis=(1.0, 0.0, 0.0), sub=8,
          mutation=None, rule=None):
    """dict: hit (h, w, 3) bool, r, az (h, w, 3) f64 (radius and azimuth in
    turns in [0, 1) of each crossing, nan where the ray never got there), x
    (h, w) = |b/b_c - 1| (inf for rs = 0), theta (h, w), cond (h, w) = hypot(A, B)
    of a_0 = atan2(-B, A) (the docstring's conditioning of a_0); with sub=1 also
    angle (h, w), the traveled angle of the sphere crossing (NO_VALUE where the ray
    never crosses), steps (h, w), the executed steps, and node (h, w, 3) = floor(a_k / step).

    rule: one of RULES; None is "full" with sub=1 (the scene's own step: the hit rule
    stated in full) and "u_only" otherwise (the three clauses of the module's docstring
    left to u(a_k), as before they were stated; the only rule off the scene's own step).
    "no_angle_clause" drops the clause a_k < angle alone: what
    tests/test_disk_step_truth_cpu.py's named seeds are shown on.

    mutation: None, or one of MUTATIONS: a deliberately wrong trace that
    tests/disk_truth.py's checks must refuse (nothing else reads it)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    rule = ("full" if sub == 1 else "u_only") if rule is None else rule
    assert rule in RULES and (sub == 1 or rule == "u_only"), (sub, rule)
    rs, R, r0 = float(scene.rs), float(scene.sphere_r), float(scene.r_obs)
    step, budget = float(scene.step), int(scene.max_steps)
    c2 = camera(frame, width, height, k=0.0 if mutation == "no_aberration" else None)
    rho = np.hypot(c2[..., 0], c2[..., 1])
    st = np.clip(c2[..., 2], -1.0, 1.0)
    theta = np.arctan2(st, rho)
    cphi, sphi = c2[..., 0] / rho, c2[..., 1] / rho
    m2, _ = _m3(frame.central_to_uv)
    n, ex, ey = disk_basis(normal, axis)
    N, Ex, Ey = m2.T @ n, m2.T @ ex, m2.T @ ey
    A = N[0] * cphi + N[1] * sphi
    B = N[2]
    a0 = np.mod(np.arctan2(-B, A), math.pi)
    a0 = np.where(a0 <= 0.0, math.pi, a0)  # in (0, pi]
    E = math.sqrt(1.0 - rs / r0) if rs > 0.0 else 1.0
    u = np.full(rho.shape, 1.0 / r0)
    v = ((1.0 if mutation == "slope_e1" else E) / r0) * st / rho
    c = 0.0 if mutation == "flat_c" else 1.5 * rs
    su, hu = 1.0 / R, (1.0 / rs if rs > 0.0 else math.inf)
    h = step / sub
    ak = a0[..., None] + math.pi * np.arange(MAX_CROSSINGS)[None, None, :]
    if mutation == "slot_shift":
        ak = ak + math.pi
    if mutation == "budget_ignored":
        budget = 2 ** 30
    t_end = min(float(ak.max()) + step, budget * step)
    nsub = int(math.ceil(t_end / h))
    full = rule != "u_only"  # the rule's remaining clauses (the docstring)
    alive = np.ones(rho.shape, dtype=bool)
    angle = np.full(rho.shape, NO_VALUE)
    steps = np.full(rho.shape, budget, dtype=np.int64)
    if full:
        alive &= ~_ended_before_the_loop(rs, R, r0, E, st, rho / np.hypot(rho, st)) & (budget > 0)
        steps[~alive] = 0
        bound = 0.9 * min(1.0 / r0, 1.0 / max(R, 1.5 * rs))
        if step > NEWTON_STEP_MAX:
            nsub = int(scene.max_steps)  # (the loop ends with the last ray)
    uk = np.full(ak.shape, np.nan)
    for i in range(nsub):
        if not alive.any():
            break
        t0, t1 = i * h, (i + 1) * h
        for k in range(MAX_CROSSINGS):
            m = alive & (ak[..., k] >= t0) & (ak[..., k] < t1) & (ak[..., k] < budget * step)
            if m.any():
                uu, _ = _rk4(u[m], v[m], ak[..., k][m] - t0, c)
                # the ray may leave the sphere or pass the horizon inside this
                # substep before a_k: then u(a_k) itself shows it (outside the annulus)
                uk[..., k][m] = uu
        nu, nv = _rk4(u, v, h, c)
        gone = (nu <= su) | ((nu > hu) & (nv > 0.0)) | ~np.isfinite(nu)
        if full:
            # the loop's exit as the reference states it (sphere_ray_tracer.rs:134-191): the step
            # that crosses the sphere ends the ray at angle + Newton's step length, one that
            # falls below `bound` or into the horizon ends it with NO_VALUE
            cross = alive & ((nu > su) != (u > su))
            gone = cross | (nu < bound) | ((nu > hu) & (nv > 0.0)) | ~np.isfinite(nu)
            if cross.any():
                angle[cross] = t0 + _newton(u[cross], v[cross], nu[cross], nv[cross], su, h, c)
            steps[alive & gone] = i + 1
        u = np.where(alive, nu, u)
        v = np.where(alive, nv, v)
        alive &= ~gone
    if rule == "full":
        # (a crossing's node lies below the step count exactly where the ray was alive when its
        # step began, which the loop above already asks; the angle is known only now)
        uk = np.where(ak < angle[..., None], uk, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / uk
    hit = np.isfinite(r) & (r >= r_in) & (r <= r_out)
    sa, ca = np.sin(ak), np.cos(ak)
    X = sa * (Ex[0] * cphi + Ex[1] * sphi)[..., None] + ca * Ex[2]
    Y = sa * (Ey[0] * cphi + Ey[1] * sphi)[..., None] + ca * Ey[2]
    az = np.mod(np.arctan2(-Y if mutation == "az_flipped" else Y, X) / (2.0 * math.pi), 1.0)
    if rs > 0.0 and r0 > rs:
        x = np.abs(r0 * np.cos(theta) / E / (1.5 * math.sqrt(3.0) * rs) - 1.0)
    else:
        x = np.full(theta.shape, np.inf)
    with np.errstate(invalid="ignore"):
        node = np.floor(ak / step)
    return dict(hit=hit, r=r, az=az, x=x, theta=theta, cond=np.hypot(A, B), angle=angle, steps=steps, node=node)


def az_err(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.minimum(d, 1.0 - d)


def compare(cpu_hits, ref, r_in, r_out, slots=(0, 1, 2), use_band=True):
    """cpu_hits: (h, w, 3, 2) f32 (r, U) slots of the CPU path or the kernel.
    Returns per-slot statistics and the worst errors; raises nothing."""
    out = {}
    keep = (ref["x"] >= BAND_X) if use_band else np.ones(ref["x"].shape, dtype=bool)
    out["excluded_share"] = 1.0 - float(keep.mean())
    worst_r = worst_az = 0.0
    bad_edges = 0
    for k in slots:
        got = cpu_hits[..., k, 0] > 0.0
        want = ref["hit"][..., k]
        both = got & want & keep
        if both.any():
            er = np.abs(cpu_hits[..., k, 0][both].astype(np.float64) / ref["r"][..., k][both] - 1.0)
            ea = az_err(cpu_hits[..., k, 1][both], ref["az"][..., k][both])
            worst_r = max(worst_r, float(er.max()))
            worst_az = max(worst_az, float(ea.max()))
        dis = (got != want) & keep
        rr = ref["r"][..., k]
        with np.errstate(invalid="ignore"):
            near_edge = (np.abs(rr / r_in - 1.0) <= TOL_R) | (np.abs(rr / r_out - 1.0) <= TOL_R)
        bad_edges += int((dis & ~near_edge).sum())
        out[f"total{k}"] = int(got.sum())
        out[f"ref_total{k}"] = int(want.sum())
        out[f"hits{k}"] = int((got & keep).sum())
        out[f"ref_hits{k}"] = int((want & keep).sum())
        out[f"disagree{k}"] = int(dis.sum())
    out["max_rel_r"] = worst_r
    out["max_az"] = worst_az
    out["disagree_off_edge"] = bad_edges
    return out
