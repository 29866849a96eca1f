"""An independent f64 answer for the disk's Doppler and redshift shading
(geo_set_disk_shift): the frequency ratio g = received / emitted of every
crossing of tests/disk_ref.py's trace.

numpy, f64, no code shared with csrc/geo_disk.h, and without that header's
conserved-angular-momentum shortcut: the photon's direction is taken locally,
at the hit.

* the hit point x_hat = cos(a_k) o + sin(a_k) q in the sky frame, o the
  observer's direction (central_to_uv's third column) and q the in-plane unit
  vector the traced ray turns towards (central_to_uv applied to the pixel's
  azimuth direction), a_k the crossing angle;
* t = -sin(a_k) o + cos(a_k) q, the unit tangent of the traced ray's angular
  motion there (the photon itself moves along -t);
* tau = spin * (n x x_hat), the direction of the disk's matter on its circular
  orbit, angular velocity Omega = sqrt(rs / (2 r^3));
* the emitter measures the photon energy u^t (E - Omega r p_tau) with
  p_tau = -(b E / r) (tau . t) and u^t = 1 / sqrt(1 - 1.5 rs/r), the static
  observer E / sqrt(1 - rs/r_obs), the moving one that times its own Doppler
  factor sqrt(1 - k^2) / (1 - k d_z/|d|) (k = psi_factor_and_position[0], d the
  pixel's ray before the aberration):

      g = sqrt(1 - 1.5 rs/r) / sqrt(1 - rs/r_obs) / (1 + Omega b (tau . t)) * g_obs,
      b = r_obs cos(theta) / sqrt(1 - rs/r_obs).

The band.  disk_ref.compare leaves out the pixels with |b/b_c - 1| <
disk_ref.BAND_X = 0.02, 0.15 % and 1.8 % of the frame on its two curved test
poses.  The disk's secondary and third images lie along the capture orbit,
so of the pixels that hit the disk that band holds 0.4 % and 15 %: more than
compare leaves out, for any code.  g is compared down to BAND_G = 0.002 =
BAND_X / 10 instead, the widest of 0.02, 0.01, 0.005, 0.002 at which the band
holds a smaller share of the hit pixels than compare leaves out of the frame
on both poses (0 and 0.96 %).  What stays excluded is the third image
(within 0.1 % of the capture orbit wherever the test poses show it): its g
runs through the same code as slots 0 and 1 and is held by the bit-equality
tests.

Tolerance (disk_ref's scheme): the CPU path (geo_render_cpu_disk_shift, bit-
equal to the kernel) against this module on disk_ref.CAL_DISKS x CAL_CAMS,
spin +1, every slot hit on both sides with |b/b_c - 1| >= BAND_G:

    max relative error of g   7.2e-5  (CAL_G; slot 0 alone: 6.8e-6)

times 4 and rounded up to a power of two (disk_ref.tol_rule).  The reference
g is formed from the f64 trace's radius, so the f32 path's radius error
(CAL_R, 2.46e-5 outside BAND_X, more towards the capture orbit) shows
through sqrt(1 - 1.5 rs/r) and Omega(r).
tests/test_disk_shift_cpu.py::test_calibration_record re-measures it.
"""
from __future__ import annotations

import math

import numpy as np

import disk_ref as D

BAND_G = 0.002       # |b/b_c - 1| below which g is not compared (the docstring's rule)
CAL_G = 7.5e-5       # measured maximum 7.2e-5, relative error of g (calibration set above)
TOL_G = 2.0 ** -11   # 4.88e-4: 4 * CAL_G = 3.0e-4 rounded up to a power of two


def observer_doppler(frame, width, height):
    """(h, w) f64: sqrt(1 - k^2) / (1 - k d_z/|d|), d the pixel's ray in the
    moving observer's frame (disk_ref.camera's d, before the aberration)."""
    m0_3, m0 = D._m3(frame.display_to_movement)
    k = float(frame.psi_factor_and_position[0])
    px = np.arange(width, dtype=np.float64)[None, :]
    py = np.arange(height, dtype=np.float64)[:, None]
    nx = (2.0 * px + 1.0 - width) / width + 0.0 * py
    ny = (height - 2.0 * py - 1.0) / height + 0.0 * px
    v = np.stack([-ny * m0[0, 3], -nx * m0[1, 3], np.full_like(nx, m0[2, 3])], axis=-1)
    d = v @ m0_3.T
    return math.sqrt(1.0 - k * k) / (1.0 - k * d[..., 2] / np.linalg.norm(d, axis=-1))


def shift(frame, scene, width, height, ref, normal=(0.0, 0.0, 1.0), axis=(1.0, 0.0, 0.0), spin=1):
    """(h, w, 3) f64: g of every crossing of `ref` (disk_ref.trace of the same
    arguments), nan where the ray never got there; meaningful where ref["hit"]."""
    rs, r0 = float(scene.rs), float(scene.r_obs)
    c2 = D.camera(frame, width, height)
    rho = np.hypot(c2[..., 0], c2[..., 1])
    m2, _ = D._m3(frame.central_to_uv)
    n, _, _ = D.disk_basis(normal, axis)
    o = m2 @ np.array([0.0, 0.0, 1.0])
    q = np.stack([c2[..., 0] / rho, c2[..., 1] / rho, np.zeros_like(rho)], axis=-1) @ m2.T
    # the crossing angles: x_hat(a) . n = 0, a_0 in (0, pi]
    a0 = np.mod(np.arctan2(-o.dot(n), q @ n), math.pi)
    a0 = np.where(a0 <= 0.0, math.pi, a0)
    ak = a0[..., None] + math.pi * np.arange(D.MAX_CROSSINGS)[None, None, :]
    sa, ca = np.sin(ak)[..., None], np.cos(ak)[..., None]
    xh = ca * o[None, None, None, :] + sa * q[..., None, :]
    t = -sa * o[None, None, None, :] + ca * q[..., None, :]
    tau = spin * np.cross(np.broadcast_to(n, xh.shape), xh)
    h_obs = 1.0 - rs / r0 if rs > 0.0 else 1.0
    b = r0 * np.cos(ref["theta"]) / math.sqrt(h_obs)
    r = ref["r"]
    with np.errstate(invalid="ignore", divide="ignore"):
        omega = np.sqrt(rs / (2.0 * r ** 3))
        g = np.sqrt(1.0 - 1.5 * rs / r) / math.sqrt(h_obs) / (1.0 + omega * b[..., None] * (tau * t).sum(axis=-1))
    return g * observer_doppler(frame, width, height)[..., None]


def compare(cpu_g, cpu_hits, ref, g_ref, slots=(0, 1, 2)):
    """Worst relative error of g over the slots hit on both sides outside the
    band BAND_G, the compared hits per slot, and the band's share of the hit
    pixels."""
    keep = ref["x"] >= BAND_G
    worst, n = 0.0, []
    for k in slots:
        both = (cpu_hits[..., k, 0] > 0.0) & ref["hit"][..., k] & keep
        if both.any():
            worst = max(worst, float(np.abs(cpu_g[..., k][both].astype(np.float64) / g_ref[..., k][both] - 1.0).max()))
        n.append(int(both.sum()))
    hit_px = (cpu_hits[..., 0] > 0.0).any(axis=-1)
    return dict(max_rel_g=worst, compared=n,
                band_share_of_hits=float((hit_px & ~keep).sum()) / max(1, int(hit_px.sum())))
