"""The bar for the disk's capture band in f64 (geo_set_disk_ring_f64).

The definition of the state is the reference's fixed-step integration in f64:
a band pixel's hit radius is compared with tests/disk_ref.py's trace at the
scene's own step (sub=1), so what is measured is the rounding of the path
(the crossing angles and the ray plane's azimuth are the f32 ray's, r is
rounded once to f32), not RK4 truncation.

Tolerance (disk_ref's scheme): the CPU path (geo_render_cpu_disk_ring_f64 with
ring_f64 = 1, bit-equal to the kernels) against disk_ref.trace(sub=1) on
disk_ref.CAL_DISKS x CAL_CAMS (96 x 54, fov pi/2) and on CAL_RING, a narrow
camera (fov 0.004) of CAL_DISKS[0]'s observer at rest, raised from the
direction to the centre onto the photon ring's edge, which is none of the
test poses; every slot hit on both sides with |b/b_c - 1| < BAND (the band's
own width, GEO_RING_X):

    max relative radius error, in-band hits   2.84e-6  (CAL_R_BAND; 290 hits)

times 4 and rounded up to a power of two (disk_ref.tol_rule).
tests/test_disk_ring_cpu.py::test_calibration_record re-measures it.

The flat TOL_R_BAND holds on the three poses of tests/test_disk_ring_cpu.py.
On fuzzed scenes it is one unlucky seed from failing: the crossing angles are
the f32 ray's, so the radius carries a term u / H (H = disk_ref.trace's `cond`),
and tests/fuzz_disk_scenes.py's seed 281 (H = 0.0215) reaches 1.32e-5, 0.86 of
this bar.  The fuzzed layer, tests/disk_band_truth.py, therefore has a model with
the 1/H term and not this constant.
"""
from __future__ import annotations

import math

import numpy as np

import disk_ref as D

BAND = 5e-3     # GEO_RING_X
GUARD = 1e-5    # the band test is on the f32 ray: pixels this close to the edge belong to neither side
CAL_R_BAND = 3.0e-6     # measured maximum 2.84e-6, relative radius of the in-band hits (calibration set above)
TOL_R_BAND = 2.0 ** -16  # 1.53e-5: 4 * CAL_R_BAND = 1.2e-5 rounded up to a power of two

# CAL_DISKS[0]'s observer and disk, at rest, fov 0.004, the camera raised by
# this much above the photon ring's angular radius asin(b_c sqrt(1 - rs/r) / r)
CAL_RING_FOV = 0.004
CAL_RING_LIFT = 2.0e-4


def cal_ring_camera(pos, rs=1.0):
    """(phi, theta) of the narrow calibration camera for an observer at pos."""
    r = math.sqrt(sum(p * p for p in pos))
    alpha = math.asin(1.5 * math.sqrt(3.0) * rs * math.sqrt(1.0 - rs / r) / r)
    phi0 = math.atan2(-pos[1], -pos[0])
    th0 = -math.atan2(pos[2], math.hypot(pos[0], pos[1]))
    return phi0, th0 + alpha + CAL_RING_LIFT


def band_compare(cpu_hits, ref, r_in, r_out, slots=(0, 1, 2)):
    """disk_ref.compare on the pixels inside the band, |b/b_c - 1| < BAND -
    GUARD: hits per slot on both sides, the worst errors of the hits both
    sides report, and the hit / no-hit disagreements away from the annulus'
    edges."""
    keep = ref["x"] < BAND - GUARD
    out = dict(pixels=int(keep.sum()))
    worst_r = worst_az = 0.0
    bad = 0
    for k in slots:
        got = (cpu_hits[..., k, 0] > 0.0) & keep
        want = ref["hit"][..., k] & keep
        both = got & want
        if both.any():
            er = np.abs(cpu_hits[..., k, 0][both].astype(np.float64) / ref["r"][..., k][both] - 1.0)
            worst_r = max(worst_r, float(er.max()))
            worst_az = max(worst_az, float(D.az_err(cpu_hits[..., k, 1][both], ref["az"][..., k][both]).max()))
        rr = ref["r"][..., k]
        with np.errstate(invalid="ignore"):
            near_edge = (np.abs(rr / r_in - 1.0) <= D.TOL_R) | (np.abs(rr / r_out - 1.0) <= D.TOL_R)
        bad += int(((got != want) & ~near_edge).sum())
        out[f"hits{k}"] = int(got.sum())
        out[f"ref_hits{k}"] = int(want.sum())
        out[f"both{k}"] = int(both.sum())
    out["max_rel_r"] = worst_r
    out["max_az"] = worst_az
    out["disagree_off_edge"] = bad
    return out
