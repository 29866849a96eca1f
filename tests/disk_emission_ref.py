"""An independent f64 answer for the disk's blackbody emission
(geo_set_disk_emission): q = T_obs / t_ref = g tau(r) of every crossing of
tests/disk_ref.py's trace, g from tests/disk_shift_ref.py, and a numpy
restatement of the colour step (ramp position, 8-bit ramp blend, the f32
multiply) that turns the path's own q into bytes.

numpy, f64, no code shared with csrc/geo_disk.h: tau is written with powers,
    POWER  tau = (r_in/r)^(3/4)
    THIN   tau = (r_in/r)^(3/4) (1 - sqrt(r_in/r))^(1/4) / ((6/7)^(3/2) (1/7)^(1/4)),
where the header takes nested square roots.

What is compared.  POWER: the relative error of q.  THIN: the absolute error
of q, because its tau is ill-conditioned at the inner edge (d tau / d r is
infinite at r_in; q itself is at most GEO_DISK_G_MAX tau <= 16 and of order 1).
Left out: (a) the pixels inside disk_shift_ref.BAND_G of the capture orbit, as
the shift's comparison leaves them out, and (b) for THIN the hits whose
reference radius lies within r_in 2^-8 of r_in.

Tolerances (disk_ref's scheme): the CPU path (geo_render_cpu_disk_emission,
bit-equal to the kernel) against this module on disk_ref.CAL_DISKS x CAL_CAMS,
spin +1, every slot hit on both sides outside (a) and (b):

    POWER  max relative error of q   5.97e-5  (CAL_Q_POWER)
    THIN   max absolute error of q   9.69e-5  (CAL_Q_THIN)

each times 4 and rounded up to a power of two (disk_ref.tol_rule).  The
reference q is formed from the f64 trace's radius, so the f32 path's radius
error (disk_ref.CAL_R, more towards the capture orbit) shows through g and
through tau; THIN's (1 - sqrt x)^(1/4) amplifies it towards the inner edge,
at the strip's border (r = r_in (1 + 2^-8)) by 1 / (4 * 2^-8) = 64 in relative terms.
tests/test_disk_emission_cpu.py::test_calibration_record re-measures both.
"""
from __future__ import annotations

import numpy as np

import disk_shift_ref as S

POWER, THIN = 0, 1   # GEO_DISK_PROFILE_*
STRIP = 2.0 ** -8    # THIN: reference radii within r_in * STRIP of r_in are not compared
F_MAX = (6.0 / 7.0) ** 1.5 * (1.0 / 7.0) ** 0.25

CAL_Q_POWER = 6.0e-5      # measured maximum 5.97e-5, relative error of q (calibration set above)
TOL_Q_POWER = 2.0 ** -12  # 2.44e-4: 4 * CAL_Q_POWER = 2.4e-4 rounded up to a power of two
CAL_Q_THIN = 1.0e-4       # measured maximum 9.69e-5, absolute error of q
TOL_Q_THIN = 2.0 ** -11   # 4.88e-4: 4 * CAL_Q_THIN = 4.0e-4 rounded up to a power of two


def tau(profile, r_in, r):
    """The radial profile at radius r >= r_in (f64; nan where r is nan)."""
    with np.errstate(invalid="ignore"):
        x = r_in / np.asarray(r, dtype=np.float64)
        t = x ** 0.75
        if profile == THIN:
            t = t * np.maximum(1.0 - np.sqrt(x), 0.0) ** 0.25 / F_MAX
    return t


def q_ref(frame, scene, width, height, ref, r_in, normal=(0.0, 0.0, 1.0), axis=(1.0, 0.0, 0.0), spin=1, profile=THIN):
    """(h, w, 3) f64: q of every crossing of `ref` (disk_ref.trace of the same
    arguments); meaningful where ref["hit"]."""
    return S.shift(frame, scene, width, height, ref, normal, axis, spin) * tau(profile, r_in, ref["r"])


def compare(cpu_q, cpu_hits, ref, qr, profile, r_in, slots=(0, 1, 2)):
    """Worst error of q (POWER: relative, THIN: absolute) over the slots hit on
    both sides outside the band BAND_G and, for THIN, outside the inner-edge
    strip; the compared hits per slot; the band's share of the hit pixels and
    the strip's share of the compared hits."""
    keep = ref["x"] >= S.BAND_G
    worst, n, strip = 0.0, [], 0
    for k in slots:
        both = (cpu_hits[..., k, 0] > 0.0) & ref["hit"][..., k] & keep
        if profile == THIN:
            with np.errstate(invalid="ignore"):
                edge = both & (ref["r"][..., k] - r_in < r_in * STRIP)
            strip += int(edge.sum())
            both &= ~edge
        if both.any():
            got, want = cpu_q[..., k][both].astype(np.float64), qr[..., k][both]
            err = np.abs(got / want - 1.0) if profile == POWER else np.abs(got - want)
            worst = max(worst, float(err.max()))
        n.append(int(both.sum()))
    hit_px = (cpu_hits[..., 0] > 0.0).any(axis=-1)
    return dict(max_err_q=worst, compared=n, strip=strip, strip_share=strip / max(1, sum(n)),
                band_share_of_hits=float((hit_px & ~keep).sum()) / max(1, int(hit_px.sum())))


def ramp_consts(t_ref, t_lo, t_hi, n):
    """ka, kb of csrc/geo_disk.h (f64, each rounded once to f32)."""
    il = 1.0 / float(np.float32(t_lo))
    d = il - 1.0 / float(np.float32(t_hi))
    return np.float32(-(n - 1) / (float(np.float32(t_ref)) * d)), np.float32((n - 1) * il / d)


def ramp_np(q, ramp, t_ref, t_lo, t_hi):
    """The ramp's colour at f32 q, (..., 4) int64: the ramp position in f32
    (each operation rounded once; the fma as an exact f64 product and one sum)
    and the integer blend of the two neighbouring entries."""
    f32 = np.float32
    n = ramp.shape[0]
    ka, kb = ramp_consts(t_ref, t_lo, t_hi, n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rq = (f32(1.0) / q.astype(f32)).astype(f32)
        pos = (rq.astype(np.float64) * float(ka) + float(kb)).astype(f32)
    pos = np.minimum(np.where(pos > 0.0, pos, f32(0.0)), f32(n - 1))  # NaN and -inf -> 0
    i = np.minimum(np.floor(pos).astype(np.int64), n - 2)
    w = np.floor(((pos - i.astype(f32)).astype(f32) * f32(256.0)).astype(f32)).astype(np.int64)
    a, b = ramp[i].astype(np.int64), ramp[i + 1].astype(np.int64)
    return (a * (256 - w[..., None]) + b * w[..., None] + 128) >> 8


def colour_np(sample, q, ramp, t_ref, t_lo, t_hi, exposure):
    """geo_disk.h's colour step on (..., 4) uint8 texture samples and f32 q:
    ramp_np's colour e and min(255, floor(fma(t e, m / 255, 0.5))), the product
    t e (m / 255) exact in f64 and the sum rounded once to f32."""
    f32 = np.float32
    q = q.astype(f32)
    q2 = (q * q).astype(f32)
    m = np.minimum((f32(exposure) * (q2 * q2).astype(f32)).astype(f32), f32(65536.0))
    e = ramp_np(q, ramp, t_ref, t_lo, t_hi)
    mk = (m * f32(1.0 / 255.0)).astype(f32).astype(np.float64)
    te = sample[..., :3].astype(np.int64) * e[..., :3]
    v = np.floor((te.astype(np.float64) * mk[..., None] + 0.5).astype(f32)).astype(np.int64)
    out = sample.copy()
    out[..., :3] = np.minimum(v, 255).astype(np.uint8)
    return out
