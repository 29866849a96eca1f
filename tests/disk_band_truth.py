"""The f64 capture band (geo_set_disk_ring_f64) on fuzzed scenes against the
independent f64 answer: tests/disk_truth.py's layer for the pixels that module
leaves out, x = |b/b_c - 1| < disk_ring_ref.BAND - GUARD, where the band's lanes
run in f64 (csrc/geo_band.h).  tests/test_disk_ring_cpu.py holds the band to
truth on three fixed poses; here it meets the generator's observers: a falling
observer's aberration on the band's own f64 camera ray, tilted and nearly
edge-on disks, observers inside the photon sphere and under a small sky sphere,
and g and q of in-band hits for a moving observer.

No product code: the checks take a renderer with ring(case, what, on) (tests/
test_disk_band_truth_cpu.py's Cpu, tests/test_gpu_disk_step_truth.py's Gpu).

Scenes.  disk_truth.Case's direct truth scene (step pi/100, the seed's budget),
the seeds with rs > 0 (flat space has no capture orbit and no band), the state
on: geo_render_cpu_disk_ring_f64 unshaded and with the seed's emission,
geo_render_cpu_disk_shift_ring_f64 with the seed's shift.  The reference is
disk_ref.trace(sub=1), the same discrete map in f64 with the rule in full: it
measures the rounding of the path, not RK4 truncation (disk_ring_ref.py).

Seeds.  Tested: 0..399.  Calibration: 1000..1199, never tested.

Error model (u = 2^-24, H = disk_ref.trace's `cond`).  The band integrates in
f64, but the crossing angles a_k and the ray plane's azimuth are the f32 ray's
(geo_band.h), so a_0's few u / H stay, and the radius is rounded once to f32.
Per slot hit on both sides with x < BAND - GUARD and H >= disk_truth.H_MIN:

    azimuth (turns)     <= K_AZ_BAND u / H
    relative radius     <= R0_BAND + K_RH_BAND u / H
    relative g          <= G0_BAND
    q, POWER (relative) <= Q0_POWER_BAND + 0.75 K_RH_BAND u / H
    q, THIN (absolute)  <= Q0_THIN_BAND   (outside disk_emission_ref's strip)
    hit/no-hit disagreements: 0 where the reference radius is farther from both
    edges of the annulus than the pixel's own radius bar

The POWER q bar's second term is the one the calibration shows beyond the
issue's flat bars; it has no constant of its own.  q = g tau(r), so to first
order q's relative error is g's plus d ln tau / d ln r (-3/4 for POWER) times the
radius error.  `carried` measures that on the calibration seeds with signed errors:
on their 309 POWER slots the largest q error is 8.96e-7, and what is left of it
once g's error and -3/4 of the radius error are taken out is 1.55e-7 at most
(CARRIED; the correlation of q's error less g's with the radius error is -0.95).
POWER's q therefore carries the radius error whole, and with it the radius bar's
own u / H term, times 3/4.  THIN shows no such thing (467 slots: largest error
4.80e-6, 5.54e-6 left; its absolute error is set elsewhere), so its bar stays
flat, as G0_BAND does.  The radius maximum itself is 7.2e-7 to 9.9e-7 in every
range of H and of x over the calibration's 777 in-band hits, so nothing else
is added.  The flat bar alone would fail on one test slot, which is how the term
was looked for: seed 281's only in-band slot (near_disk, slot 0, H = 0.0215,
x = 0.0016) has a radius error of 1.32e-5 (0.88 of its bar; 0.86 of the three
poses' flat disk_ring_ref.TOL_R_BAND, which lacks the 1/H term), a g error of
4.13e-6 and a q error of -5.67e-6 = 4.13e-6 - 0.75 x 1.32e-5 to 7e-8, against
2^-18 = 3.81e-6 flat and 1.21e-5 with the term (0.47).

Constants.  Each is the CPU path's maximum over the calibration seeds (recorded
at most 10 % above the measurement), times 4 and rounded up to a power of two
(disk_ref.tol_rule); R0_BAND over H >= disk_truth.H_WELL, K_RH_BAND the maximum
of (error - that maximum) H / u over all H.  CONSTANTS holds each beside its
measurement; tests/test_disk_band_truth_cpu.py::test_calibration_record
re-measures them and `carried`'s figures, and asserts that no calibration slot
lies outside a bar (the derived term is not fitted there).

Ceiling (check_ceiling): R0_BAND <= 4 x disk_ring_ref.TOL_R_BAND, and the g and
q bars are no looser than disk_truth's direct-mode G0 and Q0, POWER's taken at
H = H_MIN where its term is largest (the constants come out 64 to 256 times
tighter, which is the point of the state).

Reach (asserted from the reference alone, test_reach) and the mutations of the
reference with the assertion that refuses each: below.  The far family sees the
band under too few pixels at 64 x 36 to carry a floor of its own (24 in-band
hits on 80 seeds, none with 10).
"""
from __future__ import annotations

import numpy as np

import disk_emission_ref as E
import disk_ref as D
import disk_ring_ref as R
import disk_truth as DT

W, H = DT.W, DT.H
U32 = DT.U32
TEST_SEEDS = tuple(s for s in DT.TEST_SEEDS if DT.family_of(s) != "flat")
CAL_SEEDS = tuple(s for s in DT.CAL_SEEDS if DT.family_of(s) != "flat")
BAND_FAMILIES = ("near_disk", "inside_photon_sphere", "small_sphere")

# name: (the calibration's maximum as recorded, the constant = disk_ref.tol_rule of it)
CONSTANTS = {
    "az_band": (1.3, 8.0),  # measured 1.278 (u/H, turns)
    "r0_band": (8.8e-07, 2.0 ** -18),  # measured 8.693e-07
    "k_rh_band": (0.82, 4.0),  # measured 0.8086 (u/H)
    "g0_band": (1.1e-06, 2.0 ** -17),  # measured 1.077e-06
    "q0_power_band": (9.0e-07, 2.0 ** -18),  # measured 8.961e-07
    "q0_thin_band": (4.9e-06, 2.0 ** -15),  # measured 4.797e-06
}
# `carried` on the calibration seeds, POWER: (the largest q error, what is left of it without
# g's error and -3/4 of the radius error), each as recorded (at most 10 % above the measurement)
CARRIED = {"power": (9.0e-07, 1.6e-07)}  # measured 8.961e-07, 1.549e-07
POWER_AMP = 0.75  # |d ln tau / d ln r| of the POWER profile
K_AZ_BAND, R0_BAND, K_RH_BAND, G0_BAND, Q0_POWER_BAND, Q0_THIN_BAND = (
    CONSTANTS[n][1] for n in ("az_band", "r0_band", "k_rh_band", "g0_band", "q0_power_band", "q0_thin_band"))

# name: (mode, the outputs the render is checked in).  A renderer's ring(case, what, on)
# draws the case's direct scene with the state on (or off) and returns hits, g, q.
WHAT = {
    "ring": ("band", ("hits",)),
    "ring_shift": ("band", ("hits", "g")),
    "ring_emission": ("band", ("hits", "g", "q")),
}

case_of = DT.case_of
_TRACES = {}


def check_ceiling():
    assert R0_BAND <= 4.0 * R.TOL_R_BAND
    assert G0_BAND <= DT.G0["direct"]
    assert Q0_POWER_BAND + POWER_AMP * K_RH_BAND * U32 / DT.H_MIN <= DT.Q0_POWER["direct"]
    assert Q0_THIN_BAND <= DT.Q0_THIN["direct"]


def _trace(key):
    seed, mutation = key
    c = case_of(seed)
    return D.trace(c.frame, c.direct, W, H, *c.disk_args, sub=1, mutation=mutation)


def reference(seed, mutation=None):
    """disk_ref.trace(sub=1) of the seed's direct truth scene, traced once and kept."""
    key = (seed, mutation)
    if key not in _TRACES:
        prefetch([seed], (mutation,), workers=1)
    return _TRACES[key]


def prefetch(seeds, mutations=(None,), workers=None):
    keys = [k for k in dict.fromkeys((s, m) for s in seeds for m in mutations) if k not in _TRACES]
    for key, ref in DT.trace_all(_trace, keys, workers):
        for a in ref.values():
            a.setflags(write=False)
        _TRACES[key] = ref


def in_band(ref):
    return ref["x"] < R.BAND - R.GUARD


def render(r, what, c, on=True):
    return r.ring(c, what, on)


def errors(c, what, got, mutation=None):
    """disk_truth.errors on the band's pixels against trace(sub=1)."""
    true = reference(c.seed)
    ref = reference(c.seed, mutation) if mutation in D.MUTATIONS else true
    return DT.errors(c, what, got, mutation, refs=(true, ref), spec=WHAT[what], region=in_band(true))


def bars(e):
    with np.errstate(divide="ignore"):
        b = dict(azimuth=K_AZ_BAND * U32 / e["h"], radius=R0_BAND + K_RH_BAND * U32 / e["h"],
                 hits=R0_BAND + K_RH_BAND * U32 / e["dis_h"])
    if "eg" in e:
        b["g"] = G0_BAND + 0.0 * e["g_h"]
    if "eq" in e:
        if e["q_profile"] == E.THIN:
            b["q"] = Q0_THIN_BAND + 0.0 * e["q_h"]
        else:  # the radius bar's u / H term, carried into q = g tau(r) by |d ln tau / d ln r|
            with np.errstate(divide="ignore"):
                b["q"] = Q0_POWER_BAND + POWER_AMP * K_RH_BAND * U32 / e["q_h"]
    return b


def judge(e):
    return DT.judge(e, bars(e))


# ---- the mutations ---------------------------------------------------------------
# mutation: (the render it is shown on, the assertions of `judge` of which one must refuse
# it, the least number of seeds 0..MUTATION_SEEDS-1 (rs > 0) on which it must: a round number
# no higher than half of the measured count beside it)
MUTATION_SEEDS = 120
MUTATIONS = {
    "no_aberration": ("ring", ("hits", "radius"), 10),      # 20 (moving observers only; hits 20, radius 1)
    "slope_e1": ("ring", ("hits", "radius"), 15),           # 31 (hits 28, radius 5)
    "az_flipped": ("ring", ("azimuth",), 10),               # 20
    "slot_shift": ("ring", ("hits", "radius"), 14),         # 29
    "g_no_doppler": ("ring_shift", ("g",), 10),             # 20 (moving observers only)
    "g_spin": ("ring_shift", ("g",), 12),                   # 25
    "q_profiles_swapped": ("ring_emission", ("q",), 14),    # 29
}
# the state off (ring = 0, the f32 path) must break the radius bar on at least this many
# test seeds: a round number no higher than half of the measured count
STATE_OFF_FLOOR = 40  # measured 89 of 320


# ---- reach: what the reference alone says about the seeds --------------------------
def band_hits(seed):
    """(h, w, 3): the reference's in-band hit slots the checks compare."""
    ref = reference(seed)
    return ref["hit"] & (in_band(ref) & (ref["cond"] >= DT.H_MIN))[..., None]


def reach(seeds):
    out = dict(hit_slots=0, slots=[0, 0, 0], dropped=0, moving_seeds=0, seeds10=[],
               family={f: 0 for f in DT.FAMILIES})
    for seed in seeds:
        c = case_of(seed)
        ref = reference(seed)
        m = band_hits(seed)
        n = int(m.sum())
        out["hit_slots"] += n
        for k in range(D.MAX_CROSSINGS):
            out["slots"][k] += int(m[..., k].sum())
        out["dropped"] += int((ref["hit"] & (in_band(ref) & (ref["cond"] < DT.H_MIN))[..., None]).sum())
        out["family"][c.family] += n
        out["moving_seeds"] += bool(n and c.moving)
        if n >= 10:
            out["seeds10"].append(seed)
    return out


def gpu_seeds(per_family=6):
    """The first `per_family` test seeds with at least 10 in-band hits from each of BAND_FAMILIES."""
    out, need = [], {f: per_family for f in BAND_FAMILIES}
    for seed in TEST_SEEDS:
        f = DT.family_of(seed)
        if need.get(f, 0) and int(band_hits(seed).sum()) >= 10:
            out.append(seed)
            need[f] -= 1
    assert not any(need.values()), need
    return out


# ---- calibration ---------------------------------------------------------------------
def calibrate(r, seeds=CAL_SEEDS):
    """The measured maxima behind the constants, from `r` on the calibration seeds."""
    es = [errors(case_of(s), "ring_emission", render(r, "ring_emission", case_of(s))) for s in seeds]
    eg = [errors(case_of(s), "ring_shift", render(r, "ring_shift", case_of(s))) for s in seeds]
    er, ea, h = (np.concatenate([e[n] for e in es]) for n in ("er", "ea", "h"))
    m = dict(az_band=DT._max(ea * h / U32))
    r0 = m["r0_band"] = DT._max(er, h >= DT.H_WELL)
    m["k_rh_band"] = DT._max((er - r0) * h / U32)
    m["g0_band"] = DT._max(np.concatenate([e["eg"] for e in es + eg]))
    for name, p in (("power", E.POWER), ("thin", E.THIN)):
        m[f"q0_{name}_band"] = DT._max(np.concatenate([e["eq"] for e in es if e["q_profile"] == p]))
    m["compared"] = int(er.size)
    return m


def carried(r, seeds=CAL_SEEDS):
    """The measurement behind the q bars' u/H term: per profile, over the compared slots
    of `seeds`, (slots, the largest q error, the largest q error left once g's own
    error and the radius error carried through tau are taken out), in the profile's
    measure (POWER relative, THIN absolute and outside the strip).  With the signed errors
    dr = r/r_ref - 1, dg = g/g_ref - 1 and s = d ln tau / d ln r at the reference radius,
    q = g tau(r) gives q/q_ref - 1 = dg + s dr to first order."""
    import disk_shift_ref as S

    out = {}
    for name, p in (("power", E.POWER), ("thin", E.THIN)):
        n, worst, left = 0, 0.0, 0.0
        for seed in seeds:
            c = case_of(seed)
            if c.em[1] != p:
                continue
            got, ref = render(r, "ring_emission", c), reference(seed)
            r_in, _, normal, axis = c.disk_args
            both = (got["hits"][..., 0] > 0.0) & ref["hit"] & (in_band(ref) & (ref["cond"] >= DT.H_MIN))[..., None]
            if p == E.THIN:
                with np.errstate(invalid="ignore"):
                    both &= ~(ref["r"] - r_in < r_in * E.STRIP)
            if not both.any():
                continue
            rr = ref["r"][both]
            gr = S.shift(c.frame, c.direct, W, H, ref, normal, axis, c.em[0])[both]
            qr = gr * E.tau(p, r_in, ref["r"])[both]
            dr = got["hits"][..., 0][both].astype(np.float64) / rr - 1.0
            dg = got["g"][both].astype(np.float64) / gr - 1.0
            dq = got["q"][both].astype(np.float64) / qr - 1.0
            sq = np.sqrt(r_in / rr)
            s = -0.75 if p == E.POWER else -0.75 + 0.125 * sq / (1.0 - sq)
            scale = 1.0 if p == E.POWER else qr
            n += int(both.sum())
            worst = max(worst, float(np.abs(scale * dq).max()))
            left = max(left, float(np.abs(scale * (dq - dg - s * dr)).max()))
        out[name] = (n, worst, left)
    return out
