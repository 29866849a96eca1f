"""The thin disk on fuzzed scenes against the independent f64 answers
(tests/disk_ref.py, disk_shift_ref.py, disk_emission_ref.py): the layer between
the bit-equality tests, which tie every disk kernel to the CPU path on
tests/fuzz_disk_scenes.py's seeds, and the truth tests, which so far knew three
poses with the disk normal (0, 0, 1), an observer outside the photon sphere and
a 50 rs sky sphere.  Here the f64 answers meet what the generator varies:
observers inside the photon sphere and between it and the disk, a sky sphere a
few rs out, tilted, edge-on and nearly edge-on disks in curved space, the
falling observer's aberration at random energies, fov 0.3 to 2.4.

No product code: the checks take a renderer object (tests/test_disk_truth_cpu.py's
Cpu, tests/test_gpu_disk_truth.py's Gpu), as tests/test_sampler_cpu.py's builders do.

Scenes.  fuzz_disk_scenes.disk_scene(seed, 64, 36)'s frame, disk, shift and
emission, with a truth scene in place of the seed's: step pi/100 (the f64
answer, RK4 at step/8, is an answer only where the f32 path's RK4 truncation is
below the bar), max_steps 2048, every third seed one of SHORT_BUDGETS instead
(the budget then cuts crossings), in the direct mode or in the adaptive mode
(tol 0, 1000 attempts: neither the attempts nor disk_ref's angle budget
1000 step = 10 pi binds).  The seed's own step and budget (kCurvedIn
among them) meet the f64 answer in tests/disk_step_truth.py, and the band
x < 0.005 with the f64 state on in tests/disk_band_truth.py, both against
disk_ref.trace(sub=1); the bit-equality tests (tests/test_host_disk_fuzz.py,
test_gpu_disk_fuzz.py) and the per-step definition (tests/test_disk_probe_host.py)
stay as they are.

Seeds.  Tested: 0..399.  Calibration: 1000..1199, never tested.

Error model (tests/f64_bar.py's style; u = 2^-24, H = disk_ref.trace's `cond`,
x = |b/b_c - 1|).  a_0 = atan2(-B, A) is formed in f32 from A and B with
absolute errors of a few u, so a_0 is off by a few u / H, and every crossing's
azimuth and (through u'(a_k)/u(a_k)) radius with it.  Per slot hit on both
sides, outside the band x < disk_ref.BAND_X and with H >= H_MIN:

    azimuth (turns)     <= K_AZ u / H
    relative radius     <= R0 + K_RH u / H   (+ K_XA u / x in the adaptive mode for x < X_ADAPTIVE)
    relative g          <= G0                (x >= disk_shift_ref.BAND_G)
    q, POWER (relative) <= Q0_POWER          (x >= BAND_G)
    q, THIN (absolute)  <= Q0_THIN           (x >= BAND_G, outside disk_emission_ref's strip)
                           (+ q |d ln tau / d ln r| K_XA u / x in the adaptive mode for x < X_ADAPTIVE)
    hit/no-hit disagreements: 0 where the reference radius is farther from both
    edges of the annulus than the pixel's own radius bar

The adaptive mode's K_XA term is the integrator's local error at the default
tol under the capture orbit's 1/x (f64_bar's K_AMP form; at tol 1e-7 it is gone:
DESIGN.md §3c); R0[adaptive] is measured on x >= X_ADAPTIVE only, not widened
for it.  THIN's q carries the same term, not a constant of its own: the radius
error times the profile's own amplification |d ln tau / d ln r| (thin_amp; 64 at
the strip's border) times q.  It is the finding of the calibration: a flat
Q0_THIN over every x would be 7.6e-4 in the adaptive mode (seed 1056, x = 0.021,
amplification 13.7) and ask for 2^-8, twice the ceiling; from X_ADAPTIVE on the
maximum is 2.6e-4.  The direct mode's flat bar needs no such term (4.1e-4).
g and q have no 1/H term: their maxima over every H are what is recorded (g's
largest errors lie at x < 0.005, the radius error next to the band showing
through, at any H).  Every third seed's budget: budget_of.

Constants.  Each is the CPU path's maximum against the reference over the
calibration seeds (recorded at most 10 % above the measurement), times 4 and
rounded up to a power of two (disk_ref.tol_rule); CONSTANTS holds each beside
its measurement and tests/test_disk_truth_cpu.py::test_calibration_record
re-measures them.  R0 is the maximum over H >= H_WELL = 0.5, K_RH the maximum
of (error - that maximum) H / u over all H; in the adaptive mode both over
x >= X_ADAPTIVE, and K_XA the maximum of (error - R0's) x / u over H >= H_WELL,
x < X_ADAPTIVE.  Adaptive slots with x < X_ADAPTIVE and H < H_WELL enter none of
the three measurements: on them only the sum of the terms is tested (here and,
as the record asserts, on the calibration seeds themselves).

    constant             direct: measured  value     adaptive: measured  value
    K_AZ   (u/H, turns)          6.88      32                  6.88      32
    R0     (relative)            3.26e-5   2^-12               3.52e-5   2^-12
    K_RH   (u/H)                 19.3      128                 17.7      128
    K_XA   (u/x, x < 0.05)       -         -                   6.59      32
    G0     (relative)            1.02e-4   2^-11               1.25e-4   2^-10
    Q0_POWER (relative)          1.53e-4   2^-10               2.08e-4   2^-10
    Q0_THIN  (absolute)          4.11e-4   2^-9                2.59e-4   2^-9  (x >= 0.05)

Ceiling (check_ceiling, asserted by test_calibration_record): R0[direct] and
the bar `bars` applies to a slot at H = 0.5, with THIN's largest amplification,
stay within 4 x the committed TOL_R, TOL_AZ, TOL_G, TOL_Q_POWER, TOL_Q_THIN of
the three poses (the adaptive 1/x terms beside it, as the issue's K_AMP-form
term is).  K_AZ, Q0_POWER and Q0_THIN sit exactly on it.

On the test seeds (the CPU path; the kernels are bit-equal) the maxima are
1.56e-4 (radius, direct, H = 0.011), 1.95e-4 (radius, adaptive, x = 0.022),
1.43e-5 turns (azimuth, H = 0.0011), 1.5e-4 (g), 9.9e-4 (THIN's q, direct):
at most 0.55 of the bar.

What the test seeds reach is asserted from the reference alone
(tests/test_disk_truth_cpu.py::test_reach).  Mutations of the reference, and the
assertion of `judge` that refuses each: MUTATIONS below.
"""
from __future__ import annotations

import math

import numpy as np

import disk_emission_ref as E
import disk_ref as D
import disk_shift_ref as S
import fuzz_disk_scenes as F
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK, GEO_MODE_ADAPTIVE, GEO_MODE_DIRECT

W, H = 64, 36
STEP = math.pi / 100
BUDGET = 2048
SHORT_BUDGETS = (47, 99, 102, 301)
ADAPTIVE_BUDGET, ADAPTIVE_TOL = 1000, 0.0
TEST_SEEDS = tuple(range(400))
CAL_SEEDS = tuple(range(1000, 1200))
FAMILIES = F.OBSERVERS
U32 = 2.0 ** -24
H_MIN = 1e-3     # pixels with H below it are dropped (the tests allow 0.1 % of the compared slots)
H_WELL = 0.5     # H from which a pixel counts as well conditioned
GEO_DISK_G_MAX = 16.0  # geo.h: the largest g, so q = g tau <= 16
X_ADAPTIVE = 0.05  # x below which the adaptive mode's radius bar carries the K_XA u / x term

# name: (the calibration's maximum as recorded, the constant = disk_ref.tol_rule of it)
CONSTANTS = {
    "az_direct": (7.0, 32.0),  # measured 6.881
    "az_adaptive": (7.0, 32.0),  # measured 6.881
    "r0_direct": (3.3e-05, 2.0 ** -12),  # measured 3.261e-05
    "r0_adaptive": (3.6e-05, 2.0 ** -12),  # measured 3.521e-05
    "k_rh_direct": (20.0, 128.0),  # measured 19.31
    "k_rh_adaptive": (18.0, 128.0),  # measured 17.71
    "k_xa": (6.7, 32.0),  # measured 6.593
    "g0_direct": (0.000105, 2.0 ** -11),  # measured 0.0001018
    "g0_adaptive": (0.000128, 2.0 ** -10),  # measured 0.0001254 (over every H, like every g0 and q0)
    "q0_power_direct": (0.000155, 2.0 ** -10),  # measured 0.0001528
    "q0_power_adaptive": (0.00021, 2.0 ** -10),  # measured 0.0002081
    "q0_thin_direct": (0.00042, 2.0 ** -9),  # measured 0.0004108
    "q0_thin_adaptive": (0.000265, 2.0 ** -9),  # measured 0.0002587 (x >= X_ADAPTIVE; nearer the band the derived term)
}
MODES = ("direct", "adaptive")
K_AZ, R0, K_RH, G0, Q0_POWER, Q0_THIN = (
    {m: CONSTANTS[f"{n}_{m}"][1] for m in MODES}
    for n in ("az", "r0", "k_rh", "g0", "q0_power", "q0_thin"))
K_XA = CONSTANTS["k_xa"][1]


def check_ceiling():
    """R0[direct], and the bars `bars` really applies to a slot at H = H_WELL (the most a
    well-conditioned slot is allowed), stay within 4 x the committed bars of the three
    poses: evaluated through `bars` itself, for both profiles, at the strip's border
    where THIN's amplification is largest.  The adaptive mode's 1/x terms stand beside
    this as the issue's K_AMP-form term does: the adaptive slot is taken at x = X_ADAPTIVE,
    from where they are off."""
    assert R0["direct"] <= 4.0 * D.TOL_R
    for m in MODES:
        for profile, tol in ((E.POWER, E.TOL_Q_POWER), (E.THIN, E.TOL_Q_THIN)):
            one = np.array([1.0])
            amp = float(thin_amp(1.0, 1.0 + E.STRIP)) if profile == E.THIN else 0.75
            e = dict(mode=m, h=H_WELL * one, x=X_ADAPTIVE * one, dis_h=H_WELL * one, dis_x=X_ADAPTIVE * one,
                     eg=one, g_h=H_WELL * one, g_x=X_ADAPTIVE * one, eq=one, q_profile=profile,
                     q_x=X_ADAPTIVE * one, q_h=H_WELL * one, q_amp=GEO_DISK_G_MAX * amp * one)
            b = bars(e)
            assert b["azimuth"][0] <= 4.0 * D.TOL_AZ, m
            assert b["radius"][0] <= 4.0 * D.TOL_R and b["hits"][0] <= 4.0 * D.TOL_R, m
            assert b["g"][0] <= 4.0 * S.TOL_G, m
            assert b["q"][0] <= 4.0 * tol, (m, profile)


def family_of(seed):
    return F.OBSERVERS[seed % len(F.OBSERVERS)]


def normal_kind_of(seed):
    return F.NORMALS[(seed // len(F.OBSERVERS)) % len(F.NORMALS)]


def budget_of(seed):
    """Every third seed (seed % 3 == 2: of the three residues the one whose test seeds lose
    the most reference hits to the budget, 7 777 against 4 740 and 3 603) takes a short budget."""
    return SHORT_BUDGETS[(seed // 3) % len(SHORT_BUDGETS)] if seed % 3 == 2 else BUDGET


class Case:
    """A seed's truth scenes and state."""

    def __init__(self, seed):
        self.seed = seed
        self.frame, sc, self.disk_args, self.shift, (self.em, self.ramp), self.desc = F.disk_scene(seed, W, H)
        self.rs, self.sphere_r, self.r_obs = float(sc.rs), float(sc.sphere_r), float(sc.r_obs)
        self.budget = budget_of(seed)
        self.direct = make_scene(sc.rs, sc.sphere_r, sc.r_obs, STEP, self.budget, GEO_MODE_DIRECT, GEO_FLAG_DISK)
        self.full = make_scene(sc.rs, sc.sphere_r, sc.r_obs, STEP, BUDGET, GEO_MODE_DIRECT, GEO_FLAG_DISK)
        self.adaptive = make_scene(sc.rs, sc.sphere_r, sc.r_obs, STEP, ADAPTIVE_BUDGET, GEO_MODE_ADAPTIVE,
                                   GEO_FLAG_DISK, ADAPTIVE_TOL)
        self.family = family_of(seed)
        self.moving = float(self.frame.psi_factor_and_position[0]) != 0.0
        self.edge_on = normal_kind_of(seed) == "edge_on"
        self.kind = F.kind_of(self.rs, self.r_obs, STEP)


_CASES, _TRACES = {}, {}


def case_of(seed):
    if seed not in _CASES:
        _CASES[seed] = Case(seed)
    return _CASES[seed]


def reference(seed, cut=True, mutation=None):
    """disk_ref.trace of the seed's truth scene, traced once per seed and kept
    (never modified): with the seed's budget (cut) or with the budget that cuts
    nothing (the adaptive mode's answer, and what the short budget is counted
    against)."""
    key = (seed, cut and budget_of(seed) != BUDGET, mutation)
    if key not in _TRACES:
        _keep(key, _trace(key))
    return _TRACES[key]


def _trace(key):
    seed, cut, mutation = key
    c = case_of(seed)
    return D.trace(c.frame, c.direct if cut else c.full, W, H, *c.disk_args, mutation=mutation)


def _keep(key, ref):
    for a in ref.values():
        a.setflags(write=False)
    _TRACES[key] = ref


def prefetch(seeds, mutations=(None,), workers=None):
    """Traces the references of `seeds` (both budgets where the seed's is short)
    ahead of the checks, in forked worker processes: the traces are numpy on
    2304 pixels, one Python loop each, and independent.  At most 8 workers; one
    process where this one has a GPU context (a fork would share it) or cannot
    fork.  tests/test_gpu_disk_truth.py does not call it."""
    keys = [k for k in dict.fromkeys((s, c and budget_of(s) != BUDGET, m) for s in seeds for m in mutations
                                     for c in ((True, False) if m is None else (True,))) if k not in _TRACES]
    for key, ref in trace_all(_trace, keys, workers):
        _keep(key, ref)


def trace_all(trace_of, keys, workers=None):
    """[(key, trace_of(key))]: prefetch's forked workers, with its guard (the other
    layers' references go through it too)."""
    import multiprocessing
    import os
    import sys

    workers = min(8, os.cpu_count() or 1, len(keys)) if workers is None else workers
    torch = sys.modules.get("torch")
    if workers > 1 and "fork" in multiprocessing.get_all_start_methods() and \
            not (torch is not None and torch.cuda.is_initialized()):
        with multiprocessing.get_context("fork").Pool(workers) as pool:
            return list(zip(keys, pool.map(trace_of, keys, chunksize=1)))
    return [(key, trace_of(key)) for key in keys]


# ---- what is rendered -----------------------------------------------------------
# name: (the truth scene's mode, the outputs the render is checked in).  A renderer
# has disk(case), shift(case), emission(case) (the direct mode's three entry points) and
# adaptive(case, shaded) (the adaptive disk, unshaded or with the seed's emission); each
# returns a dict with hits (h, w, 3, 2) and, where the entry point has them, g and q (h, w, 3).
WHAT = {
    "disk": ("direct", ("hits",)),
    "shift": ("direct", ("hits", "g")),
    "emission": ("direct", ("hits", "g", "q")),
    "adaptive": ("adaptive", ("hits",)),
    "adaptive_emission": ("adaptive", ("hits", "g", "q")),
}


def render(r, what, c):
    if what == "disk":
        return r.disk(c)
    if what == "shift":
        return r.shift(c)
    if what == "emission":
        return r.emission(c)
    return r.adaptive(c, what == "adaptive_emission")


# ---- the mutations ---------------------------------------------------------------
# mutation: (the entry point it is shown on, the assertion of `judge` that refuses it, the
# least number of seeds 0..MUTATION_SEEDS-1 on which it must: a round number no higher than
# half of the measured count beside it).  The first six are disk_ref.MUTATIONS (wrong traces);
# the last four are wrong shadings of the right trace.  The first three move the image of
# the disk by more than its width on most seeds, so it is the hit/no-hit assertion that
# refuses them (the radius assertion does on 9, 38 and 19 seeds); each must be refused in
# every curved observer family (CURVED_FAMILIES, at least FAMILY_FLOOR seeds; measured 9..19).
MUTATION_SEEDS = 120
MUTATIONS = {
    "no_aberration": ("disk", "hits", 20),             # 48 (moving observers only)
    "slope_e1": ("disk", "hits", 25),                  # 56 (curved families only)
    "flat_c": ("disk", "hits", 30),                    # 67 (curved families only)
    "az_flipped": ("disk", "azimuth", 25),             # 56
    "slot_shift": ("disk", "hits", 30),                # 69
    "budget_ignored": ("disk", "hits", 7),             # 14 (seeds with a short budget only)
    "g_spin": ("shift", "g", 20),                      # 47 (g = 1 in flat space at rest)
    "g_no_doppler": ("shift", "g", 20),                # 47 (moving observers only)
    "q_profiles_swapped": ("emission", "q", 30),       # 70
    "q_thin_edge_shifted": ("emission", "q", 14),      # 29 of the 55 seeds with the THIN profile
}
EDGE_SHIFT = 2.0 ** -10
CURVED_FAMILIES = tuple(f for f in FAMILIES if f != "flat")
IN_EVERY_CURVED_FAMILY = ("no_aberration", "slope_e1", "flat_c")
FAMILY_FLOOR = 4


def thin_amp(r_in, r):
    """|d ln tau / d ln r| of the THIN profile, tau = x^(3/4) (1 - sqrt x)^(1/4), x = r_in/r:
    how a relative radius error shows in tau (disk_emission_ref's docstring: 64 at the
    strip's border)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(r_in / r)
        return np.abs(-0.75 + 0.125 * s / (1.0 - s))


def errors(c, what, got, mutation=None, refs=None, spec=None, region=None):
    """The per-slot errors of one render against the seed's reference (mutated or
    not), as flat arrays: what `judge` holds to the bars and `calibrate` takes the
    maxima of.  The masks (band, H) always come from the unmutated trace.

    The other layers (tests/disk_band_truth.py, disk_step_truth.py) pass their own
    refs = (the unmutated trace, the trace compared with), spec = (mode, outputs) for a
    render WHAT does not name, and region = the (h, w) mask of the pixels they compare
    in place of x >= BAND_X (and BAND_G); H >= H_MIN is always asked."""
    mode, outputs = WHAT[what] if spec is None else spec
    cut = mode != "adaptive"
    true = reference(c.seed, cut) if refs is None else refs[0]
    ref = (reference(c.seed, cut, mutation) if mutation in D.MUTATIONS else true) if refs is None else refs[1]
    r_in, r_out, normal, axis = c.disk_args
    x, cond = true["x"], true["cond"]
    region_g = (x >= S.BAND_G) if region is None else region
    region = (x >= D.BAND_X) if region is None else region
    keep = region & (cond >= H_MIN)
    hits = got["hits"]
    e = dict(mode=mode, seed=c.seed)
    rows = {n: [] for n in ("er", "ea", "h", "x", "slot", "dis_edge", "dis_h", "dis_x")}
    dropped = 0
    for k in range(D.MAX_CROSSINGS):
        g, w = hits[..., k, 0] > 0.0, ref["hit"][..., k]
        both = g & w & keep
        dropped += int((g & w & region & (cond < H_MIN)).sum())
        rr = ref["r"][..., k]
        rows["er"].append(np.abs(hits[..., k, 0][both].astype(np.float64) / rr[both] - 1.0))
        rows["ea"].append(D.az_err(hits[..., k, 1][both], ref["az"][..., k][both]))
        rows["h"].append(cond[both])
        rows["x"].append(x[both])
        rows["slot"].append(np.full(int(both.sum()), k))
        dis = (g != w) & keep
        with np.errstate(invalid="ignore"):
            edge = np.minimum(np.abs(rr / r_in - 1.0), np.abs(rr / r_out - 1.0))
        rows["dis_edge"].append(np.where(np.isfinite(edge), edge, np.inf)[dis])
        rows["dis_h"].append(cond[dis])
        rows["dis_x"].append(x[dis])
    e.update({n: np.concatenate(v) for n, v in rows.items()})
    e["dropped"] = dropped
    if "g" in outputs:
        spin = c.em[0] if "q" in outputs else c.shift[0]
        scene = c.direct if cut else c.adaptive
        gr = S.shift(c.frame, scene, W, H, ref, normal, axis, -spin if mutation == "g_spin" else spin)
        if mutation == "g_no_doppler":
            gr = gr / S.observer_doppler(c.frame, W, H)[..., None]
        keepg = region_g & (cond >= H_MIN)
        both = (hits[..., 0] > 0.0) & ref["hit"] & keepg[..., None]
        e["eg"] = np.abs(got["g"][both].astype(np.float64) / gr[both] - 1.0)
        e["g_h"] = np.broadcast_to(cond[..., None], both.shape)[both]
        e["g_x"] = np.broadcast_to(x[..., None], both.shape)[both]
        if "q" in outputs:
            profile = c.em[1]
            wrong = (E.POWER if profile == E.THIN else E.THIN) if mutation == "q_profiles_swapped" else profile
            # (the subtle one: THIN's inner edge 2^-10 too far out, which shows next to the edge only)
            qr = gr * E.tau(wrong, r_in * (1.0 + EDGE_SHIFT) if mutation == "q_thin_edge_shifted" else r_in, ref["r"])
            if profile == E.THIN:
                with np.errstate(invalid="ignore"):
                    both &= ~(ref["r"] - r_in < r_in * E.STRIP)
                e["eq"] = np.abs(got["q"][both].astype(np.float64) - qr[both])
                e["q_amp"] = qr[both] * thin_amp(r_in, ref["r"][both])
            else:
                e["eq"] = np.abs(got["q"][both].astype(np.float64) / qr[both] - 1.0)
                e["q_amp"] = np.full(e["eq"].shape, 0.75)
            e["q_profile"] = profile
            e["q_x"] = np.broadcast_to(x[..., None], both.shape)[both]
            e["q_h"] = np.broadcast_to(cond[..., None], both.shape)[both]
    return e


def bars(e):
    """The model's bar for every compared slot of `errors`' output."""
    mode = e["mode"]
    with np.errstate(divide="ignore"):
        ih = U32 / e["h"]
        b = dict(azimuth=K_AZ[mode] * ih, radius=R0[mode] + K_RH[mode] * ih)
        if mode == "adaptive":
            b["radius"] = b["radius"] + np.where(e["x"] < X_ADAPTIVE, K_XA * U32 / e["x"], 0.0)
        if "eg" in e:
            b["g"] = G0[mode] + 0.0 * e["g_h"]
        if "eq" in e:
            b["q"] = (Q0_THIN if e["q_profile"] == E.THIN else Q0_POWER)[mode] + 0.0 * e["q_h"]
            if mode == "adaptive" and e["q_profile"] == E.THIN:
                # the radius bar's near-band term, carried into q = g tau(r) by q |d ln tau / d ln r|
                b["q"] = b["q"] + np.where(e["q_x"] < X_ADAPTIVE, e["q_amp"] * K_XA * U32 / e["q_x"], 0.0)
        # a hit/no-hit disagreement is explained where the reference radius lies within the
        # pixel's own radius bar of an edge of the annulus
        b["hits"] = R0[mode] + K_RH[mode] * U32 / e["dis_h"]
        if mode == "adaptive":
            b["hits"] = b["hits"] + np.where(e["dis_x"] < X_ADAPTIVE, K_XA * U32 / e["dis_x"], 0.0)
    return b


ASSERTIONS = ("hits", "radius", "azimuth", "g", "q")


def judge(e, b=None):
    """Per assertion, the number of slots outside the model's bar (b: another layer's bars)."""
    b = bars(e) if b is None else b
    out = dict(hits=int((e["dis_edge"] > b["hits"]).sum()), radius=int((e["er"] > b["radius"]).sum()),
               azimuth=int((e["ea"] > b["azimuth"]).sum()), g=0, q=0)
    if "eg" in e:
        out["g"] = int((e["eg"] > b["g"]).sum())
    if "eq" in e:
        out["q"] = int((e["eq"] > b["q"]).sum())
    return out


def _max(a, w=None):
    a = a if w is None else a[w]
    return float(a.max()) if a.size else 0.0


def check(r, what, seeds, layer=None):
    """Renders `what` on every seed, holds it to the model and prints the maxima.
    Returns the statistics the reach assertions read; raises on the first
    assertion of ASSERTIONS that any seed fails.  layer: this module, or another
    layer's (its WHAT, case_of, render, errors and bars)."""
    import sys

    layer = sys.modules[__name__] if layer is None else layer
    mode = layer.WHAT[what][0]
    bad, worst = [], {}
    stats = dict(compared=0, slot1=0, slot2=0, dropped=0, per_seed={}, kinds=set())
    for seed in seeds:
        c = layer.case_of(seed)
        e = layer.errors(c, what, layer.render(r, what, c))
        b = layer.bars(e)
        v = judge(e, b)
        if any(v.values()):
            bad.append(f"{c.desc}: {what} on {r.name}: outside the bar: {v}")
        for name, err, bar in (("radius", e["er"], b["radius"]), ("azimuth", e["ea"], b["azimuth"]),
                               ("g", e.get("eg"), b.get("g")), ("q", e.get("eq"), b.get("q"))):
            if err is not None and err.size:
                w = worst.setdefault(name, [0.0, 0.0])
                w[0], w[1] = max(w[0], float(err.max())), max(w[1], float((err / bar).max()))
        stats["compared"] += e["er"].size
        stats["slot1"] += int((e["slot"] == 1).sum())
        stats["slot2"] += int((e["slot"] == 2).sum())
        stats["dropped"] += e["dropped"]
        stats["per_seed"][seed] = e["er"].size
        stats["kinds"].add(c.kind)
    print(f"{r.name} {what} ({mode}): {len(stats['per_seed'])} seeds, {stats['compared']} slots compared, "
          f"{stats['dropped']} dropped for H < {H_MIN}; max error (and its share of the bar): " +
          ", ".join(f"{n} {w[0]:.3g} ({w[1]:.2f})" for n, w in worst.items()))
    assert not bad, f"{len(bad)} seeds; first: {bad[0]}"
    return stats


# ---- reach: what the reference alone says about the seeds --------------------------
def reach(seeds):
    """Counts from the reference traces alone (no renderer): the hit slots, the
    band's share of them overall and per family, the hits a short budget cuts,
    the moving and the edge-on seeds."""
    out = dict(hit_slots=0, band_slots=0, cut=0, moving=0, edge_on_with_hits=0,
               family={f: dict(hit_slots=0, band_slots=0, compared=0, seeds50=[]) for f in FAMILIES})
    for seed in seeds:
        c = case_of(seed)
        ref = reference(seed)
        hit = ref["hit"]
        band = hit & (ref["x"] < D.BAND_X)[..., None]
        comp = hit & ((ref["x"] >= D.BAND_X) & (ref["cond"] >= H_MIN))[..., None]
        f = out["family"][c.family]
        n, nb, nc = int(hit.sum()), int(band.sum()), int(comp.sum())
        out["hit_slots"] += n
        out["band_slots"] += nb
        f["hit_slots"] += n
        f["band_slots"] += nb
        f["compared"] += nc
        if nc >= 50:
            f["seeds50"].append(seed)
        if c.budget != BUDGET:
            out["cut"] += int((reference(seed, cut=False)["hit"] & ~hit).sum())
        out["moving"] += c.moving
        out["edge_on_with_hits"] += bool(c.edge_on and n)
    return out


def gpu_seeds(per_family=8):
    """The first `per_family` test seeds of every observer family whose reference
    holds at least 50 compared slots."""
    out, need = [], {f: per_family for f in FAMILIES}
    for seed in TEST_SEEDS:
        f = family_of(seed)
        if need[f] == 0:
            continue
        ref = reference(seed)
        if int((ref["hit"] & ((ref["x"] >= D.BAND_X) & (ref["cond"] >= H_MIN))[..., None]).sum()) >= 50:
            out.append(seed)
            need[f] -= 1
        if not any(need.values()):
            break
    assert not any(need.values()), need
    return out


# ---- calibration ---------------------------------------------------------------------
def calibrate(r, seeds=CAL_SEEDS):
    """The measured maxima behind the constants (the docstring's table), from
    `r` on the calibration seeds."""
    m = {}
    for mode, plain, shaded in (("direct", "disk", "emission"), ("adaptive", "adaptive", "adaptive_emission")):
        es = [errors(case_of(s), shaded, render(r, shaded, case_of(s))) for s in seeds]
        if mode == "direct":  # the shift's g is the emission's with the shift's own spin
            eg = [errors(case_of(s), "shift", render(r, "shift", case_of(s))) for s in seeds]
        else:
            eg = []
        er, ea, h, x = (np.concatenate([e[n] for e in es]) for n in ("er", "ea", "h", "x"))
        well = h >= H_WELL
        far = (x >= X_ADAPTIVE) if mode == "adaptive" else np.ones(x.shape, bool)
        m[f"az_{mode}"] = _max(ea * h / U32)
        r0 = m[f"r0_{mode}"] = _max(er, well & far)
        m[f"k_rh_{mode}"] = _max((er - r0) * h / U32, far)
        if mode == "adaptive":
            m["k_xa"] = _max((er - r0) * x / U32, well & ~far)
        m[f"g0_{mode}"] = _max(np.concatenate([e["eg"] for e in es + eg]))
        for name, p in (("power", E.POWER), ("thin", E.THIN)):
            q, qx = (np.concatenate([e[n] for e in es if e["q_profile"] == p]) for n in ("eq", "q_x"))
            # (the adaptive THIN bar has the near-band term: its Q0 is the maximum from X_ADAPTIVE on)
            m[f"q0_{name}_{mode}"] = _max(q, qx >= X_ADAPTIVE if (mode, p) == ("adaptive", E.THIN) else None)
    return m


def outside_on(r, what, seeds=CAL_SEEDS):
    """Per assertion, the slots of `seeds` outside the model's bar (the calibration
    record: the terms that are derived, not fitted, must hold there too)."""
    out = {a: 0 for a in ASSERTIONS}
    for s in seeds:
        for a, n in judge(errors(case_of(s), what, render(r, what, case_of(s)))).items():
            out[a] += n
    return out
