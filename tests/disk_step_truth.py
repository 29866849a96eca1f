"""The thin disk at the scene's own step against the independent f64 answer:
tests/disk_truth.py's checks on fuzz_disk_scenes.disk_scene(seed, 64, 36) exactly
as generated (own step 0.01 to 3, own budget, on and off the group grid, all five
observer families), where tests/disk_truth.py puts a truth scene at step pi/100
in the seed's place.  This is the layer that reaches the kCurvedIn disk kernels:
GEO_FLAG_DISK refuses an observer inside the horizon, so for a disk scene
kCurvedIn means a step outside [2^-10, 1/2], where RK4 truncation is large and
the step/8 answer is no longer an answer.  The answer that exists there is
disk_ref.trace(sub=1): the same discrete map in f64 at the scene's own step, with
the hit rule stated in full (disk_ref's docstring).  It measures the rounding of
the path, not truncation, so it holds at every step and budget the generator
draws.

Renders.  disk, shift and emission on the direct CPU entry points (a renderer's
disk(case), shift(case), emission(case), as disk_truth's), and ring: the seed's
emission with the f64 band on (ring(case, "ring_emission", True)), for the seeds
with rs > 0, judged on the in-band slots with tests/disk_band_truth.py's model.

Bars.  Outside the band disk_truth's direct-mode model as it stands (K_AZ, R0,
K_RH, G0, Q0_*, BAND_X, H_MIN), not recalibrated: the comparison removes
truncation, so the rounding model holds at every step.  Measured on the CPU path
over the test seeds (72 214 compared slots, 14 122 of them on 78 kCurvedIn seeds):
the largest share of a bar is 0.84 (g; radius 0.33, azimuth 0.23, q 0.68), and
on the kCurvedIn seeds the largest radius error is 8.6e-6 for 1/2 < step <= 1,
3.4e-5 for 1 < step <= 2 and 5.1e-5 for step > 2 (0.20 of its bar).  No term is
missing at large steps.

Seeds.  0..399 with fuzz_disk_scenes.TAIL_SEEDS and GROUP_SEEDS on top (hits probed
in the budget's tail, and as the second or third probe of a group of four steps).
"""
from __future__ import annotations

import disk_band_truth as B
import disk_ref as D
import disk_truth as DT
import fuzz_disk_scenes as F

W, H = DT.W, DT.H
TEST_SEEDS = tuple(dict.fromkeys(DT.TEST_SEEDS + F.TAIL_SEEDS + F.GROUP_SEEDS))
CURVED_SEEDS = tuple(s for s in TEST_SEEDS if DT.family_of(s) != "flat")
STEP_BUCKETS = ((0.5, 1.0), (1.0, 2.0), (2.0, 4.0))  # kCurvedIn's large steps: lo < step <= hi

# Seeds whose frames hold slots with u(a_k) inside the annulus and a_k at or beyond the
# traveled angle the loop returns: the clause `a_k < the returned traveled angle` of geo.h's
# rule, which disk_ref.trace left to u(a_k) until this layer stated it.  All have step > 2.28,
# where Newton's three iterations on an RK4 step of that length do not converge: the length
# they return is negative on every such slot (from -0.2 step to -1271 steps), so the returned
# angle lies below the stopping step's start and below a crossing the loop had already probed.
# seed: (the slots on which the CPU path and the trace disagree without the clause, all "the
# trace hits, the CPU path does not"; what the seed is)
ANGLE_CLAUSE_SEEDS = {
    2: (25, "inside the photon sphere, step 2.49: slots 0 and 2, rays whose step count is 1 or 4"),
    57: (65, "inside the photon sphere, step 2.40: slots 0 and 2; Newton's length down to -1271 steps"),
    69: (1, "small sky sphere, step 2.42: a single slot 0 at node 1, Newton's length -1.5 steps"),
    100: (11, "far observer, step 2.93: slot 0 at node 0 of rays that stop in step 2 (length -0.2 step); "
              "the frame's only hits without the clause"),
    165: (140, "far observer, step 2.98: the largest count, slot 0 at node 1 (length -0.3 step)"),
    206: (2, "between the photon sphere and the disk, step 2.29: the smallest step that shows it"),
}

WHAT = {
    "disk": ("direct", ("hits",)),
    "shift": ("direct", ("hits", "g")),
    "emission": ("direct", ("hits", "g", "q")),
    "ring": ("band", ("hits", "g", "q")),
}


class Case:
    """A seed's own scene and state, with the attributes disk_truth's renderers read
    (`direct` is the seed's scene as generated)."""

    def __init__(self, seed):
        self.seed = seed
        self.frame, sc, self.disk_args, self.shift, (self.em, self.ramp), self.desc = F.disk_scene(seed, W, H)
        self.direct = sc
        self.rs, self.sphere_r, self.r_obs = float(sc.rs), float(sc.sphere_r), float(sc.r_obs)
        self.step, self.budget = float(sc.step), int(sc.max_steps)
        self.family = DT.family_of(seed)
        self.moving = float(self.frame.psi_factor_and_position[0]) != 0.0
        self.kind = F.kind_of(self.rs, self.r_obs, sc.step)


_CASES, _TRACES = {}, {}


def case_of(seed):
    if seed not in _CASES:
        _CASES[seed] = Case(seed)
    return _CASES[seed]


def _trace(key):
    seed, rule = key
    c = case_of(seed)
    return D.trace(c.frame, c.direct, W, H, *c.disk_args, sub=1, rule=rule)


def reference(seed, rule="full"):
    """disk_ref.trace(sub=1) of the seed's own scene, traced once and kept."""
    if (seed, rule) not in _TRACES:
        prefetch([seed], rule, workers=1)
    return _TRACES[(seed, rule)]


def prefetch(seeds, rule="full", workers=None):
    keys = [k for k in dict.fromkeys((s, rule) for s in seeds) if k not in _TRACES]
    for key, ref in DT.trace_all(_trace, keys, workers):
        for a in ref.values():
            a.setflags(write=False)
        _TRACES[key] = ref


def render(r, what, c):
    return r.ring(c, "ring_emission", True) if what == "ring" else DT.render(r, what, c)


def errors(c, what, got, rule="full"):
    ref = reference(c.seed, rule)
    region = B.in_band(ref) if what == "ring" else None
    return DT.errors(c, what, got, refs=(ref, ref), spec=WHAT[what], region=region)


def bars(e):
    return B.bars(e) if e["mode"] == "band" else DT.bars(e)


def compared(seed):
    """(h, w, 3): the reference's hit slots the direct renders are compared on."""
    ref = reference(seed)
    return ref["hit"] & ((ref["x"] >= D.BAND_X) & (ref["cond"] >= DT.H_MIN))[..., None]


def paths(seed):
    """From the reference alone: the compared hits whose probe runs in the budget's tail
    (node >= (max_steps / 4) * 4) and those probed second or third in their group of
    four steps (tests/test_disk_probe_host.py's hit_paths, on the f64 nodes)."""
    c, ref, hit = case_of(seed), reference(seed), compared(seed)
    node, whole = ref["node"], (c.budget // 4) * 4
    tail = hit & (node >= whole)
    grouped = hit[..., 1:] & (node[..., 1:] // 4 == node[..., :-1] // 4) & (node[..., 1:] < whole)
    return int(tail.sum()), int(grouped.sum())


def curved_in_seeds(seeds=DT.TEST_SEEDS, least=50):
    """The kCurvedIn seeds whose reference holds at least `least` compared slots."""
    return [s for s in seeds if case_of(s).kind == 1 and int(compared(s).sum()) >= least]


def gpu_seeds(n=8):
    """The first n kCurvedIn test seeds with at least 50 compared slots, and the named seeds."""
    out = []
    for s in DT.TEST_SEEDS:
        if len(out) < n and case_of(s).kind == 1 and int(compared(s).sum()) >= 50:
            out.append(s)
    assert len(out) == n
    return list(dict.fromkeys(out + list(ANGLE_CLAUSE_SEEDS)))


def off_edge_disagreements(c, got, rule="full"):
    """The slots of a direct render that disagree with the trace on hit/no-hit off the edges."""
    e = errors(c, "disk", got, rule)
    return int((e["dis_edge"] > DT.bars(e)["hits"]).sum())
