"""The thin disk's CPU path at the scene's own step against disk_ref.trace(sub=1):
tests/disk_step_truth.py's checks over seeds 0..399 and the tail and group seeds,
the kCurvedIn reach, the seeds that show the rule's angle clause, and that the
clauses change nothing at the truth layers' step.
tests/test_gpu_disk_step_truth.py holds the kernels' own buffers to the same checks."""
import numpy as np
import pytest

import disk_band_truth as B
import disk_ref as D
import disk_step_truth as ST
import disk_truth as DT
import fuzz_disk_scenes as F
import test_disk_band_truth_cpu as TB


@pytest.fixture(scope="module")
def cpu():
    return TB.Cpu()


@pytest.fixture(scope="module")
def traced():
    ST.prefetch(ST.TEST_SEEDS)


def test_kcurvedin_reach(traced):
    """From the reference alone: what the kCurvedIn seeds hold, by step, and the probe paths."""
    slots = {s: int(ST.compared(s).sum()) for s in DT.TEST_SEEDS if ST.case_of(s).kind == 1}
    print(f"kCurvedIn: {len(slots)} seeds, {sum(slots.values())} compared slots, "
          f"{len(ST.curved_in_seeds())} seeds with at least 50")
    assert sum(slots.values()) >= 7_000
    assert len(ST.curved_in_seeds()) >= 15
    for lo, hi in ST.STEP_BUCKETS:
        n = sum(v for s, v in slots.items() if lo < ST.case_of(s).step <= hi)
        print(f"  {lo} < step <= {hi}: {n} slots")
        assert n > 0, (lo, hi)
    tail = sum(ST.paths(s)[0] for s in ST.TEST_SEEDS)
    grouped = sum(ST.paths(s)[1] for s in ST.TEST_SEEDS)
    print(f"compared hits probed in the budget's tail: {tail}, second or third in a group: {grouped}")
    assert tail > 0 and grouped > 0
    # (each named seed holds its path on the f32 nodes: tests/test_host_disk_fuzz.py; here the
    # compared slots on the f64 nodes, which leave out the band and the smallest H)
    assert sum(ST.paths(s)[0] > 0 for s in F.TAIL_SEEDS) >= len(F.TAIL_SEEDS) // 2
    assert sum(ST.paths(s)[1] > 0 for s in F.GROUP_SEEDS) >= len(F.GROUP_SEEDS) // 2


@pytest.mark.parametrize("what", list(ST.WHAT))
def test_against_the_f64_answer(cpu, traced, what):
    """72 214 slots on 411 seeds outside the band (67 199 on 0..399), 7 dropped; the largest
    errors: radius 1.56e-4 (0.33 of its bar), azimuth 1.43e-5 turns (0.23), g 4.09e-4 (0.84),
    q 1.33e-3 (0.68).  [ring]: 848 in-band slots on 330 seeds, 209 of them on kCurvedIn seeds:
    radius 1.31e-5 (0.88), azimuth 9.74e-7 (0.17), g 4.08e-6 (0.53), q 5.73e-6."""
    seeds = ST.CURVED_SEEDS if what == "ring" else ST.TEST_SEEDS
    s = DT.check(cpu, what, seeds, layer=ST)
    assert s["dropped"] <= 0.001 * s["compared"]
    if what == "ring":
        assert s["kinds"] == {0, 1} and s["compared"] >= 600
        assert sum(n for seed, n in s["per_seed"].items() if ST.case_of(seed).kind == 1) >= 100
        return
    assert s["kinds"] == {0, 1, 2}
    curved_in = {seed: n for seed, n in s["per_seed"].items() if ST.case_of(seed).kind == 1 and seed < 400}
    assert sum(curved_in.values()) >= 7_000
    assert sum(n >= 50 for n in curved_in.values()) >= 15
    for lo, hi in ST.STEP_BUCKETS:
        assert sum(n for seed, n in curved_in.items() if lo < ST.case_of(seed).step <= hi) > 0, (lo, hi)


def test_angle_clause_seeds(cpu, traced):
    """Each named seed: without the clause `a_k < the returned traveled angle` the CPU path
    and the trace disagree off the edges on the recorded number of slots, every one of
    them "the trace hits, the CPU path does not"; with it on none."""
    ST.prefetch(ST.ANGLE_CLAUSE_SEEDS, "no_angle_clause")
    for seed, (count, _) in ST.ANGLE_CLAUSE_SEEDS.items():
        c = ST.case_of(seed)
        got = cpu.disk(c)
        assert c.kind == 1 and c.step > 2.28, c.desc
        assert ST.off_edge_disagreements(c, got) == 0, c.desc
        assert ST.off_edge_disagreements(c, got, "no_angle_clause") == count, c.desc
        open_ref = ST.reference(seed, "no_angle_clause")
        extra = open_ref["hit"] & ~ST.reference(seed)["hit"]
        assert extra.sum() >= count and not ((got["hits"][..., 0] > 0.0) & extra).any(), c.desc
        assert (open_ref["angle"][extra.any(axis=-1)] < D.NO_VALUE).all()


def test_the_clauses_change_nothing_at_the_truth_step():
    """At step pi/100 (the band layer's scenes, seeds 0..119) the rule in full and u(a_k)
    alone give the same hits: no constant measured before the clauses were stated moves."""
    seeds = [s for s in range(B.MUTATION_SEEDS) if s in B.TEST_SEEDS]
    B.prefetch(seeds)
    keys = [(s, None) for s in seeds]
    for (seed, _), ref in DT.trace_all(_u_only, keys):
        full = B.reference(seed)
        assert np.array_equal(ref["hit"], full["hit"]), seed
        assert np.array_equal(ref["r"][ref["hit"]], full["r"][full["hit"]]), seed


def _u_only(key):
    c = B.case_of(key[0])
    return D.trace(c.frame, c.direct, B.W, B.H, *c.disk_args, sub=1, rule="u_only")

