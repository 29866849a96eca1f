"""The f64 capture band's CPU path (geo_render_cpu_disk_ring_f64 and
geo_render_cpu_disk_shift_ring_f64, include/geo/geo_cpu.h) on fuzzed scenes
against disk_ref.trace(sub=1): tests/disk_band_truth.py's checks over the test
seeds, what those seeds reach (from the reference alone), the calibration
record, that the state off fails, and the mutations of the reference the checks
must refuse.  tests/test_gpu_disk_step_truth.py holds the kernels' own buffers
to the same checks."""
import pytest

import disk_band_truth as B
import disk_ref as D
import disk_truth as DT
import test_disk_cpu as T
import test_disk_ring_cpu as RC
import test_disk_truth_cpu as TC


class Cpu(TC.Cpu):
    """test_disk_truth_cpu's renderer with the ring entry points (every render kept)."""

    def __init__(self):
        super().__init__()
        self.ring_lib = RC.load_cpu()

    def ring(self, c, what, on=True):
        kw = dict(shift=c.shift) if what == "ring_shift" else dict(em=c.em) if what == "ring_emission" else {}
        # (keyed by the scene too: tests/disk_step_truth.py's cases share the seeds)
        return self._keep((what, on, c.seed, c.direct.step, c.direct.max_steps), lambda: RC.render(
            self.ring_lib, c.frame, c.direct, T.make_disk(*c.disk_args), int(on), w=DT.W, h=DT.H, ramp=c.ramp,
            threads=TC.THREADS, **kw))


@pytest.fixture(scope="module")
def cpu():
    return Cpu()


@pytest.fixture(scope="module")
def reach():
    B.prefetch(B.TEST_SEEDS)
    return B.reach(B.TEST_SEEDS)


def test_reach(reach):
    """What the band holds on the test seeds, from the reference alone (the far family:
    disk_band_truth's docstring)."""
    print({k: (len(v) if k == "seeds10" else v) for k, v in reach.items()})
    assert reach["hit_slots"] >= 600
    assert reach["slots"][2] >= 60
    for f in B.BAND_FAMILIES:
        assert reach["family"][f] >= 100, f
        assert sum(DT.family_of(s) == f for s in reach["seeds10"]) >= 6, f
    assert reach["moving_seeds"] >= 35  # (77 seeds with in-band hits have a moving observer)
    assert reach["dropped"] <= 0.001 * reach["hit_slots"]


@pytest.mark.parametrize("what", list(B.WHAT))
def test_against_the_f64_answer(cpu, reach, what):
    """1 084 slots on 320 seeds; the largest errors: radius 1.32e-5 (0.88 of its bar),
    azimuth 9.74e-7 turns (0.13), g 4.13e-6 (0.54), THIN's q 7.48e-6 (0.25), POWER's q
    5.67e-6 (0.47: seed 281's slot, disk_band_truth's docstring)."""
    s = DT.check(cpu, what, B.TEST_SEEDS, layer=B)
    assert s["compared"] >= 600 and s["slot2"] >= 60
    assert s["dropped"] <= 0.001 * s["compared"]
    assert s["kinds"] == {0}  # (kCurvedIn in the band: tests/test_disk_step_truth_cpu.py)


def test_calibration_record(cpu):
    B.prefetch(B.CAL_SEEDS)
    m = B.calibrate(cpu)
    print("calibration:", {k: float(f"{v:.4g}") for k, v in m.items()})
    assert m.pop("compared") >= 400
    assert set(m) == set(B.CONSTANTS)
    for name, (recorded, value) in B.CONSTANTS.items():
        assert value == D.tol_rule(recorded), name
        assert recorded / 1.1 <= m[name] <= recorded, (name, m[name], recorded)
    B.check_ceiling()
    # the POWER q bar's u/H term: q carries the radius error (disk_band_truth's docstring)
    got = B.carried(cpu)
    print("carried:", got)
    n, worst, left = got["power"]
    rec_worst, rec_left = B.CARRIED["power"]
    assert n >= 200 and rec_worst / 1.1 <= worst <= rec_worst and rec_left / 1.1 <= left <= rec_left
    assert rec_left <= rec_worst / 4.0
    n, worst, left = got["thin"]
    assert n >= 200 and left > worst / 4.0  # THIN shows no such term: its bar stays flat
    # the derived term is not fitted: no calibration slot lies outside a bar
    for what in B.WHAT:
        for s in B.CAL_SEEDS:
            c = B.case_of(s)
            v = B.judge(B.errors(c, what, B.render(cpu, what, c)))
            assert not any(v.values()), (what, s, v)


def test_state_off_fails(cpu, reach):
    """ring = 0 (the f32 path) breaks the band's radius bar: the layer sees 1e-3 errors."""
    failed = 0
    for seed in B.TEST_SEEDS:
        c = B.case_of(seed)
        failed += B.judge(B.errors(c, "ring", B.render(cpu, "ring", c, on=False)))["radius"] > 0
    print(f"state off: the radius bar fails on {failed} seeds (floor {B.STATE_OFF_FLOOR})")
    assert failed >= B.STATE_OFF_FLOOR


def test_mutations_are_caught(cpu):
    seeds = [s for s in range(B.MUTATION_SEEDS) if s in B.TEST_SEEDS]
    B.prefetch(seeds, (None,) + tuple(m for m in B.MUTATIONS if m in D.MUTATIONS))
    for m, (what, assertions, floor) in B.MUTATIONS.items():
        caught = {f: 0 for f in DT.FAMILIES}
        for seed in seeds:
            c = B.case_of(seed)
            v = B.judge(B.errors(c, what, B.render(cpu, what, c), m))
            caught[c.family] += any(v[a] > 0 for a in assertions)
        print(f"mutation {m}: {assertions} refuse {sum(caught.values())} of {len(seeds)} seeds (floor {floor}): {caught}")
        assert sum(caught.values()) >= floor, m
