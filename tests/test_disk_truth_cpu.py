"""The thin disk's CPU path (geo_render_cpu_disk, _disk_shift, _disk_emission
and geo_render_cpu_disk_adaptive, include/geo/geo_cpu.h) on fuzzed scenes
against the independent f64 answers: tests/disk_truth.py's checks over test
seeds 0..399, what those seeds reach (asserted from the reference alone), the
calibration record of the model's constants, and the mutations of the reference
that the checks must refuse.  tests/test_gpu_disk_truth.py holds the kernels'
own buffers to the same checks."""
import pytest

import disk_ref as D
import disk_truth as DT
import test_disk_adaptive_cpu as TA
import test_disk_cpu as T
import test_disk_emission_cpu as TE
import test_disk_shift_cpu as TS
from schwarzschild_raytracer_wgpu_amd._lib import GEO_OK

THREADS = 16


class Cpu:
    """The CPU path's disk entry points as disk_truth's checks call them; every
    render is kept (the mutation test and the calibration record read them again)."""
    name = "cpu"

    def __init__(self):
        self.lib = TA.load_cpu()
        self.kept = {}

    def _keep(self, key, draw):
        if key not in self.kept:
            rc, a = draw()
            assert rc == GEO_OK, key
            self.kept[key] = {f: a[f] for f in ("hits", "g", "q") if f in a}
        return self.kept[key]

    def disk(self, c):
        return self._keep(("disk", c.seed), lambda: T.render(self.lib, c.frame, c.direct, T.SKY, DT.W, DT.H,
                                                             T.make_disk(*c.disk_args), T.TEX, threads=THREADS))

    def shift(self, c):
        return self._keep(("shift", c.seed), lambda: TS.render(self.lib, c.frame, c.direct, DT.W, DT.H,
                                                               T.make_disk(*c.disk_args), shift=c.shift,
                                                               threads=THREADS))

    def emission(self, c):
        return self._keep(("emission", c.seed), lambda: TE.render(self.lib, c.frame, c.direct, DT.W, DT.H,
                                                                  T.make_disk(*c.disk_args), em=c.em, ramp=c.ramp,
                                                                  threads=THREADS))

    def adaptive(self, c, shaded):
        kw = dict(em=c.em, ramp=c.ramp) if shaded else {}
        return self._keep(("adaptive", shaded, c.seed),
                          lambda: TA.render(self.lib, c.frame, c.adaptive, DT.W, DT.H, T.make_disk(*c.disk_args),
                                            threads=THREADS, **kw))


@pytest.fixture(scope="module")
def cpu():
    return Cpu()


@pytest.fixture(scope="module")
def reach():
    DT.prefetch(DT.TEST_SEEDS)
    return DT.reach(DT.TEST_SEEDS)


def test_reach(reach):
    """What the test seeds hold, from the reference traces alone: the conditions
    that keep the checks below from passing on empty frames or on one family."""
    fam = reach["family"]
    print({k: v for k, v in reach.items() if k != "family"})
    for f, v in fam.items():
        print(f, {k: (len(x) if k == "seeds50" else x) for k, x in v.items()})
    assert reach["band_slots"] <= 0.08 * reach["hit_slots"]
    for f, v in fam.items():
        assert v["band_slots"] <= 0.15 * v["hit_slots"], f
        assert len(v["seeds50"]) >= 25, f
    assert sum(v["compared"] for v in fam.values()) >= 10_000
    assert fam["inside_photon_sphere"]["compared"] >= 2_000
    assert reach["cut"] >= 5_000
    assert reach["moving"] >= 60
    assert reach["edge_on_with_hits"] >= 15


@pytest.mark.parametrize("what", list(DT.WHAT))
def test_against_the_f64_answer(cpu, reach, what):
    s = DT.check(cpu, what, DT.TEST_SEEDS)
    assert s["compared"] >= 10_000 and s["slot1"] >= 1_000
    assert s["dropped"] <= 0.001 * s["compared"]
    inside = sum(n for seed, n in s["per_seed"].items() if DT.family_of(seed) == "inside_photon_sphere")
    assert inside >= 2_000, inside
    # kCurvedOut and kFlat: at step pi/100 no GEO_FLAG_DISK scene is kCurvedIn (geo_pixel.h's
    # make_consts takes it for other steps or an observer inside the horizon, which the flag
    # refuses); that kind's probes meet the f64 answer at the seeds' own steps
    # (tests/disk_step_truth.py, test_disk_step_truth_cpu.py)
    assert s["kinds"] == {0, 2}


def test_calibration_record(cpu):
    """Every constant follows the rule (4 x the calibration maximum, rounded up
    to a power of two) for its recorded maximum, the calibration seeds still
    measure no more than what is recorded, and the ceiling holds."""
    DT.prefetch(DT.CAL_SEEDS)
    m = DT.calibrate(cpu)
    print("calibration:", {k: float(f"{v:.4g}") for k, v in m.items()})
    assert set(m) == set(DT.CONSTANTS)
    for name, (recorded, value) in DT.CONSTANTS.items():
        assert value == D.tol_rule(recorded), name
        # the record stays beside the measurement: no more than 10 % above it
        assert recorded / 1.1 <= m[name] <= recorded, (name, m[name], recorded)
    DT.check_ceiling()
    # the adaptive THIN bar's near-band term is derived from the radius', not fitted
    for what in DT.WHAT:
        out = DT.outside_on(cpu, what)
        assert not any(out.values()), (what, out)


def test_mutations_are_caught(cpu):
    """Every mutation of the reference fails the assertion named for it, on at
    least the stated number of seeds 0..119 (the first three in every curved
    observer family); the unmutated reference fails none
    (test_against_the_f64_answer)."""
    seeds = range(DT.MUTATION_SEEDS)
    DT.prefetch(seeds, (None,) + D.MUTATIONS)
    assert set(D.MUTATIONS) < set(DT.MUTATIONS)
    for m, (what, assertion, floor) in DT.MUTATIONS.items():
        caught = {f: 0 for f in DT.FAMILIES}
        for seed in seeds:
            c = DT.case_of(seed)
            v = DT.judge(DT.errors(c, what, DT.render(cpu, what, c), m))
            caught[c.family] += v[assertion] > 0
        print(f"mutation {m}: `{assertion}` refuses {sum(caught.values())} of {len(seeds)} seeds (floor {floor}): {caught}")
        assert sum(caught.values()) >= floor, m
        if m in DT.IN_EVERY_CURVED_FAMILY:
            assert all(caught[f] >= DT.FAMILY_FLOOR for f in DT.CURVED_FAMILIES), (m, caught)
