"""The accuracy bars of geo_math.h's f32 transcendentals and the reader of
tests/native/transcendentals_exhaustive.hip's output, shared by the GPU sweep
(tests/test_gpu_transcendentals.py) and its host twin
(tests/test_transcendentals_host.py).

Each bar is the project's own statement (geo_math.h, DESIGN.md §3,
tests/test_math.py), in the unit the program reports:
  asinf_         3 ulp(ref) + 1e-12         (the program reports the error beyond 1e-12, in ulp)
  acosf_         3 ulp(ref)
  atanf_/atan2f_ 4 ulp(ref) + 1e-9          (likewise beyond 1e-9)
  sincosf_       2e-7 absolute, |x| < 1e4
  acos_pi_       1.5e-7 absolute
  atan2_turns_   1e-7, distance on the circle
  sincos_sky_    2e-7 absolute on [-7, fl(pi/2) + 2^-20], what a sampled pixel
                 hands it (the mask is lambda' < -7); for every |x| < 2^21 the
                 derived SKY_A + SKY_B |x| (geo_math.h, above sincos_sky_),
                 asserted per binade at the binade's upper end.
Range properties (asinf_ outside [-1, 1], acos_pi_ and atan2_turns_ in [0, 1])
are counted by the program: range_violations must be 0."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "native", "transcendentals_exhaustive.hip")

FUNCTIONS = ("asinf_", "acosf_", "acos_pi_", "sincosf_", "sincos_sky_", "atanf_", "atan2f_", "atan2_turns_")
TWO_ARGS = ("atan2f_", "atan2_turns_")

BARS = {
    "asinf_": 3.0,
    "acosf_": 3.0,
    "atanf_": 4.0,
    "atan2f_": 4.0,
    "sincosf_": 2e-7,
    "acos_pi_": 1.5e-7,
    "atan2_turns_": 1e-7,
}
SKY_SAMPLED = 2e-7   # sincos_sky_ on [-7, fl(pi/2) + 2^-20]
SKY_A = 2.10e-7      # sincos_sky_ for |x| < 2^21: SKY_A + SKY_B |x| (derived in geo_math.h)
SKY_B = 2.0e-12

_ROW = re.compile(r"^(binade (-?\d+)|set (\w+)) count (\d+) worst (\S+) at (.*)$")


def parse(out: str) -> dict:
    """The figures of one run: rows [(binade or set name, count, worst, where)],
    worst, worst_sampled_range, measured, range_violations, mismatches,
    oracle_mismatches (None where the run printed none)."""
    r = {"rows": [], "worst": None, "worst_at": None, "worst_sampled_range": None, "measured": None,
         "range_violations": None, "mismatches": None, "oracle_mismatches": None}
    for line in out.splitlines():
        m = _ROW.match(line)
        if m:
            key = int(m.group(2)) if m.group(2) is not None else m.group(3)
            r["rows"].append((key, int(m.group(4)), float(m.group(5)), m.group(6)))
            continue
        w = line.split()
        if not w:
            continue
        if w[0] == "worst" and len(w) >= 3:
            r["worst"], r["worst_at"] = float(w[1]), " ".join(w[3:])
        elif w[0] == "worst_sampled_range":
            r["worst_sampled_range"] = float(w[1])
        elif w[0] in ("measured", "range_violations", "mismatches"):
            r[w[0]] = int(w[1])
        elif w[:2] == ["oracle", "mismatches"] and w[2].isdigit():
            r["oracle_mismatches"] = int(w[2])
    return r


def check_bars(fn: str, r: dict) -> None:
    """Asserts fn's accuracy bar and range properties on the figures r."""
    assert r["range_violations"] == 0, (fn, r["range_violations"])
    if not r["measured"]:
        return  # this part of the inputs lies outside the function's domain
    assert r["worst"] is not None
    if fn == "sincos_sky_":
        if r["worst_sampled_range"] is not None:
            assert r["worst_sampled_range"] <= SKY_SAMPLED, r["worst_sampled_range"]
        for key, _, worst, where in r["rows"]:
            bound = SKY_A + SKY_B * 2.0 ** (key + 1)
            assert worst <= bound, (key, worst, bound, where)
        return
    assert r["worst"] <= BARS[fn], (fn, r["worst"], r["worst_at"])
    for key, _, worst, where in r["rows"]:
        assert worst <= BARS[fn], (fn, key, worst, where)
