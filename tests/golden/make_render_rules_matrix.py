"""Writes tests/golden/render_rules_matrix.npz: the status and the launcher of
every case of tests/render_rules_cases.py, by the host build of
csrc/geo_render_rules.h.  Run it only when the rules are meant to change.

    python tests/golden/make_render_rules_matrix.py [--cases FILE --expected FILE]

--cases / --expected also write the cases (raw RuleCase records) and the
expected bytes (statuses, then launchers) for the stand-alone program
(tests/native/render_rules_host.cpp with -DRENDER_RULES_MAIN)."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import render_rules_cases as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases")
    ap.add_argument("--expected")
    ap.add_argument("--out", default=os.path.join(HERE, "render_rules_matrix.npz"))
    a = ap.parse_args()
    lib = R.load()
    status, launcher = [], []
    cf = open(a.cases, "wb") if a.cases else None
    for _, c in R.blocks():
        s, l = R.run(lib, c)
        status.append(s)
        launcher.append(l)
        if cf:
            c.tofile(cf)
    status, launcher = np.concatenate(status), np.concatenate(launcher)
    if a.expected:
        with open(a.expected, "wb") as f:
            status.tofile(f)
            launcher.tofile(f)
    np.savez_compressed(a.out, status=status, launcher=launcher)
    print(f"{len(status)} cases: {int((status == R.GEO_OK).sum())} GEO_OK, {int((status == R.GEO_ESTATE).sum())} "
          f"GEO_ESTATE, {int((status == R.GEO_EINVAL).sum())} GEO_EINVAL; {os.path.getsize(a.out)} bytes")
    print("returns taken:", R.hits(lib).tolist())


if __name__ == "__main__":
    main()
