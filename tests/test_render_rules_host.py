"""The render call rules (csrc/geo_render_rules.h: the entry points' argument
stages, check_scene, check_frames and choose_launcher) as a host build
(tests/native/render_rules_host.cpp), against the committed matrix
tests/golden/render_rules_matrix.npz: the status of every described call and,
for GEO_OK, the launcher taken, case for case.

The matrix (tests/render_rules_cases.py) is the full product of the 11 entry
points x mode 0, 1, 2 and an invalid one x 66 flag words (the 64 combinations
of the known bits, an unknown bit alone and with GEO_FLAG_DISK) x the 16 states
of disk, shift, emission and ring x 4 armed buffers x 2 side outputs x 1, 2 and
8 frames (the one-frame entry points: 1) x 4 geometries = 3 379 200 calls, and
after it 61 inputs varied one at a time over 11 entry points x 3 modes x 8 flag
words x 6 states (96 624 calls): 3 475 824 calls, of which 118 901 are GEO_OK,
6 555 GEO_ESTATE and 3 350 368 GEO_EINVAL.  The fixture was written from the
rules as they stood in geo_render.hip before they moved (they agreed on every
case with that file's text compiled for the host).

Every `return` of the rules is taken by the matrix; the test asserts it from
the counters of the host build (GEO_RULE).  Measured, by return number:

    band_set_ok            0: 10 080    1: 2 592      2: 3 888
    frame_call             3: 2 304     4: 432        5: 1 008     6: 1 152    7: 288    8: 432    9: 3 456
    batch_call            10: 6 048    11: 13 104
    check_scene           12: 844 800  13: 76 800    14: 397 412  15: 1 040 148  16: 151 992  17: 439 368
                          18: 232 272  19: 9 216     20: 1 016    21: 1 962    22: 93 474   23: 126
                          24: 26 493   25: 1 602     26: 435      27: 133      28: 435 (no sky)
                          29: 156 (no fan)           30: 1 428    31: 4 968 (no disk)      32: 360 (no emission)
                          33: 636 (ring state off)   34: 1 157    35: 690      36: 480
    check_frames          37: 876      38: 96        39: 168
"""
import numpy as np
import pytest

import render_rules_cases as R

GOLDEN = R.os.path.join(R.HERE, "golden", "render_rules_matrix.npz")


@pytest.fixture(scope="module")
def lib():
    return R.load()


def test_matrix_equals_the_committed_one(lib):
    want = np.load(GOLDEN)
    want_status, want_launcher = want["status"], want["launcher"]
    at = 0
    for name, cases in R.blocks():
        status, launcher = R.run(lib, cases)
        ws, wl = want_status[at:at + len(cases)], want_launcher[at:at + len(cases)]
        assert len(ws) == len(cases), "the matrix is longer than the fixture: " + name
        bad = np.flatnonzero((status != ws) | (launcher != wl))
        if len(bad):
            i = int(bad[0])
            word = lambda s, l: {0: "GEO_OK by " + (R.LAUNCHERS[l] if l < len(R.LAUNCHERS) else "?"), -1: "GEO_EINVAL",
                                 -5: "GEO_ESTATE"}.get(int(s), str(int(s)))
            pytest.fail(f"{len(bad)} of {len(cases)} cases of \"{name}\" differ; the first (case {at + i}): "
                        f"{R.describe(cases[i])}: {word(status[i], launcher[i])}, the fixture has {word(ws[i], wl[i])}")
        at += len(cases)
    assert at == len(want_status) == 3_475_824
    # every return of the rules was taken (the module's docstring has the counts)
    taken = R.hits(lib)
    print("returns taken:", taken.tolist())
    assert len(taken) == 40 and (taken > 0).all(), np.flatnonzero(taken == 0).tolist()


def test_matrix_holds_every_status_of_every_entry_point():
    """What the matrix says of itself: every entry point is accepted, refused
    and out of order somewhere, and every launcher is taken."""
    want = np.load(GOLDEN)
    status, launcher = want["status"], want["launcher"]
    entry = np.concatenate([c["entry"] for _, c in R.blocks()])
    for e in range(len(R.ENTRIES)):
        assert {int(s) for s in np.unique(status[entry == e])} == {R.GEO_OK, R.GEO_EINVAL, R.GEO_ESTATE}, R.ENTRIES[e]
    assert set(np.unique(launcher[status == 0]).tolist()) == set(range(len(R.LAUNCHERS)))
    assert (launcher[status != 0] == 255).all()
