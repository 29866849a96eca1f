"""The render call rules for geo_render_disk_adaptive_ring
(Entry::kDiskAdaptiveRing, csrc/geo_render_rules.h) as a host build
(tests/native/render_rules_adaptive_ring_host.cpp), with the expected values
taken from the committed matrix tests/golden/render_rules_matrix.npz, not from
the rules under test.

The entry is geo_render_disk_adaptive with the state of geo_set_disk_ring_f64
required instead of refused, so every case C of the matrix
(tests/render_rules_cases.py) with entry geo_render_disk_adaptive and the state
off says what the new entry answers for the same call:

    with the state on   C's committed status, and on GEO_OK launch_disk_frame
    with the state off  never GEO_OK: GEO_ESTATE wherever C is GEO_OK or
                        GEO_ESTATE (rule 33, or the earlier GEO_ESTATE that C
                        met), GEO_EINVAL or GEO_ESTATE elsewhere

tests/test_render_rules_host.py keeps the committed matrix itself, entries
0..10, against the same header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import render_rules_cases as R

SRC = os.path.join(R.HERE, "native", "render_rules_adaptive_ring_host.cpp")
SO = os.path.join(R.HERE, "native", "librender_rules_adaptive_ring_host.so")
GOLDEN = os.path.join(R.HERE, "golden", "render_rules_matrix.npz")
DISK_ADAPTIVE = R.ENTRIES.index("geo_render_disk_adaptive")
DISK_FRAME = R.LAUNCHERS.index("launch_disk_frame")


@pytest.fixture(scope="module")
def lib():
    deps = [SRC, os.path.join(R.HERE, "..", "include", "geo", "geo.h")] + [
        os.path.join(R.CSRC, h) for h in ("geo_render_rules.h", "geo_pixel.h", "geo_math.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", *R.GXX_FLAGS, "-fPIC", "-shared", "-o", SO, SRC], check=True)
    so = ctypes.CDLL(SO)
    so.adaptive_ring_run.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    assert so.adaptive_ring_case_bytes() == R.CASE.itemsize
    assert so.adaptive_ring_entry() == len(R.ENTRIES) == 11  # appended after the matrix's entries
    assert so.adaptive_ring_disk_frame_launcher() == DISK_FRAME
    return so


def run(so, cases):
    cases = np.ascontiguousarray(cases)
    status = np.zeros(len(cases), np.int8)
    launcher = np.zeros(len(cases), np.uint8)
    assert so.adaptive_ring_run(cases.ctypes.data, len(cases), status.ctypes.data, launcher.ctypes.data) == 0
    return status, launcher


@pytest.fixture(scope="module")
def committed():
    """The matrix's cases of geo_render_disk_adaptive with the state off, and their committed status and launcher."""
    want = np.load(GOLDEN)
    cases, status, launcher, at = [], [], [], 0
    for _, c in R.blocks():
        m = (c["entry"] == DISK_ADAPTIVE) & (c["disk_ring"] == 0)
        cases.append(c[m])
        status.append(want["status"][at:at + len(c)][m])
        launcher.append(want["launcher"][at:at + len(c)][m])
        at += len(c)
    assert at == len(want["status"])
    return np.concatenate(cases), np.concatenate(status), np.concatenate(launcher)


def test_state_on_is_the_adaptive_disk_calls_answer(lib, committed):
    cases, want_status, want_launcher = committed
    assert len(cases) >= 10_000
    c = cases.copy()
    c["entry"] = lib.adaptive_ring_entry()
    c["disk_ring"] = 1
    status, launcher = run(lib, c)
    bad = np.flatnonzero(status != want_status)
    assert not len(bad), f"{len(bad)} of {len(c)} differ; the first: {R.describe(cases[bad[0]])}: {status[bad[0]]}, " \
                         f"geo_render_disk_adaptive with the state off has {want_status[bad[0]]}"
    ok = status == R.GEO_OK
    assert (want_launcher[ok] == DISK_FRAME).all()  # (what the committed matrix has for the older call)
    assert (launcher[ok] == DISK_FRAME).all() and (launcher[~ok] == 255).all()
    # the case set holds all three statuses for the new entry
    assert {int(s) for s in np.unique(status)} == {R.GEO_OK, R.GEO_EINVAL, R.GEO_ESTATE}
    print("state on:", {n: int((status == v).sum()) for n, v in (("GEO_OK", 0), ("GEO_EINVAL", -1), ("GEO_ESTATE", -5))})


def test_state_off_is_never_drawn(lib, committed):
    cases, want_status, _ = committed
    c = cases.copy()
    c["entry"] = lib.adaptive_ring_entry()
    status, launcher = run(lib, c)
    assert not (status == R.GEO_OK).any() and (launcher == 255).all()
    drawn_or_out_of_order = (want_status == R.GEO_OK) | (want_status == R.GEO_ESTATE)
    assert (want_status == R.GEO_OK).sum() > 0
    assert (status[drawn_or_out_of_order] == R.GEO_ESTATE).all()
    assert np.isin(status[~drawn_or_out_of_order], (R.GEO_EINVAL, R.GEO_ESTATE)).all()
    assert (status == R.GEO_EINVAL).any()
    print("state off:", {n: int((status == v).sum()) for n, v in (("GEO_EINVAL", -1), ("GEO_ESTATE", -5))})
