"""The render call rules for geo_render_disk_adaptive_ring_batch
(Entry::kDiskAdaptiveRingBatch, csrc/geo_render_rules.h) as a host build
(tests/native/render_rules_adaptive_ring_batch_host.cpp), with the expected
values taken from the committed matrix tests/golden/render_rules_matrix.npz,
not from the rules under test.

The entry is geo_render_disk_adaptive_batch with the state of
geo_set_disk_ring_f64 required instead of refused, so every case C of the
matrix (tests/render_rules_cases.py) with entry geo_render_disk_adaptive_batch
and the state off says what the new entry answers for the same call:

    with the state on   C's committed status; on GEO_OK launch_ring_frames
                        where there is a capture orbit to draw (rs > 0 and
                        r_obs > rs), launch_adaptive_frames otherwise (rs = 0:
                        the state is ignored)
    with the state off  never GEO_OK: GEO_ESTATE wherever C is GEO_OK or
                        GEO_ESTATE (rule 33, or the earlier GEO_ESTATE that C
                        met), GEO_EINVAL or GEO_ESTATE elsewhere

tests/test_render_rules_host.py keeps the committed matrix itself, entries
0..10, against the same header, and
tests/test_render_rules_adaptive_ring_host.py entry 11."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import render_rules_cases as R

SRC = os.path.join(R.HERE, "native", "render_rules_adaptive_ring_batch_host.cpp")
SO = os.path.join(R.HERE, "native", "librender_rules_adaptive_ring_batch_host.so")
GOLDEN = os.path.join(R.HERE, "golden", "render_rules_matrix.npz")
ADAPTIVE_BATCH = R.ENTRIES.index("geo_render_disk_adaptive_batch")
RING_FRAMES = R.LAUNCHERS.index("launch_ring_frames")
ADAPTIVE_FRAMES = R.LAUNCHERS.index("launch_adaptive_frames")


@pytest.fixture(scope="module")
def lib():
    deps = [SRC, os.path.join(R.HERE, "..", "include", "geo", "geo.h")] + [
        os.path.join(R.CSRC, h) for h in ("geo_render_rules.h", "geo_pixel.h", "geo_math.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", *R.GXX_FLAGS, "-fPIC", "-shared", "-o", SO, SRC], check=True)
    so = ctypes.CDLL(SO)
    so.adaptive_ring_batch_run.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    assert so.adaptive_ring_batch_case_bytes() == R.CASE.itemsize
    assert so.adaptive_ring_batch_entry() == len(R.ENTRIES) + 1 == 12  # appended after the one-frame ring entry
    assert so.adaptive_ring_batch_ring_launcher() == RING_FRAMES
    assert so.adaptive_ring_batch_adaptive_launcher() == ADAPTIVE_FRAMES
    return so


def run(so, cases):
    cases = np.ascontiguousarray(cases)
    status = np.zeros(len(cases), np.int8)
    launcher = np.zeros(len(cases), np.uint8)
    assert so.adaptive_ring_batch_run(cases.ctypes.data, len(cases), status.ctypes.data, launcher.ctypes.data) == 0
    return status, launcher


@pytest.fixture(scope="module")
def committed():
    """The matrix's cases of geo_render_disk_adaptive_batch with the state off, and their committed status and
    launcher."""
    want = np.load(GOLDEN)
    cases, status, launcher, at = [], [], [], 0
    for _, c in R.blocks():
        m = (c["entry"] == ADAPTIVE_BATCH) & (c["disk_ring"] == 0)
        cases.append(c[m])
        status.append(want["status"][at:at + len(c)][m])
        launcher.append(want["launcher"][at:at + len(c)][m])
        at += len(c)
    assert at == len(want["status"])
    return np.concatenate(cases), np.concatenate(status), np.concatenate(launcher)


def test_state_on_is_the_adaptive_batchs_answer(lib, committed):
    cases, want_status, want_launcher = committed
    assert len(cases) >= 10_000
    c = cases.copy()
    c["entry"] = lib.adaptive_ring_batch_entry()
    c["disk_ring"] = 1
    status, launcher = run(lib, c)
    bad = np.flatnonzero(status != want_status)
    assert not len(bad), f"{len(bad)} of {len(c)} differ; the first: {R.describe(cases[bad[0]])}: {status[bad[0]]}, " \
                         f"geo_render_disk_adaptive_batch with the state off has {want_status[bad[0]]}"
    ok = status == R.GEO_OK
    assert (want_launcher[ok] == ADAPTIVE_FRAMES).all()  # (what the committed matrix has for the older call)
    # a capture orbit to draw: frame 0's scene, as the rules decide it (a batch's frames share rs, and an
    # accepted batch's observers are all outside the horizon)
    s0 = c["scene"][:, 0]
    orbit = (s0["rs"] > 0) & (s0["r_obs"] > s0["rs"])
    assert (launcher[ok & orbit] == RING_FRAMES).all()
    assert (launcher[ok & ~orbit] == ADAPTIVE_FRAMES).all()
    assert (launcher[~ok] == 255).all()
    # the case set holds all three statuses and both launchers for the new entry
    assert {int(s) for s in np.unique(status)} == {R.GEO_OK, R.GEO_EINVAL, R.GEO_ESTATE}
    assert {int(l) for l in np.unique(launcher[ok])} == {RING_FRAMES, ADAPTIVE_FRAMES}
    print("state on:", {n: int((status == v).sum()) for n, v in (("GEO_OK", 0), ("GEO_EINVAL", -1), ("GEO_ESTATE", -5))},
          {"launch_ring_frames": int((launcher == RING_FRAMES).sum()),
           "launch_adaptive_frames": int((launcher == ADAPTIVE_FRAMES).sum())})


def test_state_off_is_never_drawn(lib, committed):
    cases, want_status, _ = committed
    c = cases.copy()
    c["entry"] = lib.adaptive_ring_batch_entry()
    status, launcher = run(lib, c)
    assert not (status == R.GEO_OK).any() and (launcher == 255).all()
    drawn_or_out_of_order = (want_status == R.GEO_OK) | (want_status == R.GEO_ESTATE)
    assert (want_status == R.GEO_OK).sum() > 0
    assert (status[drawn_or_out_of_order] == R.GEO_ESTATE).all()
    assert np.isin(status[~drawn_or_out_of_order], (R.GEO_EINVAL, R.GEO_ESTATE)).all()
    assert (status == R.GEO_EINVAL).any()
    print("state off:", {n: int((status == v).sum()) for n, v in (("GEO_EINVAL", -1), ("GEO_ESTATE", -5))})
