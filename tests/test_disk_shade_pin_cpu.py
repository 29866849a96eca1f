"""The CPU path's disk renders pinned to recorded digests
(tests/golden/disk_shade_pin.json, written by tests/golden/make_disk_shade_pin.py
on a build of commit 284f746).  csrc/geo_disk.h has two shading paths for the
same f32 operations, disk_shade / _shift / _emit on Uk, steps and angle beside
disk_hits_f32 + disk_shade_hits on DiskHits, and a change that folds them into
one has to leave every byte below where it is.

The GPU tests compare the kernels with the CPU path, and both sides include the
same header, so a change to the shading moves both together and those tests stay
green.  This one holds the CPU side still: SHA-256 of every output array (rgba,
mask, uv, steps, hits, g, q, total) of

  pose    A, B, ring, tilted of tests/test_disk_cpu.py at 40 x 20
  shade   plain, shift, emission
  mode    GEO_MODE_DIRECT, GEO_MODE_ADAPTIVE
  ring    geo_set_disk_ring_f64's state off, on

48 cases, every one GEO_OK (pose tilted has rs = 0: the state is accepted and
ignored).  hits, g and q are prefilled with -1, so a render that stops writing
one of them, or starts to, changes its digest too.  A mismatch names the case
and the array."""
import hashlib
import json
import os

import numpy as np
import pytest

import test_disk_adaptive_ring_cpu as AR
import test_disk_cpu as T
import test_disk_emission_cpu as TE
import test_disk_ring_cpu as RC
from schwarzschild_raytracer_wgpu_amd._lib import GEO_OK

W, H = 40, 20
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disk_shade_pin.json")
ARRAYS = ("rgba", "mask", "uv", "steps", "hits", "g", "q", "total")
POSES = ("A", "B", "ring", "tilted")
# (gain 2: at rest in flat space g = 1, and gain 1 would draw the unshaded frame)
SHADES = {"plain": dict(), "shift": dict(shift=(1, 4, 2.0)), "emission": dict(em=TE.emission())}
CASES = [(p, s, m, r) for p in POSES for s in SHADES for m in ("direct", "adaptive") for r in (0, 1)]
IDS = [f"{p}-{s}-{m}-ring_{'on' if r else 'off'}" for p, s, m, r in CASES]


def digests(lib, pose, shade, mode, ring):
    """The case's status and the SHA-256 of each output array."""
    frame, scene, disk, _ = T.pose(pose, W, H)
    if mode == "adaptive":
        rc, c = AR.render(lib, frame, AR.scenes_of(scene)[0], disk, ring, W, H, **SHADES[shade])
    else:
        rc, c = RC.render(lib, frame, scene, disk, ring, W, H, **SHADES[shade])
    out = {"rc": int(rc)}
    for a in ARRAYS:
        v = np.uint64(c[a]) if a == "total" else np.ascontiguousarray(c[a])
        out[a] = hashlib.sha256(v.tobytes()).hexdigest()
    return out


@pytest.fixture(scope="module")
def cpu():
    return AR.load_cpu()


@pytest.fixture(scope="module")
def pinned():
    return json.load(open(FIXTURE))


def test_the_fixture_holds_every_case(pinned):
    assert sorted(pinned) == sorted(IDS) and len(IDS) == 48
    assert all(v["rc"] == GEO_OK for v in pinned.values())
    # the cases are told apart: the state moves the hits of the poses with band pixels (B, ring; the
    # colour too on ring) and nothing on A and tilted, and no other two colour digests are equal
    for p, s, m, _ in CASES:
        off, on = (pinned[f"{p}-{s}-{m}-ring_{r}"] for r in ("off", "on"))
        assert (off["hits"] != on["hits"]) == (p in ("B", "ring")), (p, s, m)
        assert (off["rgba"] != on["rgba"]) == (p == "ring"), (p, s, m)
        assert (off == on) == (p in ("A", "tilted")), (p, s, m)
    assert len({v["rgba"] for v in pinned.values()}) == 48 - 3 * 3 * 2


@pytest.mark.parametrize("pose,shade,mode,ring", CASES, ids=IDS)
def test_digests(cpu, pinned, pose, shade, mode, ring):
    case = IDS[CASES.index((pose, shade, mode, ring))]
    got = digests(cpu, pose, shade, mode, ring)
    assert got["rc"] == pinned[case]["rc"], case
    bad = [a for a in ARRAYS if got[a] != pinned[case][a]]
    assert not bad, f"{case}: {', '.join(bad)} differ from the pinned render"
