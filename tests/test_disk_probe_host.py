"""The disk probes of geo_disk.h (geodesic_angle_disk: the crossing cursor,
the `due` ballot, the several-probes-per-group arm and the budget tail) against
a per-step definition that has none of them (tests/native/disk_probe_host.cpp,
a host build of the product header): for r = 0 .. max_steps - 1, every crossing
whose node is r takes its partial step from the state at node r, then one RK4
step, until the first step StopTest flags.

Per lane, exactly: the traveled angle and step count of geodesic_angle_disk are
geodesic_angle_v's and the definition's; every crossing with a node below the
step count has the definition's U; disk_hit gives the same verdict and the same
(r, Ud, Vd) from either U.

The sweep is the product of SCENES x STEPS x BUDGETS x NORMALS x 48 x 8 rays =
1 866 240 lanes, and the test asserts that it reaches the paths the render
tests do not (budgets off the group grid, steps above pi/4, pi/2 and pi,
edge-on disks).  The lanes are classified from DiskRay and the definition's
step count alone.  Measured on the definition's side, with the floor asserted
beside each:

    probes compared (node < steps)                          1 176 853   (500 000)
    ... at a node >= (max_steps / 4) * 4 (the budget tail)    200 210   (100 000)
    ... in a whole group that holds the previous crossing     324 756   (150 000)
    ... at the previous crossing's node                        206 700   (100 000)
    crossings due in the stopping group at a node >= steps     983 021   (450 000)
    lanes with no crossing (jn[0] == 0xFFFFFFFF)                38 880    (19 000)
    lanes with N_z == 0                                        933 120   (450 000)
    probes disk_hit accepts                                    265 875   (130 000)
    lanes of kind kCurvedOut / kCurvedIn / kFlat   552 960 / 691 200 / 622 080
                                                  (250 000 / 300 000 / 300 000)
    mismatches                                                       0

What a host build cannot see: it has one lane per wave, so the `live` mask is
all or nothing and the group loop ends when it empties; `due & live` is `due`
here.  tests/test_gpu_disk_fuzz.py runs the kernels' waves against this path.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "disk_probe_host.cpp")
SO = os.path.join(HERE, "native", "libdisk_probe_host.so")

SCENES = ((1.0, 50.0, 14.9), (1.0, 50.0, 2.4), (0.0, 50.0, 10.8), (1.0, 50.0, 1.3), (1.0, 3.0, 2.5), (0.0, 50.0, 0.5))
STEPS = (math.pi / 100, 0.093, 0.3, 0.5, 0.8, 1.6, 3.0, 3.5, 7.0)
BUDGETS = (1, 2, 3, 4, 5, 7, 8, 9, 17, 47, 99, 102, 301, 2047, 2048)
NORMALS = ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.3, -0.2, 1.0), (1.0, 0.0, 1e-4), (0.6, 0.8, 0.0))
N_THETA, N_PHI = 48, 8

# the counters of disk_probe_sweep, in its order
NAMES = ("lanes", "mismatch", "first", "what", "compared", "tail", "same_group", "same_node", "refused", "no_crossing",
         "edge_on", "accepted", "stopped_lanes", "curved_out", "curved_in", "flat")
WHAT = ((1, "angle != geodesic_angle_v"), (2, "steps != geodesic_angle_v"), (4, "steps != the definition"),
        (8, "Uk != the definition"), (16, "disk_hit differs"))
# floors: round numbers no higher than half of the measured counts (docstring)
FLOORS = {"compared": 500_000, "tail": 100_000, "same_group": 150_000, "same_node": 100_000, "refused": 450_000,
          "no_crossing": 19_000, "edge_on": 450_000, "accepted": 130_000, "curved_out": 250_000, "curved_in": 300_000,
          "flat": 300_000}


def load():
    deps = [SRC] + [os.path.join(HERE, "..", "schwarzschild_raytracer_wgpu_amd", "csrc", h)
                    for h in ("geo_disk.h", "geo_pixel.h", "geo_math.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-mfma",
                        "-msse4.1", "-o", SO, SRC], check=True)
    so = ctypes.CDLL(SO)
    so.disk_probe_counters.restype = ctypes.c_uint32
    so.disk_probe_sweep.argtypes = [ctypes.c_void_p, ctypes.c_uint32] * 4 + [ctypes.c_uint32] * 3 + [ctypes.c_void_p]
    so.disk_probe_sweep.restype = ctypes.c_int
    so.disk_probe_lane.argtypes = [ctypes.c_float] * 4 + [ctypes.c_uint32, ctypes.c_void_p] + [ctypes.c_uint32] * 4 + \
        [ctypes.c_void_p]
    so.disk_probe_lane.restype = ctypes.c_int
    so.disk_probe_pixel.argtypes = [ctypes.c_void_p] + [ctypes.c_float] * 4 + [ctypes.c_uint32, ctypes.c_void_p] + \
        [ctypes.c_uint32] * 4 + [ctypes.c_void_p]
    so.disk_probe_pixel.restype = ctypes.c_int
    so.disk_probe_frame_nodes.argtypes = [ctypes.c_void_p] + [ctypes.c_float] * 4 + [ctypes.c_uint32, ctypes.c_void_p] + \
        [ctypes.c_uint32] * 2 + [ctypes.c_void_p]
    so.disk_probe_frame_nodes.restype = ctypes.c_int
    assert so.disk_probe_counters() == len(NAMES)
    return so


@pytest.fixture(scope="module")
def lib():
    return load()


def frame_nodes(lib, frame, scene, disk_args, w, h):
    """(h, w, 3) uint32: the nodes jn of every pixel's three crossings (0xFFFFFFFF: none)."""
    r_in, r_out, normal, axis = disk_args
    disk = np.array([r_in, r_out, *normal, *axis], dtype=np.float32)
    jn = np.zeros((h, w, 3), dtype=np.uint32)
    rc = lib.disk_probe_frame_nodes(ctypes.addressof(frame), scene.rs, scene.sphere_r, scene.r_obs, scene.step,
                                    scene.max_steps, disk.ctypes.data, w, h, jn.ctypes.data)
    assert rc == 0
    return jn


def hit_paths(jn, hit, max_steps):
    """From a frame's nodes and its hit slots (h, w, 3): the hits whose probe ran
    in the budget tail (node >= (max_steps / 4) * 4), and the hits whose probe
    was the second or third of its whole group of four (the previous crossing's
    node lies in the same group)."""
    whole = (max_steps // 4) * 4
    tail = hit & (jn >= whole)
    grouped = hit[..., 1:] & (jn[..., 1:] // 4 == jn[..., :-1] // 4) & (jn[..., 1:] < whole)
    return int(tail.sum()), int(grouped.sum())


def pixel(lib, frame, scene, disk_args, w, h, x, y):
    """Pixel (x, y) of a disk frame by the per-step definition: its crossings'
    nodes jn, its step count and its U at the crossings (bits)."""
    r_in, r_out, normal, axis = disk_args
    disk = np.array([r_in, r_out, *normal, *axis], dtype=np.float32)
    out = np.zeros(8, dtype=np.uint32)
    rc = lib.disk_probe_pixel(ctypes.addressof(frame), scene.rs, scene.sphere_r, scene.r_obs, scene.step,
                              scene.max_steps, disk.ctypes.data, w, h, x, y, out.ctypes.data)
    assert rc == 0
    return {"jn": [hex(v) for v in out[0:3]], "steps": int(out[3]), "U": [hex(v) for v in out[4:7]], "kind": int(out[7])}


def sweep(lib, scenes, steps, budgets, normals):
    sc = np.ascontiguousarray(scenes, dtype=np.float32)
    st = np.ascontiguousarray(steps, dtype=np.float32)
    bu = np.ascontiguousarray(budgets, dtype=np.uint32)
    no = np.ascontiguousarray(normals, dtype=np.float32)
    out = np.zeros(len(NAMES), dtype=np.uint64)
    rc = lib.disk_probe_sweep(sc.ctypes.data, len(sc), st.ctypes.data, len(st), bu.ctypes.data, len(bu),
                              no.ctypes.data, len(no), N_THETA, N_PHI, min(16, os.cpu_count() or 1), out.ctypes.data)
    assert rc == 0, rc
    return {n: int(v) for n, v in zip(NAMES, out)}


def describe(lib, c, scenes, steps, budgets, normals):
    """The first differing lane of a sweep: its frame, ray and both sides' values."""
    q, ray = divmod(c["first"], N_THETA * N_PHI)
    q, i_n = divmod(q, len(normals))
    q, i_b = divmod(q, len(budgets))
    i_s, i_h = divmod(q, len(steps))
    i, jp = divmod(ray, N_PHI)
    out = np.zeros(13, dtype=np.uint32)
    nv = np.ascontiguousarray(normals[i_n], dtype=np.float32)
    lib.disk_probe_lane(*scenes[i_s], steps[i_h], budgets[i_b], nv.ctypes.data, i, N_THETA, jp, N_PHI, out.ctypes.data)
    return (f"{c['mismatch']} lanes differ; first: scene={scenes[i_s]} step={steps[i_h]:.5f} max_steps={budgets[i_b]} "
            f"normal={normals[i_n]} theta#{i} phi#{jp} kind={out[12]}: "
            f"{', '.join(t for b, t in WHAT if c['what'] & b)}; steps={out[1]} definition's={out[2]} "
            f"jn={[hex(x) for x in out[3:6]]} Uk={[hex(x) for x in out[6:9]]} definition's={[hex(x) for x in out[9:12]]}")


def test_probes_equal_the_per_step_definition(lib):
    c = sweep(lib, SCENES, STEPS, BUDGETS, NORMALS)
    print("disk probe sweep:", {n: c[n] for n in NAMES if n not in ("first", "what")})
    assert c["lanes"] == len(SCENES) * len(STEPS) * len(BUDGETS) * len(NORMALS) * N_THETA * N_PHI
    # the reach conditions: a sweep that stops visiting a path fails here
    for name, floor in FLOORS.items():
        assert c[name] >= floor, (name, c[name], floor)
    assert c["mismatch"] == 0, describe(lib, c, SCENES, STEPS, BUDGETS, NORMALS)


def test_grid_budgets_at_the_render_tests_step(lib):
    """The corner the render tests live in (step pi/100, budgets on the group
    grid): no tail probe and no two probes in a group (9 444 probes compared,
    floor 4 000), and it agrees as well."""
    steps, budgets = (math.pi / 100,), (256, 512, 2048)
    c = sweep(lib, SCENES, steps, budgets, NORMALS)
    assert c["tail"] == 0 and c["same_group"] == 0 and c["same_node"] == 0 and c["compared"] >= 4_000
    assert c["mismatch"] == 0, describe(lib, c, SCENES, steps, budgets, NORMALS)
