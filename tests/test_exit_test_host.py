"""The end-state exit test of the group loop (geo_pixel.h, kTestEnd) against
the exact one (kTestLow), on the CPU: the host build of the product header
with the test form forced (tests/native/exit_test_host.cpp).  Every lane the
selector of make_consts admits must give the same angle bits and step count
both ways; a lane or frame it refuses must take the exact loop.  The corner
cases sit on both sides of each limit of the selector."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from fuzz_scenes import REGRESSION_SEEDS, random_scene

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "exit_test_host.cpp")
SO = os.path.join(HERE, "native", "libexit_test_host.so")

f32 = np.float32
BUDGETS = (1, 3, 4, 5, 7, 8, 9, 2048)


@pytest.fixture(scope="module")
def lib():
    deps = [SRC] + [os.path.join(HERE, "..", "schwarzschild_raytracer_wgpu_amd", "csrc", h)
                    for h in ("geo_pixel.h", "geo_math.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-mfma",
                        "-msse4.1", "-o", SO, SRC], check=True)
    so = ctypes.CDLL(SO)
    so.exit_selector.argtypes = [ctypes.c_float] * 4 + [ctypes.c_uint32, ctypes.c_void_p]
    so.exit_selector.restype = None
    so.exit_compare.argtypes = [ctypes.c_float] * 4 + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32] + \
        [ctypes.c_void_p] * 7
    so.exit_compare.restype = ctypes.c_int
    so.exit_sweep.argtypes = [ctypes.c_float] * 3 + [ctypes.c_uint32, ctypes.c_float, ctypes.c_float, ctypes.c_uint32,
                                                      ctypes.c_uint32, ctypes.c_float, ctypes.c_float, ctypes.c_uint32,
                                                      ctypes.c_void_p]
    so.exit_sweep.restype = ctypes.c_int
    return so


def selector(lib, rs, sphere_r, r, step, max_steps=2048):
    out = np.zeros(7, dtype=np.uint32)
    lib.exit_selector(rs, sphere_r, r, step, max_steps, out.ctypes.data)
    fl = out.view(np.float32)
    return {"admit": bool(out[0] & 8), "above0": bool(out[0] & 1), "kind": int(out[1]), "end_lo": float(fl[2]), "end_hi": float(fl[3]),
            "lo": fl[4], "U0": fl[5], "hi": float(fl[6])}


def compare(lib, rs, sphere_r, r, step, max_steps, ub):
    ub = np.ascontiguousarray(ub, dtype=np.float32)
    n = len(ub)
    o = [np.zeros(n, dtype=np.uint32) for _ in range(6)]
    inside = np.zeros(n, dtype=np.uint8)
    rc = lib.exit_compare(rs, sphere_r, r, step, max_steps, ub.ctypes.data, n, *[a.ctypes.data for a in o],
                          inside.ctypes.data)
    assert rc == 0, "not a frame with the observer inside the sphere"
    return o, inside.astype(bool)


def check(lib, rs, sphere_r, r, step, max_steps, ub, what):
    """Admitted lanes: kTestEnd == kTestLow; every lane: the selector's loop
    == kTestLow.  Returns the admitted lanes."""
    (al, sl, ae, se, aa, sa), inside = compare(lib, rs, sphere_r, r, step, max_steps, ub)
    bad = inside & ((al != ae) | (sl != se))
    assert not bad.any(), (what, step, max_steps, np.asarray(ub)[bad][:4], sl[bad][:4], se[bad][:4])
    bad = (al != aa) | (sl != sa)
    assert not bad.any(), (what, "selector", step, max_steps, np.asarray(ub)[bad][:4])
    return inside


def lane_values(B):
    """UB0 around the lane bound B and across the falling side."""
    B = f32(B)
    out = [-B, -np.nextafter(B, f32(np.inf)), -np.nextafter(B, f32(0)), -f32(10) * B, -f32(0.5) * B, f32(-0.0),
           f32(0.0), f32(-1e-30), f32(1e-30), f32(-1e-6), f32(1e-6), f32(-1e-3), f32(1e-3), f32(-0.1), f32(0.1),
           f32(0.3), f32(0.55), f32(0.6), f32(1.0), f32(10.0), f32(1e6), f32(2.0 ** 40),
           np.nextafter(f32(2.0 ** 40), f32(np.inf)), f32(1e20), f32(np.inf), f32(-np.inf), f32(np.nan),
           # near-radial outgoing rays: UB0 = -ub_k tan, rotation = r cos just above 1e-10
           f32(-4.6e9), f32(-1e8), f32(-3e4), f32(-50.0)]
    return np.array(out, dtype=np.float32)


def h_bound(lib, rs, sphere_r, r):
    """The largest step the selector admits for the scene (bisection on the
    floats between the known sides)."""
    lo, hi = f32(0.03), f32(0.0625)
    assert selector(lib, rs, sphere_r, r, lo)["admit"] and not selector(lib, rs, sphere_r, r, hi)["admit"]
    a, b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while b - a > 1:
        m = (a + b) // 2
        if selector(lib, rs, sphere_r, r, np.uint32(m).view(np.float32))["admit"]:
            a = m
        else:
            b = m
    return np.uint32(a).view(np.float32)


def test_step_bound_and_lane_bound(lib):
    rs, sphere_r, r = 1.0, 50.0, 2.5
    hb = h_bound(lib, rs, sphere_r, r)
    # h (sqrt(B^2 + 1) + 2 h) = 1/20 at B = 0
    assert abs(float(hb) - (math.sqrt(1.4) - 1.0) / 4.0) < 1e-6
    above = np.nextafter(hb, f32(1))
    for h in (hb, np.nextafter(hb, f32(0)), f32(0.045), f32(math.pi / 100), f32(0.01), f32(2.0 ** -10)):
        s = selector(lib, rs, sphere_r, r, h)
        assert s["admit"] and s["end_lo"] <= 0.0
        B = -s["end_lo"]
        # the derived lane bound: B^2 = w^2 - 1, w = 1/(20 h) - 2 h evaluated in
        # f32 (three roundings, at most 4e-7 w in all)
        w = 0.05 / float(h) - 2.0 * float(h)
        assert B * B <= max(w * w - 1.0, 0.0) + 1e-6 * w * w
        for ms in BUDGETS:
            inside = check(lib, rs, sphere_r, r, h, ms, lane_values(max(B, 1e-3)), "inside")
            ub = lane_values(max(B, 1e-3))
            assert inside[ub == f32(-B)].all() and not inside[ub < f32(-B)].any()
            assert not inside[np.isnan(ub)].any() and not inside[ub > f32(2.0 ** 40)].any()
    assert not selector(lib, rs, sphere_r, r, 2.0 ** -11)["admit"]  # (a kCurvedIn frame: the per-step test)
    for h in (above, f32(0.05), f32(0.0625), f32(0.093), f32(0.3)):
        s = selector(lib, rs, sphere_r, r, h)
        assert not s["admit"], h
        for ms in BUDGETS:
            inside = check(lib, rs, sphere_r, r, h, ms, lane_values(1.0), "refused")
            assert not inside.any()


def scene_just_inside(lib, rs, sphere_r, ulps):
    """r (the observer) with U0 at least `ulps` floats above lo = SU+, the
    closest such r below sphere_r."""
    r = f32(sphere_r)
    for _ in range(200000):
        r = np.nextafter(r, f32(0))
        s = selector(lib, rs, sphere_r, r, math.pi / 100)
        d = int(s["U0"].view(np.uint32)) - int(s["lo"].view(np.uint32))
        if s["above0"] and d >= ulps:  # (U0 == SU is still "outside": the interval is then [BD, SU])
            return float(r), d
    raise AssertionError("no such observer")


@pytest.mark.parametrize("rs", [0.9, 0.0], ids=["curved", "flat"])
@pytest.mark.parametrize("ulps", [1, 2, 1000])
def test_observer_just_inside_the_sphere(lib, rs, ulps):
    """The grazing exit: U0 a few floats above lo, rays tangential to steep."""
    sphere_r = 1.9
    r, d = scene_just_inside(lib, rs, sphere_r, ulps)
    assert ulps <= d <= 2 * ulps + 2
    for h in (f32(math.pi / 100), f32(0.045), f32(2.0 ** -10)):
        s = selector(lib, rs, sphere_r, r, h)
        assert s["admit"]
        for ms in BUDGETS:
            inside = check(lib, rs, sphere_r, r, h, ms, lane_values(max(-s["end_lo"], 1e-3)), f"ulps={d}")
            assert inside.any()


@pytest.mark.parametrize("rs,sphere_r,r", [(1.0, 50.0, 2.5), (1.0, 50.0, 1.6), (1.0, 50.0, 40.0), (1.0, 3.0, 2.9),
                                           (1.0, 2.01, 1.8), (0.0, 50.0, 2.5), (0.0, 50.0, 49.0), (0.0, 2.0, 0.5),
                                           (0.0, 1e4, 1e-3)])
def test_scenes_and_budgets(lib, rs, sphere_r, r):
    """kCurvedOut and kFlat (rs = 0) scenes, odd and even group budgets."""
    for h in (f32(math.pi / 100), f32(0.02), f32(0.045)):
        s = selector(lib, rs, sphere_r, r, h)
        assert s["admit"]
        if rs == 0.0:
            assert s["end_lo"] == -2.0 ** 40  # the flat map is linear: no bound but the finite range
        for ms in BUDGETS + (300,):
            check(lib, rs, sphere_r, r, h, ms, lane_values(max(-s["end_lo"], 1e-3) if rs else 1.0), "scene")


def test_frames_outside_the_selector(lib):
    """The frame-uniform limits: lo above 3/4 or below 2^-20, the observer
    inside the photon sphere with the sphere inside it too, a huge U0."""
    for rs, sphere_r, r in ((1.0, 1.9, 1.5), (1.0, 1.4, 1.2), (1.0, 2e6, 2.5), (0.0, 2e6, 2.5), (0.0, 1.0, 1e-7)):
        s = selector(lib, rs, sphere_r, r, math.pi / 100)
        assert not s["admit"], (rs, sphere_r, r)
        inside = check(lib, rs, sphere_r, r, math.pi / 100, 2048, lane_values(1.0), "frame")
        assert not inside.any()
    # lo on either side of 3/4 (rs = 1: lo = next_up(1.5 / sphere_r))
    assert selector(lib, 1.0, 2.001, 1.9, math.pi / 100)["admit"]
    assert not selector(lib, 1.0, 1.999, 1.9, math.pi / 100)["admit"]


def test_regression_seed_is_refused(lib):
    """Seed 70751 (step 0.093: RK4 overshoots U = 0 and comes back within a
    group) is outside the step bound."""
    for seed in REGRESSION_SEEDS:
        _, scene, desc = random_scene(seed, 64, 36)
        assert not selector(lib, scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps)["admit"], desc


@pytest.mark.parametrize("rs,sphere_r,r,budget", [(1.0, 50.0, 49.0, 64), (1.0, 50.0, 30.0, 128), (1.0, 2.1, 2.0, 64),
                                                  (0.0, 50.0, 45.0, 64)])
def test_dense_sweep_inside_the_bound(lib, rs, sphere_r, r, budget):
    """(UB0, h) pairs inside the bound, 4.2 million over the four scenes: h
    over [2^-10, the step bound], |UB0| from 1e-7 to the lane bound (outgoing)
    and to 2 (falling).  The observers sit close enough to the sphere for the
    outgoing rays to cross it within the budget."""
    hb = h_bound(lib, rs if rs else 1.0, 50.0, 2.5)
    out = np.zeros(4, dtype=np.uint64)
    n_h, n_ub = 1024, 1024
    lib.exit_sweep(rs, sphere_r, r, budget, 2.0 ** -10, float(hb), n_h, n_ub, 1e-7, 2.0, min(16, os.cpu_count() or 1),
                   out.ctypes.data)
    compared, differ, stopped, first = (int(x) for x in out)
    print(f"sweep rs={rs} sphere_r={sphere_r} r={r}: {compared} pairs, {stopped} stopped in the budget, {differ} differ")
    assert compared > 0.9 * n_h * n_ub and stopped > compared // 10
    assert differ == 0, (first // n_ub, first % n_ub)
