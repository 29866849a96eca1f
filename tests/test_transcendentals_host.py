"""The host twin of tests/test_gpu_transcendentals.py, and the range of
lambda' that reaches sincos_sky_.  No GPU.

test_host_header_*: tests/native/transcendentals_exhaustive.hip built for the
host only (g++ with the float flags of the CPU baseline; its kernels are
compiled out), --host mode: every 64th bit pattern and +-4096 patterns around
each function's edges (0, the denormals, 0.5, 1, k pi/2, the atan2 thresholds
tan(pi/8) and tan(3 pi/8), 1e4, 2^21, the worst inputs of the exhaustive
sweep), the scaled and hashed pairs of the atan2 forms in full.  Reference:
glibc in f64.  The bars and range properties are the GPU sweep's
(tests/transcendental_bars.py), and the header equals the oracle's exported
mirror bit for bit on the same inputs.  The signaling NaNs next to +-inf
(0x7f800001.., 0xff800001..) are the regression case of the sweep's one
finding: a g++ build and the mirror clamped |x| with glibc's fminf, which
answers a signaling NaN with NaN, where the kernel's v_min_f32 gives
asin(+-1) and an acos_pi_ in [0, 1] (geo_math.h min_nan_b_).

test_unmasked_lambda_*: which lambda' = fl(fl(pi/2) - angle) the fuzzed
scenes hand to sincos_sky_ unmasked (lambda' >= -7), against the reduction's
precondition |x| < 2^21 and the range [-7, fl(pi/2) + 2^-20] on which its
2e-7 bound is stated."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from fuzz_scenes import adversarial_scene, random_scene
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import GEO_MODE_DIRECT
from transcendental_bars import FUNCTIONS, SOURCE, check_bars, parse

HOST_FLAGS = ["-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-msse4.1", "-pthread"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tx") / "transcendentals_host")
    subprocess.run(["g++", *HOST_FLAGS, SOURCE, "-o", path, "-ldl"], check=True)
    return path


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_host_header_meets_its_bar_and_equals_the_oracle(exe, fn):
    threads = str(min(8, os.cpu_count() or 1))
    r = subprocess.run([exe, fn, "--host", "--oracle", O.LIB_PATH, "--threads", threads], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    fig = parse(r.stdout)
    print(fn, "worst", fig["worst"], "at", fig["worst_at"], "measured", fig["measured"])
    assert fig["measured"] > 0
    assert fig["oracle_mismatches"] == 0 or fn == "acosf_"  # acosf_ has no exported mirror
    check_bars(fn, fig)


# ---- the lambda' that reaches sincos_sky_ ----

F32_PI2 = np.float32(math.pi / 2)
SAMPLED_HI = float(F32_PI2) + 2.0 ** -20
THETAS = np.unique(np.concatenate([
    np.linspace(-math.pi / 2, math.pi / 2, 257),
    -math.pi / 2 + np.logspace(-9, -1, 33),
    math.pi / 2 - np.logspace(-9, -1, 33),
]))
ST = np.sin(THETAS).astype(np.float32)
CT = np.cos(THETAS).astype(np.float32)


def lambdas(scene):
    """lambda' of every sampled theta, as the kernel forms it."""
    lam = np.empty(len(ST), dtype=np.float32)
    for i in range(len(ST)):
        a, _ = O.geodesic_f32(scene, float(ST[i]), float(CT[i]))
        lam[i] = F32_PI2 - np.float32(a)
    return lam


def sweep(gen, adaptive):
    """(lo, hi, seed of hi) of the unmasked lambda' over seeds 0..119; asserts
    no NaN and the reduction's precondition on every one."""
    lo, hi, hi_seed = math.inf, -math.inf, None
    for seed in range(120):
        _, scene, desc = gen(seed, 64, 36, adaptive)
        lam = lambdas(scene)
        assert not np.isnan(lam).any(), desc
        un = lam[lam >= -7.0]
        if un.size == 0:
            continue
        assert np.abs(un).max() < 2.0 ** 21, (desc, float(np.abs(un).max()))
        lo = min(lo, float(un.min()))
        if float(un.max()) > hi:
            hi, hi_seed = float(un.max()), seed
    return lo, hi, hi_seed


@pytest.mark.parametrize("gen,adaptive", [(random_scene, False), (random_scene, True), (adversarial_scene, True)],
                         ids=["random-direct", "random-adaptive", "adversarial-adaptive"])
def test_unmasked_lambda_stays_in_the_sampled_range(gen, adaptive):
    lo, hi, hi_seed = sweep(gen, adaptive)
    print("unmasked lambda' in [%.6g, %.9g] (largest at seed %s)" % (lo, hi, hi_seed))
    assert -7.0 <= lo and hi <= SAMPLED_HI, (lo, hi, hi_seed)


def test_unmasked_lambda_of_large_direct_steps_keeps_the_precondition():
    """Direct mode at the adversarial scenes' large steps: Newton's refinement
    from a far overshoot returns a negative traveled angle, so lambda' leaves
    [-7, pi/2] upward (tens of radians; printed with its seed).  It stays far
    inside |x| < 2^21, where sincos_sky_ still reduces, with the derived error
    bound of geo_math.h.  Also one targeted family: the largest step the
    generator allows (3.0) at budgets 1..17."""
    lo, hi, hi_seed = sweep(adversarial_scene, False)
    print("adversarial direct: unmasked lambda' in [%.6g, %.6g], largest at seed %s (%s)" %
          (lo, hi, hi_seed, adversarial_scene(hi_seed, 64, 36, False)[2]))
    worst = (0.0, None)
    for r in (1.01, 1.3, 1.6, 5.0, 39.0):
        for sphere_r in (50.0, 2.0):
            for budget in range(1, 18):
                scene = make_scene(1.0, sphere_r, r, 3.0, budget, GEO_MODE_DIRECT)
                lam = lambdas(scene)
                assert not np.isnan(lam).any(), (r, sphere_r, budget)
                un = lam[lam >= -7.0]
                if un.size:
                    assert np.abs(un).max() < 2.0 ** 21, (r, sphere_r, budget, float(np.abs(un).max()))
                    if float(un.max()) > worst[0]:
                        worst = (float(un.max()), (r, sphere_r, budget))
    print("step 3.0, budgets 1..17: largest unmasked lambda' %.6g at (r, sphere_r, budget) = %s" % worst)
