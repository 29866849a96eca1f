"""The f32 transcendentals of geo_math.h on the GPU, over every input
(tests/native/transcendentals_exhaustive.hip, built here with hipcc for
gfx950 with the flags of tests/test_gpu_math.py):
  * the device's result bits equal the host build's of the same header, and
    the host build's equal the oracle's exported mirror (liboracle.so), for
    all 2^32 inputs of the one-argument functions and the input sets of the
    atan2 forms, so device = host header = oracle mirror input by input;
  * the device's error against the device's f64 library function stays
    inside the project's bars (tests/transcendental_bars.py), per binade;
  * the range properties hold on every input;
  * a sweep with one result bit of one input flipped on the device side
    fails and names the input.
A function's sweep is cut into equal parts, one test each, so that the host
side of a part (2^30 evaluations of the header and of the mirror for a
one-argument function, some 1.2e9 for an atan2 form, on at most 16 threads,
slowest where the intermediates are denormal) stays within seconds.

With GEO_TX_TABLES set to a directory each part's printed tables are kept
there (profiles/transcendentals_exhaustive_gpu.txt is those tables, the parts
of a function merged by binade)."""
import os
import shutil
import subprocess

import pytest

from transcendental_bars import FUNCTIONS, SOURCE, TWO_ARGS, check_bars, parse

pytestmark = pytest.mark.gpu

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero"]

# A part runs as long as its host pass: up to 2.6 s on an MI355X host's 16
# threads (the device side is under a second), and 11 to 12 s on 8 threads of a
# core on which a denormal result costs ~150 cycles (the parts of the small
# inputs).  Ten times the slower figure, so that only a hang reaches it.
TIMEOUT = 120

PARTS = {fn: (14 if fn in TWO_ARGS else 4) for fn in FUNCTIONS}  # 14 divides the atan2 sets by whole binades
CHUNKS = {fn: ((4 << 32) + (1 << 26) + (1 << 24) if fn in TWO_ARGS else 1 << 32) >> 16 for fn in FUNCTIONS}
# the input whose result the mutated sweep flips: x = 0.3f (a finite, inexact result in every
# function); for the atan2 forms (+1, 0.3f), the third form
MUTATE = {fn: ((2 << 32) if fn in TWO_ARGS else 0) | 0x3E99999A for fn in FUNCTIONS}


def part_of(fn: str, index: int) -> int:
    c = index >> 16
    for k in range(PARTS[fn]):
        if CHUNKS[fn] * k // PARTS[fn] <= c < CHUNKS[fn] * (k + 1) // PARTS[fn]:
            return k
    raise ValueError(index)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    path = str(tmp_path_factory.mktemp("tx") / "transcendentals_exhaustive")
    subprocess.run([HIPCC, *FLAGS, SOURCE, "-o", path, "-ldl"], check=True)
    return path


@pytest.fixture(scope="module")
def oracle_lib():
    import oracle as O

    return O.LIB_PATH


_abnormal = []  # a sweep that ended by a signal or its time limit: nothing more is started on the GPU


def run(args):
    if _abnormal:
        pytest.fail("not started: an earlier sweep ended abnormally (%s)" % _abnormal[0])
    try:
        r = subprocess.run(args, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _abnormal.append("time limit: " + " ".join(args[1:]))
        raise
    if r.returncode not in (0, 1):
        _abnormal.append("status %d: %s" % (r.returncode, " ".join(args[1:])))
    return r


def keep_tables(name: str, out: str) -> None:
    d = os.environ.get("GEO_TX_TABLES")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".txt"), "w") as f:
            f.write(out)


@pytest.mark.parametrize("fn,part", [(fn, k) for fn in FUNCTIONS for k in range(PARTS[fn])])
def test_device_equals_host_equals_oracle_and_meets_its_bar(exe, oracle_lib, fn, part):
    r = run([exe, fn, "--part", str(part), str(PARTS[fn]), "--oracle", oracle_lib])
    keep_tables("%s_%02d" % (fn, part), r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    fig = parse(r.stdout)
    print(fn, part, "worst", fig["worst"], "at", fig["worst_at"], "measured", fig["measured"])
    assert fig["mismatches"] == 0
    assert fig["oracle_mismatches"] == 0 or fn == "acosf_"  # acosf_ has no exported mirror
    check_bars(fn, fig)


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_a_flipped_result_bit_fails_the_sweep(exe, fn):
    index = MUTATE[fn]
    r = run([exe, fn, "--part", str(part_of(fn, index)), str(PARTS[fn]), "--mutate", hex(index)])
    assert r.returncode == 1, r.stdout[-4000:] + r.stderr
    fig = parse(r.stdout)
    assert fig["mismatches"] == 1, r.stdout[-4000:]
    assert "index %s " % hex(index) in r.stdout, r.stdout[-4000:]
