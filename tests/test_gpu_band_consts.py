"""The f64 band's constants and step on the device against the host build of
geo_band.h, by bytes (tests/native/band_consts_device.hip, built here with
hipcc for gfx950): geo::band_consts_into as a batched GEO_FLAG_RING_F64
launch runs it (one lane per case, into zero-filled global memory) and
geo::band_kx over 8192 frames and scenes with the edges of every branch,
geo::min64_ (inline-asm v_min_f64) against fmin over 72 x 72 pairs with zeros,
denormals, infinities and NaNs, and geo::band_rk4 on 2^16 states.  Until now
these were compared only through rendered frame bytes."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_band_consts_min64_and_rk4_device_equals_host(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "band_consts_device")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero",
                    os.path.join(HERE, "native", "band_consts_device.hip"), "-o", exe], check=True)
    # three launches of at most 2^16 lanes and their host twins: well under a second
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches 0" in r.stdout, r.stdout + r.stderr
    for line in ("band_consts_into, band_kx: 8192 cases", "min64_: 5184 pairs", "band_rk4: 65536 states"):
        assert line in r.stdout, r.stdout
