"""sr::ThinDisk's emission setter (include/geo/sr.hpp) through a native program
(tests/native/sr_thin_disk_emission.cpp): it compiles warning-free, and on the
GPU its three frames (unshaded, set_emission, clear_emission) are the CPU
path's."""
import math
import os
import subprocess

import numpy as np
import pytest

import test_cpp_host as C
import test_cpp_thin_disk_shift as CS
import test_disk_emission_cpu as X
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK, GEO_OK

SRC = os.path.join(C.HERE, "native", "sr_thin_disk_emission.cpp")
EMISSION = (-1, X.THIN, 7000.0, 1500.0, 30000.0, 1.5)  # spin, profile, t_ref, t_lo, t_hi, exposure
N = 33


def test_builds(tmp_path):
    C.build(tmp_path, SRC)


def ramp_of(n):
    i = np.arange(n, dtype=np.uint32)
    r = np.empty((n, 4), np.uint8)
    r[:, 0] = 255 - 255 * i // (n - 1)
    r[:, 1] = (i * 37) & 0xFF
    r[:, 2] = 255 * i // (n - 1)
    r[:, 3] = 255
    return r


@pytest.mark.gpu
def test_frames_equal_the_cpu_path(tmp_path):
    if not C._has_gpu():
        pytest.skip("no HIP device")
    import schwarzschild_raytracer_wgpu_amd as g

    W, H = 96, 54
    exe = C.build(tmp_path, SRC)
    r = subprocess.run([exe, str(W), str(H)] + [str(v) for v in EMISSION] + [str(N)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {l.split(" fnv1a ")[0]: int(l.split(" fnv1a ")[1], 16) for l in r.stdout.splitlines() if "fnv1a" in l}
    obs = g.Observer(1.0, math.pi / 2, W, H)
    obs.set_position(2.4, 0.0, 0.7)
    frame = obs.calc_transformation_pipeline()
    scene = g.make_scene(1.0, 50.0, obs.get_radial_position(), math.pi / 100, 2048, flags=GEO_FLAG_DISK)
    cpu = X.load_cpu()
    disk = X.T.make_disk(1.6, 2.2)
    want = {}
    for name, em in (("disk", None), ("disk+emission", EMISSION)):
        rc, a = X.render(cpu, frame, scene, W, H, disk, CS.pattern(64, 16), em=em, ramp=ramp_of(N),
                         sky=CS.pattern(512, 256))
        assert rc == GEO_OK
        want[name] = C.fnv1a(a["rgba"].tobytes())
    assert got["disk"] == want["disk"] and got["disk+emission"] == want["disk+emission"]
    assert got["disk cleared"] == want["disk"] and want["disk"] != want["disk+emission"]
