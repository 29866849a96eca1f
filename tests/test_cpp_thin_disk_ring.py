"""sr::ThinDisk::set_ring_f64 (include/geo/sr.hpp) through a native program
(tests/native/sr_thin_disk_ring.cpp): it compiles warning-free, and on the GPU
its three frames (the plain disk, set_ring_f64, set_ring_f64(false)) are the
CPU path's."""
import math
import os
import subprocess

import pytest

import test_cpp_host as C
import test_cpp_thin_disk_shift as CS
import test_disk_ring_cpu as X
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK, GEO_OK

SRC = os.path.join(C.HERE, "native", "sr_thin_disk_ring.cpp")
W, H = 96, 54
THETA = X.T.POSES["ring"][1][1]  # the camera's elevation, handed to the program as text that parses back exactly


def test_builds(tmp_path):
    C.build(tmp_path, SRC)


def cpu_frames():
    """FNV-1a of the CPU path's frame of the program's scene, the state off and on."""
    import schwarzschild_raytracer_wgpu_amd as g

    obs = g.Observer(1.0, 0.004, W, H)
    obs.set_position(14.0, 0.0, 5.1)
    obs.set_camera(math.pi, float(repr(THETA)))
    obs.start_unmoving()
    frame = obs.calc_transformation_pipeline()
    scene = g.make_scene(1.0, 50.0, obs.get_radial_position(), math.pi / 100, 2048, flags=GEO_FLAG_DISK)
    cpu = X.load_cpu()
    want = {}
    for name, ring in (("disk", 0), ("disk+ring", 1)):
        rc, a = X.render(cpu, frame, scene, X.T.make_disk(3.0, 9.0), ring, tex=CS.pattern(64, 16),
                         sky=CS.pattern(512, 256))
        assert rc == GEO_OK
        want[name] = C.fnv1a(a["rgba"].tobytes())
    return want


def test_the_scene_has_band_hits():
    """The program's scene draws disk hits inside the band: its two frames differ."""
    want = cpu_frames()
    assert want["disk"] != want["disk+ring"]


@pytest.mark.gpu
def test_frames_equal_the_cpu_path(tmp_path):
    if not C._has_gpu():
        pytest.skip("no HIP device")
    exe = C.build(tmp_path, SRC)
    r = subprocess.run([exe, str(W), str(H), repr(THETA)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {l.split(" fnv1a ")[0]: int(l.split(" fnv1a ")[1], 16) for l in r.stdout.splitlines() if "fnv1a" in l}
    want = cpu_frames()
    assert got["disk"] == want["disk"] and got["disk+ring"] == want["disk+ring"]
    assert got["disk off"] == want["disk"] and want["disk"] != want["disk+ring"]
