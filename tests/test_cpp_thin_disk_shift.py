"""sr::ThinDisk's shading setter (include/geo/sr.hpp) through a native program
(tests/native/sr_thin_disk_shift.cpp): it compiles warning-free, and on the
GPU its three frames (unshaded, set_shift, clear_shift) are the CPU path's."""
import math
import os
import subprocess

import numpy as np
import pytest

import test_cpp_host as C
import test_disk_shift_cpu as X
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK, GEO_OK

SRC = os.path.join(C.HERE, "native", "sr_thin_disk_shift.cpp")
SHIFT = (-1, 3, 0.75)


def test_builds(tmp_path):
    C.build(tmp_path, SRC)


def pattern(w, h):
    x = np.arange(w, dtype=np.uint32)[None, :]
    y = np.arange(h, dtype=np.uint32)[:, None]
    t = np.empty((h, w, 4), np.uint8)
    t[..., 0] = ((x * 7) ^ (y * 13)) & 0xFF
    t[..., 1] = (x + y) & 0xFF
    t[..., 2] = (x * y) & 0xFF
    t[..., 3] = 255
    return t


@pytest.mark.gpu
def test_frames_equal_the_cpu_path(tmp_path):
    if not C._has_gpu():
        pytest.skip("no HIP device")
    import schwarzschild_raytracer_wgpu_amd as g

    W, H = 96, 54
    exe = C.build(tmp_path, SRC)
    r = subprocess.run([exe, str(W), str(H)] + [str(v) for v in SHIFT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {l.split(" fnv1a ")[0]: int(l.split(" fnv1a ")[1], 16) for l in r.stdout.splitlines() if "fnv1a" in l}
    obs = g.Observer(1.0, math.pi / 2, W, H)
    obs.set_position(2.4, 0.0, 0.7)
    frame = obs.calc_transformation_pipeline()
    scene = g.make_scene(1.0, 50.0, obs.get_radial_position(), math.pi / 100, 2048, flags=GEO_FLAG_DISK)
    cpu = X.load_cpu()
    disk = X.T.make_disk(1.6, 2.2)
    want = {}
    for name, shift in (("disk", None), ("disk+shift", SHIFT)):
        rc, a = X.render(cpu, frame, scene, W, H, disk, pattern(64, 16), shift=shift, sky=pattern(512, 256))
        assert rc == GEO_OK
        want[name] = C.fnv1a(a["rgba"].tobytes())
    assert got["disk"] == want["disk"] and got["disk+shift"] == want["disk+shift"]
    assert got["disk cleared"] == want["disk"] and want["disk"] != want["disk+shift"]
