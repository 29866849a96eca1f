"""Seeded random thin-disk scenes for the disk fuzz parity tests
(tests/test_host_disk_fuzz.py on the CPU, tests/test_gpu_disk_fuzz.py on the
GPU), beside fuzz_scenes.py: observers far out, between the photon sphere and
the disk, inside the photon sphere, in flat space and under a small sky sphere;
random, exactly edge-on, nearly edge-on and face-on disks; budgets on and off
the group grid of 4 steps; steps from 0.01 to 3 (up to three disk crossings
between two nodes); and a shading and an emission state per seed.  Every scene
is within GEO_FLAG_DISK's rules (geo.h) for all three entry points: direct
mode, rs < r_in < r_out < sphere_r, rs < r_obs < sphere_r (or rs = 0) and
r_in > 1.5 rs."""
import math

import numpy as np

from schwarzschild_raytracer_wgpu_amd import Observer, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK, GEO_MODE_DIRECT
from schwarzschild_raytracer_wgpu_amd.scenes import blackbody_ramp

# seeds that once differed between two paths, with one line on what it was (none so far)
REGRESSION_SEEDS = ()

# seeds found by running the generator at 64 x 36 whose frames hold disk hits probed in the
# budget's tail (TAIL_SEEDS) and hits probed as the second or third probe of one group of
# four steps (GROUP_SEEDS); tests/test_host_disk_fuzz.py asserts that they still do, and
# the GPU tests run them on top of their seed ranges
TAIL_SEEDS = (300, 302, 322, 323, 324, 344, 350, 370, 382, 391, 403, 410)
GROUP_SEEDS = (309, 334, 342, 420, 424, 430, 444, 479, 491, 505, 679, 690)

OBSERVERS = ("far", "near_disk", "inside_photon_sphere", "flat", "small_sphere")
NORMALS = ("random", "edge_on", "near_edge_on", "face_on")
# budgets off and on the grid of kGroup = 4 steps; half of the seeds get one of each
OFF_GRID = (1, 3, 5, 7, 9, 17, 47, 99, 102, 301, 2047)
ON_GRID = (2048, 4096)
RAMP_SIZES = (2, 7, 64, 1024)

_RAMPS = {}


def ramp_of(n):
    """The colour ramp of n entries (rendered once per size, never modified)."""
    if n not in _RAMPS:
        r = blackbody_ramp(n, 1500.0, 24000.0)
        r.setflags(write=False)
        _RAMPS[n] = r
    return _RAMPS[n]


def kind_of(rs, r_obs, step):
    """The integration kind make_consts (geo_pixel.h) picks: 0 kCurvedOut (rs > 0,
    the observer outside the horizon, step in [2^-10, 1/2]), 1 kCurvedIn (rs > 0
    otherwise), 2 kFlat (rs = 0).  step as the scene's f32."""
    if rs == 0.0:
        return 2
    step = float(np.float32(step))
    return 0 if r_obs > rs and 2.0 ** -10 <= step <= 0.5 else 1


def disk_scene(seed: int, w: int, h: int, index: int = 0):
    """(frame, scene, disk_args, shift_args, emission_args, description) for seed:
    disk_args = (r_in, r_out, normal, axis), shift_args = (spin, exponent, gain),
    emission_args = ((spin, profile, t_ref, t_lo, t_hi, exposure), ramp).
    index: frame `index` of the seed's batch (disk_batch); 0 is the seed's scene."""
    rng = np.random.default_rng(seed)
    observer = OBSERVERS[seed % len(OBSERVERS)]
    normal_kind = NORMALS[(seed // len(OBSERVERS)) % len(NORMALS)]
    rs, sphere_r = 1.0, 50.0
    if observer == "far":
        r_in = rng.uniform(1.55, 4.0)
        r_out = r_in * rng.uniform(1.5, 5.0)
        r = rng.uniform(6.0, 40.0)
    elif observer == "near_disk":
        r_in = rng.uniform(2.0, 4.0)
        r_out = r_in * rng.uniform(1.5, 5.0)
        r = rng.uniform(1.52, r_in)
    elif observer == "inside_photon_sphere":
        r_in = rng.uniform(1.55, 3.0)
        r_out = r_in * rng.uniform(1.5, 5.0)
        r = rng.uniform(1.02, 1.48)
    elif observer == "flat":
        rs = 0.0
        r_in = rng.uniform(1.0, 4.0)
        r_out = r_in * rng.uniform(1.5, 6.0)
        r = rng.uniform(0.5, 40.0)
    else:  # small_sphere: the sky sphere a few rs out, the disk and the observer under it
        sphere_r = rng.uniform(3.5, 6.0)
        r_in = rng.uniform(1.55, 2.0)
        r_out = rng.uniform(1.2 * r_in, 0.9 * sphere_r)
        r = rng.uniform(1.05, 0.95 * sphere_r)
    r_in, r_out, r = float(r_in), float(r_out), float(r)
    # the observer's direction and the disk's normal (the sky texture's frame)
    if normal_kind in ("edge_on", "near_edge_on"):
        d = np.array([1.0, 0.0, 0.0])
        n = np.array([0.0, 0.0, 1.0]) if rng.random() < 0.5 else np.array([0.0, 1.0, 0.0])
        if normal_kind == "near_edge_on":
            n = n + float(10.0 ** rng.uniform(-4.0, -2.0)) * (1.0 if rng.random() < 0.5 else -1.0) * d
    else:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        if normal_kind == "face_on":
            n = d.copy()
        else:
            n = rng.normal(size=3)
            n /= np.linalg.norm(n)
    axis = np.zeros(3)
    axis[int(np.argmin(np.abs(n)))] = 1.0  # the coordinate axis farthest from the normal
    r *= 1.0 + 0.004 * index  # (a batch's observer drifts outwards: within every family's margin)
    pos = tuple(float(x) for x in r * d)
    fov = float(rng.uniform(0.3, 2.4))
    o = Observer(rs, fov, w, h)
    o.set_position(*pos)
    # mostly toward the centre (phi = pi, theta = 0 looks down the -x axis from
    # (r, 0, 0)): a frame without the disk in it tests nothing
    toward = rng.random() < 0.85
    if toward:
        phi = math.atan2(pos[1], pos[0]) + math.pi + float(rng.normal(0.0, 0.2 * fov))
        theta = -math.asin(max(-1.0, min(1.0, pos[2] / r))) + float(rng.normal(0.0, 0.15 * fov))
        theta = max(-1.4, min(1.4, theta))
    else:
        phi, theta = float(rng.uniform(0.0, 2.0 * math.pi)), float(rng.uniform(-1.3, 1.3))
    o.set_camera(phi + 0.05 * fov * index, max(-1.45, min(1.45, theta - 0.03 * fov * index)))
    o.set_energy(float(rng.uniform(1.0, 1.6)))
    unmoving = rng.random() < 0.4
    if unmoving:
        o.start_unmoving()
    else:
        o.start_frozen_fall()
    frame = o.calc_transformation_pipeline()
    step = math.pi / 100 if rng.random() < 0.4 else float(10.0 ** rng.uniform(-2.0, math.log10(3.0)))
    if rng.random() < 0.5:
        # off the grid; mostly a budget that ends where rays cross the disk plane (the first
        # crossing lies at a traveled angle in (0, pi]), so that the budget's tail holds probes
        near = [b for b in OFF_GRID if 0.3 <= b * step <= 3.3]
        max_steps = int(rng.choice(near) if near and rng.random() < 0.7 else rng.choice(OFF_GRID))
    else:
        max_steps = int(rng.choice(ON_GRID))
    scene = make_scene(rs, sphere_r, o.get_radial_position(), step, max_steps, GEO_MODE_DIRECT, GEO_FLAG_DISK)
    disk_args = (r_in, r_out, tuple(float(x) for x in n), tuple(float(x) for x in axis))
    shift_args = (1 if rng.random() < 0.5 else -1, int(rng.integers(0, 5)), float(rng.uniform(0.5, 4.0)))
    n_ramp = int(rng.choice(RAMP_SIZES))
    em = (1 if rng.random() < 0.5 else -1, int(rng.integers(0, 2)), float(rng.uniform(3000.0, 9000.0)),
          float(rng.uniform(1000.0, 2000.0)), float(rng.uniform(12000.0, 30000.0)),
          float(10.0 ** rng.uniform(-0.3, 1.6)))
    desc = (f"disk seed={seed}{f' frame={index}' if index else ''} observer={observer} normal={normal_kind} "
            f"r={r:.4f} sphere_r={sphere_r:.3f} rs={rs} disk={r_in:.3f}..{r_out:.3f} "
            f"n=({n[0]:.5f},{n[1]:.5f},{n[2]:.5f}) fov={fov:.3f} toward={toward} unmoving={unmoving} "
            f"steps={max_steps} step={step:.4f} shift={shift_args[0]:+d},{shift_args[1]},{shift_args[2]:.2f} "
            f"emission=spin{em[0]:+d},profile{em[1]},ramp{n_ramp}")
    return frame, scene, disk_args, shift_args, (em, ramp_of(n_ramp)), desc


def disk_batch(seed: int, w: int, h: int, n: int):
    """(frames, scenes, disk_args, shift_args, description): n frames of the
    seed's scene for one batched launch, the camera turning and the observer
    drifting outwards by 0.4 % a frame; the scenes differ in r_obs only and
    share the integration kind, as the batched entry points require."""
    out = [disk_scene(seed, w, h, i) for i in range(n)]
    scenes = [o[1] for o in out]
    assert len({kind_of(s.rs, s.r_obs, s.step) for s in scenes}) == 1
    return [o[0] for o in out], scenes, out[0][2], out[0][3], out[0][5] + f" batch={n}"
