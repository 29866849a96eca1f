"""The three CPU disk entry points (geo_render_cpu_disk, _disk_shift,
_disk_emission; csrc/geo_disk.h) on seeded random disk scenes
(tests/fuzz_disk_scenes.py): budgets off the group grid, steps up to 3, edge-on
disks.  The disk must not move the geodesic (mask, uv, steps and the total are
the plain render's), a pixel without a hit keeps the plain colour, the three
entry points find the same hits, and g and q are 0 exactly where a slot is no
hit.  tests/test_disk_probe_host.py ties the probes themselves to a per-step
definition; tests/test_gpu_disk_fuzz.py ties the kernels to this path on the
same seeds.

The seeds must reach what the named poses of the other disk tests do not.
Measured over SEEDS at 64 x 36 (floors asserted, no higher than half):

    seeds with a slot-0 / slot-1 / slot-2 hit            154 / 86 / 38    (75 / 40 / 19)
    seeds with a hit on a budget-exhausted pixel
      (steps == max_steps, max_steps % 4 != 0)           27               (13)
    seeds with a hit probed in the budget's tail
      (its node >= (max_steps / 4) * 4)                  23               (11)
    seeds with step > pi/4 and two hit slots on a pixel  6                (3)
    seeds with a hit probed second or third in its group
      of four steps                                      14               (7)
    edge-on seeds (N_z == 0 exactly) with a hit          32               (15)
    seeds with max_steps % 4 != 0                        159              (75)
    seeds of kind kCurvedOut / kCurvedIn / kFlat         177 / 63 / 60    (85 / 30 / 30)

The last two paths are rare among random seeds, so fuzz_disk_scenes also names
seeds picked for them (TAIL_SEEDS, GROUP_SEEDS); test_path_seeds holds each to
the path it was picked for.
"""
import math

import numpy as np
import pytest

import test_disk_cpu as T
import test_disk_probe_host as P
import test_disk_emission_cpu as XE
import test_disk_shift_cpu as XS
from fuzz_disk_scenes import GROUP_SEEDS, REGRESSION_SEEDS, TAIL_SEEDS, disk_scene, kind_of
from schwarzschild_raytracer_wgpu_amd._lib import GEO_OK

W, H = 64, 36
SEEDS = range(300)
G_MAX = 16.0  # GEO_DISK_G_MAX
FLOORS = {"slot0": 75, "slot1": 40, "slot2": 19, "tail_hit": 13, "tail_probe_hit": 11, "two_slots_big_step": 3,
          "grouped_probe_hit": 7, "edge_on_hit": 15, "off_grid": 75, "curved_out": 85, "curved_in": 30, "flat": 30}


@pytest.fixture(scope="module")
def cpu():
    return XE.load_cpu()


@pytest.fixture(scope="module")
def probe():
    return P.load()


def renders(cpu, seed, w=W, h=H):
    """The plain frame and the three disk frames of a seed."""
    frame, scene, disk_args, shift, (em, ramp), desc = disk_scene(seed, w, h)
    disk = T.make_disk(*disk_args)
    rc, p = T.render(cpu, frame, T.plain_of(scene), T.SKY, w, h)
    assert rc == GEO_OK, desc
    rc, d = T.render(cpu, frame, scene, T.SKY, w, h, disk, T.TEX)
    assert rc == GEO_OK, desc
    rc, s = XS.render(cpu, frame, scene, w, h, disk, shift=shift)
    assert rc == GEO_OK, desc
    rc, e = XE.render(cpu, frame, scene, w, h, disk, em=em, ramp=ramp)
    assert rc == GEO_OK, desc
    return frame, scene, disk_args, desc, p, d, s, e


def first(bad):
    """(x, y[, slot]) of the first set element of a (h, w[, 3]) mask."""
    i = np.argwhere(bad)[0]
    return (int(i[1]), int(i[0])) + tuple(int(v) for v in i[2:])


def check_seed(cpu, probe, seed, count):
    frame, scene, disk_args, desc, p, d, s, e = renders(cpu, seed)
    hit = d["hits"][..., 0] != 0.0  # (h, w, 3): the slot's r
    for name, a in (("disk", d), ("shift", s), ("emission", e)):
        # the disk does not move the geodesic
        for f in ("mask", "steps"):
            assert np.array_equal(a[f], p[f]), (desc, name, f, first(a[f] != p[f]))
        assert np.array_equal(a["uv"].view(np.uint32), p["uv"].view(np.uint32)), (desc, name, "uv")
        assert a["total"] == p["total"], (desc, name, "steps_total")
        # the same hits from every entry point; no hit, no colour
        same_hits = a["hits"].view(np.uint32) == d["hits"].view(np.uint32)
        assert same_hits.all(), (desc, name, "hits", first(~same_hits.all(axis=-1)))
        untouched = (a["rgba"] == p["rgba"]).all(axis=-1) | hit.any(axis=-1)
        assert untouched.all(), (desc, name, "colour without a hit", first(~untouched))
        assert ((a["hits"][..., 1] == 0.0) | hit).all(), (desc, name, "Ud without a hit")
    for name, a, fields in (("shift", s, ("g",)), ("emission", e, ("g", "q"))):
        for f in fields:
            v = a[f]
            assert (v.view(np.uint32)[~hit] == 0).all(), (desc, name, f, "nonzero without a hit", first((v != 0) & ~hit))
            ok = (v[hit] >= 0.0) & (v[hit] <= G_MAX)
            assert ok.all(), (desc, name, f, v[hit][~ok][:4])
    ms = scene.max_steps
    exhausted = d["steps"] == ms
    for c in range(3):
        count[f"slot{c}"] += bool(hit[..., c].any())
    count["tail_hit"] += bool(ms % 4 != 0 and (exhausted & hit.any(axis=-1)).any())
    tail, grouped = P.hit_paths(P.frame_nodes(probe, frame, scene, disk_args, W, H), hit, ms)
    count["tail_probe_hit"] += bool(tail)
    count["grouped_probe_hit"] += bool(grouped)
    count["two_slots_big_step"] += bool(scene.step > math.pi / 4 and (hit.sum(axis=-1) >= 2).any())
    m2 = frame.central_to_uv
    n = disk_args[2]
    n_z = sum(float(m2[8 + i]) * n[i] for i in range(3))  # N_z = column 2 of central_to_uv . n
    count["edge_on_hit"] += bool("normal=edge_on" in desc and np.float32(n_z) == 0.0 and hit.any())
    count["off_grid"] += ms % 4 != 0
    count[("curved_out", "curved_in", "flat")[kind_of(scene.rs, scene.r_obs, scene.step)]] += 1


def test_disk_entry_points_on_seeded_scenes(cpu, probe):
    count = dict.fromkeys(FLOORS, 0)
    for seed in tuple(SEEDS) + REGRESSION_SEEDS:
        check_seed(cpu, probe, seed, count)
    print("disk fuzz reach:", count)
    for name, floor in FLOORS.items():
        assert count[name] >= floor, (name, count[name], floor)


def test_path_seeds(cpu, probe):
    """fuzz_disk_scenes.TAIL_SEEDS and GROUP_SEEDS pass the same checks, and
    every one of them still holds the path it was picked for."""
    for seeds, name in ((TAIL_SEEDS, "tail_probe_hit"), (GROUP_SEEDS, "grouped_probe_hit")):
        for seed in seeds:
            count = dict.fromkeys(FLOORS, 0)
            check_seed(cpu, probe, seed, count)
            assert count[name] == 1, (seed, name)


def test_rendered_pixels_follow_the_per_step_definition(cpu, probe):
    """The per-step definition of tests/native/disk_probe_host.cpp from a
    rendered frame's own pixels (the camera and the aberration included): the
    render's step count is the definition's, and a slot is a hit only if its
    crossing's node lies below it."""
    w, h = 16, 9
    checked = 0
    for seed in range(40):
        frame, scene, disk_args, desc, p, d, s, e = renders(cpu, seed, w, h)
        for y in range(h):
            for x in range(w):
                px = P.pixel(probe, frame, scene, disk_args, w, h, x, y)
                assert px["steps"] == d["steps"][y, x], (desc, x, y, px, d["steps"][y, x])
                for c in range(3):
                    if d["hits"][y, x, c, 0] != 0.0:
                        assert int(px["jn"][c], 16) < px["steps"], (desc, x, y, c, px)
                        checked += 1
    print("hit slots checked against the definition:", checked)
    assert checked >= 100, checked


def test_every_seed_is_a_legal_disk_scene():
    """GEO_FLAG_DISK's rules (geo.h) hold for every seed, with the f32 values the
    entry points see, and an exactly edge-on seed has N_z == 0."""
    f32 = np.float32
    for seed in range(2000):
        frame, scene, (r_in, r_out, normal, axis), shift, (em, ramp), desc = disk_scene(seed, W, H)
        rs, sphere_r, r_obs = f32(scene.rs), f32(scene.sphere_r), f32(scene.r_obs)
        assert scene.mode == 0 and scene.step > 0 and 1 <= scene.max_steps <= 4096, desc
        assert 0.01 <= scene.step <= 3.0001, desc
        assert rs < f32(r_in) < f32(r_out) < sphere_r, desc
        assert rs == 0 or (rs < r_obs and f32(r_in) > f32(1.5) * rs), desc
        assert r_obs < sphere_r, desc
        assert abs(np.dot(normal, axis)) < 0.9 * np.linalg.norm(normal), desc
        assert shift[0] in (1, -1) and 0 <= shift[1] <= 4 and 0.5 <= shift[2] <= 4.0, desc
        assert em[0] in (1, -1) and em[1] in (0, 1) and 0 < em[3] < em[4] and 2 <= len(ramp) <= 1024, desc
        if "normal=edge_on" in desc:
            m2 = frame.central_to_uv
            assert f32(sum(float(m2[8 + i]) * normal[i] for i in range(3))) == 0.0, desc
