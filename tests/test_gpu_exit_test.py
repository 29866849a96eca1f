"""The per-wave choice between the exact exit test and the end-state test of
the direct-mode group loop (geo_pixel.h, kTestLow / kTestEnd) on the GPU:
the corner scenes of tests/test_exit_test_host.py as small frames against the
oracle, byte for byte (RGBA, mask, per-pixel steps, steps_total), as one-frame
renders and as 8-frame batched launches, with and without GEO_FLAG_RING_F64.
64 x 36 and 33 x 17 (partial tiles and partial waves)."""
import math

import numpy as np
import pytest

import oracle as O
from helpers import default_frame

pytestmark = pytest.mark.gpu

# (position, camera, fov, sphere_r, step, budgets): observer inside the sphere
STEP = math.pi / 100
SCENES = {
    # every lane falling (the benchmark's pose): the end-state loop on every wave
    "toward": ((2.5, 0.0, 0.1), (math.pi, 0.0), math.pi / 2, 50.0, STEP, (2048, 7)),
    # looking away through a wide view: near-radial outgoing lanes in the
    # middle (|UB0| far above the lane bound: the exact loop), lanes inside the
    # bound towards the left and right edges: both loops in one launch
    "away_wide": ((2.5, 0.0, 0.1), (0.0, 0.0), 2.4, 50.0, STEP, (2048, 9)),
    # near-radial outgoing rays only (rotation down to the radial cut-off)
    "away_narrow": ((2.5, 0.0, 0.0), (1e-4, 1e-4), 1e-3, 50.0, STEP, (2048, 5)),
    # sideways: falling and outgoing lanes, tangential rays
    "sideways": ((2.5, 0.0, 0.1), (math.pi / 2, 0.2), 2.0, 50.0, STEP, (2048, 3)),
    # the observer just inside the sphere: the grazing exit, stops in the first groups
    "just_inside": ((49.999, 0.0, 0.0), (math.pi / 2, 0.0), 2.0, 50.0, STEP, (2048, 1, 4, 8)),
    "small_sphere": ((2.05, 0.0, 0.3), (math.pi / 2, -0.3), 2.2, 2.1, STEP, (300, 4)),
    # the step at the selector's bound, just above it, and the regression seed's
    "step_at_bound": ((2.5, 0.0, 0.1), (0.4, 0.1), 2.4, 50.0, 0.0458, (2048, 8)),
    "step_above": ((2.5, 0.0, 0.1), (0.4, 0.1), 2.4, 50.0, 0.0459, (2048,)),
    "step_large": ((1.3, 0.0, 0.1), (0.2, 0.0), 2.0, 50.0, 0.093, (300,)),
}


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def geo():
    import schwarzschild_raytracer_wgpu_amd as g

    return g


@pytest.fixture(scope="module")
def sky():
    from schwarzschild_raytracer_wgpu_amd.scenes import make_sky

    return make_sky("equirect", (256, 128))


def _scene(geo, rs, sphere_r, r, step, max_steps, ring):
    flags = geo._lib.GEO_FLAG_RING_F64 if ring else 0
    return geo.make_scene(rs, sphere_r, r, step, max_steps, geo.GEO_MODE_DIRECT, flags=flags)


def _render(torch, ctx, frame, scene, w, h):
    dev = torch.device("cuda:0")
    rgba = torch.empty(h * w * 4, dtype=torch.uint8, device=dev)
    mask = torch.empty(h * w, dtype=torch.uint8, device=dev)
    steps = torch.empty(h * w, dtype=torch.int32, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.render_rows(frame, scene, w, h, 0, h, rgba, mask, None, steps, tot)
    torch.cuda.synchronize()
    return dict(rgba=rgba.cpu().numpy().reshape(h, w, 4), mask=mask.cpu().numpy().reshape(h, w),
                steps=steps.cpu().numpy().view(np.uint32).reshape(h, w), total=int(tot.item()))


@pytest.mark.parametrize("w,h", [(64, 36), (33, 17)])
@pytest.mark.parametrize("rs", [1.0, 0.0], ids=["rs1", "rs0"])
def test_corner_scenes_against_the_oracle(geo, torch_mod, sky, rs, w, h):
    ctx = geo.Context(0)
    ctx.set_sky(sky)
    stops = 0
    for name, (pos, cam, fov, sphere_r, step, budgets) in SCENES.items():
        frame = default_frame(w, h, pos=pos, camera=cam, rs=rs, fov=fov)
        r = math.sqrt(sum(x * x for x in pos))
        for ms in budgets:
            for ring in (False, True):
                scene = _scene(geo, rs, sphere_r, r, step, ms, ring)
                hip = _render(torch_mod, ctx, frame, scene, w, h)
                ref = O.render_f32(frame, scene, sky, w, h, threads=8)
                for f in ("mask", "steps", "rgba"):
                    assert np.array_equal(hip[f], ref[f]), (name, ms, ring, f, int((hip[f] != ref[f]).sum()))
                assert hip["total"] == ref["steps_total"], (name, ms, ring)
                stops += int((ref["steps"] < ms).sum())
    assert stops > 0
    ctx.close()


@pytest.mark.parametrize("w,h", [(64, 36), (33, 17)])
@pytest.mark.parametrize("rs", [1.0, 0.0], ids=["rs1", "rs0"])
def test_batched_launches_against_the_oracle(geo, torch_mod, sky, rs, w, h):
    """8 frames per launch, the camera turning from the black hole to away
    from it through the batch: frames of every mix of the two loops."""
    torch = torch_mod
    dev = torch.device("cuda:0")
    ctx = geo.Context(0)
    ctx.set_sky(sky)
    n = geo._lib.GEO_MAX_BATCH_FRAMES
    pos = (2.5, 0.0, 0.1)
    r = math.sqrt(sum(x * x for x in pos))
    frames = [default_frame(w, h, pos=pos, camera=(math.pi * (1.0 - i / (n - 1)), 0.1 * (i % 3) - 0.1), rs=rs, fov=2.2)
              for i in range(n)]
    band_rows = 8
    nbands = (h + band_rows - 1) // band_rows
    packed = nbands * band_rows * w * 4
    for step, ms in ((STEP, 2048), (STEP, 9), (0.0458, 300)):
        for ring in (False, True):
            scene = _scene(geo, rs, 50.0, r, step, ms, ring)
            out = torch.zeros(n * packed, dtype=torch.uint8, device=dev)
            tot = torch.zeros(1, dtype=torch.int64, device=dev)
            ctx.render_band_set_frames(frames, scene, w, h, band_rows, 0, band_rows, nbands, out, steps_total=tot)
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(n, nbands * band_rows, w, 4)
            total = 0
            for f in range(n):
                ref = O.render_f32(frames[f], scene, sky, w, h, threads=8)
                assert np.array_equal(got[f, :h], ref["rgba"]), (step, ms, ring, f)
                total += ref["steps_total"]
            assert int(tot.item()) == total, (step, ms, ring)
    ctx.close()
