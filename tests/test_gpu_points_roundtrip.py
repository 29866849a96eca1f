"""Round trip on the device: the HIP point path (geo_rays_* / geo_points_* /
geo_draw_points) against places whose pixel is known.

* Reference -> HIP: the points of tests/points_roundtrip_ref.py (the f64
  render's sky points, disk_ref.trace's plane crossings) through
  RayConnectors.reset_ray and draw_points, and once through PointCloud.draw:
  every near point and every far point far_is_physical keeps lands on the pixel
  it came from.  tests/test_points_roundtrip_cpu.py does the same on the
  oracle's mirror over every pose, and holds the measured figures.
* HIP -> HIP: the render kernels' own answers -- the disk hits (r, U) of a
  GEO_FLAG_DISK render, the sky UV of a plain one -- turned into points and
  sent through the HIP point path land on the pixel whose answer they were;
  no mirror in between.
* Angle: reset_ray's near-side incoming angle against f64 shooting, within
  the reference's 5e-4 rad.

The point counts fall out ragged (never a multiple of the 64-connector tile).
profiles/points_roundtrip.json holds one device run's figures."""
import math

import numpy as np
import pytest

import disk_ref as D
import points_roundtrip_ref as R

pytestmark = pytest.mark.gpu

MIN_NEAR, MIN_FAR_PHYSICAL = 1000, 100
# one pose per observer state, one of them at narrow fov
HIP_POSES = ("r25_rest_fine", "r9_fall", "orbit")
DISK_POSE, SKY_POSE, CLOUD_POSE = "r3_fall", "r1p2_rest", "r9_fall"


@pytest.fixture(scope="module")
def geo():
    import schwarzschild_raytracer_wgpu_amd as g

    return g


@pytest.fixture(scope="module")
def ctx(geo, dev):
    c = geo.Context(dev.index or 0)
    yield c
    c.close()


def project(geo, ctx, dev, frame, verts, n):
    """geo_draw_points of n device vertices over a blank frame: xy (n, 2)."""
    import torch

    tgt = geo.RenderTarget(R.W, R.H, torch.zeros(R.W * R.H * 4, dtype=torch.uint8, device=dev))
    xy = torch.full((n, 2), -7, dtype=torch.int32, device=dev)
    geo.draw_points(ctx, frame, verts, n, tgt, out_xy=xy)
    torch.cuda.synchronize()
    return xy.cpu().numpy()


def hip_xy(geo, ctx, dev, frame, obs, P):
    """Near + far connectors of the points P, reset at obs and projected:
    (xy (2n, 2), vertices (2n, 4)), near side first."""
    rays = geo.RayConnectors(ctx, R.RS, P, sides=geo.GEO_RAYS_NEAR | geo.GEO_RAYS_FAR)
    verts = rays.reset_ray(obs)
    xy = project(geo, ctx, dev, frame, verts, rays.count)
    return xy, verts.cpu().numpy()


def landing(name, xy, idx, pix, n_near, n_far):
    """The landing assertions on the connectors idx (near ones first)."""
    d = np.abs(xy[idx] - pix).max(axis=1)
    n_phys = idx.size - n_near
    stats = dict(near=n_near, near_exact=int((d[:n_near] == 0).sum()), far=n_far, far_physical=n_phys,
                 far_exact=int((d[n_near:] == 0).sum()))
    print(name, stats)
    assert n_near >= MIN_NEAR, (name, n_near)
    if n_far:
        assert n_phys >= MIN_FAR_PHYSICAL, (name, n_far, n_phys)
    bad = np.flatnonzero(d[:n_near] > 0)
    assert bad.size == 0, f"{name}: {bad.size} of {n_near} near points off their pixel, first {pix[bad[:3]]} -> " \
                          f"{xy[idx[bad[:3]]]}"
    bad = n_near + np.flatnonzero(d[n_near:] > 0)
    assert bad.size == 0, f"{name}: {bad.size} of {n_phys} physical far points off their pixel ({n_far - n_phys} " \
                          f"of {n_far} far points left out by far_is_physical), first {pix[bad[:3]]} -> " \
                          f"{xy[idx[bad[:3]]]}"
    return stats


def reference_to_hip(geo, ctx, dev, name):
    frame, _, obs = R.frame_of(name)
    pts = R.pose_points(name)
    assert pts["far"].size % 64 != 0
    xy, _ = hip_xy(geo, ctx, dev, frame, obs, pts["P"])
    idx, pix = R.connectors(pts)
    return landing(name, xy, idx, pix, int((~pts["far"]).sum()), int(pts["far"].sum()))


@pytest.mark.parametrize("name", HIP_POSES)
def test_reference_points_land_on_their_pixel(geo, ctx, dev, name):
    reference_to_hip(geo, ctx, dev, name)


def cloud_to_hip(geo, ctx, dev, name=CLOUD_POSE):
    """The same points as a PointCloud (no orbits): its constructor resets
    every connector at the observer, draw() projects near then far."""
    import torch

    frame, _, obs = R.frame_of(name)
    pts = R.pose_points(name)
    n = pts["far"].size
    pc = geo.PointCloud(ctx, pts["P"], R.RS, obs, True, False)
    tgt = geo.RenderTarget(R.W, R.H, torch.zeros(R.W * R.H * 4, dtype=torch.uint8, device=dev))
    xy = torch.full((2 * n, 2), -7, dtype=torch.int32, device=dev)
    pc.draw(frame, tgt, out_xy=xy)
    torch.cuda.synchronize()
    idx, pix = R.connectors(pts)
    stats = landing(name + " (PointCloud)", xy.cpu().numpy(), idx, pix, int((~pts["far"]).sum()),
                    int(pts["far"].sum()))
    # the overlay itself: every landed point's pixel is drawn
    rgba = tgt.rgba.cpu().numpy().reshape(R.H, R.W, 4)
    assert (rgba[pix[:, 1], pix[:, 0]] == np.array([255, 0, 0, 255], np.uint8)).all()
    return stats


def test_point_cloud_draw_lands_on_the_source_pixels(geo, ctx, dev):
    cloud_to_hip(geo, ctx, dev)


def _physical_by_pixel(pts, plane):
    """Per pixel (flat index): the reference has a far point of this kind there
    and far_is_physical keeps it."""
    ok = np.zeros(R.W * R.H, bool)
    m = (pts["plane"] == plane) & pts["far"] & pts["physical"]
    ok[pts["pix"][m, 1] * R.W + pts["pix"][m, 0]] = True
    return ok


def disk_hits_to_hip(geo, ctx, dev, name=DISK_POSE):
    """Points from the disk kernel's own hits: slot 0 near, slot 1 far."""
    import torch
    from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK
    from schwarzschild_raytracer_wgpu_amd.scenes import make_disk_texture, make_sky

    frame, scene, obs = R.frame_of(name)
    normal, axis = R.POSES[name][5], (1.0, 0.0, 0.0)
    ctx.set_sky(make_sky("equirect", (128, 64)))
    ctx.set_disk(make_disk_texture((64, 16)), R.R_IN, R.R_OUT, normal, axis)
    dscene = geo.make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps, flags=GEO_FLAG_DISK)
    rgba = torch.zeros(R.W * R.H * 4, dtype=torch.uint8, device=dev)
    hits = torch.full((R.W * R.H * 6,), -1.0, dtype=torch.float32, device=dev)
    ctx.disk_hits_next_render(hits)
    ctx.render_rows(frame, dscene, R.W, R.H, 0, R.H, rgba)
    torch.cuda.synchronize()
    ctx.clear_disk()
    hits = hits.cpu().numpy().reshape(-1, 3, 2).astype(np.float64)
    _, ex, ey = D.disk_basis(normal, axis)
    physical = _physical_by_pixel(R.pose_points(name), plane=True)
    pixels = R._pixels(R.W, R.H)
    P, pix, far, keep = [], [], [], []
    for k in (0, 1):
        hit = hits[:, k, 0] > 0.0
        r, az = hits[hit, k, 0], 2.0 * math.pi * hits[hit, k, 1]
        P.append(r[:, None] * (np.cos(az)[:, None] * ex + np.sin(az)[:, None] * ey))
        pix.append(pixels[hit])
        far.append(np.full(r.size, k == 1))
        keep.append(physical[hit] if k == 1 else np.ones(r.size, bool))
    P, pix, far, keep = (np.concatenate(a) for a in (P, pix, far, keep))
    xy, _ = hip_xy(geo, ctx, dev, frame, obs, P.astype(np.float32))
    n = far.size
    near_i, far_i = np.flatnonzero(~far), np.flatnonzero(far & keep)
    idx = np.concatenate([near_i, n + far_i])
    return landing(name + " (disk kernel's hits)", xy, idx, pix[np.concatenate([near_i, far_i])], near_i.size,
                   int(far.sum()))


def test_disk_kernel_hits_land_on_their_pixel(geo, ctx, dev):
    disk_hits_to_hip(geo, ctx, dev)


def sky_uv_to_hip(geo, ctx, dev, name=SKY_POSE):
    """Points from the sphere kernel's own out_mask / out_uv; each ray's class
    and the far side's filter come from the f64 reference's sweep for the
    pixel (a pixel where the reference sees no sky point is left out, counted)."""
    import torch
    from schwarzschild_raytracer_wgpu_amd.scenes import make_sky

    frame, scene, obs = R.frame_of(name)
    ctx.set_sky(make_sky("equirect", (128, 64)))
    rgba = torch.zeros(R.W * R.H * 4, dtype=torch.uint8, device=dev)
    mask = torch.zeros(R.W * R.H, dtype=torch.uint8, device=dev)
    uv = torch.zeros(R.W * R.H * 2, dtype=torch.float32, device=dev)
    ctx.render_rows(frame, scene, R.W, R.H, 0, R.H, rgba, mask, uv)
    torch.cuda.synchronize()
    sky = mask.cpu().numpy() == 0
    uv = uv.cpu().numpy().reshape(-1, 2).astype(np.float64)
    pts = R.pose_points(name)
    ref = ~pts["plane"]
    flat = pts["pix"][ref, 1] * R.W + pts["pix"][ref, 0]
    is_near, is_far = np.zeros(R.W * R.H, bool), np.zeros(R.W * R.H, bool)
    is_near[flat[~pts["far"][ref]]] = True
    is_far[flat[pts["far"][ref]]] = True
    physical = _physical_by_pixel(pts, plane=False)
    unmatched = int((sky & ~is_near & ~is_far).sum() + (~sky & (is_near | is_far)).sum())
    lon, lat = 2.0 * math.pi * uv[:, 0], math.pi * (0.5 - uv[:, 1])
    P = float(scene.sphere_r) * np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], -1)
    sel = np.flatnonzero(sky & (is_near | is_far))
    xy, _ = hip_xy(geo, ctx, dev, frame, obs, P[sel].astype(np.float32))
    n = sel.size
    near_i, far_i = np.flatnonzero(is_near[sel]), np.flatnonzero(is_far[sel] & physical[sel])
    idx = np.concatenate([near_i, n + far_i])
    pix = R._pixels(R.W, R.H)[sel]
    stats = landing(name + " (sphere kernel's UV)", xy, idx, pix[np.concatenate([near_i, far_i])], near_i.size,
                    int(is_far[sel].sum()))
    stats["unmatched_pixels"] = unmatched
    return stats


def test_sphere_kernel_uv_lands_on_its_pixel(geo, ctx, dev):
    sky_uv_to_hip(geo, ctx, dev)


def hip_angles(geo, ctx):
    """max |reset_ray's near-side angle - exact_angle| per observer radius."""
    import torch

    pos, obs = R.angle_cases()
    want, ok = R.angle_reference()
    assert ok.all(), f"shooting did not converge for {(~ok).sum()} points"
    worst = {}
    for i, r in enumerate(R.ANGLE_RADII):
        out = geo.RayConnectors(ctx, R.RS, pos[i]).reset_ray(obs[i])
        torch.cuda.synchronize()
        worst[r] = float(np.abs(out.cpu().numpy()[:, 3].astype(np.float64) - want[i]).max())
    print("max |angle error| per r_obs:", worst)
    return worst


def test_hip_angle_near_side(geo, ctx, dev):
    for r, e in hip_angles(geo, ctx).items():
        assert e < R.ANGLE_TOL, (r, e)
