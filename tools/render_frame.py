#!/usr/bin/env python3
"""Render the reference's scene (SR/lib.rs:62-94: sky sphere, planet sphere,
translucent cloud sphere, accretion disk) on the GPU and save it as PNG/PPM —
the present step of the absent wgpu_renderer loop.

  python tools/render_frame.py out.png [--width 1920 --height 1080]
        [--sky eso0932a.jpg --planet world_8k.png --clouds transparent_clouds.png]
        [--frames 60 --orbit 3.2] [--mipmaps] [--fan]
  python tools/render_frame.py out.jpg --disk 1.6 2.2 [--cpu] [--pos 2.4 0 0.7 --camera 3.1416 -0.28]
        [--disk-shift SPIN EXP GAIN] [--ss]
        [--disk-emission T_REF T_LO T_HI EXPOSURE [--disk-profile power|thin] [--disk-spin 1|-1]]
        [--disk-ring-f64] [--adaptive [--tol T] [--ss] [--disk-ring-f64]]

--disk R_IN R_OUT draws the ray-traced thin accretion disk (GEO_FLAG_DISK:
the sky sphere alone plus the textured disk with its secondary and third
images) instead of the reference's scene; --cpu renders it with the CPU path
(libgeo_cpu.so, the same bytes, no GPU needed).  --disk-shift SPIN EXP GAIN
shades the disk by its Doppler and redshift factor g (geo_set_disk_shift:
matter orbiting about SPIN * normal, colours times GAIN * g**EXP).  --ss
draws the disk frame 2 x 2 supersampled (GEO_FLAG_SS4: four rays per pixel,
resolved in the kernel), on the GPU or with --cpu.  --disk-emission T_REF T_LO
T_HI EXPOSURE colours the disk by its observed blackbody temperature
(geo_set_disk_emission: T = T_REF tau(r) with the --disk-profile, shifted by g
for matter orbiting about --disk-spin * normal, a 256-entry
scenes.blackbody_ramp from T_LO to T_HI, brightness EXPOSURE (T_obs/T_REF)**4);
it takes the place of --disk-shift and works with --cpu and --ss.
--disk-ring-f64 takes the pixels of the capture band through the f64 path
(geo_set_disk_ring_f64: the third image's radii and colours to the disk's
accuracy bar), on the GPU or with --cpu, with --ss only beside --adaptive.
--adaptive draws the disk frame with the error-controlled integrator
(GEO_MODE_ADAPTIVE through geo_render_disk_adaptive, --tol its tolerance in u,
0 = the default 1e-6), unshaded, with --disk-shift or with --disk-emission, on
the GPU or with --cpu.  With --disk-ring-f64 the frame goes through
geo_render_disk_adaptive_ring (--cpu: geo_render_cpu_disk_adaptive_ring_f64):
the capture band's pixels in f64, the rest by the adaptive integrator.  With
--ss the GPU frame goes through geo_render_disk_adaptive_batch with one frame
(the only call that supersamples an adaptive disk frame; with --disk-ring-f64
geo_render_disk_adaptive_ring_batch, likewise), and --cpu renders
geo_render_cpu_disk_adaptive (geo_render_cpu_disk_adaptive_ring_f64) at twice
the size and box-resolves it here (GEO_FLAG_SS4's definition: the CPU functions
refuse the flag).

Without texture files the synthetic equirect sky of the benchmarks is used for
the sky sphere and the planet/cloud spheres are skipped.  Units: rs = 1 (the
reference's rs = 10 scene divided by 10).
"""
from __future__ import annotations

import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def disk_frame(args):
    """One GEO_FLAG_DISK frame: sky sphere 50, rs = 1, step pi/100, 2048 steps."""
    import ctypes

    import numpy as np

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib, imageio
    from schwarzschild_raytracer_wgpu_amd.scenes import blackbody_ramp, make_disk_texture, make_sky

    w, h = args.width, args.height
    emission = ramp = None
    if args.disk_emission:
        t_ref, t_lo, t_hi, exposure = args.disk_emission
        profile = _lib.GEO_DISK_PROFILE_POWER if args.disk_profile == "power" else _lib.GEO_DISK_PROFILE_THIN
        emission = _lib.GeoDiskEmission(args.disk_spin, profile, t_ref, t_lo, t_hi, exposure)
        ramp = blackbody_ramp(256, t_lo, t_hi)
    obs = g.Observer(1.0, args.fov, w, h)
    obs.set_position(*args.pos)
    obs.set_camera(*args.camera)
    frame = obs.calc_transformation_pipeline()
    scene = g.make_scene(1.0, 50.0, obs.get_radial_position(), math.pi / 100, 2048,
                         _lib.GEO_MODE_ADAPTIVE if args.adaptive else _lib.GEO_MODE_DIRECT,
                         _lib.GEO_FLAG_DISK | (_lib.GEO_FLAG_SS4 if args.ss else 0), args.tol)
    sky = imageio.load_texture(args.sky) if args.sky else make_sky("equirect", (2048, 1024))
    tex = make_disk_texture((1024, 128))
    r_in, r_out = args.disk
    cpu_resolve = args.cpu and args.adaptive and args.ss
    if cpu_resolve:  # the one-sample frame at 2w x 2h, resolved below
        scene = g.make_scene(1.0, 50.0, obs.get_radial_position(), math.pi / 100, 2048, _lib.GEO_MODE_ADAPTIVE,
                             _lib.GEO_FLAG_DISK, args.tol)
        w, h = 2 * w, 2 * h
    if args.cpu:
        lib = ctypes.CDLL(os.path.join(ROOT, "schwarzschild_raytracer_wgpu_amd", "libgeo_cpu.so"))
        disk = _lib.GeoDisk(r_in, r_out, (ctypes.c_float * 3)(*args.disk_normal), (ctypes.c_float * 3)(1.0, 0.0, 0.0))
        sky = np.ascontiguousarray(sky)
        rgba = np.zeros((h, w, 4), np.uint8)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        common = [ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1], sky.shape[0], None, 0,
                  w, h, 0, h, 1, 0, rgba.ctypes.data, None, None, None, None, ctypes.addressof(disk), tex.ctypes.data,
                  tex.shape[1], tex.shape[0], None]
        base = [vp, vp, vp, u32, u32, vp, u32, u32, u32, u32, u32, u32, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, u32,
                u32, vp]
        ring = 1 if args.disk_ring_f64 else 0
        if args.adaptive:
            # (with ring = 0 the function is geo_render_cpu_disk_adaptive)
            name = "geo_render_cpu_disk_adaptive_ring_f64"
            shift = None
            if args.disk_shift:
                shift = _lib.GeoDiskShift(int(args.disk_shift[0]), int(args.disk_shift[1]), args.disk_shift[2])
            lib.geo_render_cpu_disk_adaptive_ring_f64.restype = ctypes.c_int
            lib.geo_render_cpu_disk_adaptive_ring_f64.argtypes = base + [vp, vp, u32, vp, vp, vp, ctypes.c_int]
            rc = lib.geo_render_cpu_disk_adaptive_ring_f64(
                *common, ctypes.addressof(emission) if emission is not None else None,
                ramp.ctypes.data if ramp is not None else None, ramp.shape[0] if ramp is not None else 0, None, None,
                ctypes.addressof(shift) if shift else None, ring)
        elif emission is not None:
            name = "geo_render_cpu_disk_ring_f64"
            lib.geo_render_cpu_disk_ring_f64.restype = ctypes.c_int
            lib.geo_render_cpu_disk_ring_f64.argtypes = base + [vp, vp, u32, vp, vp, ctypes.c_int]
            rc = lib.geo_render_cpu_disk_ring_f64(*common, ctypes.addressof(emission), ramp.ctypes.data, ramp.shape[0],
                                                  None, None, ring)
        else:
            name = "geo_render_cpu_disk_shift_ring_f64"
            shift = None
            if args.disk_shift:
                shift = _lib.GeoDiskShift(int(args.disk_shift[0]), int(args.disk_shift[1]), args.disk_shift[2])
            lib.geo_render_cpu_disk_shift_ring_f64.restype = ctypes.c_int
            lib.geo_render_cpu_disk_shift_ring_f64.argtypes = base + [vp, vp, ctypes.c_int]
            rc = lib.geo_render_cpu_disk_shift_ring_f64(*common, ctypes.addressof(shift) if shift else None, None, ring)
        if rc != 0:
            raise SystemExit(f"{name}: {rc}")
        if cpu_resolve:  # per channel (s00 + s01 + s10 + s11 + 2) >> 2
            s4 = rgba.astype(np.uint16)
            rgba = ((s4[0::2, 0::2] + s4[0::2, 1::2] + s4[1::2, 0::2] + s4[1::2, 1::2] + 2) >> 2).astype(np.uint8)
            w, h = w // 2, h // 2
    else:
        import torch

        ctx = g.Context(0)
        ctx.set_sky(sky)
        ctx.set_disk(tex, r_in, r_out, normal=args.disk_normal)
        if args.disk_shift:
            ctx.set_disk_shift(int(args.disk_shift[0]), int(args.disk_shift[1]), args.disk_shift[2])
        if emission is not None:
            ctx.set_disk_emission(ramp, emission.t_ref, emission.t_lo, emission.t_hi, emission.profile,
                                  emission.exposure, emission.spin)
        if args.disk_ring_f64:
            ctx.set_disk_ring_f64(True)
        rgba = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda:0")
        if args.adaptive and args.ss:  # (a whole frame of 8-row bands, the last one clipped)
            nb = (h + 7) // 8
            rgba = torch.empty(nb * 8 * w * 4, dtype=torch.uint8, device="cuda:0")
            render = ctx.render_disk_adaptive_ring_batch if args.disk_ring_f64 else ctx.render_disk_adaptive_batch
            render([frame], scene, w, h, 8, 0, 8, nb, rgba)
            rgba = rgba[:w * h * 4]
        elif args.adaptive and args.disk_ring_f64:
            ctx.render_disk_adaptive_ring(frame, scene, w, h, h, 0, h, 1, rgba)
        elif args.adaptive:
            ctx.render_disk_adaptive(frame, scene, w, h, h, 0, h, 1, rgba)
        else:
            ctx.render_rows(frame, scene, w, h, 0, h, rgba)
    if args.out.endswith(".ppm"):
        imageio.save_ppm(args.out, rgba, w, h)
    elif args.out.endswith((".jpg", ".jpeg")):
        from PIL import Image

        Image.fromarray(imageio.frame_to_host(rgba, w, h)[..., :3].copy(), "RGB").save(args.out, quality=88)
    else:
        imageio.save_png(args.out, rgba, w, h)
    print(f"wrote {args.out} ({w}x{h}{', 2x2 supersampled' if args.ss else ''}"
          f"{', adaptive' if args.adaptive else ''}{', f64 band' if args.disk_ring_f64 else ''}, "
          f"thin disk {r_in}..{r_out}, "
          f"{'CPU path' if args.cpu else 'GPU'})")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--sky")
    p.add_argument("--planet")
    p.add_argument("--clouds")
    p.add_argument("--frames", type=int, default=1, help="frames of motion before the saved one (dt = 1/60 s)")
    p.add_argument("--orbit", type=float, default=0.0, help="start an orbit with this rotation (observer.rs:162)")
    p.add_argument("--no-disk", action="store_true")
    p.add_argument("--mipmaps", action="store_true", help="trilinear mip-mapped textures, as the reference samples them")
    p.add_argument("--fan", action="store_true",
                   help="the reference's display path: per-frame 400-node f64 ray fans and the fan lerp "
                        "(GEO_MODE_FAN) instead of a geodesic per pixel")
    p.add_argument("--disk", type=float, nargs=2, metavar=("R_IN", "R_OUT"),
                   help="the ray-traced thin disk (GEO_FLAG_DISK) over the sky sphere")
    p.add_argument("--disk-normal", type=float, nargs=3, default=(0.0, 0.0, 1.0))
    p.add_argument("--disk-shift", type=float, nargs=3, metavar=("SPIN", "EXP", "GAIN"),
                   help="with --disk: Doppler and redshift shading (geo_set_disk_shift)")
    p.add_argument("--disk-emission", type=float, nargs=4, metavar=("T_REF", "T_LO", "T_HI", "EXPOSURE"),
                   help="with --disk: blackbody emission (geo_set_disk_emission), in place of --disk-shift")
    p.add_argument("--disk-profile", choices=("power", "thin"), default="thin", help="with --disk-emission")
    p.add_argument("--disk-spin", type=int, choices=(1, -1), default=1, help="with --disk-emission")
    p.add_argument("--disk-ring-f64", action="store_true",
                   help="with --disk: the capture band's pixels in f64 (geo_set_disk_ring_f64); with --ss only "
                        "beside --adaptive")
    p.add_argument("--adaptive", action="store_true",
                   help="with --disk: the error-controlled integrator (geo_render_disk_adaptive; with --ss "
                        "geo_render_disk_adaptive_batch with one frame; with --disk-ring-f64 "
                        "geo_render_disk_adaptive_ring; with both geo_render_disk_adaptive_ring_batch with one frame)")
    p.add_argument("--tol", type=float, default=0.0, help="with --adaptive: the tolerance in u (0 = 1e-6)")
    p.add_argument("--cpu", action="store_true", help="with --disk: the CPU path (libgeo_cpu.so)")
    p.add_argument("--ss", action="store_true", help="with --disk: 2 x 2 supersampling (GEO_FLAG_SS4)")
    p.add_argument("--pos", type=float, nargs=3, default=(2.4, 0.0, 0.7), help="with --disk: observer position")
    p.add_argument("--camera", type=float, nargs=2, default=(math.pi, -0.28), help="with --disk: camera (phi, theta)")
    p.add_argument("--fov", type=float, default=math.pi / 2, help="with --disk")
    args = p.parse_args()
    if args.disk_ring_f64 and (not args.disk or (args.ss and not args.adaptive)):
        p.error("--disk-ring-f64 goes with --disk, and with --ss only beside --adaptive (a supersampled direct disk "
                "frame refuses the state)")
    if args.adaptive and not args.disk:
        p.error("--adaptive goes with --disk")
    if args.tol != 0.0 and not args.adaptive:
        p.error("--tol goes with --adaptive")
    if args.disk:
        return disk_frame(args)
    if args.ss:
        p.error("--ss goes with --disk (the scene's spheres are composited, which GEO_FLAG_SS4 refuses)")

    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import imageio
    from schwarzschild_raytracer_wgpu_amd.scenes import make_sky

    w, h = args.width, args.height
    obs = g.Observer(1.0, math.pi / 2, w, h)
    obs.set_position(2.5, 0.0, 0.1)
    if args.orbit:
        obs.start_orbit(args.orbit)
    sky = imageio.load_texture(args.sky) if args.sky else make_sky("equirect", (4096, 2048))
    mode = g.GEO_MODE_FAN if args.fan else g.GEO_MODE_DIRECT
    spheres = [g.BasicSphereBuffer(0, 50.0, 1.0, sky, mode=mode, mipmaps=args.mipmaps)]
    if args.planet:
        spheres.append(g.BasicSphereBuffer(0, 1.1, 1.0, imageio.load_texture(args.planet), mode=mode,
                                           mipmaps=args.mipmaps))
    if args.clouds:
        spheres.append(g.BasicSphereBuffer(0, 1.2, 1.0, imageio.load_texture(args.clouds), mode=mode,
                                           mipmaps=args.mipmaps))
    disk = None if args.no_disk else g.PointCloud.new_accretion_disk(spheres[0].ctx, 1.0, obs.get_position(), True)
    tgt = g.RenderTarget(w, h, torch.empty(w * h * 4, dtype=torch.uint8, device="cuda:0"))
    renderer = g.Renderer(obs)
    for _ in range(args.frames):
        obs.update_position((0.0, 0.0, 0.0), 1 / 60)
        r = obs.get_radial_position()
        for s in spheres:
            s.update_ray_fan(r)
        if disk is not None:
            disk.update(obs.get_position(), 1 / 60)
        renderer.render(spheres, tgt, point_clouds=[disk] if disk is not None else [])
    if args.out.endswith(".ppm"):
        imageio.save_ppm(args.out, tgt.rgba, w, h)
    else:
        imageio.save_png(args.out, tgt.rgba, w, h)
    print(f"wrote {args.out} ({w}x{h}, {len(spheres)} sphere(s){', accretion disk' if disk else ''}, "
          f"{'fan lerp' if args.fan else 'per-pixel geodesics'})")


if __name__ == "__main__":
    main()
