#!/usr/bin/env python3
"""Waves of a direct-mode render by the exit test their group loop takes
(geo_pixel.h: the exact kTestLow loop, or the end-state kTestEnd loop where
every lane of the wave passes the selector of make_consts).

Needs the diagnostic build (python tools/build_variant.py
tools/ab/libgeo_wavelog.so -DGEO_WAVE_LOG=1), whose kernels count each wave
once at its loop's entry (geo_debug_loop_waves); the product library has no
such counter.  One frame per config; a wave none of whose lanes reaches the
loop (radial or pre-filtered rays only) counts in neither column.

    python tools/loop_waves.py [--lib tools/ab/libgeo_wavelog.so] [--configs cfg3_4k,cfg2_1080p] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lib", default=os.path.join(ROOT, "tools", "ab", "libgeo_wavelog.so"))
    p.add_argument("--configs", default="cfg3_4k,cfg2_1080p")
    p.add_argument("--out", default=None)
    a = p.parse_args()

    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd._lib import SIGNATURES
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, make_sky

    lib = ctypes.CDLL(a.lib)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.geo_debug_loop_waves.restype = ctypes.c_int
    lib.geo_debug_loop_waves.argtypes = [ctypes.c_void_p, ctypes.c_void_p]

    def check(st, what):
        if st != 0:
            raise SystemExit(f"{what}: {st}")

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        W, H = cfg.width, cfg.height
        obs = g.Observer(cfg.rs, cfg.fov, W, H)
        obs.set_position(*cfg.position)
        obs.set_camera(*cfg.camera)
        obs.set_energy(cfg.energy)
        frame = obs.calc_transformation_pipeline()
        scene = g.make_scene(cfg.rs, cfg.sphere_r, obs.get_radial_position(), cfg.step, cfg.max_steps, 0)
        sky = make_sky(cfg.sky, cfg.sky_size)
        h = ctypes.c_void_p()
        check(lib.geo_ctx_create(0, ctypes.byref(h)), "ctx")
        check(lib.geo_set_sky(h, sky.ctypes.data, sky.shape[1], sky.shape[0]), "sky")
        out = torch.empty(H * W * 4, dtype=torch.uint8, device=dev)
        counts = (ctypes.c_ulonglong * 2)()
        check(lib.geo_debug_loop_waves(h, counts), "clear")
        check(lib.geo_render_rows(h, frame, scene, W, H, 0, H, out.data_ptr(), None, None, None, None, stream),
              "render")
        check(lib.geo_debug_loop_waves(h, counts), "read")
        lib.geo_ctx_destroy(h)
        r = {"config": name, "waves_exact_loop": int(counts[0]), "waves_end_state_loop": int(counts[1]),
             "waves_launched": -(-W // 32) * -(-H // 8) * 4}
        results.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
