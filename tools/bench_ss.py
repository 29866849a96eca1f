#!/usr/bin/env python3
"""Cost of a GEO_FLAG_SS4 frame against the one-sample frame of the same rays:
config 3's scene (observer (2.5, 0, 0.1), 2048 steps) at 1920 x 1080 with the
flag traces the rays of the plain 3840 x 2160 frame, whose kernels this build
has unchanged from the commit before the flag, so the 4K frame is that
commit's baseline inside one process.  The same for the disk frame (the disk
1.6..2.2 of tools/bench_disk.py) and the shifted disk frame against their 4K
one-sample renders.

A session warms every kind up (long enough for each grid's learned dispatch
order to be adopted; each kind has a context of its own, the order is kept per
context), then runs --rounds alternations; in one alternation the SS frame and
its 4K frame take turns --n times, each dispatch timed by its own event pair
(geo_time_next_render), and each kind's median of the n is the alternation's
figure.  Per pair a session reports the median of those medians for both kinds,
their ratio, and the 4K frame's spread, (max - min) / median of its own
alternation medians: the noise floor of the comparison on that box.  The
margin the SS frame is held to is 1 + 2 x that spread.  Writes one JSON object
with every session (profiles/ss_bench_cfg3.json by default) and prints it.

  python tools/bench_ss.py [--n 30] [--rounds 5] [--sessions 2] [--out profiles/ss_bench_cfg3.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def session(args, cfg, frame, scenes, sky, tex):
    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    W, H = cfg.width, cfg.height
    dev = torch.device("cuda:0")
    out = torch.empty(W * H * 4, dtype=torch.uint8, device=dev)

    def make_ctx(kind):
        c = g.Context(0)
        c.set_sky(sky)
        if kind != "plain":
            c.set_disk(tex, 1.6 * cfg.rs, 2.2 * cfg.rs)
        if kind == "shift":
            c.set_disk_shift(1, 4, 1.0)
        return c

    res = {}
    for kind in ("plain", "disk", "shift"):
        one, ss = scenes[kind]
        # (name, context, scene, width, height)
        pair = [("one_4k", make_ctx(kind), one, W, H), ("ss_1080p", make_ctx(kind), ss, W // 2, H // 2)]
        for _ in range(args.warmup):
            for _, c, sc, w, h in pair:
                c.render_rows(frame, sc, w, h, 0, h, out)
        torch.cuda.synchronize()
        med = {name: [] for name, *_ in pair}
        for _ in range(args.rounds):
            ev = {name: [] for name, *_ in pair}
            for _ in range(args.n):
                for name, c, sc, w, h in pair:
                    a, b = HipEvent(), HipEvent()
                    c.time_next_render(a, b)
                    c.render_rows(frame, sc, w, h, 0, h, out)
                    ev[name].append((a, b))
            torch.cuda.synchronize()
            for name, v in ev.items():
                med[name].append(float(np.median([a.elapsed_time(b) for a, b in v])))
        for _, c, *_ in pair:
            c.close()
        one_m, ss_m = float(np.median(med["one_4k"])), float(np.median(med["ss_1080p"]))
        spread = (max(med["one_4k"]) - min(med["one_4k"])) / one_m
        res[kind] = {
            "one_4k_ms_medians": med["one_4k"], "ss_1080p_ms_medians": med["ss_1080p"],
            "one_4k_ms": one_m, "ss_1080p_ms": ss_m, "ss_over_one": ss_m / one_m,
            "one_4k_spread": spread,
            "ss_1080p_spread": (max(med["ss_1080p"]) - min(med["ss_1080p"])) / ss_m,
            "margin": 1.0 + 2.0 * spread, "within_margin": bool(ss_m <= one_m * (1.0 + 2.0 * spread)),
        }
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=30, help="timed dispatches of each kind per alternation")
    p.add_argument("--rounds", type=int, default=5, help="alternations per session")
    p.add_argument("--sessions", type=int, default=2)
    p.add_argument("--warmup", type=int, default=40, help="untimed renders of each kind first")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ss_bench_cfg3.json"))
    args = p.parse_args()

    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, make_disk_texture, make_sky

    if not torch.cuda.is_available():
        raise SystemExit("bench_ss.py needs a HIP device")
    cfg = CONFIGS["cfg3_4k"]
    obs = g.Observer(cfg.rs, cfg.fov, cfg.width, cfg.height)
    obs.set_position(*cfg.position)
    obs.set_camera(*cfg.camera)
    obs.set_energy(cfg.energy)
    frame = obs.calc_transformation_pipeline()  # (the same uniform at half the size: it holds no pixel count)
    r = obs.get_radial_position()

    def scene(flags):
        return g.make_scene(cfg.rs, cfg.sphere_r, r, cfg.step, cfg.max_steps, flags=flags)

    D, S = _lib.GEO_FLAG_DISK, _lib.GEO_FLAG_SS4
    scenes = {"plain": (scene(0), scene(S)), "disk": (scene(D), scene(D | S)), "shift": (scene(D), scene(D | S))}
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))
    res = {
        "config": "cfg3_4k", "one_sample": [cfg.width, cfg.height], "supersampled": [cfg.width // 2, cfg.height // 2],
        "max_steps": cfg.max_steps, "disk": [1.6 * cfg.rs, 2.2 * cfg.rs], "shift": [1, 4, 1.0],
        "n": args.n, "rounds": args.rounds, "warmup": args.warmup,
        "timing": "geo_time_next_render event pairs on each kernel dispatch; the SS frame and its 4K one-sample "
                  "frame alternate; per alternation the median of n; spread = (max - min) / median of a kind's "
                  "alternation medians; margin = 1 + 2 x the 4K frame's spread",
        "sessions": [session(args, cfg, frame, scenes, sky, tex) for _ in range(args.sessions)],
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
