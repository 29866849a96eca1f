#!/usr/bin/env python3
"""Cost of a GEO_FLAG_DISK frame over the plain one: config 3's scene (4K,
2048 steps, observer (2.5, 0, 0.1)) with the disk 1.6..2.2 of the tests'
pose B, which that scene's observer sees almost edge-on at the same scale.

Plain and disk renders alternate in one process (after a warm-up of both,
long enough for each grid's learned dispatch order to be adopted); each
render's kernel dispatch is timed by its own event pair
(geo_time_next_render), and the medians of N >= 20 of each are compared.
Writes one JSON object (profiles/disk_bench_cfg3.json by default) and prints
it.

  python tools/bench_disk.py [--n 30] [--out profiles/disk_bench_cfg3.json]
  python tools/bench_disk.py --shift [--n 30] [--out profiles/disk_shift_bench_cfg3.json]

--shift adds the shaded disk frame (geo_set_disk_shift: spin +1, exponent 4,
gain 1) as a third kind in the same alternation and reports it against the
unshaded disk frame; its output file is a JSON list that every run appends to.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=30, help="timed renders of each kind (>= 20)")
    p.add_argument("--warmup", type=int, default=40, help="untimed renders of each kind first")
    p.add_argument("--shift", action="store_true", help="also time the Doppler-shaded disk frame")
    p.add_argument("--out")
    args = p.parse_args()
    if not args.out:
        args.out = os.path.join(ROOT, "profiles", "disk_shift_bench_cfg3.json" if args.shift else "disk_bench_cfg3.json")
    if args.n < 20:
        raise SystemExit("--n must be at least 20")

    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, make_disk_texture, make_sky
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    if not torch.cuda.is_available():
        raise SystemExit("bench_disk.py needs a HIP device")
    cfg = CONFIGS["cfg3_4k"]
    W, H = cfg.width, cfg.height
    obs = g.Observer(cfg.rs, cfg.fov, W, H)
    obs.set_position(*cfg.position)
    obs.set_camera(*cfg.camera)
    obs.set_energy(cfg.energy)
    frame = obs.calc_transformation_pipeline()
    r = obs.get_radial_position()
    plain = g.make_scene(cfg.rs, cfg.sphere_r, r, cfg.step, cfg.max_steps)
    disk = g.make_scene(cfg.rs, cfg.sphere_r, r, cfg.step, cfg.max_steps, flags=_lib.GEO_FLAG_DISK)
    r_in, r_out = 1.6 * cfg.rs, 2.2 * cfg.rs
    ctx = g.Context(0)
    ctx.set_sky(make_sky(cfg.sky, cfg.sky_size))
    ctx.set_disk(make_disk_texture((1024, 128)), r_in, r_out)
    dev = torch.device("cuda:0")
    out = torch.empty(W * H * 4, dtype=torch.uint8, device=dev)
    hits = torch.zeros(W * H * 6, dtype=torch.float32, device=dev)
    # the learned order is per grid key, and the two kinds alternate: period 1
    # would re-learn at every switch, so each kind runs on its own context
    ctx2 = g.Context(0)
    ctx2.set_sky(make_sky(cfg.sky, cfg.sky_size))
    kinds = [("plain", ctx2, plain), ("disk", ctx, disk)]
    if args.shift:
        ctx3 = g.Context(0)
        ctx3.set_sky(make_sky(cfg.sky, cfg.sky_size))
        ctx3.set_disk(make_disk_texture((1024, 128)), r_in, r_out)
        ctx3.set_disk_shift(1, 4, 1.0)
        kinds.append(("shift", ctx3, disk))
    for _ in range(args.warmup):
        for _, c, sc in kinds:
            c.render_rows(frame, sc, W, H, 0, H, out)
    torch.cuda.synchronize()
    ev = {k: [] for k, _, _ in kinds}
    for _ in range(args.n):
        for kind, c, sc in kinds:
            a, b = HipEvent(), HipEvent()
            c.time_next_render(a, b)
            c.render_rows(frame, sc, W, H, 0, H, out)
            ev[kind].append((a, b))
    torch.cuda.synchronize()
    ms = {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
    # what the disk frame draws (one more render, untimed)
    ctx.disk_hits_next_render(hits)
    ctx.render_rows(frame, disk, W, H, 0, H, out)
    torch.cuda.synchronize()
    hv = hits.view(H, W, 3, 2)[..., 0] > 0
    res = {
        "config": "cfg3_4k", "width": W, "height": H, "max_steps": cfg.max_steps, "disk": [r_in, r_out],
        "n": args.n, "warmup": args.warmup,
        "plain_ms_median": float(np.median(ms["plain"])), "disk_ms_median": float(np.median(ms["disk"])),
        "plain_ms_min": float(ms["plain"].min()), "disk_ms_min": float(ms["disk"].min()),
        "plain_ms_iqr": float(np.subtract(*np.percentile(ms["plain"], [75, 25]))),
        "disk_ms_iqr": float(np.subtract(*np.percentile(ms["disk"], [75, 25]))),
        "disk_over_plain": float(np.median(ms["disk"]) / np.median(ms["plain"])),
        "hit_pixels_per_slot": [int(hv[..., k].sum()) for k in range(3)],
        "timing": "geo_time_next_render event pairs on each kernel dispatch, the kinds alternating",
    }
    if args.shift:
        res.update({
            "shift": [1, 4, 1.0],
            "shift_ms_median": float(np.median(ms["shift"])), "shift_ms_min": float(ms["shift"].min()),
            "shift_ms_iqr": float(np.subtract(*np.percentile(ms["shift"], [75, 25]))),
            "shift_over_disk": float(np.median(ms["shift"]) / np.median(ms["disk"])),
            "hit_pixel_share": float(hv.any(axis=-1).float().mean()),
        })
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    doc = res
    if args.shift:  # every run is kept
        doc = []
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc.append(res)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
