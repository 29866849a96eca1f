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

  python tools/bench_ss.py --batch 8 [--n 30] [--rounds 5] [--sessions 1] [--out profiles/ss_batch_bench_cfg3.json]

--batch K measures the batched SS launch (geo_render_ss_batch) where it is
used: a peer's share of the 1920 x 1080 supersampled frame at N = 8 (8-row
bands, BandLayout rank 1 of 8; the sample frame is the 4K frame).  One launch of
K frames alternates with K one-frame geo_render_band_set launches of the same
frames back to back (the kernels this build has unchanged from the commit
before the batch), each on its own context, for the plain, the disk and the
shifted disk frame.  Every alternation takes --n samples of each side and keeps
their medians; --rounds alternations are timed by a pair of stream events
around the launches (what a pipeline waits for: dispatch gaps included) and
--rounds more by geo_time_next_render pairs on the kernel dispatches alone (the
K one-frame times added up).  Per kind and timing: the median of the
alternation medians per frame, the ratio batch over one-frame launches, the
one-frame side's spread ((max - min) / median of its alternation medians) and
the margin 1 + 2 x that spread the batch is held to.
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


def batch_session(args, cfg, frame, scenes, sky, tex):
    import ctypes

    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.dist import BandLayout
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent, hipEventDefault

    K = args.batch
    W, H = cfg.width // 2, cfg.height // 2
    L = BandLayout(H, 8, 8, 1)  # a peer's share at N = 8
    band = (L.band_height(), L.row0(), L.cycle_rows, L.nbands())
    packed = L.packed_rows() * W * 4
    dev = torch.device("cuda:0")
    out = torch.empty(K * packed, dtype=torch.uint8, device=dev)
    sh = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib

    def make_ctx(kind):
        c = g.Context(0)
        c.set_sky(sky)
        if kind != "plain":
            c.set_disk(tex, 1.6 * cfg.rs, 2.2 * cfg.rs)
        if kind == "shift":
            c.set_disk_shift(1, 4, 1.0)
        return c

    res = {"layout": {"world": 8, "rank": 1, "band_rows": band[0], "row0": band[1], "row_stride": band[2],
                      "nbands": band[3], "rows": L.rows_mine()}}
    for kind in ("plain", "disk", "shift"):
        scene = scenes[kind][1]
        frames = (_lib.GeoFrame * K)(*([frame] * K))
        sarr = (_lib.GeoScene * K)(*([scene] * K))

        def run_batch(c, pairs=None):
            if pairs is not None:
                c.time_next_render(*pairs[0])
            _lib.check("geo_render_ss_batch", lib.geo_render_ss_batch(
                c._h, frames, sarr, K, W, H, *band, out.data_ptr(), packed, None, sh))

        def run_singles(c, pairs=None):
            for k in range(K):
                if pairs is not None:
                    c.time_next_render(*pairs[k])
                _lib.check("geo_render_band_set", lib.geo_render_band_set(
                    c._h, ctypes.byref(frame), ctypes.byref(scene), W, H, *band, out.data_ptr() + k * packed, None,
                    None, None, None, sh))

        # (each side on its own context: the learned dispatch order is kept per context)
        sides = [("batch", make_ctx(kind), run_batch, 1), ("single", make_ctx(kind), run_singles, K)]
        for _ in range(args.warmup):
            for _, c, run, _ in sides:
                run(c)
        torch.cuda.synchronize()
        res[kind] = {}
        for how in ("stream_events", "dispatch_events"):
            med = {name: [] for name, *_ in sides}
            for _ in range(args.rounds):
                ev = {name: [] for name, *_ in sides}
                for _ in range(args.n):
                    for name, c, run, m in sides:
                        if how == "stream_events":
                            a, b = HipEvent(hipEventDefault), HipEvent(hipEventDefault)
                            a.record(sh)
                            run(c)
                            b.record(sh)
                            ev[name].append([(a, b)])
                        else:
                            pairs = [(HipEvent(), HipEvent()) for _ in range(m)]
                            run(c, pairs)
                            ev[name].append(pairs)
                    torch.cuda.synchronize()  # the next sample's launches queue behind nothing
                for name, v in ev.items():
                    med[name].append(float(np.median([sum(a.elapsed_time(b) for a, b in pairs) for pairs in v]) / K))
            b_m, s_m = float(np.median(med["batch"])), float(np.median(med["single"]))
            spread = (max(med["single"]) - min(med["single"])) / s_m
            res[kind][how] = {
                "batch_ms_per_frame_medians": med["batch"], "single_ms_per_frame_medians": med["single"],
                "batch_ms_per_frame": b_m, "single_ms_per_frame": s_m, "batch_over_single": b_m / s_m,
                "single_spread": spread, "batch_spread": (max(med["batch"]) - min(med["batch"])) / b_m,
                "margin": 1.0 + 2.0 * spread, "within_margin": bool(b_m <= s_m * (1.0 + 2.0 * spread)),
            }
        for _, c, *_ in sides:
            c.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=30, help="timed dispatches of each kind per alternation")
    p.add_argument("--rounds", type=int, default=5, help="alternations per session")
    p.add_argument("--sessions", type=int, default=2)
    p.add_argument("--warmup", type=int, default=40, help="untimed renders of each kind first")
    p.add_argument("--batch", type=int, default=0, metavar="K",
                   help="measure one launch of K SS frames against K one-frame launches (a peer's share at N = 8)")
    p.add_argument("--out")
    args = p.parse_args()
    if not args.out:
        args.out = os.path.join(ROOT, "profiles", "ss_batch_bench_cfg3.json" if args.batch else "ss_bench_cfg3.json")

    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, make_disk_texture, make_sky

    if args.batch and not 1 <= args.batch <= _lib.GEO_MAX_BATCH_FRAMES:
        raise SystemExit(f"--batch: 1 .. {_lib.GEO_MAX_BATCH_FRAMES}")
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
    if args.batch:
        res = {
            "config": "cfg3_4k", "supersampled": [cfg.width // 2, cfg.height // 2],
            "sample_frame": [cfg.width, cfg.height], "max_steps": cfg.max_steps, "disk": [1.6 * cfg.rs, 2.2 * cfg.rs],
            "shift": [1, 4, 1.0], "frames_per_batch": args.batch, "n": args.n, "rounds": args.rounds,
            "warmup": args.warmup,
            "timing": "stream_events: a pair of events on the stream around one launch of K frames, or around K "
                      "one-frame launches back to back; dispatch_events: geo_time_next_render pairs on the kernel "
                      "dispatches, the K one-frame times added; the two sides alternate; per alternation the median "
                      "of n; spread = (max - min) / median of a side's alternation medians; margin = 1 + 2 x the "
                      "one-frame side's spread",
            "sessions": [batch_session(args, cfg, frame, scenes, sky, tex) for _ in range(args.sessions)],
        }
        print(json.dumps(res))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return
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
