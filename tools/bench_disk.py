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

  python tools/bench_disk.py --emission [--n 30] [--out profiles/disk_emission_bench_cfg3.json]
  python tools/bench_disk.py --batch 8 [--n 30] [--out profiles/disk_batch_bench_cfg3.json]

--shift adds the shaded disk frame (geo_set_disk_shift: spin +1, exponent 4,
gain 1) as a third kind in the same alternation and reports it against the
unshaded disk frame; its output file is a JSON list that every run appends to.

--emission measures the blackbody emission frame (geo_set_disk_emission: THIN
profile, a 256-entry scenes.blackbody_ramp) against the shaded disk frame
(--shift's), each on its own context: --alternations (5) times, --n (30)
event-timed dispatches of the shaded frame, then as many of the emission frame
(after --settle alternations of the same form, which are reported apart: the
first blocks after the warm-up run slower for both kinds).
It reports each alternation's medians and their ratio, the ratio of the
medians over all alternations, and the shaded side's own spread over the
alternations ((max - min) / median of its per-alternation medians): the noise
the ratio is read against.  Its output file, profiles/disk_emission_bench_cfg3.json, is a JSON list that
every run appends to.

--batch K measures the batched disk launch (geo_render_disk_batch) where it is
used: a peer's share of the 4K frame at N = 8 (8-row bands, BandLayout rank 1 of
8).  One launch of K disk frames alternates with K one-frame
geo_render_band_set launches of the same frames back to back, unshaded and
shaded, each on its own context; every sample is timed twice over, in two
passes: by a pair of stream events around the launches (what a pipeline waits
for: dispatch gaps included), and by geo_time_next_render pairs on the kernel
dispatches alone (the K one-frame times added up).  Medians of --n samples;
the ratios are per frame, batch over one-frame launches.

--batch K --emission measures the batched emission launch
(geo_render_emission_batch) on the same layout, with --emission's state (THIN
profile, a 256-entry ramp): one launch of K emission frames, K one-frame
geo_render_band_set launches of the same frames back to back (the yardstick),
and one shaded geo_render_disk_batch launch of K frames alternate, each on its
own context.  A session builds and warms the contexts up, then takes
--alternations (5) times --n (30) samples of each side, by stream events around
the launches and then by the dispatches' own event pairs, each after --settle
(4) alternations of the same form that are reported apart; each side's median
of the n is the alternation's figure.  Per session and timing it reports the
medians of those per frame, batch over one-frame launches, the one-frame
side's spread ((max - min) / median of its alternation medians), the margin
1 - 2 x that spread the batch has to beat, and the emission batch over the
shaded batch.  --sessions (2) sessions go into one JSON object.

  python tools/bench_disk.py --batch 8 --emission [--out profiles/disk_emission_batch_bench_cfg3.json]

--ring measures the disk frame with the capture band in f64
(geo_set_disk_ring_f64) against the same frame with the state off, by
--emission's method: --alternations (5) times --n (30) event-timed dispatches
of each kind in blocks, after --settle (4) alternations of the same form that
are reported apart, each kind on its own context.  The plain frame with and
without GEO_FLAG_RING_F64 runs beside them in the same alternations: the plain
frame's own ring cost is the second yardstick.  It reports the medians over
the alternations, disk-on over disk-off and ring over plain, each off side's
spread ((max - min) / median of its alternation medians) and whether each
cost lies beyond twice that spread.  One JSON object.

  python tools/bench_disk.py --ring [--out profiles/disk_ring_bench_cfg3.json]

--batch K --ring measures the batched launch of disk frames with the f64 band
(geo_render_disk_ring_batch, geo_set_disk_ring_f64 on, unshaded) on --batch's
layout, by --batch K --emission's method: one launch of K ring frames (the
small kernel that writes the frames' band constants runs on the stream before
the render: the stream events see it, the dispatch's own event pair does not)
alternates with K one-frame geo_render_band_set launches of the same frames
back to back with the state on (the yardstick), each on its own context;
--alternations (5) times --n (30) samples of each side per timing after
--settle (4) alternations kept apart, --sessions (2) sessions.  The batch
counts as a gain where it is faster than the one-frame side by more than twice
that side's alternation spread.

  python tools/bench_disk.py --batch 8 --ring [--out profiles/disk_ring_batch_bench_cfg3.json]

--adaptive measures the adaptive disk frame (geo_render_disk_adaptive) against
the plain GEO_MODE_ADAPTIVE frame of the same scene: config 3's scene with the
disk 1.6..2.2 rs at config 5's mode, step and tol, by --ring's method, each
kind on its own context: --alternations (5) times --n (30) event-timed
dispatches of each kind in blocks, after --settle (4) alternations of the same
form that are reported apart, --sessions (2) sessions.  The direct disk frame
and the direct plain frame run beside them in the same alternations, for
orientation.  Per session it reports the medians over the alternations, the
adaptive disk frame over the plain adaptive one (the surplus), the plain
side's spread ((max - min) / median of its alternation medians) and whether
the surplus lies beyond twice that spread.  One JSON object.

  python tools/bench_disk.py --adaptive [--out profiles/disk_adaptive_bench.json]

--batch K --adaptive measures the batched adaptive disk launch
(geo_render_disk_adaptive_batch) on --batch's layout with --adaptive's scene,
by --batch K --ring's method: one launch of K frames alternates with K
one-frame geo_render_disk_adaptive launches of the same frames back to back
(the yardstick), unshaded and with --emission's state, each side on its own
context; --alternations (5) times --n (30) samples of each side per timing
(stream events around the calls, then the dispatches' own event pairs) after
--settle (4) alternations kept apart, --sessions (2) sessions.  The batch
counts as a gain where it is faster than the one-frame side by more than twice
that side's alternation spread.

  python tools/bench_disk.py --batch 8 --adaptive [--out profiles/disk_adaptive_batch_bench.json]

--adaptive --ring measures the adaptive disk frame with the capture band in f64
(geo_render_disk_adaptive_ring, geo_set_disk_ring_f64 on) against the same frame
with the state off (geo_render_disk_adaptive) on --adaptive's scene, by --ring's
method, each kind on its own context: --alternations (5) times --n (30)
event-timed dispatches of each kind in blocks, after --settle (4) alternations
of the same form that are reported apart, --sessions (2) sessions.  The plain
adaptive frame with and without GEO_FLAG_RING_F64 runs beside them in the same
alternations: the plain frame's own ring cost is the second yardstick.  Per
session it reports the medians over the alternations, on over off and ring over
plain, each off side's spread ((max - min) / median of its alternation medians)
and whether each cost lies beyond twice that spread.  One JSON object.
With --camera-away the camera is turned by pi, away from the hole: no pixel of
the frame lies in the band (steps_total_on then equals attempts_total_off), so
on over off is the cost of the ring kernel's shape alone, its registers and the
LDS copy, on lanes that all take the f32 path.

  python tools/bench_disk.py --adaptive --ring [--out profiles/disk_adaptive_ring_bench.json]
  python tools/bench_disk.py --adaptive --ring --camera-away [--out profiles/disk_adaptive_ring_away_bench.json]

--batch K --adaptive --ring measures the batched launch of adaptive disk frames
with the f64 band (geo_render_disk_adaptive_ring_batch, geo_set_disk_ring_f64
on) by --batch K --adaptive's method and on its layout and scene: one launch of
K frames alternates with K one-frame geo_render_disk_adaptive_ring launches of
the same frames back to back (the yardstick), unshaded and with --emission's
state, each side on its own context, by both timings.  The totals are in the
ring renders' mixed units (adaptive attempts outside the band, f64 steps in it).

  python tools/bench_disk.py --batch 8 --adaptive --ring [--out profiles/disk_adaptive_ring_batch_bench.json]
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
    p.add_argument("--emission", action="store_true",
                   help="time the blackbody emission frame against the shaded disk frame, in alternating blocks")
    p.add_argument("--ring", action="store_true",
                   help="time the disk frame with geo_set_disk_ring_f64 on against off, and the plain frame with and "
                        "without GEO_FLAG_RING_F64, in alternating blocks")
    p.add_argument("--adaptive", action="store_true",
                   help="time the adaptive disk frame (geo_render_disk_adaptive) against the plain adaptive frame, in "
                        "alternating blocks")
    p.add_argument("--alternations", type=int, default=5, help="with --emission: blocks of --n renders of each kind")
    p.add_argument("--settle", type=int, default=4,
                   help="with --emission: alternations run first in the timed form, reported apart and not counted")
    p.add_argument("--batch", type=int, default=0, metavar="K",
                   help="measure one launch of K disk frames against K one-frame launches (a peer's share at N = 8)")
    p.add_argument("--sessions", type=int, default=2,
                   help="with --batch K --emission: sessions (contexts built, warmed up and timed anew)")
    p.add_argument("--shaded-first", action="store_true",
                   help="with --batch K --emission: the shaded batch is each sample's first launch, the emission "
                        "batch its last (default: the other way round)")
    p.add_argument("--camera-away", action="store_true",
                   help="with --adaptive --ring: the camera turned away from the hole, a frame with no band pixel")
    p.add_argument("--out")
    args = p.parse_args()
    if args.adaptive and (args.emission or args.shift or (args.camera_away and args.batch)):
        raise SystemExit("--adaptive goes alone, with --ring, with --batch K, or with both")
    if not args.out:
        if args.adaptive and args.batch:
            name = "disk_adaptive_ring_batch_bench.json" if args.ring else "disk_adaptive_batch_bench.json"
        elif args.adaptive and args.ring:
            name = "disk_adaptive_ring_away_bench.json" if args.camera_away else "disk_adaptive_ring_bench.json"
        elif args.adaptive:
            name = "disk_adaptive_bench.json"
        elif args.batch and args.ring:
            name = "disk_ring_batch_bench_cfg3.json"
        elif args.ring:
            name = "disk_ring_bench_cfg3.json"
        elif args.batch and args.emission:
            name = "disk_emission_batch_bench_cfg3.json"
        elif args.batch:
            name = "disk_batch_bench_cfg3.json"
        elif args.emission:
            name = "disk_emission_bench_cfg3.json"
        else:
            name = "disk_shift_bench_cfg3.json" if args.shift else "disk_bench_cfg3.json"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.n < 20:
        raise SystemExit("--n must be at least 20")
    if args.adaptive and args.batch:
        return adaptive_batch_main(args)
    if args.adaptive and args.ring:
        return adaptive_ring_main(args)
    if args.adaptive:
        return adaptive_main(args)
    if args.batch and args.ring:
        return ring_batch_main(args)
    if args.ring:
        return ring_main(args)
    if args.batch and args.emission:
        return emission_batch_main(args)
    if args.batch:
        return batch_main(args)
    if args.emission:
        return emission_main(args)

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


def emission_main(args):
    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, blackbody_ramp, make_disk_texture, make_sky
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
    scene = g.make_scene(cfg.rs, cfg.sphere_r, obs.get_radial_position(), cfg.step, cfg.max_steps,
                         flags=_lib.GEO_FLAG_DISK)
    r_in, r_out = 1.6 * cfg.rs, 2.2 * cfg.rs
    emission = dict(t_ref=9000.0, t_lo=1500.0, t_hi=30000.0, profile=_lib.GEO_DISK_PROFILE_THIN, exposure=1.0, spin=1)
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))
    # (each kind on its own context: the learned dispatch order is kept per context)
    ctxs = {}
    for kind in ("shift", "emission"):
        c = g.Context(0)
        c.set_sky(sky)
        c.set_disk(tex, r_in, r_out)
        if kind == "shift":
            c.set_disk_shift(1, 4, 1.0)
        else:
            c.set_disk_emission(blackbody_ramp(256, emission["t_lo"], emission["t_hi"]), **emission)
        ctxs[kind] = c
    dev = torch.device("cuda:0")
    out = torch.empty(W * H * 4, dtype=torch.uint8, device=dev)
    for _ in range(args.warmup):
        for c in ctxs.values():
            c.render_rows(frame, scene, W, H, 0, H, out)
    torch.cuda.synchronize()
    # The first blocks after the warm-up are slower for both kinds (a block of 30 event-timed renders of one kind
    # back to back is another regime than the warm-up's untimed renders of alternating kinds, and the device takes
    # about a hundred renders to settle in it): --settle alternations are run in the timed form and kept apart
    blocks, settling = [], []
    for alt in range(args.settle + args.alternations):
        med = {}
        for kind, c in ctxs.items():
            ev = []
            for _ in range(args.n):
                a, b = HipEvent(), HipEvent()
                c.time_next_render(a, b)
                c.render_rows(frame, scene, W, H, 0, H, out)
                ev.append((a, b))
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in ev])
            med[kind + "_ms_median"] = float(np.median(ms))
            med[kind + "_ms_min"] = float(ms.min())
            med[kind + "_ms_iqr"] = float(np.subtract(*np.percentile(ms, [75, 25])))
        med["emission_over_shift"] = med["emission_ms_median"] / med["shift_ms_median"]
        (settling if alt < args.settle else blocks).append(med)
    # what the emission frame draws (one more render, untimed)
    q = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    ctxs["emission"].disk_emission_next_render(q)
    ctxs["emission"].render_rows(frame, scene, W, H, 0, H, out)
    torch.cuda.synchronize()
    qv = q.view(H, W, 3)
    hit = qv > 0
    for c in ctxs.values():
        c.close()
    sm = np.array([b["shift_ms_median"] for b in blocks])
    em = np.array([b["emission_ms_median"] for b in blocks])
    res = {
        "config": "cfg3_4k", "width": W, "height": H, "max_steps": cfg.max_steps, "disk": [r_in, r_out],
        "shift": [1, 4, 1.0], "emission": emission, "ramp_entries": 256,
        "n": args.n, "warmup": args.warmup, "settling_alternations_not_counted": settling, "alternations": blocks,
        "shift_ms_median": float(np.median(sm)), "emission_ms_median": float(np.median(em)),
        "emission_over_shift": float(np.median(em) / np.median(sm)),
        "emission_over_shift_min": float(min(b["emission_over_shift"] for b in blocks)),
        "emission_over_shift_max": float(max(b["emission_over_shift"] for b in blocks)),
        "shift_alternation_spread": float((sm.max() - sm.min()) / np.median(sm)),
        "hit_pixel_share": float(hit.any(dim=-1).float().mean()),
        "q_max": float(qv.max()),
        "timing": "geo_time_next_render event pairs on each kernel dispatch; blocks of n shaded renders and n emission "
                  "renders alternate in one process, each kind on its own context",
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    doc = []  # every run is kept, as --shift's are
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc.append(res)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def ring_main(args):
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
    scenes = {"plain": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg.step, cfg.max_steps),
              "plain_ring": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg.step, cfg.max_steps,
                                         flags=_lib.GEO_FLAG_RING_F64),
              "disk_off": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg.step, cfg.max_steps, flags=_lib.GEO_FLAG_DISK)}
    scenes["disk_on"] = scenes["disk_off"]
    r_in, r_out = 1.6 * cfg.rs, 2.2 * cfg.rs
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))
    # (each kind on its own context: the learned dispatch order is kept per context)
    ctxs = {}
    for kind in ("disk_off", "disk_on", "plain", "plain_ring"):
        c = g.Context(0)
        c.set_sky(sky)
        if kind.startswith("disk"):
            c.set_disk(tex, r_in, r_out)
            c.set_disk_ring_f64(kind == "disk_on")
        ctxs[kind] = c
    dev = torch.device("cuda:0")
    out = torch.empty(W * H * 4, dtype=torch.uint8, device=dev)
    for _ in range(args.warmup):
        for kind, c in ctxs.items():
            c.render_rows(frame, scenes[kind], W, H, 0, H, out)
    torch.cuda.synchronize()
    blocks, settling = [], []
    for alt in range(args.settle + args.alternations):
        med = {}
        for kind, c in ctxs.items():
            ev = []
            for _ in range(args.n):
                a, b = HipEvent(), HipEvent()
                c.time_next_render(a, b)
                c.render_rows(frame, scenes[kind], W, H, 0, H, out)
                ev.append((a, b))
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in ev])
            med[kind + "_ms_median"] = float(np.median(ms))
            med[kind + "_ms_min"] = float(ms.min())
            med[kind + "_ms_iqr"] = float(np.subtract(*np.percentile(ms, [75, 25])))
        med["disk_on_over_off"] = med["disk_on_ms_median"] / med["disk_off_ms_median"]
        med["plain_ring_over_plain"] = med["plain_ring_ms_median"] / med["plain_ms_median"]
        (settling if alt < args.settle else blocks).append(med)
    # what the two disk frames draw (two more renders, untimed): the state-on frame's hits, both step totals
    hits = torch.zeros(W * H * 6, dtype=torch.float32, device=dev)
    total_on = torch.zeros(1, dtype=torch.int64, device=dev)
    total_off = torch.zeros(1, dtype=torch.int64, device=dev)
    ctxs["disk_on"].disk_hits_next_render(hits)
    ctxs["disk_on"].render_rows(frame, scenes["disk_on"], W, H, 0, H, out, None, None, None, total_on)
    ctxs["disk_off"].render_rows(frame, scenes["disk_off"], W, H, 0, H, out, None, None, None, total_off)
    torch.cuda.synchronize()
    hv = hits.view(H, W, 3, 2)[..., 0] > 0
    for c in ctxs.values():
        c.close()
    m = {k: np.array([b[k + "_ms_median"] for b in blocks]) for k in ctxs}
    spread = {k: float((m[k].max() - m[k].min()) / np.median(m[k])) for k in ("disk_off", "plain")}
    on_off = float(np.median(m["disk_on"]) / np.median(m["disk_off"]))
    ring_plain = float(np.median(m["plain_ring"]) / np.median(m["plain"]))
    res = {
        "config": "cfg3_4k", "width": W, "height": H, "max_steps": cfg.max_steps, "disk": [r_in, r_out],
        "n": args.n, "warmup": args.warmup, "settling_alternations_not_counted": settling, "alternations": blocks,
        **{k + "_ms_median": float(np.median(v)) for k, v in m.items()},
        "disk_on_over_off": on_off,
        "disk_on_over_off_min": float(min(b["disk_on_over_off"] for b in blocks)),
        "disk_on_over_off_max": float(max(b["disk_on_over_off"] for b in blocks)),
        "disk_off_alternation_spread": spread["disk_off"],
        "disk_cost_beyond_twice_the_spread": bool(abs(on_off - 1.0) > 2.0 * spread["disk_off"]),
        "plain_ring_over_plain": ring_plain,
        "plain_alternation_spread": spread["plain"],
        "plain_cost_beyond_twice_the_spread": bool(abs(ring_plain - 1.0) > 2.0 * spread["plain"]),
        "hit_pixels_per_slot": [int(hv[..., k].sum()) for k in range(3)],
        "steps_total_on": int(total_on.item()), "steps_total_off": int(total_off.item()),
        "timing": "geo_time_next_render event pairs on each kernel dispatch; blocks of n renders of the disk frame with "
                  "the state off, with it on, the plain frame and the plain GEO_FLAG_RING_F64 frame alternate in one "
                  "process, each kind on its own context; spread = (max - min) / median of a kind's alternation medians",
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def adaptive_session(args, cfg, frame, scenes, sky, tex):
    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    W, H = cfg.width, cfg.height
    r_in, r_out = 1.6 * cfg.rs, 2.2 * cfg.rs
    # (each kind on its own context: the learned dispatch order is kept per context)
    ctxs = {}
    for kind in scenes:
        c = g.Context(0)
        c.set_sky(sky)
        if kind.startswith("disk"):
            c.set_disk(tex, r_in, r_out)
        ctxs[kind] = c
    dev = torch.device("cuda:0")
    out = torch.empty(W * H * 4, dtype=torch.uint8, device=dev)

    def run(kind):
        if kind == "disk_adaptive":
            ctxs[kind].render_disk_adaptive(frame, scenes[kind], W, H, H, 0, H, 1, out)
        else:
            ctxs[kind].render_rows(frame, scenes[kind], W, H, 0, H, out)

    for _ in range(args.warmup):
        for kind in ctxs:
            run(kind)
    torch.cuda.synchronize()
    blocks, settling = [], []
    for alt in range(args.settle + args.alternations):
        med = {}
        for kind, c in ctxs.items():
            ev = []
            for _ in range(args.n):
                a, b = HipEvent(), HipEvent()
                c.time_next_render(a, b)
                run(kind)
                ev.append((a, b))
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in ev])
            med[kind + "_ms_median"] = float(np.median(ms))
            med[kind + "_ms_min"] = float(ms.min())
            med[kind + "_ms_iqr"] = float(np.subtract(*np.percentile(ms, [75, 25])))
        med["disk_adaptive_over_plain_adaptive"] = med["disk_adaptive_ms_median"] / med["plain_adaptive_ms_median"]
        med["disk_direct_over_plain_direct"] = med["disk_direct_ms_median"] / med["plain_direct_ms_median"]
        (settling if alt < args.settle else blocks).append(med)
    # what the adaptive disk frame draws (untimed): its hits, and both adaptive frames' attempts
    hits = torch.zeros(W * H * 6, dtype=torch.float32, device=dev)
    tot_d = torch.zeros(1, dtype=torch.int64, device=dev)
    tot_p = torch.zeros(1, dtype=torch.int64, device=dev)
    ctxs["disk_adaptive"].disk_hits_next_render(hits)
    ctxs["disk_adaptive"].render_disk_adaptive(frame, scenes["disk_adaptive"], W, H, H, 0, H, 1, out, None, None, None,
                                               tot_d)
    ctxs["plain_adaptive"].render_rows(frame, scenes["plain_adaptive"], W, H, 0, H, out, None, None, None, tot_p)
    torch.cuda.synchronize()
    hv = hits.view(H, W, 3, 2)[..., 0] > 0
    for c in ctxs.values():
        c.close()
    m = {k: np.array([b[k + "_ms_median"] for b in blocks]) for k in ctxs}
    spread = {k: float((m[k].max() - m[k].min()) / np.median(m[k])) for k in ("plain_adaptive", "plain_direct")}
    ratio = float(np.median(m["disk_adaptive"]) / np.median(m["plain_adaptive"]))
    return {
        "settling_alternations_not_counted": settling, "alternations": blocks,
        **{k + "_ms_median": float(np.median(v)) for k, v in m.items()},
        "disk_adaptive_over_plain_adaptive": ratio,
        "disk_adaptive_over_plain_adaptive_min": float(min(b["disk_adaptive_over_plain_adaptive"] for b in blocks)),
        "disk_adaptive_over_plain_adaptive_max": float(max(b["disk_adaptive_over_plain_adaptive"] for b in blocks)),
        "surplus_ms_per_frame": float(np.median(m["disk_adaptive"]) - np.median(m["plain_adaptive"])),
        "plain_adaptive_alternation_spread": spread["plain_adaptive"],
        "surplus_beyond_twice_the_spread": bool(abs(ratio - 1.0) > 2.0 * spread["plain_adaptive"]),
        "disk_direct_over_plain_direct": float(np.median(m["disk_direct"]) / np.median(m["plain_direct"])),
        "plain_direct_alternation_spread": spread["plain_direct"],
        "hit_pixels_per_slot": [int(hv[..., k].sum()) for k in range(3)],
        "attempts_total_disk_adaptive": int(tot_d.item()), "attempts_total_plain_adaptive": int(tot_p.item()),
    }


def adaptive_main(args):
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, make_disk_texture, make_sky

    if not torch.cuda.is_available():
        raise SystemExit("bench_disk.py needs a HIP device")
    cfg, cfg5 = CONFIGS["cfg3_4k"], CONFIGS["cfg5_8k_adaptive"]
    obs = g.Observer(cfg.rs, cfg.fov, cfg.width, cfg.height)
    obs.set_position(*cfg.position)
    obs.set_camera(*cfg.camera)
    obs.set_energy(cfg.energy)
    frame = obs.calc_transformation_pipeline()
    r = obs.get_radial_position()
    A, D = _lib.GEO_MODE_ADAPTIVE, _lib.GEO_MODE_DIRECT
    scenes = {
        "plain_adaptive": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg5.step, cfg5.max_steps, A, 0, cfg5.tol),
        "disk_adaptive": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg5.step, cfg5.max_steps, A, _lib.GEO_FLAG_DISK, cfg5.tol),
        "plain_direct": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg.step, cfg.max_steps, D, 0),
        "disk_direct": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg.step, cfg.max_steps, D, _lib.GEO_FLAG_DISK),
    }
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))
    res = {
        "config": "cfg3_4k's scene at cfg5_8k_adaptive's mode, step and tol", "width": cfg.width, "height": cfg.height,
        "step": cfg5.step, "tol": cfg5.tol, "max_steps": cfg5.max_steps, "disk": [1.6 * cfg.rs, 2.2 * cfg.rs],
        "n": args.n, "alternations": args.alternations, "settle": args.settle, "warmup": args.warmup,
        "timing": "geo_time_next_render event pairs on each kernel dispatch; blocks of n renders of the plain adaptive "
                  "frame, the adaptive disk frame, the plain direct frame and the direct disk frame alternate in one "
                  "process, each kind on its own context; spread = (max - min) / median of a kind's alternation "
                  "medians; a surplus is a figure only beyond twice the plain adaptive side's spread",
        "sessions": [adaptive_session(args, cfg, frame, scenes, sky, tex) for _ in range(args.sessions)],
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def adaptive_ring_session(args, cfg, frame, scenes, sky, tex):
    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent

    W, H = cfg.width, cfg.height
    # (each kind on its own context: the learned dispatch order is kept per context)
    ctxs = {}
    for kind in ("disk_off", "disk_on", "plain", "plain_ring"):
        c = g.Context(0)
        c.set_sky(sky)
        if kind.startswith("disk"):
            c.set_disk(tex, 1.6 * cfg.rs, 2.2 * cfg.rs)
            c.set_disk_ring_f64(kind == "disk_on")
        ctxs[kind] = c
    dev = torch.device("cuda:0")
    out = torch.empty(W * H * 4, dtype=torch.uint8, device=dev)

    def run(kind, total=None):
        c = ctxs[kind]
        if kind == "disk_on":
            c.render_disk_adaptive_ring(frame, scenes["disk"], W, H, H, 0, H, 1, out, None, None, None, total)
        elif kind == "disk_off":  # (the parent's kernel)
            c.render_disk_adaptive(frame, scenes["disk"], W, H, H, 0, H, 1, out, None, None, None, total)
        else:
            c.render_rows(frame, scenes[kind], W, H, 0, H, out, None, None, None, total)

    for _ in range(args.warmup):
        for kind in ctxs:
            run(kind)
    torch.cuda.synchronize()
    blocks, settling = [], []
    for alt in range(args.settle + args.alternations):
        med = {}
        for kind, c in ctxs.items():
            ev = []
            for _ in range(args.n):
                a, b = HipEvent(), HipEvent()
                c.time_next_render(a, b)
                run(kind)
                ev.append((a, b))
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in ev])
            med[kind + "_ms_median"] = float(np.median(ms))
            med[kind + "_ms_min"] = float(ms.min())
            med[kind + "_ms_iqr"] = float(np.subtract(*np.percentile(ms, [75, 25])))
        med["disk_on_over_off"] = med["disk_on_ms_median"] / med["disk_off_ms_median"]
        med["plain_ring_over_plain"] = med["plain_ring_ms_median"] / med["plain_ms_median"]
        (settling if alt < args.settle else blocks).append(med)
    # what the two disk frames draw (two more renders, untimed): the state-on frame's hits, both step totals
    hits = torch.zeros(W * H * 6, dtype=torch.float32, device=dev)
    total_on = torch.zeros(1, dtype=torch.int64, device=dev)
    total_off = torch.zeros(1, dtype=torch.int64, device=dev)
    ctxs["disk_on"].disk_hits_next_render(hits)
    run("disk_on", total_on)
    run("disk_off", total_off)
    torch.cuda.synchronize()
    hv = hits.view(H, W, 3, 2)[..., 0] > 0
    for c in ctxs.values():
        c.close()
    m = {k: np.array([b[k + "_ms_median"] for b in blocks]) for k in ctxs}
    spread = {k: float((m[k].max() - m[k].min()) / np.median(m[k])) for k in ("disk_off", "plain")}
    on_off = float(np.median(m["disk_on"]) / np.median(m["disk_off"]))
    ring_plain = float(np.median(m["plain_ring"]) / np.median(m["plain"]))
    return {
        "settling_alternations_not_counted": settling, "alternations": blocks,
        **{k + "_ms_median": float(np.median(v)) for k, v in m.items()},
        "disk_on_over_off": on_off,
        "disk_on_over_off_min": float(min(b["disk_on_over_off"] for b in blocks)),
        "disk_on_over_off_max": float(max(b["disk_on_over_off"] for b in blocks)),
        "disk_off_alternation_spread": spread["disk_off"],
        "disk_cost_beyond_twice_the_spread": bool(abs(on_off - 1.0) > 2.0 * spread["disk_off"]),
        "plain_ring_over_plain": ring_plain,
        "plain_alternation_spread": spread["plain"],
        "plain_cost_beyond_twice_the_spread": bool(abs(ring_plain - 1.0) > 2.0 * spread["plain"]),
        "hit_pixels_per_slot": [int(hv[..., k].sum()) for k in range(3)],
        # (mixed units with the state on: adaptive attempts outside the band, fixed f64 steps inside it)
        "steps_total_on": int(total_on.item()), "attempts_total_off": int(total_off.item()),
    }


def adaptive_ring_main(args):
    import math

    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, make_disk_texture, make_sky

    if not torch.cuda.is_available():
        raise SystemExit("bench_disk.py needs a HIP device")
    cfg, cfg5 = CONFIGS["cfg3_4k"], CONFIGS["cfg5_8k_adaptive"]
    obs = g.Observer(cfg.rs, cfg.fov, cfg.width, cfg.height)
    obs.set_position(*cfg.position)
    obs.set_camera(cfg.camera[0] + (math.pi if args.camera_away else 0.0), cfg.camera[1])
    obs.set_energy(cfg.energy)
    frame = obs.calc_transformation_pipeline()
    r = obs.get_radial_position()
    A = _lib.GEO_MODE_ADAPTIVE
    scenes = {
        "plain": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg5.step, cfg5.max_steps, A, 0, cfg5.tol),
        "plain_ring": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg5.step, cfg5.max_steps, A, _lib.GEO_FLAG_RING_F64,
                                   cfg5.tol),
        "disk": g.make_scene(cfg.rs, cfg.sphere_r, r, cfg5.step, cfg5.max_steps, A, _lib.GEO_FLAG_DISK, cfg5.tol),
    }
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))
    res = {
        "config": "cfg3_4k's scene at cfg5_8k_adaptive's mode, step and tol" + (
            ", the camera turned by pi (no band pixel)" if args.camera_away else ""),
        "width": cfg.width, "height": cfg.height,
        "step": cfg5.step, "tol": cfg5.tol, "max_steps": cfg5.max_steps, "disk": [1.6 * cfg.rs, 2.2 * cfg.rs],
        "n": args.n, "alternations": args.alternations, "settle": args.settle, "warmup": args.warmup,
        "timing": "geo_time_next_render event pairs on each kernel dispatch; blocks of n renders of the adaptive disk "
                  "frame with the state off (geo_render_disk_adaptive), with it on (geo_render_disk_adaptive_ring), the "
                  "plain adaptive frame and the plain adaptive GEO_FLAG_RING_F64 frame alternate in one process, each "
                  "kind on its own context; spread = (max - min) / median of a kind's alternation medians; a cost is a "
                  "figure only beyond twice its off side's spread",
        "sessions": [adaptive_ring_session(args, cfg, frame, scenes, sky, tex) for _ in range(args.sessions)],
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def batch_main(args):
    import ctypes

    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.dist import BandLayout
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, make_disk_texture, make_sky
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent, hipEventDefault

    K = args.batch
    if not 1 <= K <= _lib.GEO_MAX_BATCH_FRAMES:
        raise SystemExit(f"--batch: 1 .. {_lib.GEO_MAX_BATCH_FRAMES}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_disk.py needs a HIP device")
    cfg = CONFIGS["cfg3_4k"]
    W, H = cfg.width, cfg.height
    obs = g.Observer(cfg.rs, cfg.fov, W, H)
    obs.set_position(*cfg.position)
    obs.set_camera(*cfg.camera)
    obs.set_energy(cfg.energy)
    frame = obs.calc_transformation_pipeline()
    scene = g.make_scene(cfg.rs, cfg.sphere_r, obs.get_radial_position(), cfg.step, cfg.max_steps,
                         flags=_lib.GEO_FLAG_DISK)
    L = BandLayout(H, 8, 8, 1)  # a peer's share at N = 8
    band = (L.band_height(), L.row0(), L.cycle_rows, L.nbands())
    packed = L.packed_rows() * W * 4
    dev = torch.device("cuda:0")
    out = torch.empty(K * packed, dtype=torch.uint8, device=dev)
    sh = torch.cuda.current_stream().cuda_stream
    frames = (_lib.GeoFrame * K)(*([frame] * K))
    scenes = (_lib.GeoScene * K)(*([scene] * K))
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))

    def make_ctx(shift):
        c = g.Context(0)
        c.set_sky(sky)
        c.set_disk(tex, 1.6 * cfg.rs, 2.2 * cfg.rs)
        if shift:
            c.set_disk_shift(1, 4, 1.0)
        return c

    lib = _lib.lib

    def run_batch(c, pairs=None):
        if pairs is not None:
            c.time_next_render(*pairs[0])
        _lib.check("geo_render_disk_batch", lib.geo_render_disk_batch(
            c._h, frames, scenes, K, W, H, *band, out.data_ptr(), packed, None, sh))

    def run_singles(c, pairs=None):
        for k in range(K):
            if pairs is not None:
                c.time_next_render(*pairs[k])
            _lib.check("geo_render_band_set", lib.geo_render_band_set(
                c._h, ctypes.byref(frame), ctypes.byref(scene), W, H, *band, out.data_ptr() + k * packed, None, None,
                None, None, sh))

    # (each kind on its own context: the learned dispatch order is kept per context)
    kinds = []
    for shade in (False, True):
        tag = "shift" if shade else "disk"
        kinds.append((tag + "_batch", make_ctx(shade), run_batch, 1))
        kinds.append((tag + "_single", make_ctx(shade), run_singles, K))
    for _ in range(args.warmup):
        for _, c, run, _ in kinds:
            run(c)
    torch.cuda.synchronize()
    # pass 1: stream events around the launches
    ev = {k: [] for k, _, _, _ in kinds}
    for _ in range(args.n):
        for kind, c, run, _ in kinds:
            a, b = HipEvent(hipEventDefault), HipEvent(hipEventDefault)
            a.record(sh)
            run(c)
            b.record(sh)
            ev[kind].append((a, b))
        torch.cuda.synchronize()  # the next sample's launches queue behind nothing
    stream_ms = {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
    # pass 2: the kernel dispatches alone
    ev = {k: [] for k, _, _, _ in kinds}
    for _ in range(args.n):
        for kind, c, run, m in kinds:
            pairs = [(HipEvent(), HipEvent()) for _ in range(m)]
            run(c, pairs)
            ev[kind].append(pairs)
        torch.cuda.synchronize()
    disp_ms = {k: np.array([sum(a.elapsed_time(b) for a, b in pairs) for pairs in v]) for k, v in ev.items()}
    for _, c, _, _ in kinds:
        c.close()

    def stats(ms):
        return {"ms_per_frame_median": float(np.median(ms) / K), "ms_per_frame_min": float(ms.min() / K),
                "ms_per_frame_iqr": float(np.subtract(*np.percentile(ms, [75, 25])) / K)}

    res = {
        "config": "cfg3_4k", "width": W, "height": H, "max_steps": cfg.max_steps, "disk": [1.6 * cfg.rs, 2.2 * cfg.rs],
        "layout": {"world": 8, "rank": 1, "band_rows": band[0], "row0": band[1], "row_stride": band[2],
                   "nbands": band[3], "rows": L.rows_mine()},
        "frames_per_batch": K, "n": args.n, "warmup": args.warmup, "shift": [1, 4, 1.0],
        "stream_events": {k: stats(v) for k, v in stream_ms.items()},
        "dispatch_events": {k: stats(v) for k, v in disp_ms.items()},
        "timing": "stream_events: a pair of events on the stream around one launch of K frames, or around K one-frame "
                  "launches back to back; dispatch_events: geo_time_next_render pairs on the kernel dispatches, the K "
                  "one-frame times added; the four kinds alternate in one process",
    }
    for how, ms in (("stream_events", stream_ms), ("dispatch_events", disp_ms)):
        for tag in ("disk", "shift"):
            res[how][tag + "_batch_over_single"] = float(np.median(ms[tag + "_batch"]) / np.median(ms[tag + "_single"]))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def emission_batch_session(args, cfg, frame, scene, sky, tex, ramp, emission):
    import ctypes

    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.dist import BandLayout
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent, hipEventDefault

    K = args.batch
    W, H = cfg.width, cfg.height
    L = BandLayout(H, 8, 8, 1)  # a peer's share at N = 8
    band = (L.band_height(), L.row0(), L.cycle_rows, L.nbands())
    packed = L.packed_rows() * W * 4
    dev = torch.device("cuda:0")
    out = torch.empty(K * packed, dtype=torch.uint8, device=dev)
    sh = torch.cuda.current_stream().cuda_stream
    frames = (_lib.GeoFrame * K)(*([frame] * K))
    scenes = (_lib.GeoScene * K)(*([scene] * K))
    lib = _lib.lib

    def make_ctx(emit):
        c = g.Context(0)
        c.set_sky(sky)
        c.set_disk(tex, 1.6 * cfg.rs, 2.2 * cfg.rs)
        if emit:
            c.set_disk_emission(ramp, **emission)
        else:
            c.set_disk_shift(1, 4, 1.0)
        return c

    def run_batch(name):
        fn = getattr(lib, name)

        def run(c, pairs=None):
            if pairs is not None:
                c.time_next_render(*pairs[0])
            _lib.check(name, fn(c._h, frames, scenes, K, W, H, *band, out.data_ptr(), packed, None, sh))
        return run

    def run_singles(c, pairs=None):
        for k in range(K):
            if pairs is not None:
                c.time_next_render(*pairs[k])
            _lib.check("geo_render_band_set", lib.geo_render_band_set(
                c._h, ctypes.byref(frame), ctypes.byref(scene), W, H, *band, out.data_ptr() + k * packed, None, None,
                None, None, sh))

    # (each side on its own context: the learned dispatch order is kept per context)
    sides = [("emission_batch", make_ctx(True), run_batch("geo_render_emission_batch"), 1),
             ("emission_single", make_ctx(True), run_singles, K),
             ("shift_batch", make_ctx(False), run_batch("geo_render_disk_batch"), 1)]
    if args.shaded_first:
        # a sample's first launch starts on an idle stream and pays its wake-up inside the stream events' pair; the
        # launches behind it are queued while it runs: which batch is first decides a few microseconds between them
        sides.reverse()
    for _ in range(args.warmup):
        for _, c, run, _ in sides:
            run(c)
    torch.cuda.synchronize()
    res = {"layout": {"world": 8, "rank": 1, "band_rows": band[0], "row0": band[1], "row_stride": band[2],
                      "nbands": band[3], "rows": L.rows_mine()}}
    for how in ("stream_events", "dispatch_events"):
        # --settle alternations are run first in the timed form and kept apart, as --emission does: without them the
        # second alternation of a session's first timing ran 10-16 % slower for all three sides together, in two runs
        # out of two (profiles/disk_emission_batch_bench_cfg3_unsettled.json)
        med = {name: [] for name, *_ in sides}
        settling = {name: [] for name, *_ in sides}
        for alt in range(args.settle + args.alternations):
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
                (settling if alt < args.settle else med)[name].append(
                    float(np.median([sum(a.elapsed_time(b) for a, b in pairs) for pairs in v]) / K))
        b_m, s_m = float(np.median(med["emission_batch"])), float(np.median(med["emission_single"]))
        sb_m = float(np.median(med["shift_batch"]))
        spread = (max(med["emission_single"]) - min(med["emission_single"])) / s_m
        res[how] = {
            "settling_alternations_not_counted": settling,
            "emission_batch_ms_per_frame_medians": med["emission_batch"],
            "emission_single_ms_per_frame_medians": med["emission_single"],
            "shift_batch_ms_per_frame_medians": med["shift_batch"],
            "emission_batch_ms_per_frame": b_m, "emission_single_ms_per_frame": s_m, "shift_batch_ms_per_frame": sb_m,
            "batch_over_single": b_m / s_m, "single_spread": spread,
            "batch_spread": (max(med["emission_batch"]) - min(med["emission_batch"])) / b_m,
            # the batch is held to a saving of more than twice the one-frame side's own spread
            "margin": 1.0 - 2.0 * spread, "faster_by_more_than_margin": bool(b_m < s_m * (1.0 - 2.0 * spread)),
            "emission_batch_over_shift_batch": b_m / sb_m,
        }
    for _, c, *_ in sides:
        c.close()
    return res


def emission_batch_main(args):
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, blackbody_ramp, make_disk_texture, make_sky

    K = args.batch
    if not 1 <= K <= _lib.GEO_MAX_BATCH_FRAMES:
        raise SystemExit(f"--batch: 1 .. {_lib.GEO_MAX_BATCH_FRAMES}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_disk.py needs a HIP device")
    cfg = CONFIGS["cfg3_4k"]
    obs = g.Observer(cfg.rs, cfg.fov, cfg.width, cfg.height)
    obs.set_position(*cfg.position)
    obs.set_camera(*cfg.camera)
    obs.set_energy(cfg.energy)
    frame = obs.calc_transformation_pipeline()
    scene = g.make_scene(cfg.rs, cfg.sphere_r, obs.get_radial_position(), cfg.step, cfg.max_steps,
                         flags=_lib.GEO_FLAG_DISK)
    emission = dict(t_ref=9000.0, t_lo=1500.0, t_hi=30000.0, profile=_lib.GEO_DISK_PROFILE_THIN, exposure=1.0, spin=1)
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))
    ramp = blackbody_ramp(256, emission["t_lo"], emission["t_hi"])
    res = {
        "config": "cfg3_4k", "width": cfg.width, "height": cfg.height, "max_steps": cfg.max_steps,
        "disk": [1.6 * cfg.rs, 2.2 * cfg.rs], "emission": emission, "ramp_entries": 256, "shift": [1, 4, 1.0],
        "frames_per_batch": K, "n": args.n, "alternations": args.alternations, "settle": args.settle,
        "order_in_a_sample": ["shift_batch", "emission_single", "emission_batch"] if args.shaded_first else [
            "emission_batch", "emission_single", "shift_batch"],
        "warmup": args.warmup,
        "timing": "stream_events: a pair of events on the stream around one launch of K frames, or around K one-frame "
                  "launches back to back; dispatch_events: geo_time_next_render pairs on the kernel dispatches, the K "
                  "one-frame times added; emission_batch (geo_render_emission_batch), emission_single (K "
                  "geo_render_band_set launches, the yardstick) and shift_batch (the shaded geo_render_disk_batch on "
                  "the same layout) alternate, each on its own context; per alternation the median of n, after settle "
                  "alternations of each timing that are kept apart; spread = "
                  "(max - min) / median of a side's alternation medians; margin = 1 - 2 x the one-frame side's spread",
        "sessions": [emission_batch_session(args, cfg, frame, scene, sky, tex, ramp, emission)
                     for _ in range(args.sessions)],
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def ring_batch_session(args, cfg, frame, scene, sky, tex):
    import ctypes

    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.dist import BandLayout
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent, hipEventDefault

    K = args.batch
    W, H = cfg.width, cfg.height
    L = BandLayout(H, 8, 8, 1)  # a peer's share at N = 8
    band = (L.band_height(), L.row0(), L.cycle_rows, L.nbands())
    packed = L.packed_rows() * W * 4
    dev = torch.device("cuda:0")
    out = torch.empty(K * packed, dtype=torch.uint8, device=dev)
    sh = torch.cuda.current_stream().cuda_stream
    frames = (_lib.GeoFrame * K)(*([frame] * K))
    scenes = (_lib.GeoScene * K)(*([scene] * K))
    lib = _lib.lib

    def make_ctx():
        c = g.Context(0)
        c.set_sky(sky)
        c.set_disk(tex, 1.6 * cfg.rs, 2.2 * cfg.rs)
        c.set_disk_ring_f64(True)
        return c

    def run_batch(c, pairs=None):
        if pairs is not None:
            c.time_next_render(*pairs[0])
        _lib.check("geo_render_disk_ring_batch", lib.geo_render_disk_ring_batch(
            c._h, frames, scenes, K, W, H, *band, out.data_ptr(), packed, None, sh))

    def run_singles(c, pairs=None):
        for k in range(K):
            if pairs is not None:
                c.time_next_render(*pairs[k])
            _lib.check("geo_render_band_set", lib.geo_render_band_set(
                c._h, ctypes.byref(frame), ctypes.byref(scene), W, H, *band, out.data_ptr() + k * packed, None, None,
                None, None, sh))

    # (each side on its own context: the learned dispatch order is kept per context)
    sides = [("ring_batch", make_ctx(), run_batch, 1), ("ring_single", make_ctx(), run_singles, K)]
    for _ in range(args.warmup):
        for _, c, run, _ in sides:
            run(c)
    torch.cuda.synchronize()
    res = {"layout": {"world": 8, "rank": 1, "band_rows": band[0], "row0": band[1], "row_stride": band[2],
                      "nbands": band[3], "rows": L.rows_mine()}}
    for how in ("stream_events", "dispatch_events"):
        med = {name: [] for name, *_ in sides}
        settling = {name: [] for name, *_ in sides}
        for alt in range(args.settle + args.alternations):
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
                (settling if alt < args.settle else med)[name].append(
                    float(np.median([sum(a.elapsed_time(b) for a, b in pairs) for pairs in v]) / K))
        b_m, s_m = float(np.median(med["ring_batch"])), float(np.median(med["ring_single"]))
        spread = (max(med["ring_single"]) - min(med["ring_single"])) / s_m
        res[how] = {
            "settling_alternations_not_counted": settling,
            "ring_batch_ms_per_frame_medians": med["ring_batch"],
            "ring_single_ms_per_frame_medians": med["ring_single"],
            "ring_batch_ms_per_frame": b_m, "ring_single_ms_per_frame": s_m,
            "batch_over_single": b_m / s_m, "single_spread": spread,
            "batch_spread": (max(med["ring_batch"]) - min(med["ring_batch"])) / b_m,
            # the batch is held to a saving of more than twice the one-frame side's own spread
            "margin": 1.0 - 2.0 * spread, "faster_by_more_than_margin": bool(b_m < s_m * (1.0 - 2.0 * spread)),
        }
    for _, c, *_ in sides:
        c.close()
    return res


def ring_batch_main(args):
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, make_disk_texture, make_sky

    K = args.batch
    if not 1 <= K <= _lib.GEO_MAX_BATCH_FRAMES:
        raise SystemExit(f"--batch: 1 .. {_lib.GEO_MAX_BATCH_FRAMES}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_disk.py needs a HIP device")
    cfg = CONFIGS["cfg3_4k"]
    obs = g.Observer(cfg.rs, cfg.fov, cfg.width, cfg.height)
    obs.set_position(*cfg.position)
    obs.set_camera(*cfg.camera)
    obs.set_energy(cfg.energy)
    frame = obs.calc_transformation_pipeline()
    scene = g.make_scene(cfg.rs, cfg.sphere_r, obs.get_radial_position(), cfg.step, cfg.max_steps,
                         flags=_lib.GEO_FLAG_DISK)
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))
    res = {
        "config": "cfg3_4k", "width": cfg.width, "height": cfg.height, "max_steps": cfg.max_steps,
        "disk": [1.6 * cfg.rs, 2.2 * cfg.rs], "disk_ring_f64": True,
        "frames_per_batch": K, "n": args.n, "alternations": args.alternations, "settle": args.settle,
        "order_in_a_sample": ["ring_batch", "ring_single"], "warmup": args.warmup,
        "timing": "stream_events: a pair of events on the stream around one geo_render_disk_ring_batch call of K frames "
                  "(the band-table kernel and the render launch), or around K one-frame geo_render_band_set launches "
                  "back to back; dispatch_events: geo_time_next_render pairs on the render dispatches alone, the K "
                  "one-frame times added; the two sides alternate, each on its own context; per alternation the median "
                  "of n, after settle alternations of each timing that are kept apart; spread = (max - min) / median of "
                  "a side's alternation medians; margin = 1 - 2 x the one-frame side's spread",
        "sessions": [ring_batch_session(args, cfg, frame, scene, sky, tex) for _ in range(args.sessions)],
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def adaptive_batch_session(args, cfg, frame, scene, sky, tex, ramp, emission):
    import ctypes

    import numpy as np
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.dist import BandLayout
    from schwarzschild_raytracer_wgpu_amd.timing import HipEvent, hipEventDefault

    K = args.batch
    W, H = cfg.width, cfg.height
    L = BandLayout(H, 8, 8, 1)  # a peer's share at N = 8
    band = (L.band_height(), L.row0(), L.cycle_rows, L.nbands())
    packed = L.packed_rows() * W * 4
    dev = torch.device("cuda:0")
    out = torch.empty(K * packed, dtype=torch.uint8, device=dev)
    sh = torch.cuda.current_stream().cuda_stream
    frames = (_lib.GeoFrame * K)(*([frame] * K))
    scenes = (_lib.GeoScene * K)(*([scene] * K))
    lib = _lib.lib
    # --ring: the same sides with geo_set_disk_ring_f64 on, through the calls that draw the band
    batch_name = "geo_render_disk_adaptive_ring_batch" if args.ring else "geo_render_disk_adaptive_batch"
    single_name = "geo_render_disk_adaptive_ring" if args.ring else "geo_render_disk_adaptive"
    batch_fn, single_fn = getattr(lib, batch_name), getattr(lib, single_name)

    def make_ctx(emit):
        c = g.Context(0)
        c.set_sky(sky)
        c.set_disk(tex, 1.6 * cfg.rs, 2.2 * cfg.rs)
        if emit:
            c.set_disk_emission(ramp, **emission)
        c.set_disk_ring_f64(bool(args.ring))
        return c

    def run_batch(c, pairs=None):
        if pairs is not None:
            c.time_next_render(*pairs[0])
        _lib.check(batch_name, batch_fn(c._h, frames, scenes, K, W, H, *band, out.data_ptr(), packed, None, sh))

    def run_singles(c, pairs=None):
        for k in range(K):
            if pairs is not None:
                c.time_next_render(*pairs[k])
            _lib.check(single_name, single_fn(
                c._h, ctypes.byref(frame), ctypes.byref(scene), W, H, *band, out.data_ptr() + k * packed, None, None,
                None, None, sh))

    # (each side on its own context: the learned dispatch order is kept per context)
    sides = [("plain_batch", make_ctx(False), run_batch, 1), ("plain_single", make_ctx(False), run_singles, K),
             ("emission_batch", make_ctx(True), run_batch, 1), ("emission_single", make_ctx(True), run_singles, K)]
    for _ in range(args.warmup):
        for _, c, run, _ in sides:
            run(c)
    torch.cuda.synchronize()
    res = {"layout": {"world": 8, "rank": 1, "band_rows": band[0], "row0": band[1], "row_stride": band[2],
                      "nbands": band[3], "rows": L.rows_mine()}}
    for how in ("stream_events", "dispatch_events"):
        med = {name: [] for name, *_ in sides}
        settling = {name: [] for name, *_ in sides}
        for alt in range(args.settle + args.alternations):
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
                (settling if alt < args.settle else med)[name].append(
                    float(np.median([sum(a.elapsed_time(b) for a, b in pairs) for pairs in v]) / K))
        res[how] = {"settling_alternations_not_counted": settling}
        for tag in ("plain", "emission"):
            bm, sm = med[tag + "_batch"], med[tag + "_single"]
            b_m, s_m = float(np.median(bm)), float(np.median(sm))
            spread = (max(sm) - min(sm)) / s_m
            res[how][tag] = {
                "batch_ms_per_frame_medians": bm, "single_ms_per_frame_medians": sm,
                "batch_ms_per_frame": b_m, "single_ms_per_frame": s_m,
                "batch_over_single": b_m / s_m, "single_spread": spread, "batch_spread": (max(bm) - min(bm)) / b_m,
                # the batch is held to a saving of more than twice the one-frame side's own spread
                "margin": 1.0 - 2.0 * spread, "faster_by_more_than_margin": bool(b_m < s_m * (1.0 - 2.0 * spread)),
            }
    # what the frames draw (untimed): the attempts of one batch and of its K one-frame renders
    tot_b = torch.zeros(1, dtype=torch.int64, device=dev)
    tot_s = torch.zeros(1, dtype=torch.int64, device=dev)
    c = sides[0][1]
    _lib.check(batch_name, batch_fn(c._h, frames, scenes, K, W, H, *band, out.data_ptr(), packed, tot_b.data_ptr(), sh))
    for k in range(K):
        _lib.check(single_name, single_fn(
            c._h, ctypes.byref(frame), ctypes.byref(scene), W, H, *band, out.data_ptr() + k * packed, None, None, None,
            tot_s.data_ptr(), sh))
    torch.cuda.synchronize()
    # (--ring: mixed units, adaptive attempts outside the band and fixed f64 steps inside it)
    res["attempts_total_batch"], res["attempts_total_singles"] = int(tot_b.item()), int(tot_s.item())
    if args.ring:  # the band's share of the frames: the same frames' attempts with the state off
        c.set_disk_ring_f64(False)
        tot_o = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.check("geo_render_disk_adaptive_batch", lib.geo_render_disk_adaptive_batch(
            c._h, frames, scenes, K, W, H, *band, out.data_ptr(), packed, tot_o.data_ptr(), sh))
        torch.cuda.synchronize()
        res["attempts_total_batch_state_off"] = int(tot_o.item())
    for _, c, *_ in sides:
        c.close()
    return res


def adaptive_batch_main(args):
    import torch

    import schwarzschild_raytracer_wgpu_amd as g
    from schwarzschild_raytracer_wgpu_amd import _lib
    from schwarzschild_raytracer_wgpu_amd.scenes import CONFIGS, blackbody_ramp, make_disk_texture, make_sky

    K = args.batch
    if not 1 <= K <= _lib.GEO_MAX_BATCH_FRAMES:
        raise SystemExit(f"--batch: 1 .. {_lib.GEO_MAX_BATCH_FRAMES}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_disk.py needs a HIP device")
    cfg, cfg5 = CONFIGS["cfg3_4k"], CONFIGS["cfg5_8k_adaptive"]
    obs = g.Observer(cfg.rs, cfg.fov, cfg.width, cfg.height)
    obs.set_position(*cfg.position)
    obs.set_camera(*cfg.camera)
    obs.set_energy(cfg.energy)
    frame = obs.calc_transformation_pipeline()
    scene = g.make_scene(cfg.rs, cfg.sphere_r, obs.get_radial_position(), cfg5.step, cfg5.max_steps,
                         _lib.GEO_MODE_ADAPTIVE, _lib.GEO_FLAG_DISK, cfg5.tol)
    emission = dict(t_ref=9000.0, t_lo=1500.0, t_hi=30000.0, profile=_lib.GEO_DISK_PROFILE_THIN, exposure=1.0, spin=1)
    sky, tex = make_sky(cfg.sky, cfg.sky_size), make_disk_texture((1024, 128))
    ramp = blackbody_ramp(256, emission["t_lo"], emission["t_hi"])
    res = {
        "config": "cfg3_4k's scene at cfg5_8k_adaptive's mode, step and tol", "width": cfg.width, "height": cfg.height,
        "step": cfg5.step, "tol": cfg5.tol, "max_steps": cfg5.max_steps, "disk": [1.6 * cfg.rs, 2.2 * cfg.rs],
        "emission": emission, "ramp_entries": 256,
        "frames_per_batch": K, "n": args.n, "alternations": args.alternations, "settle": args.settle,
        "order_in_a_sample": ["plain_batch", "plain_single", "emission_batch", "emission_single"],
        "warmup": args.warmup,
        "ring_f64": bool(args.ring),
        "calls": (["geo_render_disk_adaptive_ring_batch", "geo_render_disk_adaptive_ring"] if args.ring else
                  ["geo_render_disk_adaptive_batch", "geo_render_disk_adaptive"]),
        "timing": "stream_events: a pair of events on the stream around one batched call (calls[0]) of K "
                  "frames, or around K one-frame launches (calls[1]) back to back; dispatch_events: "
                  "geo_time_next_render pairs on the render dispatches alone, the K one-frame times added; the four "
                  "sides (unshaded and emission, batch and one-frame) alternate, each on its own context; per "
                  "alternation the median of n, after settle alternations of each timing that are kept apart; spread = "
                  "(max - min) / median of a side's alternation medians; margin = 1 - 2 x the one-frame side's spread",
        "sessions": [adaptive_batch_session(args, cfg, frame, scene, sky, tex, ramp, emission)
                     for _ in range(args.sessions)],
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
