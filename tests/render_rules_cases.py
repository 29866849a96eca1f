"""The matrix of render calls that pins csrc/geo_render_rules.h: every case as
a record of tests/native/render_rules_host.cpp's RuleCase, enumerated in a
fixed order (tests/golden/render_rules_matrix.npz holds each case's status and
launcher in that order; tests/golden/make_render_rules_matrix.py writes it).

blocks() yields (name, cases): first the full product, one block per entry
point and frame count, then the inputs varied one at a time over a smaller
base (BASE_FLAGS x BASE_STATES x the three modes x every entry point)."""
import ctypes
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "render_rules_host.cpp")
SO = os.path.join(HERE, "native", "librender_rules_host.so")
CSRC = os.path.join(HERE, "..", "schwarzschild_raytracer_wgpu_amd", "csrc")
GXX_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-msse4.1", "-Wno-unknown-pragmas"]

ENTRIES = ("geo_render_rows", "geo_render_bands", "geo_render_band_set", "geo_render_disk_adaptive",
           "geo_render_band_set_frames", "geo_render_band_set_batch", "geo_render_disk_batch", "geo_render_ss_batch",
           "geo_render_emission_batch", "geo_render_disk_ring_batch", "geo_render_disk_adaptive_batch")
ONE_FRAME = 4  # the first four take one frame (and the side outputs)
LAUNCHERS = ("launch_frames", "launch_fan", "launch_disk_frame", "launch_ss_frame", "launch_disk_frames",
             "launch_ss_frames", "launch_emit_frames", "launch_ring_frames", "launch_adaptive_frames")
GEO_OK, GEO_EINVAL, GEO_ESTATE = 0, -1, -5
DEFER, COMPOSITE, MIPS, RING_F64, DISK, SS4 = 1, 2, 4, 8, 16, 32

SCENE = np.dtype([("rs", "f4"), ("sphere_r", "f4"), ("r_obs", "f4"), ("step", "f4"), ("max_steps", "u4"),
                  ("mode", "u4"), ("flags", "u4"), ("tol", "f4")])
CASE = np.dtype([("entry", "u4"), ("nframes", "u4"), ("alt_frame", "u4"), ("nulls", "u4"), ("side", "u4"),
                 ("armed", "u4"), ("steps_total", "u4"), ("width", "u4"), ("height", "u4"), ("g", "u4", (4,)),
                 ("out_frame_stride", "u4"), ("sky", "u4"), ("n_fan", "u4"), ("disk_set", "u4"), ("shift_set", "u4"),
                 ("emit_set", "u4"), ("disk_ring", "u4"), ("r_in", "f4"), ("r_out", "f4"), ("scene", SCENE, (2,))])

# the frame of every case unless it is what varies: one tile wide, two 8-row bands
WIDTH, HEIGHT, BAND_ROWS, NBANDS = 32, 16, 8, 2
MAX_STEPS = 64
MODES = (0, 1, 2, 3)  # direct, fan, adaptive, no such mode
FLAGS = tuple(range(64)) + (64, 64 | DISK)
ARMED = (0, 1, 2, 4)
SIDE = (0, 1)
# rs, r_obs, r_in: flat space; the observer outside; inside the horizon; r_in <= 1.5 rs
GEOMETRIES = ((0.0, 10.0, 3.0), (1.0, 10.0, 3.0), (1.0, 0.5, 3.0), (1.0, 10.0, 1.4))
R_OUT, SPHERE_R = 20.0, 50.0
BASE_FLAGS = (0, DISK, SS4, DISK | SS4, DEFER, MIPS, DISK | DEFER, RING_F64)
BASE_STATES = (0, 1, 1 | 2, 1 | 4, 1 | 8, 15)  # bits: disk, shift, emission, ring


def geometry(c, band_rows=BAND_ROWS, row0=0, row_stride=BAND_ROWS, nbands=NBANDS):
    """The entry points' own row arguments for bands of band_rows rows at row0 + j row_stride."""
    e = c["entry"]
    z = np.zeros_like(e)
    br = max(band_rows, 1)
    c["g"] = np.where((e == 0)[:, None], np.stack([z + row0, z + nbands * band_rows, z, z], 1),
                      np.where((e == 1)[:, None], np.stack([z + band_rows, z + row0 // br, z + row_stride // br,
                                                            z + nbands], 1),
                               np.stack([z + band_rows, z + row0, z + row_stride, z + nbands], 1)))


def defaults(n, entry, nframes):
    c = np.zeros(n, CASE)
    c["entry"] = entry
    c["nframes"] = nframes
    c["alt_frame"] = 1
    c["width"], c["height"] = WIDTH, HEIGHT
    geometry(c)
    c["out_frame_stride"] = NBANDS * BAND_ROWS * WIDTH * 4
    c["sky"], c["n_fan"] = 1, 400
    c["r_in"], c["r_out"] = 3.0, R_OUT
    for f in (0, 1):
        s = c["scene"][:, f]
        s["rs"], s["sphere_r"], s["r_obs"] = 1.0, SPHERE_R, 10.0
        s["step"], s["max_steps"] = math.pi / 100, MAX_STEPS
    return c


def set_scene(c, **kw):
    """Fields of every frame's scene."""
    for k, v in kw.items():
        c["scene"][k] = np.asarray(v)[..., None] if np.ndim(v) else v


def set_state(c, bits):
    for i, k in enumerate(("disk_set", "shift_set", "emit_set", "disk_ring")):
        c[k] = (np.asarray(bits) >> i) & 1


def product_block(entry, nframes):
    dims = (len(MODES), len(FLAGS), 16, len(ARMED), len(SIDE), len(GEOMETRIES))
    n = int(np.prod(dims))
    mode, flags, state, armed, side, geo = np.unravel_index(np.arange(n), dims)
    c = defaults(n, entry, nframes)
    gm = np.asarray(GEOMETRIES, np.float32)[geo]
    set_scene(c, mode=np.asarray(MODES)[mode], flags=np.asarray(FLAGS)[flags], rs=gm[:, 0], r_obs=gm[:, 1])
    c["r_in"] = gm[:, 2]
    set_state(c, state)
    c["armed"] = np.asarray(ARMED)[armed]
    c["side"] = np.asarray(SIDE)[side]
    return c


def base_block():
    """The base of the one-at-a-time variations: every entry point (the batched ones with two frames)."""
    dims = (len(ENTRIES), 3, len(BASE_FLAGS), len(BASE_STATES))
    n = int(np.prod(dims))
    entry, mode, flags, state = np.unravel_index(np.arange(n), dims)
    c = defaults(n, entry, np.where(entry < ONE_FRAME, 1, 2))
    set_scene(c, mode=mode, flags=np.asarray(BASE_FLAGS)[flags])
    set_state(c, np.asarray(BASE_STATES)[state])
    return c


def frame1(**kw):
    def f(c):
        for k, v in kw.items():
            c["scene"][:, 1][k] = v(c["scene"][:, 0][k]) if callable(v) else v
    return f


def top(**kw):
    def f(c):
        for k, v in kw.items():
            c[k] = v
    return f


def scene(**kw):
    return lambda c: set_scene(c, **kw)


def geom(**kw):
    return lambda c: geometry(c, **kw)


def both(*fs):
    def f(c):
        for g in fs:
            g(c)
    return f


# name -> what it changes of the base; the order is the matrix's
VARIATIONS = (
    ("sky unset", top(sky=0)),
    ("fan unset", top(n_fan=0)),
    ("a fan of one node", top(n_fan=1)),
    ("tol negative", scene(tol=-1e-6)),
    ("tol positive", scene(tol=1e-5)),
    ("tol infinite", scene(tol=np.inf)),
    ("tol nan", scene(tol=np.nan)),
    ("steps_total given", top(steps_total=1)),
    ("max_steps 2^24", scene(max_steps=1 << 24)),
    ("max_steps 2^24 + 1", scene(max_steps=(1 << 24) + 1)),
    ("step 0", scene(step=0.0)),
    ("r_obs 0", scene(r_obs=0.0)),
    ("sphere_r 0", scene(sphere_r=0.0)),
    ("rs negative", scene(rs=-1.0)),
    ("r_out = sphere_r", top(r_out=SPHERE_R)),
    ("r_obs = sphere_r", scene(r_obs=SPHERE_R)),
    ("odd row0", geom(row0=1, nbands=1)),
    ("odd row_stride", geom(row_stride=9, nbands=1)),
    ("out_frame_stride short by 4", top(out_frame_stride=NBANDS * BAND_ROWS * WIDTH * 4 - 4)),
    ("out_frame_stride misaligned by 2", top(out_frame_stride=NBANDS * BAND_ROWS * WIDTH * 4 + 2)),
    ("nframes 0", top(nframes=0)),
    ("nframes 9", top(nframes=9)),
    ("nframes 8, frame 7 inside the horizon", both(top(nframes=8, alt_frame=7), frame1(r_obs=0.9))),
    ("null context", top(nulls=1)),
    ("null frames", top(nulls=2)),
    ("null scene", top(nulls=4)),
    ("null out_rgba8", top(nulls=8)),
    ("out_uv given", top(side=2)),
    ("out_steps given", top(side=4)),
    ("band_rows 0", geom(band_rows=0)),
    ("band_rows 4", geom(band_rows=4)),
    ("band_rows 12", geom(band_rows=12, row_stride=12, nbands=1)),
    ("band_rows 4104", geom(band_rows=4104, row_stride=4104, nbands=1)),
    ("band_rows 8192", geom(band_rows=8192, row_stride=8192, nbands=1)),
    ("row_stride below band_rows", geom(row_stride=4)),
    ("nbands 0", geom(nbands=0)),
    ("band_step 0", geom(row_stride=0)),
    ("a last band past the frame", geom(nbands=3)),
    ("row0 past the frame", geom(row0=16, nbands=1)),
    ("2^20 + 8 rows", both(top(height=1 << 20), geom(nbands=(1 << 17) + 1))),
    ("width 0", top(width=0)),
    ("width 2^20 + 1", top(width=(1 << 20) + 1)),
    ("height 2^20 + 1", top(height=(1 << 20) + 1)),
    ("width 2^19 + 1", top(width=(1 << 19) + 1, out_frame_stride=NBANDS * BAND_ROWS * ((1 << 19) + 1) * 4)),
    ("height 2^19 + 1", top(height=(1 << 19) + 1)),
    ("frame 1: rs differs", frame1(rs=0.9)),
    ("frame 1: sphere_r differs", frame1(sphere_r=49.0)),
    ("frame 1: r_obs differs", frame1(r_obs=11.0)),
    ("frame 1: step differs", frame1(step=lambda s: s * 0.5)),
    ("frame 1: max_steps differs", frame1(max_steps=MAX_STEPS - 1)),
    ("frame 1: mode differs", frame1(mode=lambda m: (m + 2) % 4)),
    ("frame 1: no flags (MIPS where frame 0 has none)", frame1(flags=lambda f: np.where(f == 0, MIPS, 0))),
    ("frame 1: the disk flag differs", frame1(flags=lambda f: f ^ DISK)),
    ("frame 1: the ss4 flag differs", frame1(flags=lambda f: f ^ SS4)),
    ("frame 1: tol differs", frame1(tol=1e-5)),
    ("frame 1 inside the horizon", frame1(r_obs=0.9)),
    ("frame 1 on the horizon", frame1(r_obs=1.0)),
    ("frame 1 outside the sphere", frame1(r_obs=SPHERE_R)),
    ("frame 1: r_obs 0", frame1(r_obs=0.0)),
    ("frame 0 inside the horizon, frame 1 outside", both(scene(r_obs=0.9), frame1(r_obs=10.0))),
    ("rs 0, frame 1 at r_obs 0.5", both(scene(rs=0.0), frame1(r_obs=0.5))),
)


def blocks():
    for e in range(len(ENTRIES)):
        for n in ((1,) if e < ONE_FRAME else (1, 2, 8)):
            yield f"{ENTRIES[e]}, {n} frame(s)", product_block(e, n)
    for name, change in VARIATIONS:
        c = base_block()
        change(c)
        yield name, c


def describe(k) -> str:
    """One case in words."""
    s0, s1 = k["scene"][0], k["scene"][1]
    flags = lambda f: "|".join(n for b, n in ((1, "DEFER_STEPS"), (2, "COMPOSITE"), (4, "MIPS"), (8, "RING_F64"),
                                              (16, "DISK"), (32, "SS4"), (64, "unknown bit")) if f & b) or "0"
    sc = lambda s: (f"mode {s['mode']} flags {flags(int(s['flags']))} rs {s['rs']} sphere_r {s['sphere_r']} "
                    f"r_obs {s['r_obs']} step {s['step']:.5f} max_steps {s['max_steps']} tol {s['tol']}")
    state = [n for n in ("sky", "disk_set", "shift_set", "emit_set", "disk_ring") if k[n]]
    return (f"{ENTRIES[int(k['entry'])]}: {int(k['nframes'])} frame(s), {k['width']} x {k['height']}, row arguments "
            f"{k['g'].tolist()}, out_frame_stride {k['out_frame_stride']}, null arguments {k['nulls']:#x}, side "
            f"outputs {k['side']:#x}, armed buffers {k['armed']:#x}, steps_total {'given' if k['steps_total'] else 'null'}"
            f"; state: {' '.join(state) or 'nothing set'}, fan nodes {k['n_fan']}, disk {k['r_in']} .. {k['r_out']}; "
            f"scene: {sc(s0)}; frame {k['alt_frame']}'s: {sc(s1)}")


def load(extra_flags=(), so=SO):
    """The host build of geo_render_rules.h (rebuilt when a dependency is newer)."""
    deps = [SRC, os.path.join(HERE, "..", "include", "geo", "geo.h")] + [
        os.path.join(CSRC, h) for h in ("geo_render_rules.h", "geo_pixel.h", "geo_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", *GXX_FLAGS, "-fPIC", "-shared", *extra_flags, "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.render_rules_run.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.render_rules_hits.argtypes = [ctypes.c_void_p]
    assert lib.render_rules_case_bytes() == CASE.itemsize
    return lib


def run(lib, cases):
    """(status int8, launcher uint8) of every case."""
    cases = np.ascontiguousarray(cases)
    status = np.zeros(len(cases), np.int8)
    launcher = np.zeros(len(cases), np.uint8)
    assert lib.render_rules_run(cases.ctypes.data, len(cases), status.ctypes.data, launcher.ctypes.data) == 0
    return status, launcher


def hits(lib):
    out = np.zeros(lib.render_rules_returns(), np.uint64)
    lib.render_rules_hits(out.ctypes.data)
    return out
