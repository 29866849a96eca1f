"""geo_render_disk_adaptive_ring_batch without a device: the row
tests/test_batch_entry_points_host.py would have for it (the header announces
the call, libgeo.so exports it with geo_render_band_set_batch's prototype, it
refuses null arguments and batch sizes out of range before any device work, the
Context method has the batch signature), dist's routing over that test's full
product times the new keyword disk_ring_any_mode, and the fixture check of
tests/test_gpu_disk_adaptive_ring_batch.py's frames on the CPU path
(geo_render_cpu_disk_adaptive_ring_f64): what makes those GPU tests meaningful.

The fixture check: every frame the GPU tests draw (the ring walk WALK of
test_gpu_disk_ring_batch at 96 x 54 and, for the SS4 tests' 48 x 27 output, its
samples at 96 x 54; both curved kinds; the second walk of the two-stream test; the ragged layout) holds
an in-band pixel with a slot-2 hit (the third image, which only the band
resolves), a pixel outside the band with a hit (the adaptive f32 lanes draw
disk too), and a 16 x 4 wave block with lanes of both kinds (the ballot's cold
arm runs beside f32 lanes).  The ring batch test's own walk (dx = 0.05) loses
its last non-band hit at frame 5; with dx = 0.02 every frame keeps 30 or more
(measured here: 96 x 54 curved-out 30..66 non-band hits, 86..162 in-band slot-2
hits, 6..14 mixed blocks)."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import schwarzschild_raytracer_wgpu_amd as g
import test_disk_adaptive_ring_cpu as AR
import test_disk_cpu as T
import test_gpu_disk_ring_batch as RB
from schwarzschild_raytracer_wgpu_amd import _lib, dist, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK as D
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_SS4 as S
from schwarzschild_raytracer_wgpu_amd._lib import GEO_MODE_ADAPTIVE, GEO_MODE_DIRECT, GEO_OK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "geo", "geo.h")
ENTRY, MACRO, METHOD = ("geo_render_disk_adaptive_ring_batch", "GEO_HAS_DISK_ADAPTIVE_RING_BATCH",
                        "render_disk_adaptive_ring_batch")
ARGS = ["ctx", "frames", "scenes", "nframes", "width", "height", "band_rows", "row0", "row_stride", "nbands",
        "out_rgba8", "out_frame_stride", "steps_total", "stream"]

# ---- the GPU tests' frames (tests/test_gpu_disk_adaptive_ring_batch.py imports these) -------------
N = _lib.GEO_MAX_BATCH_FRAMES
WALK = dict(dx=0.02, x0=14.0)     # the ring walk of every test
WALK_B = dict(dx=-0.02, x0=13.98)  # the second stream's walk
CURVED_IN_STEP = 1.0  # the ring cells' of tests/test_gpu_wave_block_matrix.py


def walk(w, h, n, curved_in=False, ss=False, flags=0, tol=0.0, **kw):
    """test_gpu_disk_ring_batch.walk in the adaptive mode (kCurvedIn: at the matrix's ring cells' step)."""
    frames, scenes = RB.walk(w, h, n, curved_in, **(kw or WALK))
    step = (lambda s: CURVED_IN_STEP) if curved_in else (lambda s: s.step)
    return frames, [make_scene(s.rs, s.sphere_r, s.r_obs, step(s), s.max_steps, GEO_MODE_ADAPTIVE,
                               D | (S if ss else 0) | flags, tol) for s in scenes]


def direct_of(s):
    """The direct disk scene of the same numbers (what test_gpu_disk_ring_batch.in_band takes)."""
    return make_scene(s.rs, s.sphere_r, s.r_obs, s.step, s.max_steps, GEO_MODE_DIRECT, D)


# ---- the table row ---------------------------------------------------------------------------------
def _declaration(src, name):
    m = re.search(r"int %s\((.*?)\);" % name, re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_and_lib_announce_the_batch():
    src = open(HEADER).read()
    assert re.search(r"^#define %s 1$" % MACRO, src, flags=re.M)
    assert re.search(r"^#define GEO_ABI_VERSION 8\b", src, flags=re.M)  # additions only
    assert getattr(_lib, MACRO) == 1
    assert _lib.lib.geo_abi_version() == 8


def test_exported_with_the_batch_prototype():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, ENTRY)
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["geo_render_band_set_batch"]
    fn = getattr(_lib.lib, ENTRY)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[1] == ctypes.POINTER(g.GeoFrame) and fn.argtypes[2] == ctypes.POINTER(g.GeoScene)
    assert fn.argtypes[11] is ctypes.c_size_t
    src = open(HEADER).read()
    decl = _declaration(src, ENTRY)
    assert [a.split()[-1].lstrip("*") for a in decl] == ARGS
    assert decl == _declaration(src, "geo_render_band_set_batch")


def test_null_args_rejected_without_a_device():
    fr = (g.GeoFrame * 9)()
    sc = (g.GeoScene * 9)()
    for s in sc:
        s.mode, s.flags = GEO_MODE_ADAPTIVE, D
    buf = ctypes.create_string_buffer(64)

    def call(ctx, frames, scenes, n, out):
        return getattr(_lib.lib, ENTRY)(ctx, frames, scenes, n, 8, 8, 8, 0, 8, 1, out, 256, None, None)

    assert call(None, None, None, 1, None) == _lib.GEO_EINVAL
    assert call(None, fr, sc, 1, buf) == _lib.GEO_EINVAL  # ctx
    assert _lib.GEO_MAX_BATCH_FRAMES == 8
    for n in (0, 9):  # batch sizes out of range, before any device work
        assert call(None, fr, sc, n, buf) == _lib.GEO_EINVAL
    for frames, scenes, out in ((None, sc, buf), (fr, None, buf), (fr, sc, None)):
        assert call(None, frames, scenes, 1, out) == _lib.GEO_EINVAL


def test_python_layers_exist():
    sig = inspect.signature(getattr(g.Context, METHOD))
    assert list(sig.parameters) == ["self", "frames", "scenes", "width", "height", "band_rows", "row0", "row_stride",
                                    "nbands", "out_rgba", "frame_stride", "steps_total", "stream"]
    disk = inspect.signature(g.Context.render_disk_batch)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [(p.name, p.default)
                                                                      for p in disk.parameters.values()]
    init = inspect.signature(dist.ShardedFrame.__init__)
    assert init.parameters["disk_ring_any_mode"].default is False
    assert inspect.signature(dist.batch_entry).parameters["disk_ring_any_mode"].default is False
    assert inspect.signature(dist.frame_entry).parameters["disk_ring_any_mode"].default is False
    assert list(inspect.signature(dist.batch_entry).parameters) == ["scene", "emission_set", "ring_f64",
                                                                    "emission_batch", "disk_ring_batch",
                                                                    "disk_ring_any_mode"]
    assert list(inspect.signature(dist.frame_entry).parameters) == ["scene", "ring_f64", "disk_ring_any_mode"]


# ---- dist's routes -----------------------------------------------------------------------------------
class Scene:
    def __init__(self, mode, flags, rs=1.0):
        self.mode, self.flags, self.rs = mode, flags, rs


REFUSAL = ("GEO_MODE_ADAPTIVE", "set_disk_ring_f64", "geo_render_disk_adaptive_batch", "disk_ring_any_mode=True")


def _batch_route(mode, flags, rs, emission_set, ring_f64, emission_batch, disk_ring_batch, any_mode):
    """test_batch_entry_points_host's route, restated, with the keyword: the name, or the words of the refusal."""
    if mode == GEO_MODE_ADAPTIVE and flags & D:
        if rs > 0 and ring_f64:
            return "geo_render_disk_adaptive_ring_batch" if any_mode else REFUSAL
        return "geo_render_disk_adaptive_batch"
    if flags & D and ring_f64:
        return "geo_render_disk_ring_batch" if disk_ring_batch else ("set_disk_ring_f64", "disk_ring_batch=True",
                                                                     "geo_render_disk_ring_batch")
    if flags & D and emission_set:
        return "geo_render_emission_batch" if emission_batch else ("set_disk_emission", "emission_batch=True",
                                                                   "geo_render_emission_batch")
    if flags & S:
        return "geo_render_ss_batch"
    return "geo_render_disk_batch" if flags & D else "geo_render_band_set_batch"


def test_batch_entry_routes_every_scene_state_and_keyword():
    names, changed = set(), 0
    for mode, flags, rs in itertools.product((GEO_MODE_DIRECT, _lib.GEO_MODE_FAN, GEO_MODE_ADAPTIVE),
                                             (0, D, S, D | S, _lib.GEO_FLAG_DEFER_STEPS, D | _lib.GEO_FLAG_DEFER_STEPS),
                                             (0.0, 1.0)):
        for state in itertools.product((False, True), repeat=4):
            for any_mode in (False, True):
                want = _batch_route(mode, flags, rs, *state, any_mode)
                what = (mode, flags, rs, state, any_mode)
                if isinstance(want, str):
                    assert dist.batch_entry(Scene(mode, flags, rs), *state, disk_ring_any_mode=any_mode) == want, what
                    names.add(want)
                    if not any_mode:  # the keyword's default is today's call
                        assert dist.batch_entry(Scene(mode, flags, rs), *state) == want, what
                else:
                    assert want != REFUSAL or not any_mode, what
                    calls = [lambda: dist.batch_entry(Scene(mode, flags, rs), *state, any_mode)]
                    if not any_mode:
                        calls.append(lambda: dist.batch_entry(Scene(mode, flags, rs), *state))
                    for call in calls:
                        with pytest.raises(ValueError) as e:
                            call()
                        for word in want:
                            assert word in str(e.value), (what, word)
                # only the adaptive disk + state + rs > 0 cells change with the keyword
                if any_mode and want != _batch_route(mode, flags, rs, *state, False):
                    assert mode == GEO_MODE_ADAPTIVE and flags & D and rs > 0 and state[1], what
                    assert want == "geo_render_disk_adaptive_ring_batch"
                    changed += 1
    assert changed == 3 * 8  # three disk flag sets x the other three booleans
    assert "geo_render_disk_adaptive_ring_batch" in names and len(names) == 7
    assert dist.batch_entry(Scene(2, D | S), True, True, False, False, True) == "geo_render_disk_adaptive_ring_batch"
    assert dist.batch_entry(Scene(2, D, rs=0.0), False, True, False, False, True) == "geo_render_disk_adaptive_batch"
    assert dist.batch_entry(Scene(0, D), False, True, False, True, True) == "geo_render_disk_ring_batch"


def test_frame_entry_routes_every_scene_state_and_keyword():
    for mode, flags, rs, ring, any_mode in itertools.product(
            (GEO_MODE_DIRECT, _lib.GEO_MODE_FAN, GEO_MODE_ADAPTIVE), (0, D, S, D | S, D | _lib.GEO_FLAG_DEFER_STEPS),
            (0.0, 1.0), (False, True), (False, True)):
        sc = Scene(mode, flags, rs)
        what = (mode, flags, rs, ring, any_mode)
        if not (mode == GEO_MODE_ADAPTIVE and flags & D):
            assert dist.frame_entry(sc, ring, any_mode) == "geo_render_band_set", what
        elif rs > 0 and ring and not any_mode:
            for call in (lambda: dist.frame_entry(sc, ring), lambda: dist.frame_entry(sc, ring, False)):
                with pytest.raises(ValueError) as e:
                    call()
                for word in REFUSAL:
                    assert word in str(e.value), (what, word)
        elif rs > 0 and ring:
            assert dist.frame_entry(sc, ring, True) == ("geo_render_disk_adaptive_ring_batch" if flags & S
                                                        else "geo_render_disk_adaptive_ring"), what
        else:
            assert dist.frame_entry(sc, ring, any_mode) == ("geo_render_disk_adaptive_batch" if flags & S
                                                            else "geo_render_disk_adaptive"), what


# ---- the GPU tests' frames on the CPU path ---------------------------------------------------------
def mixed_blocks(band):
    """The 16 x 4 wave blocks of the frame that hold band and non-band pixels."""
    h, w = band.shape
    n = 0
    for y in range(0, h, 4):
        for x in range(0, w, 16):
            b = band[y:y + 4, x:x + 16]
            n += bool(b.any() and not b.all())
    return n


FIXTURES = {"walk 96 x 54": (96, 54, False, 1, WALK), "walk 96 x 54 kCurvedIn": (96, 54, True, 1, WALK),
            "walk 48 x 27 at 96 x 54 (the SS4 samples)": (48, 27, False, 2, WALK),
            "walk 48 x 27 at 96 x 54 kCurvedIn (the SS4 samples)": (48, 27, True, 2, WALK),
            "the second stream's walk": (96, 54, False, 1, WALK_B), "walk 100 x 37": (100, 37, False, 1, WALK)}


@pytest.mark.parametrize("name", list(FIXTURES))
def test_gpu_fixture_frames_exercise_both_kinds_of_lane(name):
    w, h, curved_in, k, kw = FIXTURES[name]
    cpu = AR.load_cpu()
    frames, scenes = walk(w, h, N, curved_in, **kw)
    assert len({s.r_obs for s in scenes}) == N
    disk = T.make_disk(*RB.RING_DISK)
    for f in range(N):
        rc, c = AR.render(cpu, frames[f], scenes[f], disk, 1, k * w, k * h)
        assert rc == GEO_OK
        band = RB.in_band(frames[f], direct_of(scenes[f]), k * w, k * h)
        hit = c["hits"][..., 0] > 0.0
        slot2, outside, mixed = int((band & hit[..., 2]).sum()), int((~band & hit.any(axis=-1)).sum()), mixed_blocks(band)
        print(f"{name} frame {f}: band pixels {int(band.sum())}, in-band slot-2 hits {slot2}, hits outside the band "
              f"{outside}, mixed wave blocks {mixed}")
        assert slot2 >= 1 and outside >= 1 and mixed >= 1, (name, f, slot2, outside, mixed)
