"""The batched render entry points without a device, one table row each: the
header announces the call (its GEO_HAS_* macro, the ABI still 8), libgeo.so
exports it with geo_render_band_set_batch's prototype, it refuses null
arguments and batch sizes out of range before any device work, the Context
method has the batch signature, and dist routes scenes to it (batch_entry,
frame_entry: every scene x state x keyword, with the name or the refusal's
words written out).  The tests/test_gpu_*_batch.py files run the calls."""
import ctypes
import inspect
import itertools
import os
import re

import pytest

import schwarzschild_raytracer_wgpu_amd as g
from schwarzschild_raytracer_wgpu_amd import _lib, dist
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_DISK as D
from schwarzschild_raytracer_wgpu_amd._lib import GEO_FLAG_SS4 as S
from schwarzschild_raytracer_wgpu_amd._lib import GEO_MODE_ADAPTIVE, GEO_MODE_DIRECT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "geo", "geo.h")
ARGS = ["ctx", "frames", "scenes", "nframes", "width", "height", "band_rows", "row0", "row_stride", "nbands",
        "out_rgba8", "out_frame_stride", "steps_total", "stream"]
# entry point, its macro, the Context method, a valid scene's (mode, flags), dist.ShardedFrame's keyword (None:
# routed by what the scene shows)
TABLE = (
    ("geo_render_disk_batch", "GEO_HAS_DISK_BATCH", "render_disk_batch", (GEO_MODE_DIRECT, D), None),
    ("geo_render_ss_batch", "GEO_HAS_SS4_BATCH", "render_ss_batch", (GEO_MODE_DIRECT, S), None),
    ("geo_render_emission_batch", "GEO_HAS_DISK_EMISSION_BATCH", "render_emission_batch", (GEO_MODE_DIRECT, D),
     "emission_batch"),
    ("geo_render_disk_ring_batch", "GEO_HAS_DISK_RING_BATCH", "render_disk_ring_batch", (GEO_MODE_DIRECT, D),
     "disk_ring_batch"),
    ("geo_render_disk_adaptive_batch", "GEO_HAS_DISK_ADAPTIVE_BATCH", "render_disk_adaptive_batch",
     (GEO_MODE_ADAPTIVE, D), None),
)
rows = pytest.mark.parametrize("entry,macro,method,scene,keyword", TABLE, ids=[t[0] for t in TABLE])


def _declaration(src, name):
    m = re.search(r"int %s\((.*?)\);" % name, re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@rows
def test_header_and_lib_announce_the_batch(entry, macro, method, scene, keyword):
    src = open(HEADER).read()
    assert re.search(r"^#define %s 1$" % macro, src, flags=re.M)
    assert re.search(r"^#define GEO_ABI_VERSION 8\b", src, flags=re.M)  # additions only
    assert getattr(_lib, macro) == 1
    assert _lib.lib.geo_abi_version() == 8


@rows
def test_exported_with_the_batch_prototype(entry, macro, method, scene, keyword):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, entry)
    # geo_render_band_set_batch's shape: scenes[f] belongs to frames[f]
    assert _lib.SIGNATURES[entry] == _lib.SIGNATURES["geo_render_band_set_batch"]
    fn = getattr(_lib.lib, entry)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[1] == ctypes.POINTER(g.GeoFrame) and fn.argtypes[2] == ctypes.POINTER(g.GeoScene)
    assert fn.argtypes[11] is ctypes.c_size_t
    # the declaration in geo.h: geo_render_band_set_batch's, argument for argument (type and name)
    src = open(HEADER).read()
    decl = _declaration(src, entry)
    assert [a.split()[-1].lstrip("*") for a in decl] == ARGS
    assert decl == _declaration(src, "geo_render_band_set_batch")


@rows
def test_null_args_rejected_without_a_device(entry, macro, method, scene, keyword):
    fr = (g.GeoFrame * 9)()
    sc = (g.GeoScene * 9)()
    for s in sc:
        s.mode, s.flags = scene
    buf = ctypes.create_string_buffer(64)

    def call(ctx, frames, scenes, n, out):
        return getattr(_lib.lib, entry)(ctx, frames, scenes, n, 8, 8, 8, 0, 8, 1, out, 256, None, None)

    assert call(None, None, None, 1, None) == _lib.GEO_EINVAL
    assert call(None, fr, sc, 1, buf) == _lib.GEO_EINVAL  # ctx
    assert _lib.GEO_MAX_BATCH_FRAMES == 8
    for n in (0, 9):  # batch sizes out of range, before any device work
        assert call(None, fr, sc, n, buf) == _lib.GEO_EINVAL
    for frames, scenes, out in ((None, sc, buf), (fr, None, buf), (fr, sc, None)):
        assert call(None, frames, scenes, 1, out) == _lib.GEO_EINVAL


@rows
def test_python_layers_exist(entry, macro, method, scene, keyword):
    sig = inspect.signature(getattr(g.Context, method))
    assert list(sig.parameters) == ["self", "frames", "scenes", "width", "height", "band_rows", "row0", "row_stride",
                                    "nbands", "out_rgba", "frame_stride", "steps_total", "stream"]
    for name in ("frame_stride", "steps_total", "stream"):
        assert sig.parameters[name].default is None
    # the disk batch's parameters, defaults included
    disk = inspect.signature(g.Context.render_disk_batch)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [(p.name, p.default)
                                                                      for p in disk.parameters.values()]
    # ShardedFrame takes the keywords, off by default, and none for what it routes by the scene
    init = inspect.signature(dist.ShardedFrame.__init__)
    for name in ("disk_ring_batch", "emission_batch", "batch_launch"):
        assert init.parameters[name].default is False
    assert not [p for p in init.parameters if "adaptive" in p]
    if keyword:
        assert keyword in init.parameters


class Scene:
    def __init__(self, mode, flags, rs=1.0):
        self.mode, self.flags, self.rs = mode, flags, rs


def _batch_route(mode, flags, rs, emission_set, ring_f64, emission_batch, disk_ring_batch):
    """The route written out: the name, or the words of the refusal."""
    if mode == GEO_MODE_ADAPTIVE and flags & D:
        if rs > 0 and ring_f64:
            return ("GEO_MODE_ADAPTIVE", "set_disk_ring_f64", "geo_render_disk_adaptive_batch")
        return "geo_render_disk_adaptive_batch"
    if flags & D and ring_f64:
        return "geo_render_disk_ring_batch" if disk_ring_batch else ("set_disk_ring_f64", "disk_ring_batch=True",
                                                                     "geo_render_disk_ring_batch")
    if flags & D and emission_set:
        return "geo_render_emission_batch" if emission_batch else ("set_disk_emission", "emission_batch=True",
                                                                   "geo_render_emission_batch")
    if flags & S:
        return "geo_render_ss_batch"  # (the SS4 test comes before the disk's)
    return "geo_render_disk_batch" if flags & D else "geo_render_band_set_batch"


def test_batch_entry_routes_every_scene_state_and_keyword():
    names = set()
    for mode, flags, rs in itertools.product((GEO_MODE_DIRECT, _lib.GEO_MODE_FAN, GEO_MODE_ADAPTIVE),
                                             (0, D, S, D | S, _lib.GEO_FLAG_DEFER_STEPS, D | _lib.GEO_FLAG_DEFER_STEPS),
                                             (0.0, 1.0)):
        for state in itertools.product((False, True), repeat=4):
            want = _batch_route(mode, flags, rs, *state)
            what = (mode, flags, rs, state)
            if isinstance(want, str):
                assert dist.batch_entry(Scene(mode, flags, rs), *state) == want, what
                names.add(want)
            else:
                with pytest.raises(ValueError) as e:
                    dist.batch_entry(Scene(mode, flags, rs), *state)
                for word in want:
                    assert word in str(e.value), (what, word)
    assert names == {t[0] for t in TABLE} | {"geo_render_band_set_batch"}
    # the cases the entry points were added for, one by one
    assert dist.batch_entry(Scene(0, D), False, False, False, False) == "geo_render_disk_batch"
    assert dist.batch_entry(Scene(0, D | S), False, False, False, False) == "geo_render_ss_batch"
    assert dist.batch_entry(Scene(0, D | S), True, False, True, False) == "geo_render_emission_batch"
    assert dist.batch_entry(Scene(0, D), True, True, False, True) == "geo_render_disk_ring_batch"  # no emission_batch
    assert dist.batch_entry(Scene(2, D | S), True, False, False, False) == "geo_render_disk_adaptive_batch"
    assert dist.batch_entry(Scene(2, D, rs=0.0), False, True, False, False) == "geo_render_disk_adaptive_batch"


def test_frame_entry_routes_every_scene_and_state():
    for mode, flags, rs, ring in itertools.product((GEO_MODE_DIRECT, _lib.GEO_MODE_FAN, GEO_MODE_ADAPTIVE),
                                                   (0, D, S, D | S, D | _lib.GEO_FLAG_DEFER_STEPS), (0.0, 1.0),
                                                   (False, True)):
        sc = Scene(mode, flags, rs)
        if not (mode == GEO_MODE_ADAPTIVE and flags & D):
            assert dist.frame_entry(sc, ring) == "geo_render_band_set"
        elif rs > 0 and ring:
            with pytest.raises(ValueError) as e:
                dist.frame_entry(sc, ring)
            assert "set_disk_ring_f64" in str(e.value) and "GEO_MODE_ADAPTIVE" in str(e.value)
        else:  # the one-frame call, and the batched one (with one frame) for a supersampled scene
            assert dist.frame_entry(sc, ring) == ("geo_render_disk_adaptive_batch" if flags & S
                                                  else "geo_render_disk_adaptive")
