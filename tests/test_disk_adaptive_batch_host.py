"""geo_render_disk_adaptive_batch without a device: the header announces it
(GEO_HAS_DISK_ADAPTIVE_BATCH, the ABI still 8), libgeo.so exports it with
geo_render_band_set_batch's prototype, it refuses null arguments and batch
sizes out of range before any device work, and the Python layers
(Context.render_disk_adaptive_batch, dist.ShardedFrame's routing by what the
scene shows) exist.  tests/test_gpu_disk_adaptive_batch.py runs it."""
import ctypes
import inspect
import os
import re

import schwarzschild_raytracer_wgpu_amd as g
from schwarzschild_raytracer_wgpu_amd import _lib, dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "geo", "geo.h")
ARGS = ["ctx", "frames", "scenes", "nframes", "width", "height", "band_rows", "row0", "row_stride", "nbands",
        "out_rgba8", "out_frame_stride", "steps_total", "stream"]


def _declaration(src, name):
    m = re.search(r"int %s\((.*?)\);" % name, re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_and_lib_announce_the_batch():
    src = open(HEADER).read()
    assert re.search(r"^#define GEO_HAS_DISK_ADAPTIVE_BATCH 1$", src, flags=re.M)
    assert re.search(r"^#define GEO_ABI_VERSION 8\b", src, flags=re.M)  # additions only
    assert _lib.GEO_HAS_DISK_ADAPTIVE_BATCH == 1
    assert _lib.lib.geo_abi_version() == 8


def test_exported_with_the_batch_prototype():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "geo_render_disk_adaptive_batch")
    assert _lib.SIGNATURES["geo_render_disk_adaptive_batch"] == _lib.SIGNATURES["geo_render_band_set_batch"]
    fn = _lib.lib.geo_render_disk_adaptive_batch
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[1] == ctypes.POINTER(g.GeoFrame) and fn.argtypes[2] == ctypes.POINTER(g.GeoScene)
    assert fn.argtypes[11] is ctypes.c_size_t
    # the declaration in geo.h: geo_render_band_set_batch's, argument for argument (type and name)
    src = open(HEADER).read()
    decl = _declaration(src, "geo_render_disk_adaptive_batch")
    assert [a.split()[-1].lstrip("*") for a in decl] == ARGS
    assert decl == _declaration(src, "geo_render_band_set_batch")


def test_null_args_rejected_without_a_device():
    lib = _lib.lib
    fr = (g.GeoFrame * 9)()
    sc = (g.GeoScene * 9)()
    for s in sc:
        s.mode = _lib.GEO_MODE_ADAPTIVE
        s.flags = _lib.GEO_FLAG_DISK
    buf = ctypes.create_string_buffer(64)

    def call(ctx, frames, scenes, n, out):
        return lib.geo_render_disk_adaptive_batch(ctx, frames, scenes, n, 8, 8, 8, 0, 8, 1, out, 256, None, None)

    assert call(None, None, None, 1, None) == _lib.GEO_EINVAL
    assert call(None, fr, sc, 1, buf) == _lib.GEO_EINVAL  # ctx
    assert _lib.GEO_MAX_BATCH_FRAMES == 8
    for n in (0, 9):  # batch sizes out of range, before any device work
        assert call(None, fr, sc, n, buf) == _lib.GEO_EINVAL
    for frames, scenes, out in ((None, sc, buf), (fr, None, buf), (fr, sc, None)):
        assert call(None, frames, scenes, 1, out) == _lib.GEO_EINVAL


def test_python_layers_exist():
    sig = inspect.signature(g.Context.render_disk_adaptive_batch)
    assert list(sig.parameters) == ["self", "frames", "scenes", "width", "height", "band_rows", "row0", "row_stride",
                                    "nbands", "out_rgba", "frame_stride", "steps_total", "stream"]
    # the disk batch's parameters, defaults included
    disk = inspect.signature(g.Context.render_disk_batch)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [(p.name, p.default)
                                                                      for p in disk.parameters.values()]
    # ShardedFrame routes by the scene: no new keyword; render_batch names the new call and every older one
    init = inspect.signature(dist.ShardedFrame.__init__)
    assert not [p for p in init.parameters if "adaptive" in p]
    src = inspect.getsource(dist.ShardedFrame.render_batch)
    for name in ("geo_render_disk_adaptive_batch", "geo_render_disk_ring_batch", "geo_render_emission_batch",
                 "geo_render_ss_batch", "geo_render_disk_batch", "geo_render_band_set_batch"):
        assert name in src, name
    # the per-frame path names the one-frame call, and the batched one for a supersampled scene
    src = inspect.getsource(dist.ShardedFrame.step)
    assert "geo_render_disk_adaptive(" in src and "geo_render_disk_adaptive_batch(" in src
    # the refusal names the state
    msg = inspect.getsource(dist.ShardedFrame._refuse_adaptive_ring)
    assert "set_disk_ring_f64" in msg and "ValueError" in msg
