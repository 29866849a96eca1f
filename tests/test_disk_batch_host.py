"""geo_render_disk_batch without a device: the header announces it
(GEO_HAS_DISK_BATCH), libgeo.so exports it with the prototype of the ctypes
table, it refuses null arguments before any device work, and the Python layers
(Context.render_disk_batch, dist.ShardedFrame's routing of disk batches)
exist.  tests/test_gpu_disk_batch.py runs it."""
import ctypes
import inspect
import os
import re

import schwarzschild_raytracer_wgpu_amd as g
from schwarzschild_raytracer_wgpu_amd import _lib, dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "geo", "geo.h")


def test_header_and_lib_announce_the_batch():
    src = open(HEADER).read()
    assert re.search(r"^#define GEO_HAS_DISK_BATCH 1\b", src, flags=re.M)
    assert re.search(r"^#define GEO_ABI_VERSION 8\b", src, flags=re.M)  # additions only
    assert _lib.GEO_HAS_DISK_BATCH == 1


def test_exported_with_the_batch_prototype():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "geo_render_disk_batch")
    # geo_render_band_set_batch's shape: scenes[f] belongs to frames[f]
    assert _lib.SIGNATURES["geo_render_disk_batch"] == _lib.SIGNATURES["geo_render_band_set_batch"]
    fn = _lib.lib.geo_render_disk_batch
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[1] == ctypes.POINTER(g.GeoFrame) and fn.argtypes[2] == ctypes.POINTER(g.GeoScene)
    assert fn.argtypes[11] is ctypes.c_size_t
    # the declaration in geo.h, argument for argument
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int geo_render_disk_batch\((.*?)\);", src, flags=re.S)
    assert m
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["ctx", "frames", "scenes", "nframes", "width", "height", "band_rows", "row0", "row_stride",
                     "nbands", "out_rgba8", "out_frame_stride", "steps_total", "stream"]


def test_null_args_rejected_without_a_device():
    lib = _lib.lib
    fr = (g.GeoFrame * 9)()
    sc = (g.GeoScene * 9)()
    buf = ctypes.create_string_buffer(64)
    assert lib.geo_render_disk_batch(None, None, None, 1, 8, 8, 8, 0, 8, 1, None, 256, None, None) == _lib.GEO_EINVAL
    assert lib.geo_render_disk_batch(None, fr, sc, 1, 8, 8, 8, 0, 8, 1, buf, 256, None, None) == _lib.GEO_EINVAL
    for n in (0, _lib.GEO_MAX_BATCH_FRAMES + 1):  # batch sizes out of range, before any device work
        assert lib.geo_render_disk_batch(None, fr, sc, n, 8, 8, 8, 0, 8, 1, buf, 256, None, None) == _lib.GEO_EINVAL


def test_python_layers_exist():
    sig = inspect.signature(g.Context.render_disk_batch)
    assert list(sig.parameters) == ["self", "frames", "scenes", "width", "height", "band_rows", "row0", "row_stride",
                                    "nbands", "out_rgba", "frame_stride", "steps_total", "stream"]
    for name in ("frame_stride", "steps_total", "stream"):
        assert sig.parameters[name].default is None
    # ShardedFrame.render_batch sends GEO_FLAG_DISK batches to the new call and the others where they went
    src = inspect.getsource(dist.ShardedFrame.render_batch)
    assert "geo_render_disk_batch" in src and "geo_render_band_set_batch" in src and "GEO_FLAG_DISK" in src
