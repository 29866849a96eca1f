"""GEO_FLAG_SS4 on the CPU path (geo_render_cpu, geo_render_cpu_disk,
geo_render_cpu_disk_shift; include/geo/geo_cpu.h): the supersampled frame is,
byte for byte, the numpy box resolve of the existing one-sample render at twice
the size (plain, disk and shifted disk frames), it does anti-alias the
shadow's and the disk's rims, and its rows and argument rules.
tests/test_gpu_ss.py ties the kernels to this path bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import test_disk_cpu as T
import test_disk_shift_cpu as X
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_EINVAL, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4, GEO_MODE_ADAPTIVE,
                                                   GEO_MODE_FAN, GEO_OK, GeoDiskShift)

SHIFT = (1, 4, 1.0)  # test_disk_shift_cpu's default state
POSES = ("A", "B", "flat", "tilted")
SIZES = ((96, 54), (100, 37), (49, 27))  # 2W = 200 and 98 are no multiples of the 32-wide tile; 98 mod 32 = 2
KINDS = ("plain", "disk", "shift")
PREFILL = 0x5A


@pytest.fixture(scope="module")
def cpu():
    return X.load_cpu()


def with_flags(scene, flags, mode=None):
    return make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps,
                      scene.mode if mode is None else mode, flags)


def ss_scene(scene, kind, extra=0):
    return with_flags(scene, GEO_FLAG_SS4 | extra | (0 if kind == "plain" else GEO_FLAG_DISK))


def ss_render(lib, kind, frame, scene, w, h, disk=None, tex=T.TEX, sky=T.SKY, row0=0, nrows=None, row_step=1,
              threads=4, shift=SHIFT, mask=False, uv=False, steps=False, hits=False, g=False):
    """One call of the entry point of `kind` with colour and steps_total only
    (mask .. g: also pass that optional output).  Returns the status, the
    colour rows (prefilled with PREFILL) and steps_total."""
    nrows = (h - row0 + row_step - 1) // row_step if nrows is None else nrows
    sky = np.ascontiguousarray(sky, dtype=np.uint8)
    tex = np.ascontiguousarray(tex, dtype=np.uint8)
    rgba = np.full((max(nrows, 1), w if w <= 4096 else 1, 4), PREFILL, np.uint8)
    total = ctypes.c_ulonglong()
    n = rgba.shape[0] * rgba.shape[1]
    opt = {"mask": np.zeros(n, np.uint8), "uv": np.zeros(2 * n, np.float32), "steps": np.zeros(n, np.uint32),
           "hits": np.zeros(6 * n, np.float32), "g": np.zeros(3 * n, np.float32)}
    want = dict(mask=mask, uv=uv, steps=steps, hits=hits, g=g)
    p = {k: (opt[k].ctypes.data if want[k] else None) for k in opt}
    args = [ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1], sky.shape[0], None, 0, w,
            h, row0, nrows, row_step, threads, rgba.ctypes.data, p["mask"], p["uv"], p["steps"],
            ctypes.addressof(total)]
    dargs = [None if disk is None else ctypes.addressof(disk), tex.ctypes.data, tex.shape[1], tex.shape[0], p["hits"]]
    if kind == "plain":
        rc = lib.geo_render_cpu(*args)
    elif kind == "disk":
        rc = lib.geo_render_cpu_disk(*args, *dargs)
    else:
        sh = None if shift is None else GeoDiskShift(*shift)
        rc = lib.geo_render_cpu_disk_shift(*args, *dargs, None if sh is None else ctypes.addressof(sh), p["g"])
    return rc, rgba, total.value


def resolve(s):
    """(2h, 2w, 4) uint8 samples -> (h, w, 4): (s00 + s01 + s10 + s11 + 2) >> 2 per channel."""
    s = s.astype(np.uint32)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


_ONE = {}


def one_sample(lib, kind, name, w, h):
    """The existing one-sample CPU render of pose `name` at 2w x 2h with the
    w x h frame's uniform (rendered once per module, never modified)."""
    key = (kind, name, w, h)
    if key not in _ONE:
        frame, scene, disk, _ = T.pose(name, w, h)
        if kind == "plain":
            rc, a = T.render(lib, frame, T.plain_of(scene), T.SKY, 2 * w, 2 * h)
        elif kind == "disk":
            rc, a = T.render(lib, frame, scene, T.SKY, 2 * w, 2 * h, disk, T.TEX)
        else:
            rc, a = X.render(lib, frame, scene, 2 * w, 2 * h, disk, shift=SHIFT)
        assert rc == GEO_OK
        for v in a.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ONE[key] = a
    return _ONE[key]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", POSES)
@pytest.mark.parametrize("kind", KINDS)
def test_definition(cpu, kind, name, size):
    w, h = size
    frame, scene, disk, _ = T.pose(name, w, h)
    ref = one_sample(cpu, kind, name, w, h)
    rc, got, total = ss_render(cpu, kind, frame, ss_scene(scene, kind), w, h, disk)
    assert rc == GEO_OK
    want = resolve(ref["rgba"])
    diff = (got != want).any(axis=-1)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the resolve of the {2 * w} x {2 * h} render"
    assert total == ref["total"]
    if kind == "shift" and name in ("A", "B"):  # (curved space: the shifted frame is another frame)
        assert not np.array_equal(ref["rgba"], one_sample(cpu, "disk", name, w, h)["rgba"])


def quads_disagree(v):
    """(2h, 2w) bool per sample -> (h, w): the four samples of the pixel disagree."""
    n = v[0::2, 0::2].astype(np.int32) + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]
    return (n > 0) & (n < 4)


@pytest.mark.parametrize("name", POSES)
def test_it_anti_aliases(cpu, name):
    """The rims are there to be smoothed (counts from the twice-size render:
    96 x 54 gives shadow-rim 12 / 60 / 0 and disk-rim 110 / 122 / 94 pixels for
    A / B / flat; the smallest disk-rim count over poses and sizes is 42), and
    with a one-colour opaque disk over a one-colour sky every disk-rim pixel
    outside the shadow is exactly one of the three intermediate mixes, unless
    its remaining samples see the secondary image (4 pixels of pose B: the full
    disk colour); each is the mix its count of disk-coloured samples gives."""
    for w, h in SIZES:
        ref = one_sample(cpu, "disk", name, w, h)
        shadow_rim = quads_disagree(ref["mask"] == 1)
        disk_rim = quads_disagree(ref["hits"][..., 0, 0] > 0.0)
        print(name, f"{w}x{h}", "shadow rim", int(shadow_rim.sum()), "disk rim", int(disk_rim.sum()))
        if name in ("A", "B"):
            assert shadow_rim.sum() >= 8
        assert disk_rim.sum() >= 40
    w, h = SIZES[0]
    frame, scene, disk, _ = T.pose(name, w, h)
    sky_c = np.array([20, 40, 200, 255], np.uint8)
    disk_c = np.array([250, 180, 10, 255], np.uint8)
    sky = np.empty((8, 16, 4), np.uint8)
    sky[:] = sky_c
    tex = np.empty((4, 8, 4), np.uint8)
    tex[:] = disk_c
    rc, got, _ = ss_render(cpu, "disk", frame, ss_scene(scene, "disk"), w, h, disk, tex=tex, sky=sky)
    assert rc == GEO_OK
    ref = one_sample(cpu, "disk", name, w, h)  # the geometry does not depend on the textures
    hit = (ref["hits"][..., 0] > 0.0).any(axis=-1)  # an opaque disk: any slot's hit is its colour
    k = hit[0::2, 0::2].astype(np.int32) + hit[0::2, 1::2] + hit[1::2, 0::2] + hit[1::2, 1::2]
    m = ref["mask"] == 1
    in_shadow = m[0::2, 0::2] | m[0::2, 1::2] | m[1::2, 0::2] | m[1::2, 1::2]
    rim = quads_disagree(ref["hits"][..., 0, 0] > 0.0) & ~in_shadow
    mixes = {j: ((j * disk_c.astype(np.uint32) + (4 - j) * sky_c.astype(np.uint32) + 2) >> 2).astype(np.uint8)
             for j in range(5)}
    # k counts a pixel's samples that hit the disk in ANY slot.  A disk-rim pixel
    # has 1 .. 3 samples with a slot-0 hit; where the others see the secondary
    # image instead of the sky (pose B: the image under the primary's rim) they
    # are disk-coloured too and the pixel is the disk's colour, k = 4.  Every
    # other disk-rim pixel must be one of the three intermediate mixes, and
    # all of them the mix their k says.
    k0 = ref["hits"][..., 0, 0] > 0.0
    k0 = k0[0::2, 0::2].astype(np.int32) + k0[0::2, 1::2] + k0[1::2, 0::2] + k0[1::2, 1::2]
    counts = {j: int((rim & (k == j)).sum()) for j in (1, 2, 3, 4)}
    print(name, "disk-rim pixels outside the shadow by disk-coloured samples", counts)
    assert (k[rim] >= 1).all() and (k[rim & (k == k0)] <= 3).all()
    for j in (1, 2, 3, 4):
        assert (got[rim & (k == j)] == mixes[j]).all(), j
    assert counts[1] + counts[2] + counts[3] >= 40 and all(counts[j] > 0 for j in (1, 2, 3))
    inter = np.stack([(got == mixes[j]).all(axis=-1) for j in (1, 2, 3)]).any(axis=0)
    assert inter[rim & (k == k0)].all()
    # and away from every rim the frame is one of the two colours
    assert (got[(k == 0) & ~in_shadow] == sky_c).all() and (got[k == 4] == disk_c).all()


@pytest.mark.parametrize("kind", KINDS)
def test_rows(cpu, kind):
    w, h = 100, 37
    frame, scene, disk, _ = T.pose("A", w, h)
    sc = ss_scene(scene, kind)
    rc, whole, total = ss_render(cpu, kind, frame, sc, w, h, disk)
    assert rc == GEO_OK
    rc, part, ptotal = ss_render(cpu, kind, frame, sc, w, h, disk, row0=5, nrows=20)
    assert rc == GEO_OK and np.array_equal(part, whole[5:25])
    ref = one_sample(cpu, kind, "A", w, h)
    assert ptotal == int(ref["steps"][10:50].astype(np.int64).sum())  # sample rows 2 r, 2 r + 1 of rows 5..24
    rc, odd, _ = ss_render(cpu, kind, frame, sc, w, h, disk, row0=1, nrows=10, row_step=2)
    assert rc == GEO_OK and np.array_equal(odd, whole[1:21:2])
    rc, one, _ = ss_render(cpu, kind, frame, sc, w, h, disk, row0=h - 1, nrows=1, threads=1)
    assert rc == GEO_OK and np.array_equal(one, whole[h - 1:])


@pytest.mark.parametrize("kind", KINDS)
def test_argument_rules(cpu, kind):
    w, h = 16, 9
    frame, scene, disk, _ = T.pose("A", w, h)
    base = 0 if kind == "plain" else GEO_FLAG_DISK

    def call(sc, ww=w, hh=h, **kw):
        rc, rgba, _ = ss_render(cpu, kind, frame, sc, ww, hh, disk, **kw)
        if rc != GEO_OK:
            assert (rgba == PREFILL).all()  # a refused call writes nothing
        return rc

    ok = with_flags(scene, base | GEO_FLAG_SS4)
    assert call(ok) == GEO_OK
    assert call(with_flags(scene, base | GEO_FLAG_SS4 | GEO_FLAG_DEFER_STEPS)) == GEO_OK
    for mode in (GEO_MODE_FAN, GEO_MODE_ADAPTIVE):
        assert call(with_flags(scene, base | GEO_FLAG_SS4, mode)) == GEO_EINVAL, mode
    for fl in (GEO_FLAG_MIPS, GEO_FLAG_COMPOSITE, GEO_FLAG_RING_F64):
        assert call(with_flags(scene, base | GEO_FLAG_SS4 | fl)) == GEO_EINVAL, fl
    # colour only
    outs = ["mask", "uv", "steps"] + {"plain": [], "disk": ["hits"], "shift": ["hits", "g"]}[kind]
    for o in outs:
        assert call(ok, **{o: True}) == GEO_EINVAL, o
    if kind == "shift":  # out_g refuses the call whether a shift is given or not
        assert call(ok, shift=None) == GEO_OK
        assert call(ok, shift=None, g=True) == GEO_EINVAL
    # twice the size must be a size the plain render takes (2^20 a side)
    assert call(ok, ww=(1 << 19) + 1, nrows=1) == GEO_EINVAL
    assert call(ok, hh=(1 << 19) + 1, nrows=1) == GEO_EINVAL
    # the entry points' own flag rules stand: geo_render_cpu takes no disk flag, the disk ones need it
    other = with_flags(scene, GEO_FLAG_SS4 | (GEO_FLAG_DISK if kind == "plain" else 0))
    assert call(other) == GEO_EINVAL
    # rows past the frame, in output rows
    assert call(ok, row0=h - 1, nrows=2) == GEO_EINVAL
    # without the flag the optional outputs are taken as before
    assert call(with_flags(scene, base), mask=True, uv=True, steps=True) == GEO_OK


def test_golden_frame(cpu):
    """tests/golden/frame_disk_ss.png (pose B's observer and disk, 480 x 270,
    `tools/render_frame.py tests/golden/frame_disk_ss.png --disk 1.6 2.2 --ss --cpu
    --width 480 --height 270`: frame_disk.png's frame, supersampled) is what
    the CPU path draws, byte for byte."""
    from schwarzschild_raytracer_wgpu_amd import imageio
    from schwarzschild_raytracer_wgpu_amd.scenes import make_disk_texture, make_sky

    w, h = 480, 270
    frame, scene, disk, _ = T.pose("B", w, h)
    sky = make_sky("equirect", (2048, 1024))
    rc, got, _ = ss_render(cpu, "disk", frame, ss_scene(scene, "disk"), w, h, disk, tex=make_disk_texture((1024, 128)),
                           sky=sky, threads=0)
    assert rc == GEO_OK
    gold = imageio.load_texture(os.path.join(T.ROOT, "tests", "golden", "frame_disk_ss.png"))
    assert gold.shape == (h, w, 4)
    diff = (got != gold).any(axis=-1)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the golden frame"
    plain = imageio.load_texture(os.path.join(T.ROOT, "tests", "golden", "frame_disk.png"))
    assert (plain != gold).any(axis=-1).sum() > 1000  # not the one-sample frame
