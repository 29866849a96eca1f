"""The colour stage of the CPU path (include/geo/geo_cpu.h) against the
independent f64 sampler tests/sampler_ref.py: every pixel and channel of plain
sky frames (three poses, noise, ramp and extreme-size skies), GEO_FLAG_COMPOSITE,
GEO_FLAG_MIPS, the thin disk (the three images' order included) and
GEO_FLAG_SS4 must lie inside the reference's derived bound, the frames must
reach the seam, both poles, every mip level and the multiply-hit disk pixels,
and each mutation of the reference must be caught.  The builders below take a
renderer, so tests/test_gpu_sampler.py holds the kernels to the same checks."""
import ctypes
import math

import numpy as np
import pytest

import sampler_ref as SR
import test_disk_cpu as T
import test_disk_ring_cpu as R
import test_ss_cpu as S
from helpers import POS, R_OBS, default_frame
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_FLAG_COMPOSITE, GEO_FLAG_DISK, GEO_FLAG_MIPS, GEO_FLAG_SS4,
                                                   GEO_MODE_ADAPTIVE, GEO_MODE_DIRECT, GEO_OK)

W, H = 64, 36
STEP = math.pi / 100


def noise(w, h, seed=None):
    seed = w * 131 + h if seed is None else seed
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 4), dtype=np.uint8)


def ramp(w, h):
    """Opaque: R rises with x, G with y, B falls along the diagonal."""
    x = np.arange(w)[None, :] * 255 // (w - 1) + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] * 255 // (h - 1) + np.zeros((1, w), np.int64)
    return np.stack([x, y, 255 - (x + y) // 2, np.full_like(x, 255)], axis=-1).astype(np.uint8)


SKIES = {
    "noise16x8": lambda: noise(16, 8),
    "noise37x19": lambda: noise(37, 19),
    "ramp64x32": lambda: ramp(64, 32),
    "1x1": lambda: noise(1, 1),
    "1x5": lambda: noise(1, 5),
    "6x1": lambda: noise(6, 1),
    "3x3": lambda: noise(3, 3),
    "4096x2": lambda: noise(4096, 2),
    "2^20x1": lambda: noise(1 << 20, 1),  # the widest geo_set_sky takes: the tw 2^-24 term leads
    "noise128x64": lambda: noise(128, 64),
    "noise512x256": lambda: noise(512, 256),
}
_SKY = {}


def sky_of(name):
    if name not in _SKY:
        _SKY[name] = SKIES[name]()
        _SKY[name].setflags(write=False)
    return _SKY[name]


PLAIN_SKIES = ("noise16x8", "noise37x19", "ramp64x32")
EXTREME_SKIES = ("1x1", "1x5", "6x1", "3x3", "4096x2", "2^20x1")
POSES = ("default", "flat_up", "flat_down_seam")
DTEX = noise(12, 5, seed=99)


def pose(name, w=W, h=H, flags=0, mode=GEO_MODE_DIRECT):
    """frame, scene"""
    if name == "default":
        return default_frame(w, h), make_scene(1.0, 50.0, R_OBS, STEP, 2048, mode, flags)
    cam, pos = {"flat_up": ((math.pi, 1.2), POS), "flat_down_seam": ((0.0, -1.2), (-2.5, 0.0, 0.1)),
                "flat_mips": ((math.pi, 0.4), POS)}[name]
    return (default_frame(w, h, pos=pos, camera=cam, rs=0.0, state=0),
            make_scene(0.0, 50.0, R_OBS, STEP, 512, mode, flags))


class Cpu:
    """The CPU path's entry points as the builders call them."""
    name = "cpu"

    def __init__(self):
        self.lib = R.load_cpu()

    def plain(self, frame, scene, sky, w, h, target=None):
        sky = np.ascontiguousarray(sky)
        rgba = np.zeros((h, w, 4), np.uint8) if target is None else np.array(target, np.uint8, order="C")
        mask = np.empty((h, w), np.uint8)
        uv = np.empty((h, w, 2), np.float32)
        total = ctypes.c_ulonglong()
        rc = self.lib.geo_render_cpu(ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1],
                                     sky.shape[0], None, 0, w, h, 0, h, 1, 4, rgba.ctypes.data, mask.ctypes.data,
                                     uv.ctypes.data, None, ctypes.addressof(total))
        assert rc == GEO_OK
        return dict(rgba=rgba, mask=mask, uv=uv)

    def disk(self, frame, scene, sky, w, h, disk_args, tex, ring=False):
        dk = T.make_disk(*disk_args)
        if ring:
            rc, a = R.render(self.lib, frame, scene, dk, 1, w=w, h=h, tex=tex, sky=sky)
        else:
            rc, a = T.render(self.lib, frame, scene, sky, w, h, dk, tex)
        assert rc == GEO_OK
        return a

    def ss(self, kind, frame, scene, sky, w, h, disk_args=None, tex=None):
        dk = None if disk_args is None else T.make_disk(*disk_args)
        rc, rgba, _ = S.ss_render(self.lib, kind, frame, scene, w, h, dk, tex=DTEX if tex is None else tex, sky=sky)
        assert rc == GEO_OK
        return rgba


@pytest.fixture(scope="module")
def cpu():
    return Cpu()


def report(label, rgba, c, e, valid=None):
    """Prints the worst error and the mean bound; returns the pixels outside the bound."""
    err, over = SR.outside(rgba, c, e)
    if valid is not None:
        over = over & valid[..., None]
        err = err * valid[..., None]
    n = int(over.any(axis=-1).sum())
    print(f"{label}: worst error {err.max():.3f} levels, mean bound {e.mean():.3f}, outside {n}")
    return n


# ---- builders: a render and its reference as a function of the mutation ----
# Each returns (rgba, ref, valid, info): ref(mutation) -> (c, e); valid: the
# pixels that count (None: all); info: what the reach assertions read.

def build_plain(r, pname, sname, composite=False):
    sky = sky_of(sname)
    frame, scene = pose(pname, flags=GEO_FLAG_COMPOSITE if composite else 0)
    target = noise(W, H, seed=4242) if composite else None
    a = r.plain(frame, scene, sky, W, H, target)
    s = SR.bilinear(sky, a["uv"][..., 0], a["uv"][..., 1])
    live = a["mask"] == 0
    info = dict(seam=int((s.seam & live).sum()), pole_lo=int((s.pole_lo & live).sum()),
                pole_hi=int((s.pole_hi & live).sum()), captured=int((~live).sum()),
                vmin=float(a["uv"][..., 1][live].min()), vmax=float(a["uv"][..., 1][live].max()))
    return a["rgba"], (lambda m=None: SR.sky(sky, a["uv"], a["mask"], target, m)[:2]), None, info


def build_mips(r, pname, sname, w, h, mode=GEO_MODE_DIRECT):
    sky = sky_of(sname)
    frame, scene = pose(pname, w, h, GEO_FLAG_MIPS, mode)
    a = r.plain(frame, scene, sky, w, h)
    cap = a["mask"] == 1
    # whole frame-aligned quads that hold a captured pixel do not count
    q = cap[0::2, 0::2] | cap[0::2, 1::2] | cap[1::2, 0::2] | cap[1::2, 1::2]
    valid = ~np.repeat(np.repeat(q, 2, axis=0), 2, axis=1)
    lam = SR.lod(a["uv"], sky.shape[1], sky.shape[0])[valid]
    info = dict(excluded=float(1.0 - valid.mean()),
                classes=[int((lam == 0).sum()), int(((lam > 0) & (lam < 1)).sum()), int(((lam >= 1) & (lam < 2)).sum()),
                         int(((lam >= 2) & (lam < 3)).sum()), int((lam == 3).sum())])
    return a["rgba"], (lambda m=None: SR.sky_mips(sky, a["uv"], a["mask"], None, m)[:2]), valid, info


def build_disk(r, name, ring=False, w=W, h=H):
    sky = sky_of("noise16x8")
    frame, scene, _, disk_args = T.pose(name, w, h)
    a = r.disk(frame, scene, sky, w, h, disk_args, DTEX, ring)
    hit = a["hits"][..., 0] > 0.0
    info = dict(two=int((hit.sum(axis=-1) >= 2).sum()), slot2=int(hit[..., 2].sum()), any=int(hit.any(axis=-1).sum()))

    def ref(m=None):
        c, e, _ = SR.sky(sky, a["uv"], a["mask"], None, m)
        return SR.disk(c, e, a["hits"], DTEX, disk_args[0], disk_args[1], m)

    return a["rgba"], ref, None, info


def build_ss(r, kind):
    """The supersampled 32 x 18 frame against the reference built from the
    one-sample 64 x 36 render's uv, mask and hits (the same 32 x 18 uniform)."""
    w, h = W // 2, H // 2
    sky = sky_of("noise16x8")
    if kind == "plain":
        frame = default_frame(w, h)
        one = make_scene(1.0, 50.0, R_OBS, STEP, 2048)
        a = r.plain(frame, one, sky, W, H)
        got = r.ss("plain", frame, S.with_flags(one, GEO_FLAG_SS4), sky, w, h)
        disk_args = None
    else:
        frame, one, _, disk_args = T.pose("B", w, h)
        a = r.disk(frame, one, sky, W, H, disk_args, DTEX)
        got = r.ss("disk", frame, S.with_flags(one, GEO_FLAG_SS4 | GEO_FLAG_DISK), sky, w, h, disk_args, DTEX)

    def ref(m=None):
        c, e, _ = SR.sky(sky, a["uv"], a["mask"], None, m)
        if disk_args is not None:
            c, e = SR.disk(c, e, a["hits"], DTEX, disk_args[0], disk_args[1], m)
        return SR.ss4(c, e)

    return got, ref, None, {}


# ---- the checks, shared with tests/test_gpu_sampler.py ----

def check_plain(r, pname, sname):
    rgba, ref, _, info = build_plain(r, pname, sname)
    print(pname, sname, info)
    assert report(f"{r.name} plain {pname} {sname}", rgba, *ref()) == 0
    if sname == "noise16x8":
        if pname == "flat_down_seam":
            assert info["seam"] >= 50 and info["pole_hi"] >= 24
        if pname == "flat_up":
            assert info["pole_lo"] >= 24 and info["vmin"] < 0.02
        if pname == "default":
            assert info["captured"] > 0 and info["seam"] >= 1


def check_composite(r):
    """A random target under the translucent sky; and under the opaque ramp,
    which replaces it outside the shadow.  Captured pixels keep the target."""
    for sname in ("noise16x8", "ramp64x32"):
        rgba, ref, _, info = build_plain(r, "default", sname, composite=True)
        assert info["captured"] > 0
        assert report(f"{r.name} composite {sname}", rgba, *ref()) == 0


def check_mips_flat(r):
    classes = np.zeros(5, np.int64)
    for sname in ("noise128x64", "noise512x256"):
        rgba, ref, valid, info = build_mips(r, "flat_mips", sname, W, H)
        assert info["excluded"] == 0.0
        assert report(f"{r.name} mips flat {sname}", rgba, *ref(), valid) == 0
        print(sname, "lambda = 0, (0,1), [1,2), [2,3), = 3:", info["classes"])
        classes += info["classes"]
    assert (classes > 0).all(), classes


def check_mips_curved(r, mode):
    rgba, ref, valid, info = build_mips(r, "default", "noise512x256", 128, 72, mode)
    print("excluded share", info["excluded"], "lambda classes", info["classes"])
    assert 0.0 < info["excluded"] < 0.15
    assert report(f"{r.name} mips curved mode {mode}", rgba, *ref(), valid) == 0


def check_disk(r, name, ring=False):
    rgba, ref, _, info = build_disk(r, name, ring)
    print(name, info)
    assert info["any"] > 0
    if name == "A":
        assert info["two"] >= 6
    if name == "B":
        assert info["two"] >= 6 and info["slot2"] >= 1
    assert report(f"{r.name} disk {name}{' ring f64' if ring else ''}", rgba, *ref()) == 0


def check_ss(r, kind):
    rgba, ref, _, _ = build_ss(r, kind)
    assert report(f"{r.name} ss4 {kind}", rgba, *ref()) == 0


# ---- the CPU path ----

@pytest.mark.parametrize("sname", PLAIN_SKIES + EXTREME_SKIES)
@pytest.mark.parametrize("pname", POSES)
def test_plain(cpu, pname, sname):
    check_plain(cpu, pname, sname)


def test_composite(cpu):
    check_composite(cpu)


def test_mips_flat_reaches_every_level(cpu):
    check_mips_flat(cpu)


@pytest.mark.parametrize("mode", [GEO_MODE_DIRECT, GEO_MODE_ADAPTIVE], ids=["direct", "adaptive"])
def test_mips_curved(cpu, mode):
    check_mips_curved(cpu, mode)


@pytest.mark.parametrize("name", ["A", "B", "tilted"])
def test_disk(cpu, name):
    check_disk(cpu, name)


def test_disk_ring_f64(cpu):
    check_disk(cpu, "B", ring=True)


@pytest.mark.parametrize("kind", ["plain", "disk"])
def test_ss4(cpu, kind):
    check_ss(cpu, kind)


# mutation: (the frames to look in, the pixels outside the bound one of them must reach).
# 100 for every sampler and mip mutation that changes the whole frame, 10 for the
# two that change seam and pole quads only, 4 for the order of the disk's images
# (it shows only where two slots are hit), 1 for the other disk mutations.
SAMPLER_FRAMES = [("plain", p, s) for p in POSES for s in PLAIN_SKIES]
MIP_FRAMES = [("mips", "flat_mips", "noise128x64"), ("mips", "flat_mips", "noise512x256")]
DISK_FRAMES = [("disk", n) for n in ("A", "B", "tilted")]
CAUGHT = {
    "no_half_texel": (SAMPLER_FRAMES, 100),
    "swap_weights": (SAMPLER_FRAMES, 100),
    "nearest": (SAMPLER_FRAMES, 100),
    "swap_rb": (SAMPLER_FRAMES, 100),
    "lod_plus_one": (MIP_FRAMES, 100),
    "no_lod": (MIP_FRAMES, 100),
    "nearest_level": (MIP_FRAMES, 100),
    # these two differ from the truth in seam and pole quads only
    "clamp_u": ([("plain", "flat_down_seam", "noise16x8")], 10),
    "wrap_v": ([("plain", "flat_down_seam", "noise16x8")], 10),
    "disk_swap_uv": (DISK_FRAMES, 1),
    "disk_flip_v": (DISK_FRAMES, 1),
    "disk_order_reversed": ([("disk", "A")], 4),
    "disk_slot0_only": (DISK_FRAMES, 1),
}


def test_mutations_are_caught(cpu):
    """Every mutation of the reference puts the true render outside the bound:
    the bounds are tight enough, and the inputs reach far enough, to see each
    of the mistakes the specification could hold."""
    assert set(CAUGHT) == set(SR.MUTATIONS)
    built = {}
    for m, (frames, floor) in CAUGHT.items():
        best = 0
        for key in frames:
            if key not in built:
                built[key] = (build_plain(cpu, *key[1:]) if key[0] == "plain" else
                              build_mips(cpu, key[1], key[2], W, H) if key[0] == "mips" else build_disk(cpu, key[1]))
            rgba, ref, valid, _ = built[key]
            _, over = SR.outside(rgba, *ref(m))
            if valid is not None:
                over = over & valid[..., None]
            best = max(best, int(over.any(axis=-1).sum()))
        print(f"mutation {m}: {best} pixels outside the bound (floor {floor})")
        assert best >= floor, m
