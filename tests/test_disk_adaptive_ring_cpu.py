"""The adaptive disk with its capture band in f64 on the CPU path
(geo_render_cpu_disk_adaptive_ring_f64, include/geo/geo_cpu.h; geo.h,
geo_render_disk_adaptive_ring): the three properties of the call's definition,
the band against the independent f64 answer on fuzzed scenes, and the rules.
tests/test_gpu_disk_adaptive_ring.py ties the kernels to this path bit for bit.

Properties, per pixel and in every output (colour, mask, UV, steps, hits, g, q):
  1. outside the band: the state-off render, geo_render_cpu_disk_adaptive;
  2. inside the band: the GEO_MODE_DIRECT ring render of the same rs, sphere_r,
     r_obs, step and max_steps (geo_render_cpu_disk_ring_f64 /
     geo_render_cpu_disk_shift_ring_f64 with the state on), steps included;
  3. mask, UV, steps and steps_total of the frame: the plain adaptive render with
     GEO_FLAG_RING_F64 in place of GEO_FLAG_DISK.
Band membership comes from disk_ref.trace(sub=1)'s x = |b/b_c - 1| with
disk_ring_ref.BAND -/+ GUARD, as tests/disk_band_truth.py takes it: the pixels
between the two guards belong to neither side (the band test is on the f32 ray).
x depends on the ray and on rs and r_obs only, so one trace per pose serves
every step, budget and tol.

Poses `ring` (the third image: 2 212 band pixels, 148 in-band hits, all in slot
2), `B` (26 and 12, slots 0 and 1) and `A` (no band pixel) of
tests/test_disk_cpu.py at 96 x 54, unshaded, shifted and with the emission; then
properties 1 and 2 again, with the emission (which writes every output), at
steps 0.8 and 0.5 (132 and 152 in-band hits on `ring`), budget 300 (not the
budget-limited case: the in-band lanes of `ring` end after 209 to 300 steps,
some of them on the budget, and keep their 148 hits), budget 47 (the
budget-limited case: every in-band lane ends on the budget, in-band hits 0 on
`ring`, 8 on `B`) and tol 1e-7 and 1e30 at step 0.3; and on three of the
scene generator's kCurvedIn seeds (tests/disk_step_truth.py) with in-band hits.
The floors beside the measured counts are round numbers no higher than half of
them.

Truth: tests/disk_band_truth.py's layer unchanged, with a renderer that draws
the case's direct truth scene in GEO_MODE_ADAPTIVE (tol 0) through the new
function.  By property 2 the compared values are the direct ring render's, so
no constant of that module moves: 1 084 slots on 320 seeds, 116 in slot 2, 0
dropped, the largest shares of a bar 0.88 (radius), 0.54 (g), 0.47 (q).  With
the state off the radius bar fails on 89 seeds (floor 40)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import disk_band_truth as B
import disk_ref as D
import disk_ring_ref as R
import disk_step_truth as ST
import disk_truth as DT
import test_disk_adaptive_cpu as A
import test_disk_cpu as T
import test_disk_emission_cpu as TE
import test_disk_ring_cpu as RC
import test_disk_truth_cpu as TC
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import _lib, make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_EINVAL, GEO_FLAG_COMPOSITE, GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK,
                                                   GEO_FLAG_MIPS, GEO_FLAG_RING_F64, GEO_FLAG_SS4, GEO_MODE_ADAPTIVE,
                                                   GEO_MODE_DIRECT, GEO_MODE_FAN, GEO_OK, GeoDiskEmission,
                                                   GeoDiskShift)

W, H = T.W, T.H
SHIFT = (1, 4, 1.0)
VARIANTS = {"plain": dict(), "shift": dict(shift=SHIFT), "emission": dict(em=TE.emission())}
FIELDS = ("rgba", "mask", "steps")
BITS = ("uv", "hits", "g", "q")
# name: (step, max_steps (None: the pose's), tol)
CONFIGS = {
    "default": (T.STEP, None, 0.0),
    "step0.8": (0.8, None, 0.0),
    "step0.5": (0.5, None, 0.0),
    "budget300": (T.STEP, 300, 0.0),
    "budget47": (T.STEP, 47, 0.0),
    "tol1e-7_step0.3": (0.3, None, 1e-7),
    "tol1e30_step0.3": (0.3, None, 1e30),
}
# kCurvedIn scenes of the generator with in-band hits: seed -> the floor of the reference's in-band hits
CURVED_IN = {161: 25, 57: 20, 334: 18}  # (measured 50, 41 and 37)


def load_cpu():
    lib = RC.load_cpu()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    adaptive = [vp, vp, vp, u32, u32, vp, u32, u32, u32, u32, u32, u32, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, u32,
                u32, vp, vp, vp, u32, vp, vp, vp]
    lib.geo_render_cpu_disk_adaptive.restype = ctypes.c_int
    lib.geo_render_cpu_disk_adaptive.argtypes = adaptive
    lib.geo_render_cpu_disk_adaptive_ring_f64.restype = ctypes.c_int
    lib.geo_render_cpu_disk_adaptive_ring_f64.argtypes = adaptive + [ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def cpu():
    return load_cpu()


def render(lib, frame, scene, disk, ring=1, w=W, h=H, tex=T.TEX, shift=None, em=None, ramp=TE.RAMP, sky=T.SKY, row0=0,
           nrows=None, threads=4):
    """geo_render_cpu_disk_adaptive_ring_f64 (test_disk_adaptive_cpu.render's
    arguments and outputs, with the state `ring`)."""
    nrows = h - row0 if nrows is None else nrows
    sky = np.ascontiguousarray(sky, dtype=np.uint8)
    tex = np.ascontiguousarray(tex, dtype=np.uint8)
    rgba = np.zeros((nrows, w, 4), np.uint8)
    mask = np.empty((nrows, w), np.uint8)
    uv = np.empty((nrows, w, 2), np.float32)
    steps = np.empty((nrows, w), np.uint32)
    total = ctypes.c_ulonglong()
    hits = np.full((nrows, w, 3, 2), -1.0, np.float32)
    g = np.full((nrows, w, 3), -1.0, np.float32)
    q = np.full((nrows, w, 3), -1.0, np.float32)
    e = None if em is None else GeoDiskEmission(*em)
    s = None if shift is None else GeoDiskShift(*shift)
    rmp = None if (ramp is None or em is None) else np.ascontiguousarray(ramp, dtype=np.uint8)
    rc = lib.geo_render_cpu_disk_adaptive_ring_f64(
        ctypes.addressof(frame), ctypes.addressof(scene), sky.ctypes.data, sky.shape[1], sky.shape[0], None, 0, w, h,
        row0, nrows, 1, threads, rgba.ctypes.data, mask.ctypes.data, uv.ctypes.data, steps.ctypes.data,
        ctypes.addressof(total), None if disk is None else ctypes.addressof(disk), tex.ctypes.data, tex.shape[1],
        tex.shape[0], hits.ctypes.data, None if e is None else ctypes.addressof(e),
        None if rmp is None else rmp.ctypes.data, 0 if rmp is None else rmp.shape[0], g.ctypes.data, q.ctypes.data,
        None if s is None else ctypes.addressof(s), ring)
    return rc, dict(rgba=rgba, mask=mask, uv=uv, steps=steps, total=total.value, hits=hits, g=g, q=q)


def scenes_of(scene, step=None, max_steps=None, tol=0.0):
    """(the adaptive disk scene, the direct disk scene, the plain adaptive GEO_FLAG_RING_F64 scene) of one
    rs, sphere_r, r_obs, step and budget."""
    step = scene.step if step is None else step
    ms = scene.max_steps if max_steps is None else max_steps
    mk = lambda mode, flags, t: make_scene(scene.rs, scene.sphere_r, scene.r_obs, step, ms, mode, flags, t)
    return (mk(GEO_MODE_ADAPTIVE, GEO_FLAG_DISK, tol), mk(GEO_MODE_DIRECT, GEO_FLAG_DISK, 0.0),
            mk(GEO_MODE_ADAPTIVE, GEO_FLAG_RING_F64, tol))


def four(lib, frame, scene, disk, w=W, h=H, ramp=TE.RAMP, **cfg):
    """The call with the state on, geo_render_cpu_disk_adaptive (state off), the direct ring render with
    the state on, and the plain adaptive ring render, of one frame; variant: shift=, em=."""
    shade = {k: v for k, v in cfg.items() if k in ("shift", "em")}
    adaptive, direct, plain = scenes_of(scene, **{k: v for k, v in cfg.items() if k not in ("shift", "em")})
    rc, on = render(lib, frame, adaptive, disk, 1, w, h, ramp=ramp, **shade)
    assert rc == GEO_OK
    rc, off = A.render(lib, frame, adaptive, w, h, disk, ramp=ramp, **shade)
    assert rc == GEO_OK
    rc, ring = RC.render(lib, frame, direct, disk, 1, w, h, ramp=ramp, **shade)
    assert rc == GEO_OK
    rc, sky = T.render(lib, frame, plain, T.SKY, w, h)
    assert rc == GEO_OK
    return on, off, ring, sky


def differing(a, b, where):
    return [f for f in FIELDS + BITS if not np.array_equal((a[f].view(np.uint32) if f in BITS else a[f])[where],
                                                           (b[f].view(np.uint32) if f in BITS else b[f])[where])]


def check_properties(on, off, ring, sky, x):
    """Properties 1, 2 and 3 of a frame whose reference x = |b/b_c - 1| is `x`; (band pixels, in-band hits
    of the direct ring render)."""
    inside, outside = x < R.BAND - R.GUARD, x >= R.BAND + R.GUARD
    assert not differing(on, off, outside), ("property 1", differing(on, off, outside))
    assert not differing(on, ring, inside), ("property 2", differing(on, ring, inside))
    assert np.array_equal(on["mask"], sky["mask"]) and np.array_equal(on["steps"], sky["steps"]), "property 3"
    assert np.array_equal(on["uv"].view(np.uint32), sky["uv"].view(np.uint32)), "property 3"
    assert on["total"] == sky["total"] == int(on["steps"].sum(dtype=np.uint64)), "property 3"
    return int(inside.sum()), int((ring["hits"][..., 0] > 0.0)[inside].sum())


@pytest.fixture(scope="module")
def refs():
    """disk_ref.trace(sub=1) of the three poses (their own step and budget): x, and the reference's hits."""
    out = {}
    for name in ("ring", "B", "A"):
        frame, scene, _, (r_in, r_out, normal, axis) = T.pose(name)
        out[name] = D.trace(frame, scene, W, H, r_in, r_out, normal, axis, sub=1)
    return out


def test_announced():
    hdr = open(os.path.join(T.ROOT, "include", "geo", "geo.h")).read()
    assert re.search(r"^#define GEO_HAS_DISK_ADAPTIVE_RING 1$", hdr, re.M)
    assert re.search(r"^#define GEO_ABI_VERSION 8\b", hdr, re.M)
    assert _lib.GEO_HAS_DISK_ADAPTIVE_RING == 1
    assert ctypes.CDLL(_lib.LIB_PATH).geo_render_disk_adaptive_ring  # exported (no GPU needed to look it up)
    assert _lib.lib.geo_abi_version() == 8


def test_off_is_the_adaptive_entry(cpu):
    """ring_f64 = 0 is geo_render_cpu_disk_adaptive."""
    frame, scene, disk, _ = T.pose("ring")
    sc = scenes_of(scene)[0]
    for kw in VARIANTS.values():
        rc, a = render(cpu, frame, sc, disk, 0, **kw)
        rcw, want = A.render(cpu, frame, sc, W, H, disk, **kw)
        assert rc == GEO_OK and rcw == GEO_OK
        assert not differing(a, want, np.ones((H, W), bool)) and a["total"] == want["total"]


# ---- properties 1 - 3 ------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["ring", "B", "A"])
def test_properties(cpu, refs, name, variant):
    frame, scene, disk, _ = T.pose(name)
    ref = refs[name]
    on, off, ring, sky = four(cpu, frame, scene, disk, **VARIANTS[variant])
    pixels, hits = check_properties(on, off, ring, sky, ref["x"])
    between = int(((ref["x"] >= R.BAND - R.GUARD) & (ref["x"] < R.BAND + R.GUARD)).sum())
    both = int(((ring["hits"][..., 0] > 0.0) & ref["hit"] & B.in_band(ref)[..., None]).sum())
    slots = [int(((ring["hits"][..., k, 0] > 0.0) & B.in_band(ref)).sum()) for k in range(3)]
    print(name, variant, "band pixels", pixels, "in-band hits", hits, "by slot", slots, "in the reference too", both,
          "between the guards", between, "steps_total", on["total"], "state off", off["total"])
    if name == "ring":
        assert pixels >= 2000 and hits >= 100 and both >= 100 and slots[2] == hits and between == 12
        assert on["total"] != off["total"]  # mixed units: adaptive attempts outside the band, f64 steps inside
    elif name == "B":
        assert pixels >= 20 and hits >= 8 and both >= 8 and slots[0] > 0 and slots[1] > 0 and between == 0
    else:
        assert pixels == 0 and not differing(on, off, np.ones((H, W), bool)) and on["total"] == off["total"]
    if variant == "plain":
        assert (on["g"] == -1.0).all()
    if variant != "emission":
        assert (on["q"] == -1.0).all()


# config: {pose: the floor of in-band hits (the measured count beside it)}
CONFIG_HITS = {"step0.8": {"ring": 66}, "step0.5": {"ring": 76}, "budget300": {"ring": 74, "B": 6},
               "budget47": {"B": 4}}  # 132, 152, 148 and 12, 8


@pytest.mark.parametrize("config", [c for c in CONFIGS if c != "default"])
@pytest.mark.parametrize("name", ["ring", "B"])
def test_properties_at_other_steps_budgets_and_tolerances(cpu, refs, name, config):
    frame, scene, disk, _ = T.pose(name)
    step, max_steps, tol = CONFIGS[config]
    on, off, ring, sky = four(cpu, frame, scene, disk, step=step, max_steps=max_steps, tol=tol, em=TE.emission())
    x = refs[name]["x"]
    pixels, hits = check_properties(on, off, ring, sky, x)
    print(name, config, "band pixels", pixels, "in-band hits", hits)
    assert pixels >= (2000 if name == "ring" else 20)
    assert hits >= CONFIG_HITS.get(config, {}).get(name, 0)
    inside = x < R.BAND - R.GUARD
    print("in-band steps", int(on["steps"][inside].min()), "..", int(on["steps"][inside].max()))
    if config == "budget300" and name == "ring":
        assert (on["steps"][inside] == 300).any() and (on["steps"][inside] < 300).any()
    if config == "budget47":
        assert (on["steps"][inside] == 47).all()  # every in-band lane ends on the budget
        if name == "ring":
            assert hits == 0
    if tol != 0.0:
        # the tolerance is the f32 lanes' alone: the band's pixels do not read it
        other = four(cpu, frame, scene, disk, step=step, max_steps=max_steps, tol=0.0, em=TE.emission())[0]
        assert not differing(on, other, inside)
        assert differing(on, other, x >= R.BAND + R.GUARD)


@pytest.mark.parametrize("seed", list(CURVED_IN))
def test_properties_on_kcurvedin_scenes(cpu, seed):
    """The generator's own scenes (64 x 36, the seed's step, budget, observer and emission), whose
    integration kind is kCurvedIn: geodesic_angle_adaptive_disk<kCurvedIn> beside the band."""
    c = ST.case_of(seed)
    ref = ST.reference(seed)
    assert c.kind == 1, c.desc
    floor = CURVED_IN[seed]
    in_band_hits = int((ref["hit"] & B.in_band(ref)[..., None]).sum())
    print(c.desc, "in-band hits of the reference", in_band_hits)
    assert in_band_hits >= floor
    on, off, ring, sky = four(cpu, c.frame, c.direct, T.make_disk(*c.disk_args), DT.W, DT.H, ramp=c.ramp, em=c.em)
    pixels, hits = check_properties(on, off, ring, sky, ref["x"])
    assert pixels >= 40 and hits >= floor


def test_row_range_and_threads(cpu):
    frame, scene, disk, _ = T.pose("B")
    sc = scenes_of(scene)[0]
    rc, full = render(cpu, frame, sc, disk, 1, em=TE.emission())
    rc2, a = render(cpu, frame, sc, disk, 1, em=TE.emission(), row0=17, nrows=20, threads=1)
    assert rc == GEO_OK and rc2 == GEO_OK
    for f in FIELDS + BITS:
        assert np.array_equal(a[f].view(np.uint32) if f in BITS else a[f],
                              (full[f].view(np.uint32) if f in BITS else full[f])[17:37]), f
    assert a["total"] == int(full["steps"][17:37].sum(dtype=np.uint64))


# ---- the band against the f64 answer on fuzzed scenes --------------------------------------
class Cpu(TC.Cpu):
    """disk_band_truth's renderer: the case's direct truth scene (its rs, sphere_r, r_obs, step and budget)
    in GEO_MODE_ADAPTIVE, tol 0, through geo_render_cpu_disk_adaptive_ring_f64 (every render kept)."""

    def __init__(self):
        super().__init__()
        self.ring_lib = load_cpu()

    def ring(self, c, what, on=True):
        kw = dict(shift=c.shift) if what == "ring_shift" else dict(em=c.em) if what == "ring_emission" else {}
        return self._keep((what, on, c.seed), lambda: render(
            self.ring_lib, c.frame, scenes_of(c.direct)[0], T.make_disk(*c.disk_args), int(on), DT.W, DT.H,
            ramp=c.ramp, threads=TC.THREADS, **kw))


@pytest.fixture(scope="module")
def truth():
    B.prefetch(B.TEST_SEEDS)
    return Cpu()


@pytest.mark.parametrize("what", list(B.WHAT))
def test_band_against_the_f64_answer(truth, what):
    s = DT.check(truth, what, B.TEST_SEEDS, layer=B)
    assert s["compared"] >= 600 and s["slot2"] >= 60
    assert s["dropped"] <= 0.001 * s["compared"]


def test_state_off_fails(truth):
    """ring_f64 = 0 (geo_render_cpu_disk_adaptive) breaks the band's radius bar: the feature carries the
    result above, not the bar."""
    failed = 0
    for seed in B.TEST_SEEDS:
        c = B.case_of(seed)
        failed += B.judge(B.errors(c, "ring", B.render(truth, "ring", c, on=False)))["radius"] > 0
    print(f"state off: the radius bar fails on {failed} seeds (floor {B.STATE_OFF_FLOOR})")
    assert failed >= B.STATE_OFF_FLOOR


# ---- the rules -------------------------------------------------------------------------------
def test_rules(cpu):
    frame, scene, disk, _ = T.pose("A")
    w, h = 16, 9
    frame = default_frame(w, h, pos=T.POSES["A"][0], camera=T.POSES["A"][1], fov=T.POSES["A"][2])

    def rc_of(sc, dk=disk, ring=1, **kw):
        return render(cpu, frame, sc, dk, ring, w, h, **kw)[0]

    def sc(rs=1.0, mode=GEO_MODE_ADAPTIVE, flags=GEO_FLAG_DISK, tol=0.0):
        return make_scene(rs, 50.0, scene.r_obs, T.STEP, 256, mode, flags, tol)

    for ring in (0, 1):
        assert rc_of(sc(), ring=ring) == GEO_OK
        assert rc_of(sc(flags=GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS), ring=ring) == GEO_OK
        assert rc_of(sc(rs=0.0), ring=ring) == GEO_OK
        # a flag beside DISK / DEFER_STEPS, SS4 among them
        for fl in (GEO_FLAG_MIPS, GEO_FLAG_COMPOSITE, GEO_FLAG_RING_F64, GEO_FLAG_SS4):
            assert rc_of(sc(flags=GEO_FLAG_DISK | fl), ring=ring) == GEO_EINVAL
        assert rc_of(sc(flags=0), ring=ring) == GEO_EINVAL
        # the direct and fan scenes are the older functions'
        for mode in (GEO_MODE_DIRECT, GEO_MODE_FAN):
            assert rc_of(sc(mode=mode), ring=ring) == GEO_EINVAL
        assert rc_of(sc(), dk=None, ring=ring) == GEO_EINVAL
        for tol in (-1.0, math.inf, math.nan):
            assert rc_of(sc(tol=tol), ring=ring) == GEO_EINVAL
        # the shift's and the emission's rules, and r_in > 1.5 rs with either
        assert rc_of(sc(), ring=ring, shift=SHIFT) == GEO_OK and rc_of(sc(), ring=ring, em=TE.emission()) == GEO_OK
        for shift in ((0, 4, 1.0), (1, 5, 1.0), (1, 4, 0.0)):
            assert rc_of(sc(), ring=ring, shift=shift) == GEO_EINVAL
        for em in (TE.emission(spin=0), TE.emission(profile=2), TE.emission(t_lo=3000.0, t_hi=2000.0)):
            assert rc_of(sc(), ring=ring, em=em) == GEO_EINVAL
        dk = T.make_disk(3.0, 9.0)
        assert rc_of(sc(rs=2.5), dk=dk, ring=ring) == GEO_OK
        assert rc_of(sc(rs=2.5), dk=dk, ring=ring, shift=SHIFT) == GEO_EINVAL
        assert rc_of(sc(rs=2.5), dk=dk, ring=ring, em=TE.emission()) == GEO_EINVAL


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_no_capture_orbit_ignores_the_state(cpu, variant):
    """rs = 0 with the state on is geo_render_cpu_disk_adaptive byte for byte."""
    frame, scene, disk, _ = T.pose("flat")
    sc = scenes_of(scene)[0]
    rc, a = render(cpu, frame, sc, disk, 1, **VARIANTS[variant])
    rcw, want = A.render(cpu, frame, sc, W, H, disk, **VARIANTS[variant])
    assert rc == GEO_OK and rcw == GEO_OK
    assert not differing(a, want, np.ones((H, W), bool)) and a["total"] == want["total"]
    assert (a["hits"][..., 0, 0] > 0.0).sum() > 300
