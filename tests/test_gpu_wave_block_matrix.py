"""Every kernel on the wave-block grid, reached once: one cell per instantiation
of the sky-only SS4 kernel, the one-frame disk kernel, the disk batch kernel and
the ring kernels (geo_render_kernels.h), each drawn through the public entry
point that the call rules (geo_render_rules.h) give it and compared, all bytes,
with the CPU path of include/geo/geo_cpu.h.

  integration kind  kCurvedOut, kCurvedIn, kFlat
  shade             plain, shift (geo_set_disk_shift), emission (geo_set_disk_emission)
  form              frame direct / adaptive / SS4, batch direct / adaptive / SS4 / adaptive SS4
  ring              geo_set_disk_ring_f64 on, the curved kinds: frame direct / adaptive, batch, batch SS4
  sky               GEO_FLAG_SS4 without a disk: frame, batch

63 + 24 + 6 = 93 cells.  The other GPU tests compare these variants with the CPU
path on larger frames and more layouts; this one states that each instantiation
is reached, so a launcher that names the wrong one fails in exactly its cells.

Frames are 40 x 20 in bands of 8 rows: a partial tile in x (40 = 32 + 8) and a
last band clipped to rows 16 .. 19.  A batch has 2 frames, each with its own
observer radius, frame_stride larger than the packed size; the clipped rows and
the gap keep their prefill.  An SS4 cell is the box resolve
(test_ss_cpu.resolve) of the CPU path's one-sample render at 80 x 40 with the
40 x 20 frame's uniform.  A ring cell has pixels (samples, under SS4) in the
capture band (test_gpu_disk_ring_batch.in_band) and takes the band's lanes
through geo_render_cpu_disk_ring_f64 / _shift_ring_f64 with the state on.  An
adaptive ring frame is drawn through geo_render_disk_adaptive_ring on the same
band set of 8 rows (the rules take it for that entry point as they do for
geo_render_disk_adaptive) against test_disk_adaptive_ring_cpu.render, on the
ring cells' own scenes (the ring walk's frame 0; kCurvedIn at step 1): its
reference must differ from the adaptive state-off frame and from the direct
ring cell's of the same kind and shade, so a launcher that names the other
MODE fails in both of the pair's cells."""
import math

import numpy as np
import pytest

import test_disk_adaptive_cpu as A
import test_disk_adaptive_ring_cpu as AR
import test_disk_cpu as T
import test_disk_ring_cpu as RC
import test_gpu_disk_ring_batch as RB
from fuzz_disk_scenes import kind_of
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_FLAG_DISK, GEO_FLAG_SS4, GEO_MODE_ADAPTIVE, GEO_MODE_DIRECT,
                                                   GEO_OK)
from test_gpu_disk_emission import EM, set_emission
from test_ss_cpu import resolve

pytestmark = pytest.mark.gpu

W, H, BAND = 40, 20, 8
NB = (H + BAND - 1) // BAND
PACKED = NB * BAND * W * 4
STRIDE = PACKED + 4 * 37  # a batch's frame_stride
FILL = 7
SHIFT = (1, 4, 2.0)  # (gain 2: at rest in flat space g = 1, and gain 1 would draw the unshaded frame)
KINDS = {"curved_out": 0, "curved_in": 1, "flat": 2}
SHADES = ("plain", "shift", "emission")
# form: (frames, adaptive, SS4)
FORMS = {"frame": (1, False, False), "frame_adaptive": (1, True, False), "frame_ss4": (1, False, True),
         "batch": (2, False, False), "batch_adaptive": (2, True, False), "batch_ss4": (2, False, True),
         "batch_adaptive_ss4": (2, True, True)}
RING_FORMS = ("frame", "frame_adaptive", "batch", "batch_ss4")
SKY_FORMS = ("frame_ss4", "batch_ss4")

# (kind, shade or "sky", form, ring)
CELLS = ([(k, s, f, False) for k in KINDS for s in SHADES for f in FORMS] +
         [(k, s, f, True) for k in ("curved_out", "curved_in") for s in SHADES for f in RING_FORMS] +
         [(k, "sky", f, False) for k in KINDS for f in SKY_FORMS])
IDS = [f"{k}-{s}-{'ring_' if r else ''}{f}" for k, s, f, r in CELLS]


def test_the_matrix_has_a_cell_per_kernel():
    assert len(CELLS) == 93 and len(set(IDS)) == 93


def cell_scenes(kind, n, ring):
    """n frames and their direct-mode disk scenes of integration kind `kind`:
    pose "A" (pose "tilted" in flat space) of test_disk_cpu with the observer
    stepping outwards, or test_gpu_disk_ring_batch's ring walk; kCurvedIn by
    step 0.75 and 256 steps, as that walk has it (the ring cells by step 1: at
    40 x 20 the band then holds disk hits in both frames).  And the disk."""
    curved_in = kind == "curved_in"
    name = "ring" if ring else ("tilted" if kind == "flat" else "A")
    pos, cam, fov, rs, state, radii, normal, axis, ms = T.POSES[name]
    if ring:
        frames, scenes = RB.walk(W, H, n, curved_in)
        if curved_in:
            scenes = [make_scene(s.rs, s.sphere_r, s.r_obs, 1.0, s.max_steps, flags=GEO_FLAG_DISK) for s in scenes]
    else:
        frames, scenes = [], []
        for i in range(n):
            p = (pos[0] + 0.3 * i, pos[1], pos[2])
            frames.append(default_frame(W, H, pos=p, camera=cam, rs=rs, fov=fov, state=state))
            scenes.append(make_scene(rs, 50.0, math.sqrt(sum(v * v for v in p)), 0.75 if curved_in else T.STEP,
                                     256 if curved_in else ms, flags=GEO_FLAG_DISK))
    assert all(kind_of(s.rs, s.r_obs, s.step) == KINDS[kind] for s in scenes), kind
    assert len({s.r_obs for s in scenes}) == n
    return frames, scenes, radii + (normal, axis)


def scene_as(s, adaptive=False, ss=False, disk=True):
    return make_scene(s.rs, s.sphere_r, s.r_obs, s.step, s.max_steps, GEO_MODE_ADAPTIVE if adaptive else GEO_MODE_DIRECT,
                      (GEO_FLAG_DISK if disk else 0) | (GEO_FLAG_SS4 if ss else 0))


@pytest.fixture(scope="module")
def cpu():
    lib = A.load_cpu()
    ring = AR.load_cpu()  # (test_disk_ring_cpu's library with the adaptive ring entry point)
    return lib, ring


_REFS = {}


def reference(cpu, kind, shade, adaptive, ss, ring, f):
    """Frame f of the cell on the CPU path, as (H, W, 4) bytes: computed once per
    (kind, shade, integrator, SS4, ring, frame), shared and read-only."""
    key = (kind, shade, adaptive, ss, ring, f)
    if key not in _REFS:
        lib, ring_lib = cpu
        frames, scenes, disk = cell_scenes(kind, f + 1, ring)
        k = 2 if ss else 1
        state = dict(shift=SHIFT if shade == "shift" else None, em=EM if shade == "emission" else None)
        if shade == "sky":
            rc, c = T.render(lib, frames[f], scene_as(scenes[f], disk=False), T.SKY, k * W, k * H)
        elif adaptive and ring:
            rc, c = AR.render(ring_lib, frames[f], scene_as(scenes[f], adaptive=True), T.make_disk(*disk), 1, k * W,
                              k * H, **state)
        elif adaptive:
            rc, c = A.render(lib, frames[f], scene_as(scenes[f], adaptive=True), k * W, k * H, T.make_disk(*disk),
                             **state)
        else:
            rc, c = RC.render(ring_lib, frames[f], scenes[f], T.make_disk(*disk), 1 if ring else 0, w=k * W, h=k * H,
                              **state)
        assert rc == GEO_OK, key
        img = resolve(c["rgba"]) if ss else c["rgba"].copy()
        img.setflags(write=False)
        _REFS[key] = img
        # what lets a cell tell its kernel from its neighbours': the disk is in
        # view and its shade draws another frame than the unshaded disk; the
        # band holds pixels with a disk hit, and the state changes the frame
        if shade != "sky":
            hit = (c["hits"][..., 0] > 0.0).any(axis=-1)
            assert hit.any(), key
            if shade != "plain":
                assert not np.array_equal(img, reference(cpu, kind, "plain", adaptive, ss, ring, f)), key
            if ring:
                assert (RB.in_band(frames[f], scenes[f], k * W, k * H) & hit).sum() >= 1, key
                if adaptive:
                    rc, off = A.render(lib, frames[f], scene_as(scenes[f], adaptive=True), k * W, k * H,
                                       T.make_disk(*disk), **state)
                    assert not np.array_equal(img, reference(cpu, kind, shade, False, ss, ring, f)), key
                else:
                    rc, off = RC.render(ring_lib, frames[f], scenes[f], T.make_disk(*disk), 0, w=k * W, h=k * H,
                                        **state)
                assert rc == GEO_OK and not np.array_equal(off["rgba"], c["rgba"]), key
    return _REFS[key]


def draw(dev, kind, shade, form, ring):
    """The cell through its entry point: the output bytes as (frames, stride)."""
    import torch

    import schwarzschild_raytracer_wgpu_amd as g

    n, adaptive, ss = FORMS[form]
    frames, scenes, disk = cell_scenes(kind, n, ring)
    scenes = [scene_as(s, adaptive, ss, disk=shade != "sky") for s in scenes]
    ctx = g.Context(dev.index or 0)
    ctx.set_sky(T.SKY)
    if shade != "sky":
        ctx.set_disk(T.TEX, *disk)
    if shade == "shift":
        ctx.set_disk_shift(*SHIFT)
    if shade == "emission":
        set_emission(ctx, EM)
    ctx.set_disk_ring_f64(ring)
    stride = PACKED if n == 1 else STRIDE
    out = torch.full((n * stride,), FILL, dtype=torch.uint8, device=dev)
    if n == 1:
        one = ctx.render_disk_adaptive_ring if ring else ctx.render_disk_adaptive
        if not adaptive:
            one = ctx.render_band_set
        one(frames[0], scenes[0], W, H, BAND, 0, BAND, NB, out)
    else:
        if ring:
            many = ctx.render_disk_ring_batch
        elif adaptive:
            many = ctx.render_disk_adaptive_batch
        elif shade == "emission":
            many = ctx.render_emission_batch
        elif ss:
            many = ctx.render_ss_batch
        else:
            many = ctx.render_disk_batch
        many(frames, scenes, W, H, BAND, 0, BAND, NB, out, frame_stride=stride)
    torch.cuda.synchronize()
    ctx.close()
    return out.cpu().numpy().reshape(n, stride)


@pytest.mark.parametrize("kind,shade,form,ring", CELLS, ids=IDS)
def test_cell(dev, cpu, kind, shade, form, ring):
    n, adaptive, ss = FORMS[form]
    got = draw(dev, kind, shade, form, ring)
    for f in range(n):
        want = reference(cpu, kind, shade, adaptive, ss, ring, f)
        diff = int((got[f][:H * W * 4].reshape(H, W, 4) != want).sum())
        print(f"frame {f}: differing bytes {diff}")
        assert diff == 0, f
        assert (got[f][H * W * 4:] == FILL).all(), f  # the clipped rows of the last band, and a batch's gap
    if n > 1:
        assert not np.array_equal(got[0][:H * W * 4], got[1][:H * W * 4])
