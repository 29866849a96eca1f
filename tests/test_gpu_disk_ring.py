"""The disk's capture band in f64 on the device (geo_set_disk_ring_f64):
geo_render_disk_ring_kernel<KIND, SHADE, GEO_MODE_DIRECT> (unshaded, shifted, emission) against the CPU path
(geo_render_cpu_disk_ring_f64, the same headers csrc/geo_band.h and
csrc/geo_disk.h) bit for bit in every output and the hit, g and q slots; the
frame shapes and call forms; both dispatch orders; the state's rules and the
refusals while it is on (geo.h); and seeded random scenes.
tests/test_disk_ring_cpu.py ties the CPU path to the f64 restatement."""
import ctypes

import numpy as np
import pytest

import oracle as O
import test_disk_cpu as T
import test_disk_emission_cpu as X
import test_disk_ring_cpu as RC
import test_gpu_disk as G
import test_gpu_disk_emission as GE
import test_gpu_disk_shift as GS
from fuzz_disk_scenes import disk_scene, kind_of
from schwarzschild_raytracer_wgpu_amd import make_scene
from schwarzschild_raytracer_wgpu_amd._lib import (GEO_DISPATCH_LONGEST_FIRST, GEO_DISPATCH_ROW_MAJOR, GEO_EINVAL,
                                                   GEO_FLAG_DEFER_STEPS, GEO_FLAG_DISK, GEO_FLAG_RING_F64, GEO_OK, lib)

pytestmark = pytest.mark.gpu
W, H = T.W, T.H
EM, EM_POWER = GE.EM, GE.EM_POWER
VARIANTS = ("plain", "shift", "emission")


@pytest.fixture(scope="module")
def cpu():
    return RC.load_cpu()


def state_of(variant, em=EM, shift=GS.SHIFT):
    """(shift, em) for the CPU path's render."""
    return dict(shift=shift if variant == "shift" else None, em=em if variant == "emission" else None)


class Gpu(GE.Gpu):
    """test_gpu_disk_emission's context (hit, g and q slots armed) with the
    variant's shading and the f64 band on."""

    def __init__(self, dev, disk_args, variant="plain", em=EM, shift=GS.SHIFT, ramp=X.RAMP, tex=T.TEX, ring=True):
        super().__init__(dev, disk_args, None, tex)
        if variant == "shift":
            self.ctx.set_disk_shift(*shift)
        elif variant == "emission":
            GE.set_emission(self.ctx, em, ramp)
        if ring:
            self.ctx.set_disk_ring_f64(True)


def same(a, b):
    return GE.same(a, b) and a["total"] == b["total"]


def in_band(frame, scene, w, h):
    """The band's pixels as the kernels decide them (on the f32 ray)."""
    return O.ring_band(frame, RC.ring_scene(scene), w, h) == 1


def curved_in_b():
    """Pose B with a step outside kCurvedOut's range (0.75 > 1/2): kCurvedIn."""
    frame, scene, disk, args = T.pose("B")
    scene = make_scene(scene.rs, scene.sphere_r, scene.r_obs, 0.75, 256, flags=GEO_FLAG_DISK)
    assert kind_of(scene.rs, scene.r_obs, scene.step) == 1
    return frame, scene, disk, args


CASES = [("ring", "plain", EM), ("ring", "shift", EM), ("ring", "emission", EM), ("B", "plain", EM),
         ("B", "shift", EM), ("B", "emission", EM), ("B", "emission", EM_POWER), ("A", "plain", EM),
         ("A", "emission", EM), ("B_curved_in", "plain", EM), ("B_curved_in", "emission", EM_POWER)]


@pytest.mark.parametrize("name,variant,em", CASES)
def test_kernel_equals_cpu_path(dev, cpu, name, variant, em):
    frame, scene, disk, disk_args = curved_in_b() if name == "B_curved_in" else T.pose(name)
    rc, c = RC.render(cpu, frame, scene, disk, 1, **state_of(variant, em))
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args, variant, em)
    g = gpu.rows(frame, scene, W, H)
    gpu.close()
    band = in_band(frame, scene, W, H)
    hit = (c["hits"][..., 0] > 0.0).any(axis=-1)
    if name != "A":
        assert (band & hit).sum() >= 10  # hits drawn by the f64 path
    assert hit.sum() > 150 and (~band).sum() > 1000
    assert same(g, c), (name, variant)


def test_frame_shapes_and_call_forms(dev, cpu):
    import torch

    fields_eq, fields_bits = ("rgba", "mask", "steps"), ("uv", "hits", "g", "q")
    # a 100 x 37 frame (no multiple of the 32 x 8 tile), rows 5..24, pose B's observer
    w, h = 100, 37
    frame, scene, disk, disk_args = T.pose("B", w, h)
    rc, c = RC.render(cpu, frame, scene, disk, 1, w=w, h=h, em=EM, row0=5, nrows=20)
    assert rc == GEO_OK
    assert (in_band(frame, scene, w, h)[5:25] & (c["hits"][..., 0] > 0.0).any(axis=-1)).sum() >= 4
    gpu = Gpu(dev, disk_args, "emission")
    assert same(gpu.rows(frame, scene, w, h, 5, 20), c)
    gpu.close()
    # geo_render_bands, the 8-row bands 0, 2, 4, 6 of 96 x 54 (band 6 clipped to rows 48..53)
    frame, scene, disk, disk_args = T.pose("ring")
    rc, c = RC.render(cpu, frame, scene, disk, 1, shift=GS.SHIFT)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args, "shift")
    br, nb = 8, 4
    b = gpu.arm(nb * br, W)
    gpu.ctx.render_bands(frame, scene, W, H, br, 0, 2, nb, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
    got = gpu.host(b, nb * br, W)
    want_total = 0
    for i in range(nb):
        r0 = 2 * i * br
        n = min(br, H - r0)
        for f in fields_eq:
            assert np.array_equal(got[f][i * br:i * br + n], c[f][r0:r0 + n]), (f, i)
        for f in fields_bits:
            assert np.array_equal(got[f][i * br:i * br + n].view(np.uint32), c[f][r0:r0 + n].view(np.uint32)), (f, i)
        want_total += int(c["steps"][r0:r0 + n].sum())
    assert got["total"] == want_total
    assert (got["g"][3 * br + (H - 48):] == -1.0).all() and (got["hits"][3 * br + (H - 48):] == -1.0).all()
    # GEO_FLAG_DEFER_STEPS: the steps go to the context's accumulator (geo_steps_flush)
    deferred = make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps,
                          flags=GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS)
    b = gpu.arm(H, W)
    gpu.ctx.render_rows(frame, deferred, W, H, 0, H, b["rgba"], b["mask"], b["uv"], b["steps"])
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    gpu.ctx.steps_flush(total)
    got = gpu.host(b, H, W)
    gpu.close()
    assert GE.same(got, c) and int(total.item()) == c["total"]


def test_dispatch_orders(dev, cpu):
    """The learned order (its own grid key: the band's tiles cost more) and an
    explicit order draw the row-major frame."""
    import torch

    frame, scene, disk, disk_args = T.pose("ring")
    rc, c = RC.render(cpu, frame, scene, disk, 1, em=EM)
    assert rc == GEO_OK
    gpu = Gpu(dev, disk_args, "emission")
    gpu.ctx.set_dispatch(GEO_DISPATCH_ROW_MAJOR)
    assert same(gpu.rows(frame, scene, W, H), c)
    gpu.ctx.set_dispatch(GEO_DISPATCH_LONGEST_FIRST, 1)
    for i in range(3):
        assert same(gpu.rows(frame, scene, W, H), c), i
        torch.cuda.synchronize()
    rec, _ = gpu.ctx.dispatch_stats()
    assert rec >= 1
    tx, ty = (W + 31) // 32, (H + 7) // 8
    order = np.array([(t // tx) << 16 | (t % tx) for t in range(tx * ty)][::-1], np.uint32)
    gpu.ctx.set_tile_order(tx, ty, order)
    assert same(gpu.rows(frame, scene, W, H), c)
    gpu.close()


def test_state(dev, cpu):
    """On, then off: the plain disk frame again; geo_set_disk keeps the state,
    geo_clear_disk clears it; a render without the disk is untouched by it;
    rs = 0 ignores it."""
    frame, scene, disk, disk_args = T.pose("ring")
    r_in, r_out, normal, axis = disk_args
    rc, on = RC.render(cpu, frame, scene, disk, 1)
    rc0, off = RC.render(cpu, frame, scene, disk, 0)
    assert rc == GEO_OK and rc0 == GEO_OK and not np.array_equal(on["hits"], off["hits"])
    gpu = Gpu(dev, disk_args, ring=False)
    assert lib.geo_set_disk_ring_f64(None, 1) == GEO_EINVAL
    assert same(gpu.rows(frame, scene, W, H), off) and not gpu.ctx.disk_ring_f64
    gpu.ctx.set_disk_ring_f64()
    assert same(gpu.rows(frame, scene, W, H), on) and gpu.ctx.disk_ring_f64
    gpu.ctx.set_disk_ring_f64(False)
    assert same(gpu.rows(frame, scene, W, H), off)
    gpu.ctx.set_disk_ring_f64(True)
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)  # kept across geo_set_disk
    assert same(gpu.rows(frame, scene, W, H), on)
    # a render without the disk: the same with the state on and off
    plain, ringed = T.plain_of(scene), RC.ring_scene(scene)
    with_state = [gpu.rows(frame, s, W, H) for s in (plain, ringed)]
    gpu.ctx.set_disk_ring_f64(False)
    for s, a in zip((plain, ringed), with_state):
        assert G.same(gpu.rows(frame, s, W, H), a, hits=False)
    gpu.ctx.set_disk_ring_f64(True)
    # rs = 0: the plain disk frame
    fframe, fscene, fdisk, fargs = T.pose("flat")
    gpu.ctx.set_disk(T.TEX, *fargs)
    rcf, flat = RC.render(cpu, fframe, fscene, fdisk, 0)
    assert rcf == GEO_OK and same(gpu.rows(fframe, fscene, W, H), flat)
    # geo_clear_disk clears it
    gpu.ctx.clear_disk()
    assert not gpu.ctx.disk_ring_f64
    gpu.ctx.set_disk(T.TEX, r_in, r_out, normal, axis)
    assert same(gpu.rows(frame, scene, W, H), off)
    gpu.close()


def test_refusals_while_on(dev):
    """Colour-only and batched disk renders: GEO_EINVAL, nothing written, an
    armed buffer consumed; GEO_FLAG_DISK | GEO_FLAG_RING_F64 stays refused."""
    import torch

    from schwarzschild_raytracer_wgpu_amd.dist import ShardedFrame

    frame, scene, _, disk_args = T.pose("B")
    w, h = W, H
    ss = GE.ss_of(scene)
    f = ctypes.byref(frame)
    for variant in ("plain", "emission"):
        gpu = Gpu(dev, disk_args, variant)
        hd = gpu.ctx._h
        out = torch.full((w * 48 * 4,), 0x5A, dtype=torch.uint8, device=dev)
        batch = (1, w, h, 8, 0, 8, 6, out.data_ptr(), w * 48 * 4, None, None)
        assert lib.geo_render_disk_batch(hd, f, ctypes.byref(scene), *batch) == GEO_EINVAL
        assert lib.geo_render_ss_batch(hd, f, ctypes.byref(ss), *batch) == GEO_EINVAL
        assert lib.geo_render_emission_batch(hd, f, ctypes.byref(scene), *batch) == GEO_EINVAL
        assert lib.geo_render_emission_batch(hd, f, ctypes.byref(ss), *batch) == GEO_EINVAL
        # a supersampled render, with an armed hit buffer and without
        rgba = torch.full((h * w * 4,), 0x5A, dtype=torch.uint8, device=dev)
        hb = torch.full((h * w * 6,), -1.0, dtype=torch.float32, device=dev)
        assert GE._raw_rows(gpu, frame, ss, rgba) == GEO_EINVAL
        gpu.ctx.disk_hits_next_render(hb)
        assert GE._raw_rows(gpu, frame, ss, rgba) == GEO_EINVAL
        both = make_scene(scene.rs, scene.sphere_r, scene.r_obs, scene.step, scene.max_steps,
                          flags=GEO_FLAG_DISK | GEO_FLAG_RING_F64)
        assert GE._raw_rows(gpu, frame, both, rgba) == GEO_EINVAL
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0x5A).all() and (rgba.cpu().numpy() == 0x5A).all()
        # the armed buffer was consumed by the refused call: a good render leaves it alone
        assert GE._raw_rows(gpu, frame, scene, rgba) == GEO_OK
        torch.cuda.synchronize()
        assert (hb.cpu().numpy() == -1.0).all() and not (rgba.cpu().numpy() == 0x5A).all()
        # ShardedFrame names the refusal; without batch_launch it is built
        with pytest.raises(ValueError, match="set_disk_ring_f64"):
            ShardedFrame(gpu.ctx, frame, scene, w, h, 8, 0, 1, dev, frames_per_gather=2, batch_launch=True,
                         emission_batch=True)
        ShardedFrame(gpu.ctx, frame, scene, w, h, 8, 0, 1, dev, frames_per_gather=2, batch_launch=False)
        # off again: the batched and supersampled renders draw
        gpu.ctx.set_disk_ring_f64(False)
        name = "geo_render_emission_batch" if variant == "emission" else "geo_render_disk_batch"
        assert getattr(lib, name)(hd, f, ctypes.byref(scene), *batch) == GEO_OK
        assert GE._raw_rows(gpu, frame, ss, rgba) == GEO_OK
        torch.cuda.synchronize()
        assert not (out.cpu().numpy() == 0x5A).all()
        gpu.close()


# Seeded scenes (fuzz_disk_scenes: the families "far" and "near_disk", an
# observer outside the photon sphere within the disk's rules), 64 x 36, the
# render chosen by seed % 3.  BAND_HIT_SEEDS were chosen on the CPU path: each
# has at least two band pixels with a disk hit; NO_BAND_HIT_SEEDS have none.
BAND_HIT_SEEDS = (6, 20, 41, 61, 66, 71, 91, 106, 156, 161, 195, 196, 201, 241, 246, 250, 266, 281, 286, 301, 306, 315,
                  326, 341)
NO_BAND_HIT_SEEDS = (0, 1, 5, 10, 11, 15, 16, 21, 25, 26, 30, 31)
BAND_HIT_SHARE = 0.6  # of the scenes must draw hits through the f64 path (24 of 36 when chosen)


def test_fuzz_bitexact(dev, cpu):
    w, h = 64, 36
    with_band_hits, kinds = 0, set()
    seeds = BAND_HIT_SEEDS + NO_BAND_HIT_SEEDS
    for seed in seeds:
        frame, scene, disk_args, shift, (em, ramp), desc = disk_scene(seed, w, h)
        assert scene.rs > 0.0 and scene.r_obs > 1.5 * scene.rs, desc
        variant = VARIANTS[seed % 3]
        rc, c = RC.render(cpu, frame, scene, T.make_disk(*disk_args), 1, w=w, h=h, ramp=ramp,
                          **state_of(variant, em, shift))
        assert rc == GEO_OK, desc
        gpu = Gpu(dev, disk_args, variant, em, shift, ramp)
        g = gpu.rows(frame, scene, w, h)
        gpu.close()
        assert same(g, c), desc
        n = int((in_band(frame, scene, w, h) & (c["hits"][..., 0] > 0.0).any(axis=-1)).sum())
        assert (n >= 2) == (seed in BAND_HIT_SEEDS), desc
        with_band_hits += n >= 2
        kinds.add(kind_of(scene.rs, scene.r_obs, scene.step))
    assert with_band_hits >= BAND_HIT_SHARE * len(seeds)
    assert kinds == {0, 1}  # both curved integration kinds
