"""The twelve GEO_MODE_ADAPTIVE instantiations of
geo_render_disk_ring_batch_kernel (geo_render_disk_adaptive_ring_batch), one
cell each in the manner of tests/test_gpu_wave_block_matrix.py: kind (the
curved ones) x shade x one sample / GEO_FLAG_SS4, two frames with a frame
stride, every frame against the CPU path
(geo_render_cpu_disk_adaptive_ring_f64; under SS4 its render at twice the size,
resolved).  The scenes, the references and their evidence (the band holds
pixels with a disk hit, the state and the shade change the frame, the adaptive
frame is not the direct one) are that matrix's ring cells'."""
import numpy as np
import pytest

import test_disk_cpu as T
import test_gpu_wave_block_matrix as M
from test_gpu_disk_emission import set_emission

pytestmark = pytest.mark.gpu

FORMS = {"batch_adaptive": False, "batch_adaptive_ss4": True}  # form: SS4
CELLS = [(k, s, f) for k in ("curved_out", "curved_in") for s in M.SHADES for f in FORMS]
IDS = [f"{k}-{s}-ring_{f}" for k, s, f in CELLS]
N = 2


def test_a_cell_per_new_kernel():
    assert len(CELLS) == 12 and len(set(IDS)) == 12 and not set(IDS) & set(M.IDS)


def draw(dev, kind, shade, ss):
    """The cell through geo_render_disk_adaptive_ring_batch: the output bytes as (frames, stride)."""
    import torch

    import schwarzschild_raytracer_wgpu_amd as g

    frames, scenes, disk = M.cell_scenes(kind, N, True)
    scenes = [M.scene_as(s, True, ss) for s in scenes]
    ctx = g.Context(dev.index or 0)
    ctx.set_sky(T.SKY)
    ctx.set_disk(T.TEX, *disk)
    if shade == "shift":
        ctx.set_disk_shift(*M.SHIFT)
    if shade == "emission":
        set_emission(ctx, M.EM)
    ctx.set_disk_ring_f64(True)
    out = torch.full((N * M.STRIDE,), M.FILL, dtype=torch.uint8, device=dev)
    ctx.render_disk_adaptive_ring_batch(frames, scenes, M.W, M.H, M.BAND, 0, M.BAND, M.NB, out, frame_stride=M.STRIDE)
    torch.cuda.synchronize()
    ctx.close()
    return out.cpu().numpy().reshape(N, M.STRIDE)


@pytest.mark.parametrize("kind,shade,form", CELLS, ids=IDS)
def test_cell(dev, cpu, kind, shade, form):
    ss = FORMS[form]
    got = draw(dev, kind, shade, ss)
    W, H = M.W, M.H
    for f in range(N):
        want = M.reference(cpu, kind, shade, True, ss, True, f)
        diff = int((got[f][:H * W * 4].reshape(H, W, 4) != want).sum())
        print(f"frame {f}: differing bytes {diff}")
        assert diff == 0, f
        assert (got[f][H * W * 4:] == M.FILL).all(), f  # the clipped rows of the last band, and the batch's gap
    assert not np.array_equal(got[0][:H * W * 4], got[1][:H * W * 4])


cpu = M.cpu
