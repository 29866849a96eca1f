"""The colour stage of the render kernels against the independent f64 sampler
tests/sampler_ref.py, on the device's own outputs (rgba, mask, uv and the
buffers of geo_disk_hits_next_render): the one-frame plain kernels for the
three poses and every sky (the 2^20 x 1 upload included), GEO_FLAG_COMPOSITE
over a device target, GEO_FLAG_MIPS direct and adaptive, the disk kernels of
poses A, B and `tilted`, pose B with set_disk_ring_f64 on, and GEO_FLAG_SS4
against the device's one-sample render at twice the size.  Poses, textures,
bounds and reach assertions are tests/test_sampler_cpu.py's; the device-only
parts (the padded sky copy, the 24-bit multiplies, the byte permutes, the
cross-lane resolve) are held to something other than a restatement of
themselves.  The mutation test is not repeated: the reference is the same."""
import numpy as np
import pytest

import test_gpu_disk as GD
import test_gpu_ss as GS
import test_sampler_cpu as C
from schwarzschild_raytracer_wgpu_amd._lib import GEO_MODE_ADAPTIVE, GEO_MODE_DIRECT

pytestmark = pytest.mark.gpu


class Gpu:
    """The device's entry points as test_sampler_cpu's builders call them."""
    name = "gpu"

    def __init__(self, dev):
        self.dev = dev
        self.sky_ctx = GD.Gpu(dev)  # the plain renders share one context

    def plain(self, frame, scene, sky, w, h, target=None):
        import torch

        g = self.sky_ctx
        g.ctx.set_sky(sky)
        b = g.buffers(h, w, hits=False)
        if target is not None:
            b["rgba"].copy_(torch.from_numpy(np.ascontiguousarray(target).reshape(-1)))
        g.ctx.render_rows(frame, scene, w, h, 0, h, b["rgba"], b["mask"], b["uv"], b["steps"], b["total"])
        return g.host(b, h, w)

    def disk(self, frame, scene, sky, w, h, disk_args, tex, ring=False):
        g = GD.Gpu(self.dev, disk_args, tex)
        g.ctx.set_sky(sky)
        if ring:
            g.ctx.set_disk_ring_f64(True)
        a = g.rows(frame, scene, w, h)
        g.close()
        return a

    def ss(self, kind, frame, scene, sky, w, h, disk_args=None, tex=None):
        g = GS.Gpu(self.dev, kind, disk_args)
        g.ctx.set_sky(sky)
        if kind == "disk":
            g.ctx.set_disk(tex, *disk_args)
        rgba, _ = g.rows(frame, scene, w, h)
        g.close()
        return rgba

    def close(self):
        self.sky_ctx.close()


@pytest.fixture(scope="module")
def gpu(dev):
    g = Gpu(dev)
    yield g
    g.close()


@pytest.mark.parametrize("sname", C.PLAIN_SKIES + C.EXTREME_SKIES)
@pytest.mark.parametrize("pname", C.POSES)
def test_plain(gpu, pname, sname):
    C.check_plain(gpu, pname, sname)


def test_composite(gpu):
    C.check_composite(gpu)


def test_mips_flat_reaches_every_level(gpu):
    C.check_mips_flat(gpu)


@pytest.mark.parametrize("mode", [GEO_MODE_DIRECT, GEO_MODE_ADAPTIVE], ids=["direct", "adaptive"])
def test_mips_curved(gpu, mode):
    C.check_mips_curved(gpu, mode)


@pytest.mark.parametrize("name", ["A", "B", "tilted"])
def test_disk(gpu, name):
    """Poses A and B draw the curved disk kernel, `tilted` the flat one."""
    C.check_disk(gpu, name)


def test_disk_ring_f64(gpu):
    C.check_disk(gpu, "B", ring=True)


@pytest.mark.parametrize("kind", ["plain", "disk"])
def test_ss4(gpu, kind):
    C.check_ss(gpu, kind)
