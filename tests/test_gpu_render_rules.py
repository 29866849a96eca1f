"""The render call rules through the real C ABI: a sample of the matrix of
tests/test_render_rules_host.py, each case set up in a real context (sky, fan,
disk, shift, emission, ring, armed buffers) and called on a 32 x 16 frame (one
tile wide, two 8-row bands).  The status is the matrix's, a refused call leaves
the prefilled output alone, an accepted call draws into its own bytes only.
What this adds to the host test: RuleState is what the library reads from its
context, and the exported functions pass their arguments on in the right order.

The sample: every 7919th case of the matrix, and four cases spread evenly
through every (entry point, status) pair that occurs, since a stride of a few
thousand alone meets GEO_ESTATE (0.2 % of the matrix) for few entry points.
Left out: what the C ABI cannot set up (a fan of one node), and every case whose
frame is not the 32 x 16 one, whose rows exceed it or whose step budget is not
64: an accepted one would draw more than this test's buffers hold."""
import math

import numpy as np
import pytest

import render_rules_cases as R
from helpers import default_frame
from schwarzschild_raytracer_wgpu_amd import Context, GeoFrame, GeoScene, _lib

pytestmark = pytest.mark.gpu

STRIDE, PER_PAIR = 7919, 4
FILL = 0x5A
OUT_BYTES = 8 * 4096


def sample():
    """(cases, status) of the sampled matrix cases, in matrix order."""
    want = np.load(R.os.path.join(R.HERE, "golden", "render_rules_matrix.npz"))["status"]
    entry, fits = [], []
    for _, c in R.blocks():
        rows = np.where(c["entry"] == 0, c["g"][:, 1].astype(np.uint64), c["g"][:, 0].astype(np.uint64) * c["g"][:, 3])
        entry.append(c["entry"].astype(np.uint8))
        fits.append((c["width"] == R.WIDTH) & (c["height"] == R.HEIGHT) & (rows <= R.HEIGHT) &
                    (c["out_frame_stride"] <= 2050) & (c["scene"]["max_steps"] == R.MAX_STEPS).all(axis=1) &
                    (c["n_fan"] != 1))
    entry, fits = np.concatenate(entry), np.concatenate(fits)
    pick = np.zeros(len(want), bool)
    pick[STRIDE // 2::STRIDE] = True
    for e in range(len(R.ENTRIES)):
        for s in (R.GEO_OK, R.GEO_EINVAL, R.GEO_ESTATE):
            idx = np.flatnonzero((entry == e) & (want == s) & fits)
            assert len(idx), (R.ENTRIES[e], s)  # every pair occurs, and in a case this test can run
            pick[idx[np.linspace(0, len(idx) - 1, PER_PAIR).astype(int)]] = True
    pick &= fits
    assert 300 <= pick.sum() <= 700, pick.sum()
    cases, at = [], 0
    for _, c in R.blocks():
        cases.append(c[pick[at:at + len(c)]])
        at += len(c)
    return np.concatenate(cases), want[pick]


class Bench:
    """The contexts (by sky and fan) and device buffers the cases are run in."""

    def __init__(self, dev):
        import torch

        self.torch, self.dev = torch, dev
        self.ctxs, self.state = {}, {}
        self.out = torch.full((OUT_BYTES,), FILL, dtype=torch.uint8, device=dev)
        px = R.WIDTH * R.HEIGHT
        self.mask = torch.empty(px, dtype=torch.uint8, device=dev)
        self.uv = torch.empty(2 * px, dtype=torch.float32, device=dev)
        self.steps = torch.empty(px, dtype=torch.int32, device=dev)
        self.armed = [torch.empty(6 * px, dtype=torch.float32, device=dev) for _ in range(3)]
        self.total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.frames = (GeoFrame * 8)(*[default_frame(R.WIDTH, R.HEIGHT)] * 8)
        self.tex = np.array([[[255, 0, 0, 255], [0, 255, 0, 255]], [[0, 0, 255, 255], [255, 255, 255, 255]]], np.uint8)

    def ctx(self, k):
        key = (int(k["sky"]), int(k["n_fan"]))
        if key not in self.ctxs:
            c = Context(0)
            if key[0]:
                c.set_sky(self.tex)
            if key[1]:
                c.solve_ray_fan(R.SPHERE_R, 1.0, 1000, math.pi / 100, int(k["n_fan"]), 10.0)
            self.ctxs[key], self.state[key] = c, None
        c = self.ctxs[key]
        state = tuple(int(k[n]) for n in ("disk_set", "shift_set", "emit_set", "disk_ring")) + \
            (float(k["r_in"]), float(k["r_out"]))
        if self.state[key] != state:
            c.clear_disk()  # (the shift, the emission and the ring state with it)
            c.clear_disk_shift()
            if state[0]:
                c.set_disk(self.tex, state[4], state[5])
            if state[1]:
                c.set_disk_shift(1, 4, 1.0)
            if state[2]:
                c.set_disk_emission(self.tex[0], 1.0, 0.5, 2.0)
            c.set_disk_ring_f64(bool(state[3]))
            self.state[key] = state
        return c

    def call(self, k):
        lib, c = _lib.lib, self.ctx(k)
        nulls, side, e = int(k["nulls"]), int(k["side"]), int(k["entry"])
        assert not (nulls & 1 and k["armed"])  # (an armed buffer would wait in the context for the next case)
        for bit, arm in enumerate((lib.geo_disk_hits_next_render, lib.geo_disk_shift_next_render,
                                   lib.geo_disk_emission_next_render)):
            if int(k["armed"]) >> bit & 1:
                assert arm(c._h, self.armed[bit].data_ptr()) == 0
        scenes = (GeoScene * 8)(*[GeoScene(*k["scene"][1 if i == k["alt_frame"] else 0].tolist()) for i in range(8)])
        h = None if nulls & 1 else c._h
        fr = None if nulls & 2 else self.frames
        sc = None if nulls & 4 else scenes
        out = None if nulls & 8 else self.out.data_ptr()
        total = self.total.data_ptr() if k["steps_total"] else None
        g = [int(v) for v in k["g"]]
        fn = getattr(lib, R.ENTRIES[e])
        if e < R.ONE_FRAME:
            sides = (self.mask.data_ptr() if side & 1 else None, self.uv.data_ptr() if side & 2 else None,
                     self.steps.data_ptr() if side & 4 else None)
            rows = g[:2] if e == 0 else g
            return fn(h, fr, sc, R.WIDTH, R.HEIGHT, *rows, out, *sides, total, None)
        n = int(k["nframes"])
        if e == 4:  # geo_render_band_set_frames: (frames, nframes, scene)
            return fn(h, fr, n, sc, R.WIDTH, R.HEIGHT, *g, out, int(k["out_frame_stride"]), total, None)
        return fn(h, fr, sc, n, R.WIDTH, R.HEIGHT, *g, out, int(k["out_frame_stride"]), total, None)

    def close(self):
        self.torch.cuda.synchronize()
        for c in self.ctxs.values():
            c.close()


def test_sampled_cases_through_the_c_abi(dev):
    import torch

    cases, want = sample()
    b = Bench(dev)
    seen = set()
    try:
        for k, status in zip(cases, want):
            got = b.call(k)
            assert got == status, f"{R.describe(k)}: status {got}, the matrix has {status}"
            torch.cuda.synchronize()
            seen.add((int(k["entry"]), int(status)))
            if status != R.GEO_OK:
                assert bool((b.out == FILL).all()), "a refused call wrote: " + R.describe(k)
                continue
            e, g = int(k["entry"]), k["g"]
            rows = int(g[1]) if e == 0 else int(g[0]) * int(g[3])
            n = 1 if e < R.ONE_FRAME else int(k["nframes"])
            end = (n - 1) * int(k["out_frame_stride"]) + rows * R.WIDTH * 4
            assert bool((b.out[end:] == FILL).all()), "drawn past the call's bytes: " + R.describe(k)
            s0 = k["scene"][0]
            # (GEO_FLAG_COMPOSITE keeps the target under a black-hole pixel: from inside the horizon, all of them)
            if not (s0["flags"] & R.COMPOSITE and s0["rs"] > 0 and s0["r_obs"] <= s0["rs"]):
                assert not bool((b.out[:end] == FILL).all()), "an accepted call drew nothing: " + R.describe(k)
            b.out.fill_(FILL)
    finally:
        b.close()
    assert len(seen) == 33
