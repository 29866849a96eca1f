"""An independent f64 reference for the colour stage, with derived error bounds.

Everything after the geometry (UV to texel coordinates, the texel quad with U
wrapping and V clamping, the 8-bit bilinear lerp, the blend over the cleared
target, GEO_FLAG_COMPOSITE, the mip chain with its level of detail and
trilinear blend, the disk texture lookup and the far-to-near order of the
disk's images, and the 2 x 2 resolve of GEO_FLAG_SS4) is restated here in
numpy f64 from its definition: "this pixel's colour is the bilinear sample of
the texture at its UV".  The module imports nothing from csrc/ or oracle/ and
works from a render's own outputs (uv, mask, hit slots), so it checks the
colour stage alone; the geometry has its own references.

Every function returns, per pixel and channel, the exact value c and a bound e:
the render's 8-bit value must lie within e of c (tests/test_sampler_cpu.py for
the CPU path, tests/test_gpu_sampler.py for the kernels).  No bound below is a
measured maximum: each is derived from the fixed-point steps of the
specification (csrc/geo_pixel.h, csrc/geo_disk.h), named where it is used.
eps = 2^-24 is the relative rounding error of one f32 operation.

The sample bound (bilinear)
---------------------------
sample_sky_quad_f works per axis on n = floor(U * (256 tw) - 128), formed by
ONE fused multiply-add (256 tw is exact below 2^24) and one floor:
  * the fma rounds once; its value is at most 256 tw in magnitude for U in
    [0, 1], so the rounding is at most 256 tw eps in 1/256-texel units, that
    is tw 2^-24 texels;
  * the floor drops less than one unit: less than 1/256 texel, always downward.
The kernel therefore lerps, with exact weights (n & 255)/256, at a position
(x', y') with |x' - x| < dx = 1/256 + tw 2^-24 and |y' - y| < dy = 1/256 +
th 2^-24 (the issue's form has 2^-23; the half-ulp argument gives 2^-24).
The bilinear surface S is continuous and piecewise linear along each axis with
|dS/dx| <= Dx and |dS/dy| <= Dy inside a quad (Dx, Dy: the quad's largest
horizontal and vertical texel differences, per channel), so
    |S(x', y') - S(x, y)| <= Dx dx + Dy dy.
Where (x, y) lies within (dx, dy) of a texel boundary, (x', y') may fall in the
neighbouring quad, whose slopes count: there Dx and Dy are taken over the
4 x 4 texel block around the quad (a pixel in ~2 % of a frame).
The arithmetic at (x', y'): the horizontal lerps of the top and the bottom
texel pair are exact integers over 256, truncated to 8 bits (an error in
(-1, 0], and none when the pair's texels are equal); the vertical lerp of the
two truncated values adds 128 and shifts, a rounding of at most 1/2 (none when
both rows are equal too).  So
    E = Dx dx + Dy dy + [Dx > 0] + 1/2 [Dx > 0 or Dy > 0]    (<= ... + 3/2),
and a channel that is constant over the block (an opaque texture's alpha) is
exact.

Over the cleared target (over_clear)
------------------------------------
rgb = round(c8 a8 / 255) on the 8-bit sample (c8, a8) with |c8 - c| <= E_c,
|a8 - a| <= E_a:  c8 a8 - c a = a (c8 - c) + c8 (a8 - a), c8 <= min(255,
c + E_c), and the rounded division (div255_, exact for products up to 255^2)
adds 1/2:
    E_rgb = (a E_c + min(255, c + E_c) E_a) / 255 + 1/2     (<= E_c + E_a + 1/2).
An opaque texture (every alpha 255: the upload's `opaque` flag) skips the
blend: E_rgb = E_c.  Alpha is 255 exactly; a captured pixel is (0, 0, 0, 255).

composite (the reference's ALPHA_BLENDING)
------------------------------------------
f(s, a, d) = (s a + d (255 - a)) / 255 is linear in each argument:
    f(s8, a8, d8) - f(s, a, d) = (s8 - s) a8/255 + (d8 - d)(255 - a8)/255
                                 + (a8 - a)(s - d)/255,
with a8 within E_a of a, and one rounded division:
    E_rgb = E_s min(255, a + E_a)/255 + E_d min(255, 255 - a + E_a)/255
            + E_a |s - d|/255 + 1/2.
(The issue's form has a in place of a8; the min() terms carry the second
order it drops.)  Alpha: g(a, d_a) = (255 a + d_a (255 - a))/255,
    E_alpha = E_a (255 - d_a)/255 + E_da min(255, 255 - a + E_a)/255 + 1/2,
and over an exact alpha of 255 the sum is 255^2 whatever a8 is: exactly 255.

Mips (trilinear)
----------------
The chain is the 2 x 2 box filter with rounded means.  The footprint rho2
comes from the frame-aligned 2 x 2 pixel quad, each row's and column's own
difference, U not unwrapped; lambda = clip(log2(rho2)/2, 0, 3); the result is
T(lambda) = (1 - f) S_l + f S_{l+1}, l = floor(lambda), which is continuous in
lambda.  The render's lambda_q differs from lambda by at most
    dl = 1/256 + 0.95e-4 + 2^-20:
  * lod_q8 takes floor(128 log2 rho2)/256: below lambda by less than 1/256;
  * its log2 polynomial is within 1.9e-4 (the header's figure), halved;
  * rho2 in f32: a difference (eps), its product with the size (eps), the
    square (eps), the fma of the other square (exact product, eps on the
    sum): (1 + eps)^6 at most, so log2(rho2)/2 moves by 3 eps/ln 2 = 2^-21.9;
    the sum e + log2_1p in lod_q8 rounds once more at 2^-22 in log2, 2^-23
    here: together below 2^-20.
With s_l the 8-bit sample of level l, |s_l - S_l| <= E_l, and the 8-bit blend
rounding 1/2:
    E = E_0 (1 - f) + E_1 f + (|S_1 - S_0| + |E_1 - E_0|) dl + 1/2,
and where lambda is within dl of a level boundary the render may blend the
neighbouring pair of levels: there E takes the largest E_l and the largest
|S_{l+1} - S_l| of the two intervals.

Disk
----
Slot k of a pixel holds the hit's (r, U_d) as f32, the values the shader
itself samples with.  V_d = clip((r - r_in)/(r_out - r_in), 0, 1).  In f32
(geo_disk.h): r - r_in (both f32: relative eps of the difference, not of r),
the constant 1/(r_out - r_in) (a difference and a divide: 2 eps) and the
product (eps): V_d (1 + eps)^4, at most 2^-22 absolute, th 2^-22 texels on
top of dy.  The difference r - r_in is taken of two exact f32 values, so its
error scales with the difference and no r_in/(r_out - r_in) factor appears.
The images are composited over the sky's result far to near: slot 2, slot 1,
slot 0 on top.

ss4: the rounded mean of four samples: the mean of their exact values, the
mean of their bounds + 1/2.

`mutation=` changes the REFERENCE (never the render) in one plain way; the
tests require each mutated reference to put the true render outside the
bounds, which keeps bounds and inputs honest.
"""
import numpy as np

EPS = 2.0 ** -24
SLACK = 1e-9  # the f64 evaluation error of this module itself, in colour levels
MIP_LEVELS = 4
DLAMBDA = 1.0 / 256.0 + 0.95e-4 + 2.0 ** -20

MUTATIONS = ("no_half_texel", "clamp_u", "wrap_v", "swap_weights", "nearest", "swap_rb", "lod_plus_one", "no_lod",
             "nearest_level", "disk_swap_uv", "disk_flip_v", "disk_order_reversed", "disk_slot0_only")


class Sample(dict):
    """c, e: (..., 4) straight-alpha value and bound; Dx, Dy: the quad's own
    contrasts; seam, pole_lo, pole_hi: the quad wraps in U / clamps at V = 0 /
    clamps at V = 1."""
    __getattr__ = dict.__getitem__


def bilinear(tex, U, V, mutation=None, extra_dy=0.0):
    """The f64 bilinear sample of tex (th, tw, 4) uint8 at (U, V): U wraps, V
    clamps.  extra_dy: further uncertainty of y in texels (the disk's V_d)."""
    t = np.asarray(tex).astype(np.float64)
    th, tw = t.shape[:2]
    U = np.asarray(U, np.float64)
    V = np.asarray(V, np.float64)
    half = 0.0 if mutation == "no_half_texel" else 0.5
    x = U * tw - half
    y = V * th - half
    ix = np.floor(x).astype(np.int64)
    iy = np.floor(y).astype(np.int64)
    fx = x - ix
    fy = y - iy

    def col(i):
        return np.clip(i, 0, tw - 1) if mutation == "clamp_u" else np.mod(i, tw)

    def row(j):
        return np.mod(j, th) if mutation == "wrap_v" else np.clip(j, 0, th - 1)

    def at(j, i):
        return t[row(j), col(i)]

    t00, t10, t01, t11 = at(iy, ix), at(iy, ix + 1), at(iy + 1, ix), at(iy + 1, ix + 1)
    wx, wy = fx[..., None], fy[..., None]
    if mutation == "swap_weights":
        wx, wy = 1.0 - wx, 1.0 - wy
    if mutation == "nearest":
        wx, wy = np.round(wx), np.round(wy)
    c = (1.0 - wy) * ((1.0 - wx) * t00 + wx * t10) + wy * ((1.0 - wx) * t01 + wx * t11)
    Dx = np.maximum(np.abs(t10 - t00), np.abs(t11 - t01))
    Dy = np.maximum(np.abs(t01 - t00), np.abs(t11 - t10))
    # the position's uncertainty, and the 4 x 4 block's contrasts where it reaches a neighbouring quad
    rx, ry = tw * EPS, th * EPS + extra_dy
    dx, dy = 1.0 / 256.0 + rx, 1.0 / 256.0 + ry
    near = (fx < dx) | (fx > 1.0 - rx) | (fy < dy) | (fy > 1.0 - ry)
    Wx, Wy = Dx, Dy
    if near.any():
        Wx = np.zeros_like(Dx)
        Wy = np.zeros_like(Dy)
        blk = [[at(iy + j, ix + i) for i in (-1, 0, 1, 2)] for j in (-1, 0, 1, 2)]
        for j in range(4):
            for i in range(3):
                Wx = np.maximum(Wx, np.abs(blk[j][i + 1] - blk[j][i]))
                Wy = np.maximum(Wy, np.abs(blk[i + 1][j] - blk[i][j]))
        Wx = np.where(near[..., None], Wx, Dx)
        Wy = np.where(near[..., None], Wy, Dy)
    e = Wx * dx + Wy * dy + (Wx > 0) * 1.0 + ((Wx > 0) | (Wy > 0)) * 0.5
    if mutation == "swap_rb":
        c, e, Dx, Dy = (a[..., [2, 1, 0, 3]] for a in (c, e, Dx, Dy))
    return Sample(c=c, e=e, Dx=Dx, Dy=Dy, seam=(ix < 0) | (ix + 1 > tw - 1), pole_lo=iy < 0, pole_hi=iy + 1 > th - 1)


def is_opaque(tex):
    return bool((np.asarray(tex)[..., 3] == 255).all())


def over_clear(c, e, opaque):
    """A straight-alpha sample over the cleared target (0, 0, 0, 255)."""
    out_c = np.empty_like(c)
    out_e = np.zeros_like(e)
    out_c[..., 3] = 255.0
    if opaque:
        out_c[..., :3] = c[..., :3]
        out_e[..., :3] = e[..., :3]
        return out_c, out_e
    a, ea = c[..., 3:4], e[..., 3:4]
    out_c[..., :3] = c[..., :3] * a / 255.0
    out_e[..., :3] = (a * e[..., :3] + np.minimum(255.0, c[..., :3] + e[..., :3]) * ea) / 255.0 + 0.5
    return out_c, out_e


def composite(s, es, d, ed):
    """Sample s (straight alpha, bounds es) blended over d (bounds ed)."""
    a, ea = s[..., 3:4], es[..., 3:4]
    a_hi = np.minimum(255.0, a + ea)
    ia_hi = np.minimum(255.0, 255.0 - a + ea)
    c = np.empty_like(s)
    e = np.empty_like(es)
    c[..., :3] = (s[..., :3] * a + d[..., :3] * (255.0 - a)) / 255.0
    e[..., :3] = (es[..., :3] * a_hi + ed[..., :3] * ia_hi + ea * np.abs(s[..., :3] - d[..., :3])) / 255.0 + 0.5
    da, eda = d[..., 3:4], ed[..., 3:4]
    c[..., 3:] = (255.0 * a + da * (255.0 - a)) / 255.0
    e[..., 3:] = (ea * (255.0 - da) + eda * ia_hi) / 255.0 + 0.5
    exact = (da == 255.0) & (eda == 0.0)
    c[..., 3:] = np.where(exact, 255.0, c[..., 3:])
    e[..., 3:] = np.where(exact, 0.0, e[..., 3:])
    return c, e


def _finish(s, tex, mask, target):
    """A straight-alpha sky sample to the pixel: over the cleared target, or
    (GEO_FLAG_COMPOSITE) over `target`, which a captured pixel leaves as it is."""
    captured = (np.asarray(mask) == 1)[..., None]
    if target is None:
        c, e = over_clear(s.c, s.e, is_opaque(tex))
        black = np.array([0.0, 0.0, 0.0, 255.0])
        return np.where(captured, black, c), np.where(captured, 0.0, e)
    d = np.asarray(target).astype(np.float64)
    if is_opaque(tex):  # the blend is skipped: the sample itself
        c, e = s.c.copy(), s.e.copy()
        c[..., 3], e[..., 3] = 255.0, 0.0
    else:
        c, e = composite(s.c, s.e, d, np.zeros_like(d))
    return np.where(captured, d, c), np.where(captured, 0.0, e)


def sky(tex, uv, mask, target=None, mutation=None):
    """The plain render's pixel: (c, e, the Sample)."""
    s = bilinear(tex, uv[..., 0], uv[..., 1], mutation)
    c, e = _finish(s, tex, mask, target)
    return c, e, s


def box(level):
    """The next mip level: rounded 2 x 2 means, block indices clamped (odd sizes)."""
    h, w = level.shape[:2]
    h2, w2 = max(1, h // 2), max(1, w // 2)
    ys = np.minimum(np.arange(h2)[:, None] * 2 + np.array([0, 1]), h - 1)
    xs = np.minimum(np.arange(w2)[:, None] * 2 + np.array([0, 1]), w - 1)
    a = level.astype(np.int64)
    s = sum(a[ys[:, j]][:, xs[:, i]] for j in range(2) for i in range(2))
    return ((s + 2) >> 2).astype(np.uint8)


def mip_chain(tex):
    levels = [np.asarray(tex, np.uint8)]
    for _ in range(MIP_LEVELS - 1):
        levels.append(box(levels[-1]))
    return levels


def lod(uv, tw, th):
    """lambda per pixel of an even-sized frame, from its 2 x 2 quad's UV differences."""
    U, V = uv[..., 0].astype(np.float64), uv[..., 1].astype(np.float64)
    h, w = U.shape
    assert h % 2 == 0 and w % 2 == 0
    xp, yp = np.arange(w) ^ 1, np.arange(h) ^ 1
    dux, dvx = (U - U[:, xp]) * tw, (V - V[:, xp]) * th
    duy, dvy = (U - U[yp, :]) * tw, (V - V[yp, :]) * th
    rho2 = np.maximum(dux * dux + dvx * dvx, duy * duy + dvy * dvy)
    with np.errstate(divide="ignore"):
        return np.clip(0.5 * np.log2(rho2), 0.0, MIP_LEVELS - 1.0)


def trilinear(tex, uv, mutation=None):
    """The mip-mapped straight-alpha sample: a Sample with `lam` added."""
    levels = mip_chain(tex)
    th, tw = levels[0].shape[:2]
    lam = lod(uv, tw, th)
    if mutation == "lod_plus_one":
        lam = np.clip(lam + 1.0, 0.0, MIP_LEVELS - 1.0)
    if mutation == "no_lod":
        lam = np.zeros_like(lam)
    if mutation == "nearest_level":
        lam = np.round(lam)
    S = [bilinear(lv, uv[..., 0], uv[..., 1], mutation) for lv in levels]
    C = np.stack([s.c for s in S])
    E = np.stack([s.e for s in S])
    top = MIP_LEVELS - 1
    l0 = np.minimum(np.floor(lam).astype(np.int64), top)
    l1 = np.minimum(l0 + 1, top)
    f = (lam - l0)[..., None]

    def pick(A, l):
        return np.take_along_axis(A, l[None, ..., None], axis=0)[0]

    c0, c1, e0, e1 = pick(C, l0), pick(C, l1), pick(E, l0), pick(E, l1)
    c = (1.0 - f) * c0 + f * c1
    e = e0 * (1.0 - f) + e1 * f + (np.abs(c1 - c0) + np.abs(e1 - e0)) * DLAMBDA + 0.5
    # within dl of a level boundary the render may blend the neighbouring pair
    frac = lam - l0
    below = (frac < DLAMBDA) & (l0 > 0)
    above = (frac > 1.0 - DLAMBDA) & (l0 + 2 <= top)
    for cond, lo_ in ((below, np.maximum(l0 - 1, 0)), (above, np.minimum(l0 + 1, top - 1))):
        if cond.any():
            ca, cb, ea_, eb = pick(C, lo_), pick(C, lo_ + 1), pick(E, lo_), pick(E, lo_ + 1)
            emax = np.maximum(np.maximum(e0, e1), np.maximum(ea_, eb))
            slope = np.maximum(np.abs(c1 - c0), np.abs(cb - ca))
            e = np.where(cond[..., None], emax + slope * DLAMBDA + 0.5, e)
    s = Sample(c=c, e=e, lam=lam)
    return s


def sky_mips(tex, uv, mask, target=None, mutation=None):
    """The GEO_FLAG_MIPS render's pixel: (c, e, lambda)."""
    s = trilinear(tex, uv, mutation)
    c, e = _finish(s, tex, mask, target)
    return c, e, s.lam


def disk(base_c, base_e, hits, tex, r_in, r_out, mutation=None):
    """The disk's images over the sky's result.  hits: (..., 3, 2) slots
    (r, U_d), r > 0 where the slot is hit; r_in, r_out: as the entry point
    sees them (f32)."""
    r_in, r_out = float(np.float32(r_in)), float(np.float32(r_out))
    th = np.asarray(tex).shape[0]
    c, e = base_c.copy(), base_e.copy()
    order = (0, 1, 2) if mutation == "disk_order_reversed" else (2, 1, 0)
    if mutation == "disk_slot0_only":
        order = (0,)
    for k in order:
        r = hits[..., k, 0].astype(np.float64)
        Ud = hits[..., k, 1].astype(np.float64)
        hit = r > 0.0
        Vd = np.clip((r - r_in) / (r_out - r_in), 0.0, 1.0)
        if mutation == "disk_flip_v":
            Vd = 1.0 - Vd
        if mutation == "disk_swap_uv":
            Ud, Vd = Vd, Ud
        s = bilinear(tex, Ud, Vd, mutation, extra_dy=th * 2.0 ** -22)
        nc, ne = composite(s.c, s.e, c, e)
        c = np.where(hit[..., None], nc, c)
        e = np.where(hit[..., None], ne, e)
    return c, e


def ss4(c, e):
    """The 2 x 2 resolve of a (2h, 2w, 4) sample frame's exact values and bounds."""
    def mean(a):
        return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) / 4.0

    return mean(c), mean(e) + 0.5


def outside(rgba, c, e):
    """(err, over): the render's distance from c per channel, and where it exceeds the bound."""
    err = np.abs(np.asarray(rgba).astype(np.float64) - c)
    return err, err > e + SLACK
