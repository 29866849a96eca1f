// geo_disk.h — GEO_FLAG_DISK: a ray-traced thin accretion disk on the
// per-pixel path (a build extension, not in the reference).
//
// A ray lies in one plane through the centre, and the disk plane (through the
// centre, unit normal n in the sky texture's frame) cuts that plane along a
// line: the ray meets the disk plane at the traveled angles a_k = a_0 + k pi,
// known before the first RK4 step.  A disk hit is the integrator's u at a_k
// (one partial RK4 step from the grid node below a_k) inside the annulus.
//
// Shared by the render kernel (geo_render_kernels.h) and the CPU path
// (cpu_render.cpp, geo_render_cpu_disk): the same f32 operation sequence, so
// the two agree bit for bit.  The f32 specification:
//   * (cos phi, sin phi) = (c2x, c2y) * rcpf_(rho)  ((1, 0) for rho = 0)
//   * A = fma(N_x, cos phi, N_y sin phi), B = N_z, N = M2^T n (host, f64,
//     rounded once); s = +1 if B < 0 or (B = 0 and A < 0), else -1;
//     (y, x) = (-s B, s A), so y >= 0;  a_0 = 2 pi atan2_turns_(y, x) in
//     (0, pi];  H = sqrtf_(fma(y, y, x x)), (sin a_0, cos a_0) = (y, x) rcpf_(H);
//     H = 0 (or NaN): no crossing
//   * a_k = fma(k, pi, a_0);  node j_k = floor(min(a_k * (1/step), 2^24)),
//     partial step d_k = fma(-j_k, step, a_k) (may fall an ulp outside
//     [0, step]: the RK4 map is evaluated there all the same)
//   * U(a_k) = rk4_step from the main loop's state at node j_k with step d_k
//     (half steps and squares formed as newton_angle forms them)
//   * crossing k is a hit when j_k < steps (the main loop executed the step
//     that starts at node j_k), a_k < the returned traveled angle (kNoValue
//     = 15 > a_2 when the ray never crosses the sphere) and
//     u_lo <= U <= u_hi, (u_lo, u_hi) = (scale / r_out, scale / r_in)
//   * r = scale * rcpf_(U);  Vd = med3((r - r_in) * (1 / (r_out - r_in)), 0, 1);
//     Ud = med3(atan2_turns_(Y, X), 0, 1) with (X, Y) the hit direction's
//     components along the disk basis: X = fma(sin a_k, fma(Ex_x, cos phi,
//     Ex_y sin phi), cos a_k Ex_z), E = M2^T e (host, f64, rounded once),
//     (sin a_k, cos a_k) = (-1)^k (sin a_0, cos a_0).
// A ray the reference's pre-filters or radial cases end before the loop
// (geodesic_init: an observer inside the photon sphere) integrates nothing
// and draws no disk.
#pragma once

#include <stdint.h>

#include "geo_band.h"
#include "geo_pixel.h"

namespace geo {

constexpr int kDiskMaxCrossings = 3;  // GEO_DISK_MAX_CROSSINGS
constexpr float kTwoPi = 6.28318530717958647692f;
constexpr float kDiskMaxNode = 16777216.0f;  // 2^24 >= max_steps: never a hit

// Frame-uniform disk constants (host, f64, each rounded once to f32).
struct DiskConsts {
    float N[3];           // M2^T n
    float ex[3], ey[3];   // M2^T e_x, M2^T e_y
    float r_in, r_out;
    float inv_dr;         // 1 / (r_out - r_in) (f32 divide)
    float u_lo, u_hi;     // scale / r_out, scale / r_in (f32 divides)
    float inv_step;       // 1 / step (f32 divide)
};

// m2: central_to_uv (column-major 4 x 4); n, axis: the disk's normal and the
// direction of azimuth 0, in the sky texture's frame.  False for a zero normal
// or an axis parallel to it.
GEO_HD bool disk_consts(const float* m2, const float* normal, const float* axis, float r_in, float r_out,
                        const PixelConsts& k, DiskConsts* out) {
    double n[3] = {(double)normal[0], (double)normal[1], (double)normal[2]};
    const double nl = __builtin_sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(nl > 0.0) || !(nl < 1e300)) return false;
    for (int i = 0; i < 3; ++i) n[i] /= nl;
    const double an = (double)axis[0] * n[0] + (double)axis[1] * n[1] + (double)axis[2] * n[2];
    double e[3];
    for (int i = 0; i < 3; ++i) e[i] = (double)axis[i] - an * n[i];
    const double el = __builtin_sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    const double al = __builtin_sqrt((double)axis[0] * axis[0] + (double)axis[1] * axis[1] + (double)axis[2] * axis[2]);
    if (!(el > 1e-12 * al) || !(el < 1e300)) return false;
    for (int i = 0; i < 3; ++i) e[i] /= el;
    const double f[3] = {n[1] * e[2] - n[2] * e[1], n[2] * e[0] - n[0] * e[2], n[0] * e[1] - n[1] * e[0]};
    for (int i = 0; i < 3; ++i) {
        // (M2^T v)_i = column i of M2 . v
        const double c0 = (double)m2[4 * i], c1 = (double)m2[4 * i + 1], c2 = (double)m2[4 * i + 2];
        out->N[i] = (float)(c0 * n[0] + c1 * n[1] + c2 * n[2]);
        out->ex[i] = (float)(c0 * e[0] + c1 * e[1] + c2 * e[2]);
        out->ey[i] = (float)(c0 * f[0] + c1 * f[1] + c2 * f[2]);
    }
    out->r_in = r_in;
    out->r_out = r_out;
    out->inv_dr = 1.0f / (r_out - r_in);
    out->u_lo = k.scale / r_out;
    out->u_hi = k.scale / r_in;
    out->inv_step = 1.0f / k.step;
    return true;
}

// The crossings of one ray: angles, nodes and partial steps, known before the
// integration.
struct DiskRay {
    float cphi, sphi;  // the ray plane's azimuth
    float sa, ca;      // sin a_0, cos a_0
    float ak[kDiskMaxCrossings];
    uint32_t jn[kDiskMaxCrossings];  // 0xFFFFFFFF: no crossing
    float dn[kDiskMaxCrossings];
};

GEO_HD void disk_ray(const DiskConsts& d, const PixelConsts& k, float c2x, float c2y, float rho, float rrho,
                     DiskRay* r) {
    float cphi = 1.0f, sphi = 0.0f;
    if (rho > 0.0f) {
        cphi = c2x * rrho;
        sphi = c2y * rrho;
    }
    r->cphi = cphi;
    r->sphi = sphi;
    const float A = fmaf_(d.N[0], cphi, d.N[1] * sphi), B = d.N[2];
    const float s = (B < 0.0f || (B == 0.0f && A < 0.0f)) ? 1.0f : -1.0f;
    const float y = -s * B, x = s * A;
    const float H = sqrtf_(fmaf_(y, y, x * x));
    const bool crosses = H > 0.0f;
    const float rH = rcpf_(H);
    r->sa = y * rH;
    r->ca = x * rH;
    const float a0 = kTwoPi * atan2_turns_(y, x);
#pragma unroll
    for (int c = 0; c < kDiskMaxCrossings; ++c) {
        const float a = fmaf_((float)c, kPi, a0);
        const float jf = __builtin_fminf(a * d.inv_step, kDiskMaxNode);
        const uint32_t j = crosses ? (uint32_t)floor_i32_(jf) : 0xFFFFFFFFu;
        r->ak[c] = a;
        r->jn[c] = j;
        r->dn[c] = fmaf_(-(float)j, k.step, a);
    }
}

// U at the end of a partial RK4 step of length dl from (pu, pb).
template <int KIND>
GEO_HD float disk_partial_(float pu, float pb, float dl) {
    const float d2 = dl * dl;
    const float d6 = dl * kSixth;
    float wu, wub;
    rk4_step<KIND>(pu, pb, dl, dl * 0.5f, d2 * 0.25f, d2 * 0.5f, d6, dl * d6, &wu, &wub);
    return wu;
}

// geodesic_angle_v with the disk probes: the same traveled angle and step
// count, and in Uk[c] the integrator's U at crossing c for every crossing
// whose node the loop reached before the lane's stopping group ended (0
// otherwise; disk_hit decides which of them count).
//
// The loop keeps geodesic_angle_v's groups of kGroup steps, its exact group
// stop tests (group_stop_) and its finish (geodesic_finish), on one register
// set in place of the pair loop's two: a probe reads the state at a node
// inside the group, which the pair loop's alternating sets do not keep
// addressable by node.  Per group the disk costs one compare (the lane's next
// node against the group's end) and the rarely taken arm that does the
// partial step.
template <int KIND>
GEO_HD float geodesic_angle_disk(const PixelConsts& k, float st, float ct, float rct, const DiskRay& dr,
                                 uint32_t* steps, float (&Uk)[kDiskMaxCrossings]) {
    constexpr int G = kGroup;
    *steps = 0;
#pragma unroll
    for (int c = 0; c < kDiskMaxCrossings; ++c) Uk[c] = 0.0f;
    float U, UB, early;
    if (!geodesic_init<KIND>(k, st, ct, rct, &early, &U, &UB)) return early;
    float h = k.step, hh = k.hh, hh2 = k.hh2, hhh = k.hhh, h6 = k.h6, h2_6 = k.h2_6;
    StopTest<KIND> stop_at(k);
    GEO_OPAQUE(h);
    GEO_OPAQUE(hh);
    GEO_OPAQUE(hh2);
    GEO_OPAQUE(hhh);
    GEO_OPAQUE(h6);
    GEO_OPAQUE(h2_6);
    GEO_OPAQUE(stop_at.lo);
    GEO_OPAQUE(stop_at.hi);
    const uint32_t ms = k.max_steps;
    const uint32_t all = (ms / (uint32_t)G) * (uint32_t)G;
    // the lane's next crossing: slot kc at node jt with partial step dt
    uint32_t kc = 0, jt = dr.jn[0];
    float dt = dr.dn[0];
    // (three scalars and selects: a store at a per-lane slot index would put
    // the array in scratch memory)
    float u0 = 0.0f, u1 = 0.0f, u2 = 0.0f;
    auto probe = [&](float pu, float pb) {
        const float v = disk_partial_<KIND>(pu, pb, dt);
        u0 = kc == 0u ? v : u0;
        u1 = kc == 1u ? v : u1;
        u2 = kc == 2u ? v : u2;
        ++kc;
        jt = kc == 1u ? dr.jn[1] : (kc == 2u ? dr.jn[2] : 0xFFFFFFFFu);
        dt = kc == 1u ? dr.dn[1] : dr.dn[2];
    };
    float su_[G + 1], sb_[G + 1];
#pragma unroll
    for (int j = 0; j <= G; ++j) {
        GEO_UNSET(su_[j]);
        GEO_UNSET(sb_[j]);
    }
    float cu = U, cb = UB;
    // The loop's exit is wave-uniform, as in run_groups_pp and the adaptive
    // loop: the lanes still integrating are the scalar mask `live`; a lane
    // that stops records its stopping group's states in a rarely taken block,
    // leaves `live` and keeps stepping harmlessly (its registers are no longer
    // read).  One exit edge: an empty `live` ends the count.
    uint64_t live = ballot_(true);
    uint32_t it = all, n = 0;
    uint32_t rem = ms / (uint32_t)G;
    while (rem != 0) {
        float ou[G], ob[G];
        group_steps_<G, KIND>(cu, cb, h, hh, hh2, hhh, h6, h2_6, ou, ob);
        const uint64_t due = ballot_(jt < n + (uint32_t)G) & live;
        if (due != 0) {
            if (in_ballot_(due)) {
                GEO_RARE();
                do {
                    const uint32_t idx = jt - n;  // 0 .. G-1: the group's start state, or ou[idx - 1]
                    float pu = cu, pb = cb;
#pragma unroll
                    for (int j = 1; j < G; ++j) {
                        pu = idx == (uint32_t)j ? ou[j - 1] : pu;
                        pb = idx == (uint32_t)j ? ob[j - 1] : pb;
                    }
                    probe(pu, pb);
                } while (jt < n + (uint32_t)G);
            }
        }
        uint64_t hit;
        if constexpr (KIND == kCurvedIn)
            hit = group_stop_<G, KIND, kTestEach>(stop_at, ou, ob);
        else if (stop_at.above0)  // frame-uniform
            hit = group_stop_<G, KIND, kTestLow>(stop_at, ou, ob);
        else
            hit = group_stop_<G, KIND, kTestBoth>(stop_at, ou, ob);
        hit &= live;
        --rem;
        if (hit != 0) {
            if (in_ballot_(hit)) {
                GEO_RARE();
                su_[0] = cu;
                sb_[0] = cb;
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    su_[j + 1] = ou[j];
                    sb_[j + 1] = ob[j];
                }
                it = n;
            }
            live &= ~hit;
            rem = live == 0 ? 0u : rem;
        }
        cu = ou[G - 1];
        cb = ob[G - 1];
        n += (uint32_t)G;
    }
    const bool stopped = it != all;
    n = it;
    if (!stopped) {
        // the budget's tail of fewer than G steps (geodesic_finish replays
        // it for the angle): the probes at its nodes
#pragma unroll
        for (int j = 0; j <= G; ++j) {
            su_[j] = cu;
            sb_[j] = cb;
        }
        float tu = cu, tb = cb;
        for (uint32_t r = n; r < ms; ++r) {
            while (jt == r) probe(tu, tb);
            float nu, nub;
            rk4_step<KIND>(tu, tb, k.step, k.hh, k.hh2, k.hhh, k.h6, k.h2_6, &nu, &nub);
            if (stop_at(nu, nub)) break;
            tu = nu;
            tb = nub;
        }
    }
    Uk[0] = u0;
    Uk[1] = u1;
    Uk[2] = u2;
    return geodesic_finish<G, KIND>(k, stop_at, n, su_, sb_, steps);
}

// Crossing c of the ray: a hit?  Then its radius and disk texture coordinates.
GEO_HD bool disk_hit(const DiskConsts& d, const PixelConsts& k, const DiskRay& dr, int c, float Uc, uint32_t steps,
                     float angle, float* r, float* Ud, float* Vd) {
    const bool hit = (dr.jn[c] < steps) & (dr.ak[c] < angle) & (med3_(Uc, d.u_lo, d.u_hi) == Uc);
    if (!hit) return false;
    const float rr = k.scale * rcpf_(Uc);
    const float sg = (c & 1) ? -1.0f : 1.0f;
    const float sa = sg * dr.sa, ca = sg * dr.ca;
    const float X = fmaf_(sa, fmaf_(d.ex[0], dr.cphi, d.ex[1] * dr.sphi), ca * d.ex[2]);
    const float Y = fmaf_(sa, fmaf_(d.ey[0], dr.cphi, d.ey[1] * dr.sphi), ca * d.ey[2]);
    *r = rr;
    *Ud = med3_(atan2_turns_(Y, X), 0.0f, 1.0f);
    *Vd = med3_((rr - d.r_in) * d.inv_dr, 0.0f, 1.0f);
    return true;
}

template <int S, typename Sample>
GEO_HD uint32_t disk_shade_slot_(const DiskConsts& d, const PixelConsts& k, const DiskRay& dr, float Us, uint32_t steps,
                                 float angle, uint32_t c, const Sample& sample, float* hits) {
    float r = 0.0f, Ud = 0.0f, Vd = 0.0f;
    if (disk_hit(d, k, dr, S, Us, steps, angle, &r, &Ud, &Vd)) {
        c = composite_(sample(Ud, Vd), c);
    } else {
        r = 0.0f;
        Ud = 0.0f;
    }
    if (hits) {
        hits[2 * S] = r;
        hits[2 * S + 1] = Ud;
    }
    return c;
}

// The disk over a pixel's base colour (what the plain render writes): the
// hits composited far to near with the 8-bit blend; hits (optional): the
// pixel's 3 x (r, Ud) slots.  sample(Ud, Vd): the level-0 sample of the disk
// texture (U wraps, V clamps).
template <typename Sample>
GEO_HD uint32_t disk_shade(const DiskConsts& d, const PixelConsts& k, const DiskRay& dr,
                           const float (&Uk)[kDiskMaxCrossings], uint32_t steps, float angle, uint32_t base,
                           const Sample& sample, float* hits) {
    static_assert(kDiskMaxCrossings == 3, "three slots, written out (constant indices: the arrays stay in registers)");
    uint32_t c = base;
    c = disk_shade_slot_<2>(d, k, dr, Uk[2], steps, angle, c, sample, hits);
    c = disk_shade_slot_<1>(d, k, dr, Uk[1], steps, angle, c, sample, hits);
    c = disk_shade_slot_<0>(d, k, dr, Uk[0], steps, angle, c, sample, hits);
    return c;
}

// ---- Doppler and redshift shading (geo_set_disk_shift) ------------------
// The disk's matter at radius r moves on circular geodesics about spin * n
// (spin = +1: the sense in which the disk's azimuth U grows) with angular
// velocity Omega = sqrt(rs / (2 r^3)) (c = 1, scene units; circular timelike
// orbits need r > 1.5 rs: a shifted render is refused unless r_in > 1.5 rs,
// or rs = 0, where Omega = 0).  A hit's received / emitted frequency ratio is
//   g = g_grav g_dopp g_obs,
//   g_grav = sqrt(1 - 1.5 rs/r) / sqrt(1 - rs/r_obs)   (the emitter's time
//            dilation on its orbit; the static observer's potential),
//   g_dopp = 1 / (1 + spin Omega b w),  b = r_obs cos(theta) / sqrt(1 - rs/r_obs)
//            (the ray's impact parameter, GEO_FLAG_RING_F64's b) and
//            w = sigma (z x q) . N = sigma (N_y cos phi - N_x sin phi): the
//            photon travels the traced ray backwards, so its angular momentum
//            about the disk axis is -b w per unit energy, conserved along the
//            ray (one w for all three crossings).  sigma = sign(det M2): the
//            disk's sense of rotation is defined in the sky texture's frame
//            (e_y = n x e_x there), a cross product of central-frame
//            components has the other handedness when central_to_uv is a
//            reflection, and the observer's pipeline produces one (det = -1),
//   g_obs  = the observer's own Doppler factor (pixel_central_dir_g).
// The signs were checked against an f64 restatement that uses the ray's local
// tangent at the hit instead of the conserved angular momentum
// (tests/disk_shift_ref.py) and by the approaching / receding side test.
// The f32 specification (the operations of geo_math.h / geo_pixel.h):
//   per frame (host, f64, each rounded once): sb = sigma spin r_obs / sqrt(1 - rs/r_obs),
//     ih = 1 / sqrt(1 - rs/r_obs)
//   per ray:  w' = fma(N_y, cos phi, -(N_x sin phi));  bw = (rho sb) w'
//     (rho = central_rho = cos theta);  gk = g_obs ih
//   per hit (r of disk_hit):  ir = rcpf_(r);  x = rs ir;
//     den = fma(bw ir, sqrtf_(0.5 x), 1);
//     g = med3((sqrtf_(fma(-1.5, x, 1)) rcpf_(den)) gk, 0, GEO_DISK_G_MAX)
//     (a NaN, from a radicand an ulp below 0, becomes 0)
//   colour: gp = g^p by p multiplications from 1 (p = exponent, 0..4);
//     m = min(gain gp, 65536);  each of R, G, B of the hit's texture sample:
//     min(255, floor_i32_(fma(c, m, 0.5))); alpha kept.  m = 1 keeps the bytes.
// GEO_DISK_G_MAX = 16: g^4 <= 65536 = the cap of m, so no power overflows and
// fma(c, m, 0.5) < 2^24 + 1 stays far inside floor_i32_'s range.  Physical
// ratios reach it only for an observer within 0.4 % of the horizon or a ray
// within an ulp of Omega b = 1.
constexpr float kDiskGMax = 16.0f;     // GEO_DISK_G_MAX
constexpr float kDiskMMax = 65536.0f;  // the cap of the colour multiplier

struct DiskShift {
    float sb;  // sign(det M2) * spin * r_obs / sqrt(1 - rs/r_obs)
    float ih;  // 1 / sqrt(1 - rs/r_obs)
    float gain;
    uint32_t exponent;
};

// m2: central_to_uv; rs = 0, or r_obs > rs (GEO_FLAG_DISK's rule); spin = +1 or -1.
GEO_HD DiskShift disk_shift_consts(const float* m2, float rs, float r_obs, int spin, uint32_t exponent, float gain) {
    const double h = 1.0 / __builtin_sqrt(1.0 - (double)rs / (double)r_obs);
    const double a = m2[0], b = m2[1], c = m2[2], d = m2[4], e = m2[5], f = m2[6], g = m2[8], i = m2[9], j = m2[10];
    const double det = a * (e * j - f * i) - d * (b * j - c * i) + g * (b * f - c * e);
    DiskShift s;
    s.sb = (float)((det < 0.0 ? -1.0 : 1.0) * (double)spin * (double)r_obs * h);
    s.ih = (float)h;
    s.gain = gain;
    s.exponent = exponent;
    return s;
}

// The ray's shift terms, known before the integration.
struct DiskShiftRay {
    float bw;  // spin * b * w (sigma included)
    float gk;  // g_obs / sqrt(1 - rs/r_obs)
};

GEO_HD void disk_shift_ray(const DiskConsts& d, const DiskShift& s, const DiskRay& dr, float rho, float g_obs,
                           DiskShiftRay* r) {
    const float w = fmaf_(d.N[1], dr.cphi, -(d.N[0] * dr.sphi));
    r->bw = (rho * s.sb) * w;
    r->gk = g_obs * s.ih;
}

// The frequency ratio of a hit at radius r.
GEO_HD float disk_shift_g(const PixelConsts& k, const DiskShiftRay& sr, float r) {
    const float ir = rcpf_(r);
    const float x = k.rs * ir;
    const float den = fmaf_(sr.bw * ir, sqrtf_(0.5f * x), 1.0f);
    const float g = (sqrtf_(fmaf_(-1.5f, x, 1.0f)) * rcpf_(den)) * sr.gk;
    return med3_(g, 0.0f, kDiskGMax);
}

GEO_HD uint32_t disk_shift_channel_(uint32_t c, float m) {
    const int32_t v = floor_i32_(fmaf_((float)c, m, 0.5f));
    return (uint32_t)(v < 255 ? v : 255);
}

// The texture sample s scaled by the shift g (alpha kept).
GEO_HD uint32_t disk_shift_colour(const DiskShift& s, float g, uint32_t smp) {
    float gp = 1.0f;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) gp = i < s.exponent ? gp * g : gp;
    const float m = __builtin_fminf(s.gain * gp, kDiskMMax);
    return disk_shift_channel_(smp & 0xFFu, m) | (disk_shift_channel_((smp >> 8) & 0xFFu, m) << 8) |
           (disk_shift_channel_((smp >> 16) & 0xFFu, m) << 16) | (smp & 0xFF000000u);
}

// disk_shade_slot_ with the shift: the scaled sample is what composite_
// blends; gs (optional): the pixel's 3 g slots (0 where the crossing is no hit).
template <int S, typename Sample>
GEO_HD uint32_t disk_shade_shift_slot_(const DiskConsts& d, const PixelConsts& k, const DiskRay& dr,
                                       const DiskShift& sh, const DiskShiftRay& sr, float Us, uint32_t steps,
                                       float angle, uint32_t c, const Sample& sample, float* hits, float* gs) {
    float r = 0.0f, Ud = 0.0f, Vd = 0.0f, g = 0.0f;
    if (disk_hit(d, k, dr, S, Us, steps, angle, &r, &Ud, &Vd)) {
        g = disk_shift_g(k, sr, r);
        c = composite_(disk_shift_colour(sh, g, sample(Ud, Vd)), c);
    } else {
        r = 0.0f;
        Ud = 0.0f;
    }
    if (hits) {
        hits[2 * S] = r;
        hits[2 * S + 1] = Ud;
    }
    if (gs) gs[S] = g;
    return c;
}

template <typename Sample>
GEO_HD uint32_t disk_shade_shift(const DiskConsts& d, const PixelConsts& k, const DiskRay& dr, const DiskShift& sh,
                                 const DiskShiftRay& sr, const float (&Uk)[kDiskMaxCrossings], uint32_t steps,
                                 float angle, uint32_t base, const Sample& sample, float* hits, float* gs) {
    static_assert(kDiskMaxCrossings == 3, "three slots, written out");
    uint32_t c = base;
    c = disk_shade_shift_slot_<2>(d, k, dr, sh, sr, Uk[2], steps, angle, c, sample, hits, gs);
    c = disk_shade_shift_slot_<1>(d, k, dr, sh, sr, Uk[1], steps, angle, c, sample, hits, gs);
    c = disk_shade_shift_slot_<0>(d, k, dr, sh, sr, Uk[0], steps, angle, c, sample, hits, gs);
    return c;
}

// ---- Blackbody emission (geo_set_disk_emission) ---------------------------
// The disk's colour from a temperature: a radial profile T(r) = t_ref tau(r),
// the observed temperature T_obs = g T(r) with the g of the shading above (the
// emission's own spin), a colour ramp over 1/T_obs and the bolometric
// brightness (T_obs / t_ref)^4, which holds the g^4 beaming.
//   tau(r), x = r_in / r:
//     GEO_DISK_PROFILE_POWER  x^(3/4)
//     GEO_DISK_PROFILE_THIN   x^(3/4) (1 - sqrt x)^(1/4) / f_max, the zero-torque
//       inner edge; f_max = (6/7)^(3/2) (1/7)^(1/4) = 0.487871339, reached at
//       x = 36/49: tau = 0 at r_in, 1 at r = 49/36 r_in
// The f32 specification (the operations of geo_math.h / geo_pixel.h; no
// hardware log, exp or pow):
//   per frame (host, f64, each rounded once): sb, ih = disk_shift_consts with
//     the emission's spin;  inv_fmax = 1 / ((6/7)^1.5 (1/7)^0.25);
//     D = 1/t_lo - 1/t_hi;  ka = -(n - 1) / (t_ref D);  kb = (n - 1) (1/t_lo) / D;
//     n1 = n - 1 (exact)
//   per ray: disk_shift_ray, unchanged
//   per hit (r of disk_hit, g of disk_shift_g):
//     ir = rcpf_(r);  x = med3(r_in ir, 0, 1) (r can round an ulp under r_in:
//       1 - sqrt x must not go negative);  s = sqrtf_(x);  tau = s sqrtf_(s);
//     THIN: tau = min((tau sqrtf_(sqrtf_(1 - s))) inv_fmax, 1);
//     q = g tau;  q2 = q q;  m = min(exposure (q2 q2), 65536);
//     pos = med3(fma(rcpf_(q), ka, kb), 0, n1)  (q = 0: rcpf_ = +inf, ka < 0,
//       so -inf, which clamps to 0; a NaN clamps to 0 as well);
//     i = min((uint32_t)floor_i32_(pos), n - 2);  w = floor_i32_((pos - i) 256)
//   ramp colour e, per channel of entries a = ramp[i], b = ramp[i + 1]:
//     (a (256 - w) + b w + 128) >> 8  (w in 0..256; pos = n - 1 gives i = n - 2
//     and w = 256: the last entry exactly)
//   colour: mk = m (1/255) (kInv255, f32);  each of R, G, B of the hit's texture
//     sample t: min(255, floor_i32_(fma((float)(t_c e_c), mk, 0.5)));  alpha kept.
// Ranges: q <= GEO_DISK_G_MAX = 16, so q^4 <= 65536 = the cap of m;
// t_c e_c <= 65025 and 65025 * 65536 / 255 = 16711680 < 2^24, inside
// floor_i32_'s range and exact as an integer-valued f32 bound.
constexpr float kInv255 = 1.0f / 255.0f;
constexpr uint32_t kDiskProfilePower = 0u, kDiskProfileThin = 1u;  // GEO_DISK_PROFILE_*
constexpr uint32_t kDiskRampMax = 1024u;                           // GEO_DISK_RAMP_MAX

struct DiskEmission {
    DiskShift s;  // sb and ih with the emission's spin (gain and exponent unused)
    float inv_fmax;
    float ka, kb;
    float n1;  // n - 1
    float exposure;
    uint32_t profile;
    uint32_t n2;  // n - 2
};

// m2, rs, r_obs, spin: disk_shift_consts's; 0 < t_lo < t_hi, t_ref > 0, n in 2..kDiskRampMax.
GEO_HD DiskEmission disk_emission_consts(const float* m2, float rs, float r_obs, int spin, uint32_t profile,
                                         float t_ref, float t_lo, float t_hi, float exposure, uint32_t n) {
    DiskEmission e;
    e.s = disk_shift_consts(m2, rs, r_obs, spin, 0u, 1.0f);
    e.inv_fmax = (float)(1.0 / (__builtin_sqrt(6.0 / 7.0) * (6.0 / 7.0) * __builtin_sqrt(__builtin_sqrt(1.0 / 7.0))));
    const double il = 1.0 / (double)t_lo, D = il - 1.0 / (double)t_hi, n1 = (double)(n - 1u);
    e.ka = (float)(-n1 / ((double)t_ref * D));
    e.kb = (float)(n1 * il / D);
    e.n1 = (float)(n - 1u);
    e.exposure = exposure;
    e.profile = profile;
    e.n2 = n - 2u;
    return e;
}

// q = T_obs / t_ref of a hit at radius r seen at the frequency ratio g.
GEO_HD float disk_emission_q(const DiskConsts& d, const DiskEmission& e, float g, float r) {
    const float ir = rcpf_(r);
    const float x = med3_(d.r_in * ir, 0.0f, 1.0f);
    const float s = sqrtf_(x);
    float tau = s * sqrtf_(s);
    if (e.profile == kDiskProfileThin)  // frame-uniform
        tau = __builtin_fminf((tau * sqrtf_(sqrtf_(1.0f - s))) * e.inv_fmax, 1.0f);
    return g * tau;
}

// The texture sample smp shaded by the ramp's colour at q (alpha kept).
// fetch(i): entry i of the ramp, i < n.
template <typename Fetch>
GEO_HD uint32_t disk_emission_colour(const DiskEmission& e, float q, uint32_t smp, const Fetch& fetch) {
    const float q2 = q * q;
    const float m = __builtin_fminf(e.exposure * (q2 * q2), kDiskMMax);
    const float pos = med3_(fmaf_(rcpf_(q), e.ka, e.kb), 0.0f, e.n1);
    const uint32_t fi = (uint32_t)floor_i32_(pos);
    const uint32_t i = fi < e.n2 ? fi : e.n2;  // (unsigned: whatever pos is, i + 1 < n)
    const uint32_t w = (uint32_t)floor_i32_((pos - (float)i) * 256.0f);
    const uint32_t a = fetch(i), b = fetch(i + 1u);
    const uint32_t iw = 256u - w;
    // R and B in 16-bit fields (a field is at most 255 * 256 + 128: no carry), G alone
    const uint32_t rb = (((a & 0x00FF00FFu) * iw + (b & 0x00FF00FFu) * w + 0x00800080u) >> 8) & 0x00FF00FFu;
    const uint32_t gg = (((a >> 8) & 0xFFu) * iw + ((b >> 8) & 0xFFu) * w + 128u) >> 8;
    const float mk = m * kInv255;
    return disk_shift_channel_((smp & 0xFFu) * (rb & 0xFFu), mk) |
           (disk_shift_channel_(((smp >> 8) & 0xFFu) * gg, mk) << 8) |
           (disk_shift_channel_(((smp >> 16) & 0xFFu) * (rb >> 16), mk) << 16) | (smp & 0xFF000000u);
}

// disk_shade_shift_slot_ with the emission: qs (optional): the pixel's 3 q
// slots (0 where the crossing is no hit).
template <int S, typename Sample, typename Fetch>
GEO_HD uint32_t disk_shade_emit_slot_(const DiskConsts& d, const PixelConsts& k, const DiskRay& dr,
                                      const DiskEmission& em, const DiskShiftRay& sr, float Us, uint32_t steps,
                                      float angle, uint32_t c, const Sample& sample, const Fetch& fetch, float* hits,
                                      float* gs, float* qs) {
    float r = 0.0f, Ud = 0.0f, Vd = 0.0f, g = 0.0f, q = 0.0f;
    if (disk_hit(d, k, dr, S, Us, steps, angle, &r, &Ud, &Vd)) {
        g = disk_shift_g(k, sr, r);
        q = disk_emission_q(d, em, g, r);
        c = composite_(disk_emission_colour(em, q, sample(Ud, Vd), fetch), c);
    } else {
        r = 0.0f;
        Ud = 0.0f;
    }
    if (hits) {
        hits[2 * S] = r;
        hits[2 * S + 1] = Ud;
    }
    if (gs) gs[S] = g;
    if (qs) qs[S] = q;
    return c;
}

template <typename Sample, typename Fetch>
GEO_HD uint32_t disk_shade_emit(const DiskConsts& d, const PixelConsts& k, const DiskRay& dr, const DiskEmission& em,
                                const DiskShiftRay& sr, const float (&Uk)[kDiskMaxCrossings], uint32_t steps,
                                float angle, uint32_t base, const Sample& sample, const Fetch& fetch, float* hits,
                                float* gs, float* qs) {
    static_assert(kDiskMaxCrossings == 3, "three slots, written out");
    uint32_t c = base;
    c = disk_shade_emit_slot_<2>(d, k, dr, em, sr, Uk[2], steps, angle, c, sample, fetch, hits, gs, qs);
    c = disk_shade_emit_slot_<1>(d, k, dr, em, sr, Uk[1], steps, angle, c, sample, fetch, hits, gs, qs);
    c = disk_shade_emit_slot_<0>(d, k, dr, em, sr, Uk[0], steps, angle, c, sample, fetch, hits, gs, qs);
    return c;
}

// ---- The capture band's lanes in f64 (geo_set_disk_ring_f64) -------------
// While the state is on, a lane of the band |b/b_c - 1| < GEO_RING_X
// (geo::in_band on the f32 ray, GEO_FLAG_RING_F64's own test) takes its
// traveled angle, mask, step count and crossing probes from the f64 path
// (geo_band.h band_lambda_disk, which states the lane's rules); every other
// lane does what it does without the state.  Both kinds of lane meet in
// DiskHits, a ray's three crossings as (hit, r): the f32 lane's by disk_hit's
// own test and radius, the band lane's by the f64 hit rule with r rounded
// once to f32.  Everything after r (Ud, Vd, g, q, the samples and the
// far-to-near blend) is the f32 code above on that r.
struct DiskHits {
    bool hit[kDiskMaxCrossings];
    float r[kDiskMaxCrossings];  // (read only where hit)
};

// An f32 lane's crossings: disk_hit's test and radius.
GEO_HD void disk_hits_f32(const DiskConsts& d, const PixelConsts& k, const DiskRay& dr,
                          const float (&Uk)[kDiskMaxCrossings], uint32_t steps, float angle, DiskHits* h) {
#pragma unroll
    for (int c = 0; c < kDiskMaxCrossings; ++c) {
        h->hit[c] = (dr.jn[c] < steps) & (dr.ak[c] < angle) & (med3_(Uk[c], d.u_lo, d.u_hi) == Uk[c]);
        h->r[c] = k.scale * rcpf_(Uk[c]);
    }
}

// A band lane's crossing from the f64 probe's radius rr (0: not probed, its
// node was never reached) and the f64 traveled angle (geo_band.h: r_in > 0, so
// the annulus test holds "probed" and "U > 0" too).
GEO_HD void disk_band_hit(const DiskConsts& d, float ak, float rr, double angle, bool* hit, float* r) {
    *hit = ((double)ak < angle) & (d.r_in <= rr) & (rr <= d.r_out);
    *r = rr;
}

// A band lane's pixel: lambda' in f64 (band_lambda's), its steps and crossings.
GEO_HD double disk_hits_band(const BandConsts& bk, const DiskConsts& d, const DiskRay& dr, uint32_t px, uint32_t py,
                             uint32_t* steps, DiskHits* h) {
    double angle;
    float r0, r1, r2;
    const float a0 = dr.ak[0];  // (a_k = fma(k, pi, a_0), disk_ray's own values)
    const double l = band_lambda_disk(bk, px, py, a0, dr.jn[0] != 0xFFFFFFFFu, steps, &angle, &r0, &r1, &r2);
    disk_band_hit(d, a0, r0, angle, &h->hit[0], &h->r[0]);
    disk_band_hit(d, fmaf_(1.0f, kPi, a0), r1, angle, &h->hit[1], &h->r[1]);
    disk_band_hit(d, fmaf_(2.0f, kPi, a0), r2, angle, &h->hit[2], &h->r[2]);
    return l;
}

// disk_shade_slot_ and its shaded forms on a crossing of DiskHits.
// colour(r, Ud, Vd, &g, &q): the hit's colour (the texture sample, shifted or
// turned into the emission's; g and q written where the render has them).
template <int S, typename Colour>
GEO_HD uint32_t disk_shade_hits_slot_(const DiskConsts& d, const DiskRay& dr, const DiskHits& h, uint32_t c,
                                      const Colour& colour, float* hits, float* gs, float* qs) {
    float r = 0.0f, Ud = 0.0f, g = 0.0f, q = 0.0f;
    if (h.hit[S]) {
        r = h.r[S];
        const float sg = (S & 1) ? -1.0f : 1.0f;
        const float sa = sg * dr.sa, ca = sg * dr.ca;
        const float X = fmaf_(sa, fmaf_(d.ex[0], dr.cphi, d.ex[1] * dr.sphi), ca * d.ex[2]);
        const float Y = fmaf_(sa, fmaf_(d.ey[0], dr.cphi, d.ey[1] * dr.sphi), ca * d.ey[2]);
        Ud = med3_(atan2_turns_(Y, X), 0.0f, 1.0f);
        const float Vd = med3_((r - d.r_in) * d.inv_dr, 0.0f, 1.0f);
        c = composite_(colour(r, Ud, Vd, &g, &q), c);
    }
    if (hits) {
        hits[2 * S] = r;
        hits[2 * S + 1] = Ud;
    }
    if (gs) gs[S] = g;
    if (qs) qs[S] = q;
    return c;
}

template <typename Colour>
GEO_HD uint32_t disk_shade_hits(const DiskConsts& d, const DiskRay& dr, const DiskHits& h, uint32_t base,
                                const Colour& colour, float* hits, float* gs, float* qs) {
    static_assert(kDiskMaxCrossings == 3, "three slots, written out");
    uint32_t c = base;
    c = disk_shade_hits_slot_<2>(d, dr, h, c, colour, hits, gs, qs);
    c = disk_shade_hits_slot_<1>(d, dr, h, c, colour, hits, gs, qs);
    c = disk_shade_hits_slot_<0>(d, dr, h, c, colour, hits, gs, qs);
    return c;
}

// The three renders' colours for disk_shade_hits.
template <typename Sample>
GEO_HD auto disk_colour_plain(const Sample& sample) {
    return [&sample](float, float Ud, float Vd, float*, float*) { return sample(Ud, Vd); };
}
template <typename Sample>
GEO_HD auto disk_colour_shift(const PixelConsts& k, const DiskShift& sh, const DiskShiftRay& sr, const Sample& sample) {
    return [&k, &sh, &sr, &sample](float r, float Ud, float Vd, float* g, float*) {
        *g = disk_shift_g(k, sr, r);
        return disk_shift_colour(sh, *g, sample(Ud, Vd));
    };
}
template <typename Sample, typename Fetch>
GEO_HD auto disk_colour_emit(const DiskConsts& d, const PixelConsts& k, const DiskEmission& em, const DiskShiftRay& sr,
                             const Sample& sample, const Fetch& fetch) {
    return [&d, &k, &em, &sr, &sample, &fetch](float r, float Ud, float Vd, float* g, float* q) {
        *g = disk_shift_g(k, sr, r);
        *q = disk_emission_q(d, em, *g, r);
        return disk_emission_colour(em, *q, sample(Ud, Vd), fetch);
    };
}

// ---- The disk in GEO_MODE_ADAPTIVE (geo_render_disk_adaptive) -------------
// geodesic_angle_adaptive (geo_pixel.h) with the crossing probes.  The traveled
// angle and *steps (attempts) are geodesic_angle_adaptive's, bit for bit, for
// every ray: the set-up, the step control, the wave-uniform `live` loop with
// its single exit edge, the stop test and the Newton finish are its own.  The
// f32 specification of the probes:
//   * the crossings a_k = fma(k, pi, a_0), k < 3, are disk_ray's; its nodes jn
//     and partial steps dn belong to the fixed grid and are not read, except
//     that "no crossing" is still jn[0] == 0xFFFFFFFF
//   * the loop's accepted steps tile the angle axis with its own f32 values:
//     an accepted attempt goes from ang to ang' = ang + h, the f32 sum the
//     loop forms
//   * crossing k is probed in the one accepted attempt with ang <= a_k < ang',
//     and only while the lane is still in `live` at that attempt (the lane's
//     stopping attempt counts): no probe in a rejected attempt, none after
//     the lane has left `live`, none when geodesic_init ends the ray before
//     the loop
//   * the probe is U of dp5_step<KIND>(U, V, d, d d), d = a_k - ang (an f32
//     subtract), from the attempt's start state: the form the Newton finish
//     uses for an arbitrary step length
//   * hmax = 16 step can exceed pi (step 0.3: 4.8), so one accepted step can
//     hold two or three crossings: the arm loops while (a_next < ang')
//   * an unprobed crossing has U = 0 (never in [u_lo, u_hi]: u_lo > 0)
//   * a probed crossing is a hit when a_k < the returned traveled angle
//     (kNoValue = 15 > a_2 when the ray never crosses the sphere) and
//     u_lo <= U <= u_hi; r, Ud, Vd, the shift and the emission are disk_hit's
//     and the sections' above on that r.
// Per attempt the disk costs one compare (the lane's next crossing against
// ang') and one ballot; the probe sits in a rarely taken arm behind it.  The
// cursor is scalars and selects (a per-lane indexed array would go to scratch).

// disk_ray for the adaptive loop: the same crossings; disk_hit's node test
// `jn[c] < steps` then reads "the ray has a crossing and the loop ran" (jn = 0
// against steps >= 1 attempts; a ray ended by geodesic_init has steps = 0 and
// no probe).
GEO_HD void disk_ray_adaptive(const DiskConsts& d, const PixelConsts& k, float c2x, float c2y, float rho, float rrho,
                              DiskRay* r) {
    disk_ray(d, k, c2x, c2y, rho, rrho, r);
    const uint32_t j = r->jn[0] == 0xFFFFFFFFu ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int c = 0; c < kDiskMaxCrossings; ++c) {
        r->jn[c] = j;
        r->dn[c] = 0.0f;
    }
}

template <int KIND>
GEO_HD float geodesic_angle_adaptive_disk(const PixelConsts& k, float st, float ct, float rct, const DiskRay& dr,
                                          uint32_t* steps, float (&Uk)[kDiskMaxCrossings]) {
    *steps = 0;
#pragma unroll
    for (int c = 0; c < kDiskMaxCrossings; ++c) Uk[c] = 0.0f;
    float U, V, early;
    if (!geodesic_init<KIND>(k, st, ct, rct, &early, &U, &V)) return early;
    const StopTest<KIND> stop_at(k);
    const uint32_t ms = k.max_steps;
    float h = k.step, ang = 0.0f;
    float sU, sV, sh, sang, sNU, sNV;
    GEO_UNSET(sU);
    GEO_UNSET(sV);
    GEO_UNSET(sh);
    GEO_UNSET(sang);
    GEO_UNSET(sNU);
    GEO_UNSET(sNV);
    // the lane's next crossing: slot kc at angle at (+inf: none left)
    const float none = __builtin_inff();
    uint32_t kc = 0;
    float at = dr.jn[0] != 0xFFFFFFFFu ? dr.ak[0] : none;
    float u0 = 0.0f, u1 = 0.0f, u2 = 0.0f;
    uint32_t it = 0;
    uint64_t live = ballot_(true);
    for (uint32_t n = 1; n <= ms; ++n) {
        float NU, NV, SE;
        const float hh = h * h;
        dp5_step<KIND>(U, V, h, hh, &NU, &NV, &SE);
        const float err = __builtin_fabsf(SE) * hh;
        const bool acc = !(err > k.tolU);
        const uint64_t accm = ballot_(acc);
        const float angn = ang + h;
        // (the lanes of `live` as the attempt finds it: the stopping attempt probes)
        const uint64_t due = ballot_(at < angn) & accm & live;
        if (due != 0) {
            if (in_ballot_(due)) {
                GEO_RARE();
                do {
                    const float dl = at - ang;
                    float wu, wv, se;
                    dp5_step<KIND>(U, V, dl, dl * dl, &wu, &wv, &se);
                    u0 = kc == 0u ? wu : u0;
                    u1 = kc == 1u ? wu : u1;
                    u2 = kc == 2u ? wu : u2;
                    ++kc;
                    at = kc == 1u ? dr.ak[1] : (kc == 2u ? dr.ak[2] : none);
                } while (at < angn);
            }
        }
        uint64_t hit = accm & stop_at.out_mask(NU) & live;
        if (hit != 0) hit &= stop_at.exact_refine(NU, NV);
        if (hit != 0) {
            if (in_ballot_(hit)) {
                GEO_RARE();
                sU = U;
                sV = V;
                sh = h;
                sang = ang;
                sNU = NU;
                sNV = NV;
                it = n;
            }
            live &= ~hit;
            n = live == 0 ? ms : n;
        }
        const float grow = (err < k.tolG && h < k.hmax) ? 2.0f : 1.0f;
        U = acc ? NU : U;
        V = acc ? NV : V;
        ang = acc ? angn : ang;
        h = h * (acc ? grow : 0.5f);
    }
    Uk[0] = u0;
    Uk[1] = u1;
    Uk[2] = u2;
    *steps = it != 0 ? it : ms;
    if (it == 0 || (sNU > k.SU) == (sU > k.SU)) return kNoValue;
    float ns, wu, wv;
    if (__builtin_fabsf(sV) > __builtin_fabsf(sNV)) {
        ns = 0.0f; wu = sU; wv = sV;
    } else {
        ns = sh; wu = sNU; wv = sNV;
    }
    for (int n = 0; n < kNewtonIters; ++n) {
        ns = ns - divf_(wu - k.SU, wv);
        float se;
        dp5_step<KIND>(sU, sV, ns, ns * ns, &wu, &wv, &se);
    }
    return sang + ns;
}

}  // namespace geo
