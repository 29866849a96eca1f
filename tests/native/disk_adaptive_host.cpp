// Host build of geo_disk.h's adaptive probe loop (geodesic_angle_adaptive_disk)
// against the probe rule of its section written out here as plainly as it
// goes: one scalar ray, a per-ray break, dp5_step called directly, no crossing
// cursor, no ballots, no `live` mask.  Test-only (tests/test_disk_adaptive_cpu.py).
//
// The definition, after geodesic_init<KIND>: attempts n = 1 .. max_steps of
// dp5_step from (U, V) with step h; an attempt whose error |SE| h^2 exceeds
// tolU is rejected (h halves, nothing else happens); an accepted attempt goes
// from ang to ang' = ang + h, and every crossing a_c with ang <= a_c < ang'
// takes U_c = dp5_step(U, V, a_c - ang) from the attempt's start state; the ray
// stops after the first accepted attempt whose end state StopTest<KIND>::exact
// flags; otherwise h doubles below tolU / 64 (up to hmax) and the state moves on.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../schwarzschild_raytracer_wgpu_amd/csrc/geo_disk.h"

namespace {

constexpr int C = geo::kDiskMaxCrossings;

uint32_t bits(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

// equal bits, or both NaN
bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }

// The disk and the rays of a sweep frame: disk_probe_host.cpp's (identity
// central_to_uv, the annulus 2 rs .. 0.8 sphere_r, or 2 .. 0.8 sphere_r in
// flat space; theta_i = (-1/2 + (i + 1/2) / n_theta) pi, phi_j = 2 pi j / n_phi).
bool make_disk(const geo::PixelConsts& k, const float* n, geo::DiskConsts* d) {
    const float m2[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const bool along_x = n[1] == 0.0f && n[2] == 0.0f;
    const float ax[3] = {along_x ? 0.0f : 1.0f, along_x ? 1.0f : 0.0f, 0.0f};
    return geo::disk_consts(m2, n, ax, 2.0f * (k.rs > 0.0f ? k.rs : 1.0f), 0.8f * k.sphere_r, k, d);
}

struct Ray {
    float c2x, c2y, st, ct, rct;
};
Ray ray_of(uint32_t i, uint32_t n_theta, uint32_t jp, uint32_t n_phi) {
    const float theta = (-0.5f + ((float)i + 0.5f) / (float)n_theta) * geo::kPi;
    const float phi = 2.0f * geo::kPi * (float)jp / (float)n_phi;
    Ray y;
    y.c2x = std::cos(theta) * std::cos(phi);
    y.c2y = std::cos(theta) * std::sin(phi);
    y.st = geo::central_sin(std::sin(theta));
    y.ct = geo::central_rho(y.c2x, y.c2y);
    y.rct = geo::rcpf_(y.ct);
    return y;
}

// What the definition reports about one ray beside its U values.
struct Defined {
    float angle;
    uint32_t steps;
    bool done[C];       // crossing c was probed
    bool at_stop[C];    // ... in the ray's stopping attempt
    bool after_rej[C];  // ... after a rejected attempt whose span held it
    uint32_t multi;     // accepted attempts that probed two or more crossings
    bool exhausted;     // the loop ran and the budget ended it
};

template <int KIND>
void define_probes(const geo::PixelConsts& k, float st, float ct, float rct, const float* ak, bool crosses, float* Uc,
                   Defined* o) {
    for (int c = 0; c < C; ++c) {
        Uc[c] = 0.0f;
        o->done[c] = o->at_stop[c] = o->after_rej[c] = false;
    }
    o->multi = 0;
    o->exhausted = false;
    o->steps = 0;
    float U, V, early;
    if (!geo::geodesic_init<KIND>(k, st, ct, rct, &early, &U, &V)) {
        o->angle = early;
        return;
    }
    const geo::StopTest<KIND> stop_at(k);
    float h = k.step, ang = 0.0f;
    bool rej[C] = {false, false, false};
    for (uint32_t n = 1; n <= k.max_steps; ++n) {
        float NU, NV, SE;
        const float hh = h * h;
        geo::dp5_step<KIND>(U, V, h, hh, &NU, &NV, &SE);
        const float err = std::fabs(SE) * hh;
        const float angn = ang + h;
        if (err > k.tolU) {  // rejected
            for (int c = 0; c < C; ++c)
                if (crosses && ang <= ak[c] && ak[c] < angn) rej[c] = true;
            h = h * 0.5f;
            continue;
        }
        uint32_t here = 0;
        bool now[C] = {false, false, false};
        for (int c = 0; c < C; ++c)
            if (crosses && ang <= ak[c] && ak[c] < angn) {
                const float d = ak[c] - ang;
                float wv, se;
                geo::dp5_step<KIND>(U, V, d, d * d, &Uc[c], &wv, &se);
                o->done[c] = now[c] = true;
                o->after_rej[c] = rej[c];
                ++here;
            }
        if (here >= 2u) ++o->multi;
        if (stop_at.exact(NU, NV)) {
            for (int c = 0; c < C; ++c) o->at_stop[c] = now[c];
            o->steps = n;
            if ((NU > k.SU) == (U > k.SU)) {
                o->angle = geo::kNoValue;
                return;
            }
            // Newton on the step length from the steeper end
            float ns, wu, wv;
            if (std::fabs(V) > std::fabs(NV)) {
                ns = 0.0f; wu = U; wv = V;
            } else {
                ns = h; wu = NU; wv = NV;
            }
            for (int i = 0; i < geo::kNewtonIters; ++i) {
                ns = ns - geo::divf_(wu - k.SU, wv);
                float se;
                geo::dp5_step<KIND>(U, V, ns, ns * ns, &wu, &wv, &se);
            }
            o->angle = ang + ns;
            return;
        }
        const float grow = (err < k.tolG && h < k.hmax) ? 2.0f : 1.0f;
        U = NU;
        V = NV;
        ang = angn;
        h = h * grow;
    }
    o->steps = k.max_steps;
    o->exhausted = true;
    o->angle = geo::kNoValue;
}

// counters of one sweep (disk_adaptive_sweep's out[])
enum {
    kLanes,       // lanes run
    kMismatch,    // lanes with any difference
    kFirst,       // index of the first such lane (~0: none)
    kWhat,        // which assertion the first such lane failed (bits below)
    kCompared,    // probes compared (the definition probed the crossing)
    kAtStop,      // ... in the lane's stopping attempt
    kMulti,       // accepted attempts holding two or more crossings
    kAfterRej,    // probes of a crossing that a rejected attempt's span held before
    kExhausted,   // lanes whose loop the budget ended
    kNoCrossing,  // lanes with no crossing
    kAccepted,    // probes that are hits (by the definition's side)
    kStopped,     // lanes that stopped before the budget
    kKind0, kKind1, kKind2,  // lanes per integration kind
    kCounters
};
enum { kBadAngle = 1, kBadSteps = 2, kBadDef = 4, kBadU = 8, kBadHit = 16 };

template <int KIND>
uint32_t run_lane(const geo::PixelConsts& k, const geo::DiskConsts& d, const Ray& y, unsigned long long* n) {
    uint32_t bad = 0;
    geo::DiskRay dr;
    geo::disk_ray_adaptive(d, k, y.c2x, y.c2y, y.ct, y.rct, &dr);
    // the crossings by disk_ray itself (the definition takes nothing from disk_ray_adaptive)
    geo::DiskRay d0;
    geo::disk_ray(d, k, y.c2x, y.c2y, y.ct, y.rct, &d0);
    const bool crosses = d0.jn[0] != 0xFFFFFFFFu;
    // the code under test, and the plain loop it promises to follow
    uint32_t sd = 0, sv = 0;
    float Uk[C];
    const float ad = geo::geodesic_angle_adaptive_disk<KIND>(k, y.st, y.ct, y.rct, dr, &sd, Uk);
    const float av = geo::geodesic_angle_adaptive<KIND>(k, y.st, y.ct, y.rct, &sv);
    if (!same(ad, av)) bad |= kBadAngle;
    if (sd != sv) bad |= kBadSteps;
    // the definition
    float Ud[C];
    Defined o;
    define_probes<KIND>(k, y.st, y.ct, y.rct, d0.ak, crosses, Ud, &o);
    if (o.steps != sd || !same(o.angle, ad)) bad |= kBadDef;
    for (int c = 0; c < C; ++c) {
        if (!same(Uk[c], Ud[c])) bad |= kBadU;
        if (o.done[c]) {
            ++n[kCompared];
            if (o.at_stop[c]) ++n[kAtStop];
            if (o.after_rej[c]) ++n[kAfterRej];
        }
        // the verdicts: disk_hit on the code's values, the rule's words on the definition's
        float r0 = 0, u0 = 0, v0 = 0;
        const bool h0 = geo::disk_hit(d, k, dr, c, Uk[c], sd, ad, &r0, &u0, &v0);
        const bool h1 = o.done[c] && d0.ak[c] < o.angle && d.u_lo <= Ud[c] && Ud[c] <= d.u_hi;
        if (h0 != h1) bad |= kBadHit;
        if (h1) {
            ++n[kAccepted];
            if (!same(r0, k.scale * geo::rcpf_(Ud[c]))) bad |= kBadHit;
        }
    }
    n[kMulti] += o.multi;
    if (o.exhausted) ++n[kExhausted];
    if (!crosses) ++n[kNoCrossing];
    if (o.steps != 0 && !o.exhausted) ++n[kStopped];
    ++n[kKind0 + KIND];
    ++n[kLanes];
    return bad;
}

uint32_t run_kind(const geo::PixelConsts& k, const geo::DiskConsts& d, const Ray& y, unsigned long long* n) {
    switch (k.kind) {
        case geo::kCurvedOut: return run_lane<geo::kCurvedOut>(k, d, y, n);
        case geo::kCurvedIn: return run_lane<geo::kCurvedIn>(k, d, y, n);
        default: return run_lane<geo::kFlat>(k, d, y, n);
    }
}

}  // namespace

extern "C" uint32_t disk_adaptive_counters(void) { return kCounters; }

// One lane, for a failing index's message: out[0..1] = angle bits of the code
// and of the definition, out[2..3] = their steps, out[4..6] = Uk bits,
// out[7..9] = the definition's U bits, out[10] = kind, out[11] = steps of
// geodesic_angle_adaptive.
extern "C" int disk_adaptive_lane(float rs, float sphere_r, float r_obs, float step, uint32_t max_steps, float tol,
                                  const float* normal, uint32_t i, uint32_t n_theta, uint32_t jp, uint32_t n_phi,
                                  uint32_t* out) {
    const geo::PixelConsts k = geo::make_consts(rs, sphere_r, r_obs, step, max_steps, tol);
    geo::DiskConsts d;
    if (!make_disk(k, normal, &d)) return -1;
    const Ray y = ray_of(i, n_theta, jp, n_phi);
    geo::DiskRay dr;
    geo::disk_ray_adaptive(d, k, y.c2x, y.c2y, y.ct, y.rct, &dr);
    const bool crosses = dr.jn[0] != 0xFFFFFFFFu;
    float Uk[C], Ud[C];
    Defined o;
    uint32_t sd = 0, sv = 0;
    float ad;
    switch (k.kind) {
        case geo::kCurvedOut:
            ad = geo::geodesic_angle_adaptive_disk<geo::kCurvedOut>(k, y.st, y.ct, y.rct, dr, &sd, Uk);
            geo::geodesic_angle_adaptive<geo::kCurvedOut>(k, y.st, y.ct, y.rct, &sv);
            define_probes<geo::kCurvedOut>(k, y.st, y.ct, y.rct, dr.ak, crosses, Ud, &o);
            break;
        case geo::kCurvedIn:
            ad = geo::geodesic_angle_adaptive_disk<geo::kCurvedIn>(k, y.st, y.ct, y.rct, dr, &sd, Uk);
            geo::geodesic_angle_adaptive<geo::kCurvedIn>(k, y.st, y.ct, y.rct, &sv);
            define_probes<geo::kCurvedIn>(k, y.st, y.ct, y.rct, dr.ak, crosses, Ud, &o);
            break;
        default:
            ad = geo::geodesic_angle_adaptive_disk<geo::kFlat>(k, y.st, y.ct, y.rct, dr, &sd, Uk);
            geo::geodesic_angle_adaptive<geo::kFlat>(k, y.st, y.ct, y.rct, &sv);
            define_probes<geo::kFlat>(k, y.st, y.ct, y.rct, dr.ak, crosses, Ud, &o);
    }
    out[0] = bits(ad);
    out[1] = bits(o.angle);
    out[2] = sd;
    out[3] = o.steps;
    for (int c = 0; c < C; ++c) {
        out[4 + c] = bits(Uk[c]);
        out[7 + c] = bits(Ud[c]);
    }
    out[10] = (uint32_t)k.kind;
    out[11] = sv;
    return 0;
}

// The sweep: scenes x steps x tols x budgets x normals x (n_theta x n_phi
// rays), the lane index in that order.  scenes: n_scenes x (rs, sphere_r,
// r_obs); normals: n_normals x 3.  out: the counters above.
extern "C" int disk_adaptive_sweep(const float* scenes, uint32_t n_scenes, const float* steps, uint32_t n_steps,
                                   const float* tols, uint32_t n_tols, const uint32_t* budgets, uint32_t n_budgets,
                                   const float* normals, uint32_t n_normals, uint32_t n_theta, uint32_t n_phi,
                                   uint32_t threads, unsigned long long* out) {
    if (threads == 0 || threads > 16) return -1;
    const unsigned long long frames = (unsigned long long)n_scenes * n_steps * n_tols * n_budgets * n_normals;
    const unsigned long long per = (unsigned long long)n_theta * n_phi;
    std::atomic<int> rc{0};
    struct Part {
        unsigned long long n[kCounters];
        unsigned long long first;
        uint32_t what;
    };
    std::vector<Part> part(threads);
    auto work = [&](uint32_t t) {
        Part& L = part[t];
        std::memset(&L, 0, sizeof L);
        L.first = ~0ull;
        for (unsigned long long f = t; f < frames; f += threads) {
            unsigned long long q = f;
            const uint32_t in = (uint32_t)(q % n_normals); q /= n_normals;
            const uint32_t ib = (uint32_t)(q % n_budgets); q /= n_budgets;
            const uint32_t it = (uint32_t)(q % n_tols); q /= n_tols;
            const uint32_t ih = (uint32_t)(q % n_steps); q /= n_steps;
            const uint32_t is = (uint32_t)q;
            const geo::PixelConsts k = geo::make_consts(scenes[3 * is], scenes[3 * is + 1], scenes[3 * is + 2],
                                                        steps[ih], budgets[ib], tols[it]);
            geo::DiskConsts d;
            if (!make_disk(k, normals + 3 * in, &d)) {
                rc = -2;
                return;
            }
            for (uint32_t i = 0; i < n_theta; ++i)
                for (uint32_t jp = 0; jp < n_phi; ++jp) {
                    const uint32_t bad = run_kind(k, d, ray_of(i, n_theta, jp, n_phi), L.n);
                    if (bad) {
                        ++L.n[kMismatch];
                        const unsigned long long idx = f * per + (unsigned long long)i * n_phi + jp;
                        if (idx < L.first) {
                            L.first = idx;
                            L.what = bad;
                        }
                    }
                }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t) pool.emplace_back(work, t);
    for (auto& th : pool) th.join();
    if (rc != 0) return rc;
    for (uint32_t i = 0; i < kCounters; ++i) out[i] = 0;
    out[kFirst] = ~0ull;
    for (uint32_t t = 0; t < threads; ++t) {
        for (uint32_t i = 0; i < kCounters; ++i)
            if (i != kFirst && i != kWhat) out[i] += part[t].n[i];
        if (part[t].first < out[kFirst]) {
            out[kFirst] = part[t].first;
            out[kWhat] = part[t].what;
        }
    }
    return 0;
}
