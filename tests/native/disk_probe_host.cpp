// Host build of geo_disk.h's probe loop (geodesic_angle_disk) against a
// per-step definition of the probes written here: no groups, no ballots, no
// crossing cursor, no budget tail.  Test-only (tests/test_disk_probe_host.py).
//
// The definition, after geodesic_init<KIND>: for r = 0 .. max_steps - 1, every
// crossing c with jn[c] == r takes U_c = disk_partial_<KIND>(U, UB, dn[c]) from
// the state at node r; then one rk4_step with the frame's constants; the ray
// stops after the first step whose state StopTest<KIND> flags.
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

// The disk of a sweep frame: identity central_to_uv, the annulus 2 rs .. 0.8
// sphere_r (2 .. 0.8 sphere_r in flat space), azimuth 0 along x (along y for a
// normal along x).
bool make_disk(const geo::PixelConsts& k, const float* n, geo::DiskConsts* d) {
    const float m2[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const bool along_x = n[1] == 0.0f && n[2] == 0.0f;
    const float ax[3] = {along_x ? 0.0f : 1.0f, along_x ? 1.0f : 0.0f, 0.0f};
    return geo::disk_consts(m2, n, ax, 2.0f * (k.rs > 0.0f ? k.rs : 1.0f), 0.8f * k.sphere_r, k, d);
}

// Ray (i, jp) of a sweep frame: theta_i = (-1/2 + (i + 1/2) / n_theta) pi, the
// ray plane's azimuth phi_j = 2 pi j / n_phi (phi_0 = 0 exactly), and from the
// central-frame direction the render's own (sin theta, cos theta, 1 / cos theta).
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

// The definition: U at each crossing whose node the ray reached (done[c]), and
// the executed steps.
template <int KIND>
uint32_t define_probes(const geo::PixelConsts& k, float st, float ct, float rct, const geo::DiskRay& dr, float* Uc,
                       bool* done) {
    for (int c = 0; c < C; ++c) {
        Uc[c] = 0.0f;
        done[c] = false;
    }
    float U, UB, early;
    if (!geo::geodesic_init<KIND>(k, st, ct, rct, &early, &U, &UB)) return 0;
    const geo::StopTest<KIND> stop_at(k);
    for (uint32_t r = 0; r < k.max_steps; ++r) {
        for (int c = 0; c < C; ++c)
            if (dr.jn[c] == r) {
                Uc[c] = geo::disk_partial_<KIND>(U, UB, dr.dn[c]);
                done[c] = true;
            }
        float nu, nub;
        geo::rk4_step<KIND>(U, UB, k.step, k.hh, k.hh2, k.hhh, k.h6, k.h2_6, &nu, &nub);
        U = nu;
        UB = nub;
        if (stop_at(nu, nub)) return r + 1u;
    }
    return k.max_steps;
}

// counters of one sweep (disk_probe_sweep's out[])
enum {
    kLanes,        // lanes run
    kMismatch,     // lanes with any difference
    kFirst,        // index of the first such lane (~0: none)
    kWhat,         // which assertion the first such lane failed (bit set below)
    kCompared,     // probes compared (jn[c] < steps)
    kTail,         // ... at a node >= (max_steps / 4) * 4
    kSameGroup,    // ... in a whole group of four that also holds the previous crossing
    kSameNode,     // ... at the previous crossing's node
    kRefused,      // crossings due in the lane's stopping group at a node >= steps
    kNoCrossing,   // lanes with jn[0] == 0xFFFFFFFF
    kEdgeOn,       // lanes with N[2] == 0
    kAccepted,     // probes disk_hit accepts (from the definition's U)
    kStoppedLanes, // lanes that stopped before the budget
    kKind0, kKind1, kKind2,  // lanes per integration kind
    kCounters
};
enum { kBadAngle = 1, kBadSteps = 2, kBadDefSteps = 4, kBadU = 8, kBadHit = 16 };

struct Lane {
    unsigned long long n[kCounters];
};

template <int KIND>
uint32_t run_lane(const geo::PixelConsts& k, const geo::DiskConsts& d, float st, float ct, float rct,
                  const geo::DiskRay& dr, unsigned long long* n) {
    uint32_t bad = 0;
    // the code under test, and the plain loop it promises to follow
    uint32_t sd = 0, sv = 0;
    float Uk[C];
    const float ad = geo::geodesic_angle_disk<KIND>(k, st, ct, rct, dr, &sd, Uk);
    const float av = geo::geodesic_angle_v<KIND>(k, st, ct, rct, &sv);
    if (!same(ad, av)) bad |= kBadAngle;
    if (sd != sv) bad |= kBadSteps;
    // the definition
    float Ud[C];
    bool done[C];
    const uint32_t steps = define_probes<KIND>(k, st, ct, rct, dr, Ud, done);
    if (steps != sd) bad |= kBadDefSteps;
    const uint32_t all = (k.max_steps / 4u) * 4u;
    for (int c = 0; c < C; ++c) {
        const uint32_t j = dr.jn[c];
        if (j < steps) {
            if (!done[c] || !same(Uk[c], Ud[c])) bad |= kBadU;
            ++n[kCompared];
            if (j >= all) ++n[kTail];
            if (c > 0 && dr.jn[c - 1] < steps) {
                if (j < all && dr.jn[c - 1] / 4u == j / 4u) ++n[kSameGroup];
                if (dr.jn[c - 1] == j) ++n[kSameNode];
            }
        } else if (steps != 0 && steps - 1u < all && j < ((steps - 1u) / 4u) * 4u + 4u) {
            ++n[kRefused];
        }
        // disk_hit from either U (the definition's side takes nothing from the code under test)
        float r0 = 0, u0 = 0, v0 = 0, r1 = 0, u1 = 0, v1 = 0;
        const bool h0 = geo::disk_hit(d, k, dr, c, Uk[c], sd, ad, &r0, &u0, &v0);
        const bool h1 = geo::disk_hit(d, k, dr, c, Ud[c], steps, av, &r1, &u1, &v1);
        if (h0 != h1 || (h1 && (!same(r0, r1) || !same(u0, u1) || !same(v0, v1)))) bad |= kBadHit;
        if (h1) ++n[kAccepted];
    }
    if (dr.jn[0] == 0xFFFFFFFFu) ++n[kNoCrossing];
    if (d.N[2] == 0.0f) ++n[kEdgeOn];
    if (steps != 0 && steps < k.max_steps) ++n[kStoppedLanes];
    ++n[kKind0 + KIND];
    ++n[kLanes];
    return bad;
}

}  // namespace

extern "C" uint32_t disk_probe_counters(void) { return kCounters; }

// One lane, for a failing index's message: out[0..2] = angle bits, steps of
// geodesic_angle_disk and of the definition; out[3..5] = jn; out[6..8] = Uk
// bits; out[9..11] = the definition's U bits; out[12] = kind.
extern "C" int disk_probe_lane(float rs, float sphere_r, float r_obs, float step, uint32_t max_steps,
                               const float* normal, uint32_t i, uint32_t n_theta, uint32_t jp, uint32_t n_phi,
                               uint32_t* out) {
    const geo::PixelConsts k = geo::make_consts(rs, sphere_r, r_obs, step, max_steps);
    geo::DiskConsts d;
    if (!make_disk(k, normal, &d)) return -1;
    const Ray y = ray_of(i, n_theta, jp, n_phi);
    const float st = y.st, ct = y.ct, rct = y.rct;
    geo::DiskRay dr;
    geo::disk_ray(d, k, y.c2x, y.c2y, ct, rct, &dr);
    float Uk[C], Ud[C];
    bool done[C];
    uint32_t sd = 0, steps = 0;
    float ad;
    switch (k.kind) {
        case geo::kCurvedOut:
            ad = geo::geodesic_angle_disk<geo::kCurvedOut>(k, st, ct, rct, dr, &sd, Uk);
            steps = define_probes<geo::kCurvedOut>(k, st, ct, rct, dr, Ud, done);
            break;
        case geo::kCurvedIn:
            ad = geo::geodesic_angle_disk<geo::kCurvedIn>(k, st, ct, rct, dr, &sd, Uk);
            steps = define_probes<geo::kCurvedIn>(k, st, ct, rct, dr, Ud, done);
            break;
        default:
            ad = geo::geodesic_angle_disk<geo::kFlat>(k, st, ct, rct, dr, &sd, Uk);
            steps = define_probes<geo::kFlat>(k, st, ct, rct, dr, Ud, done);
    }
    out[0] = bits(ad);
    out[1] = sd;
    out[2] = steps;
    for (int c = 0; c < C; ++c) {
        out[3 + c] = dr.jn[c];
        out[6 + c] = bits(Uk[c]);
        out[9 + c] = bits(Ud[c]);
    }
    out[12] = (uint32_t)k.kind;
    return 0;
}

// One pixel of a rendered frame, for a failing pixel's message
// (tests/test_gpu_disk_fuzz.py): frame = geo_frame's 52 floats (display_to_movement,
// movement_to_central, central_to_uv, psi_factor_and_position), disk = r_in,
// r_out, normal, axis.  out[0..2] = jn, out[3] = the definition's step count,
// out[4..6] = the definition's U bits, out[7] = kind.
extern "C" int disk_probe_pixel(const float* frame, float rs, float sphere_r, float r_obs, float step,
                                uint32_t max_steps, const float* disk, uint32_t width, uint32_t height, uint32_t px,
                                uint32_t py, uint32_t* out) {
    const float *m0 = frame, *m1 = frame + 16, *m2 = frame + 32, psi_k = frame[48];
    const geo::PixelConsts k = geo::make_consts(rs, sphere_r, r_obs, step, max_steps);
    geo::DiskConsts d;
    if (!geo::disk_consts(m2, disk + 2, disk + 5, disk[0], disk[1], k, &d)) return -1;
    const geo::CameraConsts cam = geo::camera_consts(m0, m1, width, height);
    float c2x, c2y, c2z;
    geo::pixel_central_dir(cam, m1, psi_k, geo::aberration_kt(psi_k), px, py, &c2x, &c2y, &c2z);
    const float st = geo::central_sin(c2z), ct = geo::central_rho(c2x, c2y), rct = geo::rcpf_(ct);
    geo::DiskRay dr;
    geo::disk_ray(d, k, c2x, c2y, ct, rct, &dr);
    float Ud[C];
    bool done[C];
    uint32_t steps;
    switch (k.kind) {
        case geo::kCurvedOut: steps = define_probes<geo::kCurvedOut>(k, st, ct, rct, dr, Ud, done); break;
        case geo::kCurvedIn: steps = define_probes<geo::kCurvedIn>(k, st, ct, rct, dr, Ud, done); break;
        default: steps = define_probes<geo::kFlat>(k, st, ct, rct, dr, Ud, done);
    }
    for (int c = 0; c < C; ++c) {
        out[c] = dr.jn[c];
        out[4 + c] = bits(Ud[c]);
    }
    out[3] = steps;
    out[7] = (uint32_t)k.kind;
    return 0;
}

// The crossings' nodes of every pixel of a rendered frame (disk_probe_pixel's
// arguments): jn[(y * width + x) * 3 + c].  No integration.
extern "C" int disk_probe_frame_nodes(const float* frame, float rs, float sphere_r, float r_obs, float step,
                                      uint32_t max_steps, const float* disk, uint32_t width, uint32_t height,
                                      uint32_t* jn) {
    const float *m0 = frame, *m1 = frame + 16, *m2 = frame + 32, psi_k = frame[48];
    const geo::PixelConsts k = geo::make_consts(rs, sphere_r, r_obs, step, max_steps);
    geo::DiskConsts d;
    if (!geo::disk_consts(m2, disk + 2, disk + 5, disk[0], disk[1], k, &d)) return -1;
    const geo::CameraConsts cam = geo::camera_consts(m0, m1, width, height);
    const float kt = geo::aberration_kt(psi_k);
    for (uint32_t py = 0; py < height; ++py)
        for (uint32_t px = 0; px < width; ++px) {
            float c2x, c2y, c2z;
            geo::pixel_central_dir(cam, m1, psi_k, kt, px, py, &c2x, &c2y, &c2z);
            const float ct = geo::central_rho(c2x, c2y);
            geo::DiskRay dr;
            geo::disk_ray(d, k, c2x, c2y, ct, geo::rcpf_(ct), &dr);
            for (int c = 0; c < C; ++c) jn[((size_t)py * width + px) * C + c] = dr.jn[c];
        }
    return 0;
}

// The sweep: scenes x steps x budgets x normals x (n_theta x n_phi rays), the
// lane index in that order.  scenes: n_scenes x (rs, sphere_r, r_obs); normals:
// n_normals x 3 (identity central_to_uv; the disk spans 2 rs .. 0.8 sphere_r,
// or 2 .. 0.8 sphere_r in flat space); the rays are ray_of's.  out: the
// counters above.
extern "C" int disk_probe_sweep(const float* scenes, uint32_t n_scenes, const float* steps, uint32_t n_steps,
                                const uint32_t* budgets, uint32_t n_budgets, const float* normals,
                                uint32_t n_normals, uint32_t n_theta, uint32_t n_phi, uint32_t threads,
                                unsigned long long* out) {
    if (threads == 0 || threads > 16) return -1;
    const unsigned long long frames = (unsigned long long)n_scenes * n_steps * n_budgets * n_normals;
    const unsigned long long per = (unsigned long long)n_theta * n_phi;
    std::atomic<int> rc{0};
    std::vector<Lane> part(threads);
    std::vector<uint32_t> what(threads, 0);
    std::vector<unsigned long long> mine(threads, ~0ull);
    auto work = [&](uint32_t t) {
        Lane& L = part[t];
        std::memset(&L, 0, sizeof L);
        for (unsigned long long f = t; f < frames; f += threads) {
            unsigned long long q = f;
            const uint32_t in = (uint32_t)(q % n_normals); q /= n_normals;
            const uint32_t ib = (uint32_t)(q % n_budgets); q /= n_budgets;
            const uint32_t ih = (uint32_t)(q % n_steps); q /= n_steps;
            const uint32_t is = (uint32_t)q;
            const float rs = scenes[3 * is], sphere_r = scenes[3 * is + 1], r_obs = scenes[3 * is + 2];
            const geo::PixelConsts k = geo::make_consts(rs, sphere_r, r_obs, steps[ih], budgets[ib]);
            const float* nv = normals + 3 * in;
            geo::DiskConsts d;
            if (!make_disk(k, nv, &d)) {
                rc = -2;
                return;
            }
            for (uint32_t i = 0; i < n_theta; ++i)
                for (uint32_t jp = 0; jp < n_phi; ++jp) {
                    const Ray y = ray_of(i, n_theta, jp, n_phi);
                    const float st = y.st, ct = y.ct, rct = y.rct;
                    geo::DiskRay dr;
                    geo::disk_ray(d, k, y.c2x, y.c2y, ct, rct, &dr);
                    uint32_t bad;
                    switch (k.kind) {
                        case geo::kCurvedOut: bad = run_lane<geo::kCurvedOut>(k, d, st, ct, rct, dr, L.n); break;
                        case geo::kCurvedIn: bad = run_lane<geo::kCurvedIn>(k, d, st, ct, rct, dr, L.n); break;
                        default: bad = run_lane<geo::kFlat>(k, d, st, ct, rct, dr, L.n);
                    }
                    if (bad) {
                        ++L.n[kMismatch];
                        const unsigned long long idx = f * per + (unsigned long long)i * n_phi + jp;
                        if (idx < mine[t]) {
                            mine[t] = idx;
                            what[t] = bad;
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
        if (mine[t] < out[kFirst]) {
            out[kFirst] = mine[t];
            out[kWhat] = what[t];
        }
    }
    return 0;
}
