// Host build of geo_pixel.h's group loop with the exit test forced: the
// exact test of kTestLow frames against the end-state test (kTestEnd), and
// the loop the selector of make_consts picks, from chosen initial states
// (U0 of the scene, UB0 given).  Test-only (tests/test_exit_test_host.py).
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../schwarzschild_raytracer_wgpu_amd/csrc/geo_pixel.h"

namespace {

uint32_t bits(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

template <int FORCE>
float run(const geo::PixelConsts& k, float ub, uint32_t* n) {
    *n = 0;
    if (k.kind == geo::kCurvedOut) return geo::geodesic_run_<geo::kCurvedOut, geo::kGroup, FORCE>(k, k.U0, ub, n);
    return geo::geodesic_run_<geo::kFlat, geo::kGroup, FORCE>(k, k.U0, ub, n);
}

// the selector's verdict for one lane, as geodesic_run_ evaluates it
bool lane_inside(const geo::PixelConsts& k, float ub) {
    return (k.stop_bits & 8u) != 0 && geo::med3_(ub, k.end_lo, k.end_hi) == ub;
}

}  // namespace

// out[0..6] = stop_bits, kind, bits(end_lo), bits(end_hi), bits(stop_lo), bits(U0), bits(stop_hi)
extern "C" void exit_selector(float rs, float sphere_r, float r, float step, uint32_t max_steps, uint32_t* out) {
    const geo::PixelConsts k = geo::make_consts(rs, sphere_r, r, step, max_steps);
    out[0] = k.stop_bits;
    out[1] = (uint32_t)k.kind;
    out[2] = bits(k.end_lo);
    out[3] = bits(k.end_hi);
    out[4] = bits(k.stop_lo);
    out[5] = bits(k.U0);
    out[6] = bits(k.stop_hi);
}

// n lanes of one scene from (U0, ub[i]): angle bits and steps with kTestLow
// forced, kTestEnd forced and the selector's own choice; inside[i] = the
// selector admits the lane.  Returns -1 for a frame that is not a kTestLow one.
extern "C" int exit_compare(float rs, float sphere_r, float r, float step, uint32_t max_steps, const float* ub,
                            uint32_t n, uint32_t* ang_low, uint32_t* st_low, uint32_t* ang_end, uint32_t* st_end,
                            uint32_t* ang_auto, uint32_t* st_auto, uint8_t* inside) {
    const geo::PixelConsts k = geo::make_consts(rs, sphere_r, r, step, max_steps);
    if (k.kind == geo::kCurvedIn || !(k.stop_bits & 1u) || !(k.stop_bits & 4u)) return -1;
    for (uint32_t i = 0; i < n; ++i) {
        ang_low[i] = bits(run<geo::kTestLow>(k, ub[i], &st_low[i]));
        ang_end[i] = bits(run<geo::kTestEnd>(k, ub[i], &st_end[i]));
        ang_auto[i] = bits(run<-1>(k, ub[i], &st_auto[i]));
        inside[i] = lane_inside(k, ub[i]) ? 1 : 0;
    }
    return 0;
}

// Dense sweep: n_h steps spread geometrically over [h_lo, h_hi] times n_ub
// values of UB0 per step, half of them spread geometrically in magnitude over
// [ub_min, B(h)] with a negative sign (outgoing) and half over [ub_min,
// ub_fall] with a positive one (falling), each jittered by a hash of its
// index.  Pairs the selector refuses are skipped.  out[0] = pairs compared,
// out[1] = pairs that differ, out[2] = pairs that stopped before the budget,
// out[3] = the index ih * n_ub + j of the first pair that differs.
extern "C" int exit_sweep(float rs, float sphere_r, float r, uint32_t max_steps, float h_lo, float h_hi,
                          uint32_t n_h, uint32_t n_ub, float ub_min, float ub_fall, uint32_t threads,
                          unsigned long long* out) {
    std::atomic<unsigned long long> compared{0}, differ{0}, stopped{0}, first{~0ull};
    auto work = [&](uint32_t t) {
        unsigned long long c = 0, d = 0, s = 0;
        for (uint32_t ih = t; ih < n_h; ih += threads) {
            const float fh = n_h > 1 ? (float)ih / (float)(n_h - 1) : 0.0f;
            const float h = h_lo * std::pow(h_hi / h_lo, fh);
            const geo::PixelConsts k = geo::make_consts(rs, sphere_r, r, h, max_steps);
            if (!(k.stop_bits & 8u)) continue;
            const float B = -k.end_lo;
            for (uint32_t j = 0; j < n_ub; ++j) {
                uint32_t x = (ih * 2654435761u) ^ (j * 40503u + 0x9E3779B9u);
                x ^= x << 13;
                x ^= x >> 17;
                x ^= x << 5;
                const float jit = (float)(x & 0xFFFFu) * (1.0f / 65536.0f);
                const bool fall = (j & 1u) != 0;
                const float top = fall ? ub_fall : B;
                if (!(top > ub_min)) continue;
                const float f = ((float)(j >> 1) + jit) / (float)((n_ub + 1) / 2);
                float ub = ub_min * std::pow(top / ub_min, f);
                if (ub > top) ub = top;
                if (!fall) ub = -ub;
                if (!lane_inside(k, ub)) continue;
                uint32_t n0, n1;
                const uint32_t a0 = bits(run<geo::kTestLow>(k, ub, &n0));
                const uint32_t a1 = bits(run<geo::kTestEnd>(k, ub, &n1));
                ++c;
                if (n0 < max_steps) ++s;
                if (a0 != a1 || n0 != n1) {
                    ++d;
                    unsigned long long idx = (unsigned long long)ih * n_ub + j, cur = first.load();
                    while (idx < cur && !first.compare_exchange_weak(cur, idx)) {
                    }
                }
            }
        }
        compared += c;
        differ += d;
        stopped += s;
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t) pool.emplace_back(work, t);
    for (auto& th : pool) th.join();
    out[0] = compared;
    out[1] = differ;
    out[2] = stopped;
    out[3] = first.load();
    return 0;
}
