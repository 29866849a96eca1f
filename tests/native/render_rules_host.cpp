// Host build of geo_render_rules.h: a described render call goes through the
// entry point's argument stage, check_scene, check_frames and choose_launcher
// exactly as geo_render.hip's render_impl runs them, with no device and no
// context.  Test-only (tests/test_render_rules_host.py); with
// -DRENDER_RULES_MAIN a stand-alone program over a file of cases (the
// sanitizer run).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static std::atomic<uint64_t> g_rule_hits[64];
#define GEO_RULE(n) ((void)g_rule_hits[n].fetch_add(1, std::memory_order_relaxed))
#include "../../schwarzschild_raytracer_wgpu_amd/csrc/geo_render_rules.h"

static_assert(kRuleReturns <= 64, "a counter per return");

// One described call; every field 4 bytes (tests/render_rules_cases.py: CASE).
struct RuleCase {
    uint32_t entry;        // Entry
    uint32_t nframes;      // the batched entry points'
    uint32_t alt_frame;    // this frame's scene is scene[1]; every other frame's scene[0] (per-frame scenes)
    uint32_t nulls;        // null arguments: 1 the context, 2 the frames, 4 the scene(s), 8 out_rgba8
    uint32_t side;         // side outputs (one-frame entry points): 1 out_mask, 2 out_uv, 4 out_steps
    uint32_t armed;        // armed per-pixel buffers: 1 hits, 2 g, 4 q
    uint32_t steps_total;  // != 0: given
    uint32_t width, height;
    uint32_t g[4];         // the entry point's own four row arguments, in its order
    uint32_t out_frame_stride;
    uint32_t sky, n_fan, disk_set, shift_set, emit_set, disk_ring;  // RuleState
    float r_in, r_out;
    geo_scene scene[2];
};
static_assert(sizeof(RuleCase) == 22 * 4 + 2 * sizeof(geo_scene), "packed");

static int run_case(const RuleCase& k, int* launcher) {
    static int here;  // any non-null address: the rules read no pointer's target but the scenes'
    void* const p = &here;
    *launcher = 255;
    geo_scene scenes[kRuleMaxFrames];
    for (uint32_t i = 0; i < kRuleMaxFrames; ++i) scenes[i] = k.scene[i == k.alt_frame ? 1 : 0];
    static const geo_frame frames[kRuleMaxFrames] = {};
    const void* c = (k.nulls & 1u) ? nullptr : p;
    const geo_frame* fr = (k.nulls & 2u) ? nullptr : frames;
    const geo_scene* sc = (k.nulls & 4u) ? nullptr : scenes;
    uint8_t* out = (k.nulls & 8u) ? nullptr : (uint8_t*)p;
    unsigned long long* total = k.steps_total ? (unsigned long long*)p : nullptr;
    if (k.entry >= (uint32_t)kEntries) return -100;
    const Entry e = (Entry)k.entry;
    RenderCall rc;
    const bool ok =
        e <= Entry::kDiskAdaptive
            ? frame_call(rc, e, c, fr, sc, k.width, k.height, k.g[0], k.g[1], k.g[2], k.g[3], out,
                         (k.side & 1u) ? (uint8_t*)p : nullptr, (k.side & 2u) ? (float*)p : nullptr,
                         (k.side & 4u) ? (uint32_t*)p : nullptr, total, nullptr)
            : batch_call(rc, e, c, fr, sc, k.nframes, k.width, k.height, k.g[0], k.g[1], k.g[2], k.g[3], out,
                         k.out_frame_stride, total, nullptr);
    if (!ok) return GEO_EINVAL;
    RuleState s;
    s.sky = k.sky != 0;
    s.n_fan = k.n_fan;
    s.disk_set = k.disk_set != 0;
    s.shift_set = k.shift_set != 0;
    s.emit_set = k.emit_set != 0;
    s.disk_ring = k.disk_ring != 0;
    s.r_in = k.r_in;
    s.r_out = k.r_out;
    RenderRules w;
    w.out_hits = (k.armed & 1u) ? (float*)p : nullptr;
    w.out_g = (k.armed & 2u) ? (float*)p : nullptr;
    w.out_q = (k.armed & 4u) ? (float*)p : nullptr;
    int st = check_scene(s, rc, w);
    if (st) return st;
    geo::PixelConsts pk[kRuleMaxFrames];
    if ((st = check_frames(rc, w, pk))) return st;
    *launcher = (int)choose_launcher(rc, w);
    return GEO_OK;
}

extern "C" {

uint32_t render_rules_case_bytes(void) { return sizeof(RuleCase); }
uint32_t render_rules_returns(void) { return kRuleReturns; }

// status[i] and launcher[i] (255 unless GEO_OK) of cases[i]
int render_rules_run(const RuleCase* cases, uint64_t n, int8_t* status, uint8_t* launcher) {
    for (uint64_t i = 0; i < n; ++i) {
        int l;
        status[i] = (int8_t)run_case(cases[i], &l);
        launcher[i] = (uint8_t)l;
    }
    return 0;
}

// how often each return of the rules has been taken since the library was loaded
void render_rules_hits(uint64_t* out) {
    for (int i = 0; i < kRuleReturns; ++i) out[i] = g_rule_hits[i].load();
}

}  // extern "C"

#if defined(RENDER_RULES_MAIN)
// render_rules_host CASES [EXPECTED]: the cases of a raw RuleCase file; with
// EXPECTED (one status byte and one launcher byte per case, statuses first)
// compared, else summed.
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<RuleCase> cases;
    RuleCase k;
    while (std::fread(&k, sizeof(k), 1, f) == 1) cases.push_back(k);
    std::fclose(f);
    const size_t n = cases.size();
    std::vector<int8_t> status(n);
    std::vector<uint8_t> launcher(n);
    render_rules_run(cases.data(), n, status.data(), launcher.data());
    uint64_t ok = 0, einval = 0, estate = 0;
    for (size_t i = 0; i < n; ++i) (status[i] == GEO_OK ? ok : status[i] == GEO_ESTATE ? estate : einval) += 1;
    std::printf("%zu cases: %llu GEO_OK, %llu GEO_ESTATE, %llu GEO_EINVAL\n", n, (unsigned long long)ok,
                (unsigned long long)estate, (unsigned long long)einval);
    if (argc > 2) {
        std::vector<uint8_t> want(2 * n);
        FILE* e = std::fopen(argv[2], "rb");
        if (!e || std::fread(want.data(), 1, 2 * n, e) != 2 * n) return 2;
        std::fclose(e);
        for (size_t i = 0; i < n; ++i)
            if ((uint8_t)status[i] != want[i] || launcher[i] != want[n + i]) {
                std::printf("case %zu differs\n", i);
                return 1;
            }
        std::printf("equal to the expected matrix\n");
    }
    for (int i = 0; i < kRuleReturns; ++i)
        if (g_rule_hits[i].load() == 0) {
            std::printf("return %d never taken\n", i);
            return 1;
        }
    return 0;
}
#endif
