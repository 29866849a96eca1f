// Host build of geo_render_rules.h for geo_render_disk_adaptive_ring_batch
// (Entry::kDiskAdaptiveRingBatch): a described call goes through batch_call,
// check_scene, check_frames and choose_launcher as geo_render.hip's
// render_impl runs them.  The records are render_rules_host.cpp's RuleCase
// (tests/render_rules_cases.py: CASE); that driver refuses every entry from
// kEntries on, so the batched entry appended after it has this driver.
// Test-only (tests/test_render_rules_adaptive_ring_batch_host.py).
#include <cstdint>

#include "../../schwarzschild_raytracer_wgpu_amd/csrc/geo_render_rules.h"

static_assert(kEntryRows == 13 && (int)Entry::kDiskAdaptiveRingBatch == 12,
              "appended: the committed matrix indexes 0..10, the one-frame adaptive ring entry is 11");
static_assert(kRuleReturns == 40, "the entry adds no return to the rules");

struct RuleCase {  // render_rules_host.cpp's, field for field
    uint32_t entry, nframes, alt_frame, nulls, side, armed, steps_total;
    uint32_t width, height;
    uint32_t g[4];
    uint32_t out_frame_stride;
    uint32_t sky, n_fan, disk_set, shift_set, emit_set, disk_ring;
    float r_in, r_out;
    geo_scene scene[2];
};
static_assert(sizeof(RuleCase) == 22 * 4 + 2 * sizeof(geo_scene), "packed");

static int run_case(const RuleCase& k, int* launcher) {
    static int here;  // any non-null address: the rules read no pointer's target but the scenes'
    void* const p = &here;
    *launcher = 255;
    if (k.entry != (uint32_t)Entry::kDiskAdaptiveRingBatch) return -100;
    geo_scene scenes[kRuleMaxFrames];
    for (uint32_t i = 0; i < kRuleMaxFrames; ++i) scenes[i] = k.scene[i == k.alt_frame ? 1 : 0];
    static const geo_frame frames[kRuleMaxFrames] = {};
    RenderCall rc;
    if (!batch_call(rc, Entry::kDiskAdaptiveRingBatch, (k.nulls & 1u) ? nullptr : p, (k.nulls & 2u) ? nullptr : frames,
                    (k.nulls & 4u) ? nullptr : scenes, k.nframes, k.width, k.height, k.g[0], k.g[1], k.g[2], k.g[3],
                    (k.nulls & 8u) ? nullptr : (uint8_t*)p, k.out_frame_stride,
                    k.steps_total ? (unsigned long long*)p : nullptr, nullptr))
        return GEO_EINVAL;
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

uint32_t adaptive_ring_batch_case_bytes(void) { return sizeof(RuleCase); }
uint32_t adaptive_ring_batch_entry(void) { return (uint32_t)Entry::kDiskAdaptiveRingBatch; }
uint32_t adaptive_ring_batch_ring_launcher(void) { return (uint32_t)Launcher::kRingFrames; }
uint32_t adaptive_ring_batch_adaptive_launcher(void) { return (uint32_t)Launcher::kAdaptiveFrames; }

// status[i] and launcher[i] (255 unless GEO_OK) of cases[i]
int adaptive_ring_batch_run(const RuleCase* cases, uint64_t n, int8_t* status, uint8_t* launcher) {
    for (uint64_t i = 0; i < n; ++i) {
        int l;
        status[i] = (int8_t)run_case(cases[i], &l);
        launcher[i] = (uint8_t)l;
    }
    return 0;
}

}  // extern "C"
