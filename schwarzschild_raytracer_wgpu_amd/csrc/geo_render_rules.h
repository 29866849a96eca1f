// geo_render_rules.h — the rules of a render call: which entry point takes
// which scene in which state of the context, and which launcher draws it.
// Pure host logic: no HIP header, no device, no context ("Render
// call rules").  geo_render.hip runs them before it touches the device;
// tests/native/render_rules_host.cpp builds them with g++ and
// tests/test_render_rules_host.py compares every status and launcher with the
// committed matrix.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/geo/geo.h"
#include "geo_pixel.h"

// GEO_RULE(n): return number n of the rules was taken (the host test build
// counts them: every return must be reached by the matrix).
#ifndef GEO_RULE
#define GEO_RULE(n) ((void)0)
#endif
constexpr int kRuleReturns = 40;

// (geo_render_kernels.h's kMaxBatchFrames and kBandRowAlign: geo_render.hip asserts them equal)
constexpr uint32_t kRuleMaxFrames = GEO_MAX_BATCH_FRAMES;
constexpr uint32_t kRuleBandRowAlign = 8;

// The render entry points of geo.h.
enum class Entry : uint8_t {
    kRows,               // geo_render_rows
    kBands,              // geo_render_bands
    kBandSet,            // geo_render_band_set
    kDiskAdaptive,       // geo_render_disk_adaptive
    kBandSetFrames,      // geo_render_band_set_frames
    kBandSetBatch,       // geo_render_band_set_batch
    kDiskBatch,          // geo_render_disk_batch
    kSsBatch,            // geo_render_ss_batch
    kEmissionBatch,      // geo_render_emission_batch
    kDiskRingBatch,      // geo_render_disk_ring_batch
    kDiskAdaptiveBatch,  // geo_render_disk_adaptive_batch
    kDiskAdaptiveRing,   // geo_render_disk_adaptive_ring
    kDiskAdaptiveRingBatch,  // geo_render_disk_adaptive_ring_batch
};
// kEntries: the entries up to geo_render_disk_adaptive_ring.  That entry's host
// driver (tests/native/render_rules_adaptive_ring_host.cpp) asserts the value,
// so it stays; an entry appended after it counts in kEntryRows, the rows of
// the traits table.
constexpr int kEntries = 12;
constexpr int kEntryRows = 13;

enum class Ss : uint8_t { kNo, kOneFrame, kAnyFrames };  // GEO_FLAG_SS4: refused, drawn alone, drawn in any batch
enum class Needs : uint8_t { kAnyScene, kDiskScene, kSsScene };
enum class NeedsState : uint8_t { kNone, kEmission, kRing };  // GEO_ESTATE without geo_set_disk_emission / _ring_f64
// geo_set_disk_ring_f64 on, for a disk scene: refused; drawn for one-sample
// frames (refused with GEO_FLAG_SS4); drawn; or not drawn and refused where
// there is a capture orbit to draw (the adaptive disk: ignored for rs = 0)
enum class Band : uint8_t { kNo, kOneSample, kAll, kNoOrbit };

// What an entry point draws.  A new entry point is a value of Entry and a row here.
struct EntryTraits {
    bool disk;         // it draws GEO_FLAG_DISK scenes
    uint32_t mode;     // ... and GEO_FLAG_SS4 scenes in this mode only; GEO_MODE_ADAPTIVE: no other scene at all
    Ss ss;             // whether it takes GEO_FLAG_SS4, and with how many frames
    Needs scene;       // the scenes it draws
    NeedsState state;  // the state it has nothing to draw without
    bool emission;     // it draws a disk scene's emission (geo_set_disk_emission)
    Band band;         // it draws a disk scene's f64 band (geo_set_disk_ring_f64)
    bool colour_only;  // an armed per-pixel buffer refuses the call
    bool scene_per_frame;  // `scene` points at nframes scenes (they may differ in r_obs only)
};
constexpr EntryTraits kEntryTraits[kEntryRows] = {
    // disk, mode, ss, scene, state, emission, band, colour_only, scene_per_frame; in Entry's order
    {true, GEO_MODE_DIRECT, Ss::kOneFrame, Needs::kAnyScene, NeedsState::kNone, true, Band::kOneSample, false, false},
    {true, GEO_MODE_DIRECT, Ss::kOneFrame, Needs::kAnyScene, NeedsState::kNone, true, Band::kOneSample, false, false},
    {true, GEO_MODE_DIRECT, Ss::kOneFrame, Needs::kAnyScene, NeedsState::kNone, true, Band::kOneSample, false, false},
    {true, GEO_MODE_ADAPTIVE, Ss::kNo, Needs::kDiskScene, NeedsState::kNone, true, Band::kNoOrbit, false, false},
    {false, GEO_MODE_DIRECT, Ss::kNo, Needs::kAnyScene, NeedsState::kNone, false, Band::kNo, false, false},
    {false, GEO_MODE_DIRECT, Ss::kNo, Needs::kAnyScene, NeedsState::kNone, false, Band::kNo, false, true},
    {true, GEO_MODE_DIRECT, Ss::kNo, Needs::kDiskScene, NeedsState::kNone, false, Band::kNo, true, true},
    {true, GEO_MODE_DIRECT, Ss::kAnyFrames, Needs::kSsScene, NeedsState::kNone, false, Band::kNo, false, true},
    {true, GEO_MODE_DIRECT, Ss::kAnyFrames, Needs::kDiskScene, NeedsState::kEmission, true, Band::kNo, true, true},
    {true, GEO_MODE_DIRECT, Ss::kAnyFrames, Needs::kDiskScene, NeedsState::kRing, true, Band::kAll, true, true},
    {true, GEO_MODE_ADAPTIVE, Ss::kAnyFrames, Needs::kDiskScene, NeedsState::kNone, true, Band::kNoOrbit, true, true},
    {true, GEO_MODE_ADAPTIVE, Ss::kNo, Needs::kDiskScene, NeedsState::kRing, true, Band::kAll, false, false},
    {true, GEO_MODE_ADAPTIVE, Ss::kAnyFrames, Needs::kDiskScene, NeedsState::kRing, true, Band::kAll, true, true},
};
static_assert((int)Entry::kDiskAdaptiveRingBatch + 1 == kEntryRows, "a row per entry");
constexpr const EntryTraits& traits(Entry e) { return kEntryTraits[(int)e]; }

// What the rules read of the context (geo_render.hip fills it in one place).
struct RuleState {
    bool sky;        // geo_set_sky has uploaded one
    uint32_t n_fan;  // the current fan's nodes (0: none)
    bool disk_set, shift_set, emit_set, disk_ring;
    float r_in, r_out;  // the disk's, while disk_set
};

// A render call as its entry point states it.
struct RenderCall {
    Entry entry;
    const geo_frame* frames;      // nframes uniforms (1 .. kRuleMaxFrames)
    uint32_t nframes = 1;
    size_t out_frame_stride = 0;  // frame f's output starts this many bytes after frame f - 1's
    // one scene for every frame, or (traits(entry).scene_per_frame) nframes scenes, frame f's at scene[f]
    const geo_scene* scene;
    uint32_t width, height, row0, nrows, band_rows, band_stride;
    uint8_t* out_rgba8;
    uint8_t* out_mask = nullptr;  // (a batch draws colour only)
    float* out_uv = nullptr;
    uint32_t* out_steps = nullptr;
    unsigned long long* steps_total;
    void* stream;
};

// What the rules hand on to the stages of a render call (RenderWork).
struct RenderRules {
    float* out_hits;  // geo_disk_hits_next_render's buffer, geo_disk_shift_next_render's,
    float* out_g;     // geo_disk_emission_next_render's
    float* out_q;
    bool emit;  // a GEO_FLAG_DISK scene with the emission set (check_scene)
    bool disk, ring_flag, mips, adaptive, defer;  // what the scene asks for (check_scene)
    bool ss;  // GEO_FLAG_SS4: the kernels' frame is the sample frame, twice the call's in width, height and rows
    bool ring;                                    // ring_flag and a capture orbit to draw (check_frames)
    bool disk_ring;  // a disk frame with geo_set_disk_ring_f64 on and a capture orbit to draw (check_scene)
};

// The band set's arguments, checked (every entry point but geo_render_rows and geo_render_bands).
static inline bool band_set_ok(uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0, uint32_t row_stride,
                               uint32_t nbands) {
    // band_rows: a multiple of 8, at most 4096 unless a power of two (band_rows_magic)
    if (width == 0 || height == 0 || band_rows == 0 || nbands == 0 || row_stride < band_rows ||
        band_rows % kRuleBandRowAlign != 0 || ((band_rows & (band_rows - 1)) != 0 && band_rows > 4096u))
        return GEO_RULE(0), false;
    if (width > (1u << 20) || height > (1u << 20)) return GEO_RULE(1), false;
    const uint64_t last = (uint64_t)row0 + (uint64_t)(nbands - 1) * row_stride;
    const uint64_t nrows = (uint64_t)nbands * band_rows;
    if (!(row0 < height && last < height && nrows <= (1u << 20))) return GEO_RULE(2), false;
    return true;
}

// What every entry point's call has: nrows rows from row0 on in bands of
// band_rows rows band_stride apart, colour only, one frame.
static inline void set_call(RenderCall& rc, Entry e, const geo_frame* frames, const geo_scene* scene, uint32_t width,
                            uint32_t height, uint32_t row0, uint32_t nrows, uint32_t band_rows, uint32_t band_stride,
                            uint8_t* out_rgba8, unsigned long long* steps_total, void* stream) {
    rc.entry = e;
    rc.frames = frames;
    rc.scene = scene;
    rc.width = width;
    rc.height = height;
    rc.row0 = row0;
    rc.nrows = nrows;
    rc.band_rows = band_rows;
    rc.band_stride = band_stride;
    rc.out_rgba8 = out_rgba8;
    rc.steps_total = steps_total;
    rc.stream = stream;
}

// The argument stage of the one-frame entry points: rc from the arguments, or
// false (GEO_EINVAL).  g0 .. g3 are the entry point's own four row arguments
// in its order: (row0, nrows) for geo_render_rows, (band_rows, band0,
// band_step, nbands) for geo_render_bands, (band_rows, row0, row_stride,
// nbands) for geo_render_band_set, geo_render_disk_adaptive and
// geo_render_disk_adaptive_ring.
static inline bool frame_call(RenderCall& rc, Entry e, const void* c, const geo_frame* frame, const geo_scene* scene,
                              uint32_t width, uint32_t height, uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3,
                              uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv, uint32_t* out_steps,
                              unsigned long long* steps_total, void* stream) {
    if (!c || !frame || !scene || !out_rgba8) return GEO_RULE(3), false;
    uint32_t row0, nrows, band_rows = 1u << 21, band_stride = 1u << 21;  // one band covering every row (2^21 >= nrows)
    if (e == Entry::kRows) {
        row0 = g0, nrows = g1;
        if (width == 0 || height == 0 || nrows == 0) return GEO_RULE(4), false;
        if ((uint64_t)row0 + nrows > height || width > (1u << 20) || height > (1u << 20)) return GEO_RULE(5), false;
    } else if (e == Entry::kBands) {
        const uint32_t band0 = g1, band_step = g2, nbands = g3;
        band_rows = g0;
        if (width == 0 || height == 0 || band_rows == 0 || nbands == 0 || band_step == 0 ||
            band_rows < kRuleBandRowAlign || (band_rows & (band_rows - 1)) != 0)
            return GEO_RULE(6), false;
        if (width > (1u << 20) || height > (1u << 20)) return GEO_RULE(7), false;
        const uint64_t first = (uint64_t)band0 * band_rows;
        const uint64_t last = first + (uint64_t)(nbands - 1) * band_step * band_rows;
        const uint64_t rows = (uint64_t)nbands * band_rows;
        if (first >= height || last >= height || rows > (1u << 20)) return GEO_RULE(8), false;
        row0 = (uint32_t)first, nrows = (uint32_t)rows, band_stride = band_step * band_rows;
    } else {
        const uint32_t row_stride = g2, nbands = g3;
        row0 = g1, nrows = g0;
        // geo_render_disk_adaptive and geo_render_disk_adaptive_ring: a row
        // range is the one-band case: any number of rows, as one band that
        // covers them all (geo_render_rows' mapping; row_stride is not read)
        const bool one_band = (e == Entry::kDiskAdaptive || e == Entry::kDiskAdaptiveRing) && nbands == 1;
        const bool rows = one_band && nrows != 0 && nrows <= (1u << 20) && width != 0 && height != 0 &&
                          width <= (1u << 20) && height <= (1u << 20) && row0 < height;
        if (!rows && !band_set_ok(width, height, g0, row0, row_stride, nbands)) return GEO_RULE(9), false;
        if (!one_band) nrows = nbands * g0, band_rows = g0, band_stride = row_stride;
    }
    set_call(rc, e, frame, scene, width, height, row0, nrows, band_rows, band_stride, out_rgba8, steps_total, stream);
    rc.out_mask = out_mask;
    rc.out_uv = out_uv;
    rc.out_steps = out_steps;
    return true;
}

// The argument stage of the batched entry points (geo_render_band_set_frames:
// `scenes` is its one scene).
static inline bool batch_call(RenderCall& rc, Entry e, const void* c, const geo_frame* frames, const geo_scene* scenes,
                              uint32_t nframes, uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                              uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                              unsigned long long* steps_total, void* stream) {
    if (!c || !frames || !scenes || !out_rgba8 || nframes == 0 || nframes > kRuleMaxFrames)
        return GEO_RULE(10), false;
    if (!band_set_ok(width, height, band_rows, row0, row_stride, nbands)) return GEO_RULE(11), false;
    set_call(rc, e, frames, scenes, width, height, row0, nbands * band_rows, band_rows, row_stride, out_rgba8,
             steps_total, stream);
    rc.nframes = nframes;
    rc.out_frame_stride = out_frame_stride;
    return true;
}

// Stage 1: the rules a call must meet before anything is done for it, in the
// order that decides which status a call breaking several of them gets.
static inline int check_scene(const RuleState& c, const RenderCall& rc, RenderRules& w) {
    const geo_scene* scene = rc.scene;
    const EntryTraits& t = traits(rc.entry);
    const bool armed = w.out_hits || w.out_g || w.out_q;  // (consumed by render_impl)
    if (scene->mode != GEO_MODE_DIRECT && scene->mode != GEO_MODE_FAN && scene->mode != GEO_MODE_ADAPTIVE)
        return GEO_RULE(12), GEO_EINVAL;
    if ((scene->flags & ~(GEO_FLAG_DEFER_STEPS | GEO_FLAG_COMPOSITE | GEO_FLAG_MIPS | GEO_FLAG_RING_F64 |
                          GEO_FLAG_DISK | GEO_FLAG_SS4)) != 0)
        return GEO_RULE(13), GEO_EINVAL;
    // geo_render_disk_adaptive, geo_render_disk_adaptive_ring,
    // geo_render_disk_adaptive_batch and geo_render_disk_adaptive_ring_batch
    // draw GEO_MODE_ADAPTIVE disk scenes only, DISK with DEFER_STEPS (and SS4,
    // the batches) at most (the older calls draw the direct and fan scenes)
    if (t.mode == GEO_MODE_ADAPTIVE &&
        (scene->mode != GEO_MODE_ADAPTIVE ||
         (scene->flags & ~(GEO_FLAG_DEFER_STEPS | (t.ss == Ss::kNo ? 0u : GEO_FLAG_SS4))) != GEO_FLAG_DISK))
        return GEO_RULE(14), GEO_EINVAL;
    // GEO_FLAG_SS4 (every rule here, where the bit was refused as an unknown
    // one before: a call that breaks an older rule too keeps its status): the
    // entry points that take it, one frame where they draw it alone, in their
    // mode, the level-0 sampler, colour only (an armed hit or g buffer
    // refuses the call), DISK and DEFER_STEPS at most, and a sample frame of
    // twice the size that the entry points take.
    w.ss = (scene->flags & GEO_FLAG_SS4) != 0;
    if (w.ss && (t.ss == Ss::kNo || (t.ss == Ss::kOneFrame && rc.nframes != 1) || scene->mode != t.mode ||
                 (scene->flags & ~(GEO_FLAG_SS4 | GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS)) != 0 || rc.out_mask ||
                 rc.out_uv || rc.out_steps || armed || rc.width > (1u << 19) || rc.height > (1u << 19)))
        return GEO_RULE(15), GEO_EINVAL;
    // geo_render_ss_batch draws SS4 scenes only (the other batched calls draw the rest)
    if (t.scene == Needs::kSsScene && !w.ss) return GEO_RULE(16), GEO_EINVAL;
    // GEO_FLAG_DISK: the entry points that draw it, in their mode, DEFER_STEPS (and SS4, above) at most
    w.disk = (scene->flags & GEO_FLAG_DISK) != 0;
    if (w.disk && (!t.disk || scene->mode != t.mode ||
                   (scene->flags & ~(GEO_FLAG_DISK | GEO_FLAG_DEFER_STEPS | GEO_FLAG_SS4)) != 0))
        return GEO_RULE(17), GEO_EINVAL;
    // the batched disk calls draw disk scenes only
    if (t.scene == Needs::kDiskScene && !w.disk) return GEO_RULE(18), GEO_EINVAL;
    // ... and colour only: an armed per-pixel buffer refuses the call
    if (t.colour_only && armed) return GEO_RULE(19), GEO_EINVAL;
    // geo_set_disk_emission: through a call that does not draw it a disk frame
    // would come out without its emission: refused, nothing launched
    w.emit = w.disk && c.emit_set;
    if (w.emit && !t.emission) return GEO_RULE(20), GEO_EINVAL;
    // geo_set_disk_ring_f64: through a call that does not draw the band a
    // supersampled or batched disk frame would come out without it: refused,
    // nothing launched (Band::kNoOrbit has its rule below: the state is
    // ignored for rs = 0)
    if (w.disk && c.disk_ring && (t.band == Band::kNo || (t.band == Band::kOneSample && w.ss)))
        return GEO_RULE(21), GEO_EINVAL;
    // (no capture orbit, rs = 0: the state is ignored, the plain disk frame)
    w.disk_ring = w.disk && c.disk_ring && scene->rs > 0.0f && scene->r_obs > scene->rs;
    w.ring_flag = (scene->flags & GEO_FLAG_RING_F64) != 0;
    if (w.ring_flag && (scene->mode == GEO_MODE_FAN || (scene->flags & (GEO_FLAG_COMPOSITE | GEO_FLAG_MIPS)) != 0))
        return GEO_RULE(22), GEO_EINVAL;
    // frame-aligned 2 x 2 quads: the rows a wave covers start on even frame rows
    w.mips = (scene->flags & GEO_FLAG_MIPS) != 0;
    if (w.mips && ((rc.row0 | rc.band_stride) & 1u) != 0) return GEO_RULE(23), GEO_EINVAL;
    // (1 <= nframes <= kRuleMaxFrames: the argument stage)
    if (rc.nframes > 1 && (w.mips || rc.out_mask || rc.out_uv || rc.out_steps || rc.out_frame_stride % 4u != 0 ||
                           rc.out_frame_stride < (size_t)rc.nrows * rc.width * 4u))
        return GEO_RULE(24), GEO_EINVAL;
    w.adaptive = scene->mode == GEO_MODE_ADAPTIVE;
    // tol: 0 (default) or a positive finite tolerance in the adaptive mode, 0 otherwise
    if (w.adaptive ? !(scene->tol >= 0.0f && scene->tol <= 3.0e38f) : scene->tol != 0.0f)
        return GEO_RULE(25), GEO_EINVAL;
    w.defer = (scene->flags & GEO_FLAG_DEFER_STEPS) != 0;
    if (scene->max_steps > (1u << 24)) return GEO_RULE(26), GEO_EINVAL;  // a wave's step sum must fit u32
    if (w.defer && rc.steps_total) return GEO_RULE(27), GEO_EINVAL;
    if (!c.sky) return GEO_RULE(28), GEO_ESTATE;
    if (scene->mode == GEO_MODE_FAN && c.n_fan < 2) return GEO_RULE(29), GEO_ESTATE;
    // bound > 0 (escape test folding, geo_pixel.h) needs r_obs > 0 and sphere_r > 0
    if (scene->mode != GEO_MODE_FAN &&
        (!(scene->step > 0.0f) || !(scene->r_obs > 0.0f) || !(scene->sphere_r > 0.0f) || !(scene->rs >= 0.0f)))
        return GEO_RULE(30), GEO_EINVAL;
    if (w.disk) {
        if (!c.disk_set) return GEO_RULE(31), GEO_ESTATE;
        // the state the entry point has nothing to draw without
        if (t.state == NeedsState::kEmission && !c.emit_set) return GEO_RULE(32), GEO_ESTATE;
        if (t.state == NeedsState::kRing && !c.disk_ring) return GEO_RULE(33), GEO_ESTATE;
        if (!(scene->rs == 0.0f || (scene->r_obs > scene->rs && scene->rs < c.r_in)) ||
            !(c.r_out < scene->sphere_r) || !(scene->r_obs < scene->sphere_r))
            return GEO_RULE(34), GEO_EINVAL;
        // shading: circular timelike orbits down to the inner edge
        if ((c.shift_set || c.emit_set) && scene->rs > 0.0f && !(c.r_in > 1.5f * scene->rs))
            return GEO_RULE(35), GEO_EINVAL;
        // the adaptive disk with geo_set_disk_ring_f64 on and a capture orbit
        // to draw: the frame would come out without its band (a batch's
        // frames share rs, and each observer is outside the horizon by
        // check_frames' rule)
        if (t.band == Band::kNoOrbit && w.disk_ring) return GEO_RULE(36), GEO_EINVAL;
    }
    return GEO_OK;
}

// Stage 1, per frame: the scene constants pk[f], and the rules by which the
// frames of a batch must agree.
static inline int check_frames(const RenderCall& rc, RenderRules& w, geo::PixelConsts* pk) {
    const geo_scene* scene = rc.scene;
    const bool per_frame = traits(rc.entry).scene_per_frame;
    for (uint32_t i = 0; i < rc.nframes; ++i) {
        const geo_scene& si = per_frame ? scene[i] : *scene;
        if (i > 0 && per_frame) {
            // one launch, one sampler, one integration: every field but r_obs
            // agrees with frame 0's (a fan-mode batch draws one fan: r_obs too)
            if (si.rs != scene->rs || si.sphere_r != scene->sphere_r || si.step != scene->step ||
                si.max_steps != scene->max_steps || si.mode != scene->mode || si.flags != scene->flags ||
                si.tol != scene->tol || (scene->mode == GEO_MODE_FAN && si.r_obs != scene->r_obs) ||
                !(si.r_obs > 0.0f))
                return GEO_RULE(37), GEO_EINVAL;
        }
        // GEO_FLAG_DISK's rules for this frame's observer (frame 0's in check_scene)
        if (w.disk && i > 0 && (!(si.rs == 0.0f || si.r_obs > si.rs) || !(si.r_obs < si.sphere_r)))
            return GEO_RULE(38), GEO_EINVAL;
        // geo_set_disk_ring_f64 in a batch (geo_render_disk_ring_batch,
        // geo_render_disk_adaptive_ring_batch): the
        // frames share rs and each has passed the rule above, so frame 0's
        // w.disk_ring (rs > 0 and r_obs > rs: a capture orbit to draw) holds
        // for every frame; each gets band constants of its own (launch_ring_frames)
        pk[i] = geo::make_consts(si.rs, si.sphere_r, si.r_obs, si.step, si.max_steps, si.tol);
        if (geo::geodesic_kind(pk[i]) != geo::geodesic_kind(pk[0])) return GEO_RULE(39), GEO_EINVAL;
    }
    // GEO_FLAG_RING_F64 (geo_band.h): the band's lanes take the f64 path; no
    // capture orbit (rs = 0, or the observer inside the horizon): the plain draw
    w.ring = w.ring_flag && scene->rs > 0.0f && scene->r_obs > scene->rs;
    if (w.ring_flag && per_frame)  // a batch: any frame with a capture orbit (each gets its own factor)
        for (uint32_t i = 1; i < rc.nframes; ++i)
            w.ring = w.ring || (scene[i].rs > 0.0f && scene[i].r_obs > scene[i].rs);
    return GEO_OK;
}

// Stage 5's decision: the launcher (geo_render.hip's launch_frames, launch_fan, ...) that draws an accepted call.
enum class Launcher : uint8_t {
    kFrames, kFan, kDiskFrame, kSsFrame,                                // one frame (kFrames, kFan: or a plain batch)
    kDiskFrames, kSsFrames, kEmitFrames, kRingFrames, kAdaptiveFrames,  // the batched disk and SS4 launches
};
static inline Launcher choose_launcher(const RenderCall& rc, const RenderRules& w) {
    switch (rc.entry) {
        case Entry::kDiskAdaptiveBatch: return Launcher::kAdaptiveFrames;
        case Entry::kDiskAdaptiveRingBatch:
            // (no capture orbit, rs = 0: the state is ignored, geo_render_disk_adaptive_batch's kernels)
            return w.disk_ring ? Launcher::kRingFrames : Launcher::kAdaptiveFrames;
        case Entry::kDiskRingBatch:
            // (no capture orbit, rs = 0: the state is ignored, the older batches' kernels)
            if (w.disk_ring) return Launcher::kRingFrames;
            if (w.emit) return Launcher::kEmitFrames;
            return w.ss ? Launcher::kSsFrames : Launcher::kDiskFrames;
        case Entry::kEmissionBatch: return Launcher::kEmitFrames;
        case Entry::kSsBatch: return Launcher::kSsFrames;
        case Entry::kDiskBatch: return Launcher::kDiskFrames;
        default: break;
    }
    if (w.ss) return Launcher::kSsFrame;
    if (w.disk) return Launcher::kDiskFrame;
    return rc.scene->mode == GEO_MODE_FAN ? Launcher::kFan : Launcher::kFrames;
}
