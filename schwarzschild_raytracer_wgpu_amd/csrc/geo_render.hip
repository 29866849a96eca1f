// geo_render.hip — the host half of the libgeo C-ABI's render path: contexts,
// sky, fan and disk set-up, the launchers and the render entry points.  The
// kernels they launch are in geo_render_kernels.h (one translation unit).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/geo/geo.h"
#include "geo_render_kernels.h"
#include "geo_render_rules.h"

static_assert(kRuleMaxFrames == kMaxBatchFrames && kRuleBandRowAlign == kBandRowAlign,
              "the rules' limits are the kernels'");

extern "C" {

int geo_abi_version(void) { return GEO_ABI_VERSION; }

const char* geo_status_str(int status) {
    switch (status) {
        case GEO_OK: return "ok";
        case GEO_EINVAL: return "invalid argument";
        case GEO_EHIP: return "HIP runtime error";
        case GEO_ENOMEM: return "out of memory";
        case GEO_ENODEV: return "no such HIP device";
        case GEO_ESTATE: return "call out of order";
        default: return "unknown status";
    }
}

// The context's ordering events: no timestamps, and no system-scope fence
// (they order device work on one device and let the host wait for it; a
// system-scope release after every render writes back the caches again and
// cost ~2 % per 4K frame)
constexpr unsigned kCtxEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;

int geo_ctx_create(int device, geo_ctx** out) {
    if (!out) return GEO_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return GEO_ENODEV;
    DeviceGuard g(device);
    if (!g.ok) return GEO_EHIP;
    geo_ctx* c = new (std::nothrow) geo_ctx();
    if (!c) return GEO_ENOMEM;
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        delete c;
        return GEO_EHIP;
    }
    c->num_cus = prop.multiProcessorCount;
    c->fan_cur = -1;
    bool ok = true;
    for (int b = 0; b < 2 && ok; ++b)
        ok = hipEventCreateWithFlags(&c->fan_written[b], kCtxEventFlags) == hipSuccess &&
             hipEventCreateWithFlags(&c->fan_read[b], kCtxEventFlags) == hipSuccess;
    for (int i = 0; i < geo_ctx::kStepCallSets && ok; ++i)
        ok = hipEventCreateWithFlags(&c->step_set_free[i], kCtxEventFlags) == hipSuccess;
    for (int i = 0; i < geo_ctx::kRenderStreams && ok; ++i)
        ok = hipEventCreateWithFlags(&c->render_done[i], kCtxEventFlags) == hipSuccess;
    if (ok) ok = hipEventCreateWithFlags(&c->order_written, kCtxEventFlags) == hipSuccess;
    c->dispatch_mode = GEO_DISPATCH_LONGEST_FIRST;
    c->dispatch_period = kDefaultDispatchPeriod;
    c->order_cur = -1;
    int st = ok ? GEO_OK : GEO_EHIP;
    if (ok && hipMalloc(&c->step_slots, sizeof(unsigned long long) * kSlotSetU64 * kSlotSets) != hipSuccess) {
        c->step_slots = nullptr;
        st = GEO_ENOMEM;
    }
    if (st == GEO_OK &&
        hipMemset(c->step_slots, 0, sizeof(unsigned long long) * kSlotSetU64 * kSlotSets) != hipSuccess)
        st = GEO_EHIP;
    if (st != GEO_OK) {
        if (c->step_slots) (void)hipFree(c->step_slots);
        for (int b = 0; b < 2; ++b) {
            if (c->fan_written[b]) (void)hipEventDestroy(c->fan_written[b]);
            if (c->fan_read[b]) (void)hipEventDestroy(c->fan_read[b]);
        }
        for (int i = 0; i < geo_ctx::kStepCallSets; ++i)
            if (c->step_set_free[i]) (void)hipEventDestroy(c->step_set_free[i]);
        for (int i = 0; i < geo_ctx::kRenderStreams; ++i)
            if (c->render_done[i]) (void)hipEventDestroy(c->render_done[i]);
        if (c->order_written) (void)hipEventDestroy(c->order_written);
        delete c;
        return st;
    }
    *out = c;
    return GEO_OK;
}

// The context's renders (and step flushes) in flight, on every stream it has
// rendered on: after this, nothing of the context's reads the sky, the fan
// buffers or the step counters.
static int wait_renders(geo_ctx* c) {
    for (int i = 0; i < c->n_render_streams; ++i)
        if (hipEventSynchronize(c->render_done[i]) != hipSuccess) return GEO_EHIP;
    return GEO_OK;
}

// The fan buffer b's last writer and readers (geo_ctx: the chained event and
// the slots of the draws that recorded none).
static int wait_fan(geo_ctx* c, int b) {
    if (c->fan_written_rec[b] && hipEventSynchronize(c->fan_written[b]) != hipSuccess) return GEO_EHIP;
    if (c->fan_read_rec[b] && hipEventSynchronize(c->fan_read[b]) != hipSuccess) return GEO_EHIP;
    for (int i = 0; i < c->n_render_streams; ++i)
        if ((c->fan_read_slots[b] >> i & 1u) && hipEventSynchronize(c->render_done[i]) != hipSuccess) return GEO_EHIP;
    return GEO_OK;
}

// Buffer b holds no pending writer or reader (after a host wait for them).
static void fan_forget(geo_ctx* c, int b) {
    c->fan_written_rec[b] = c->fan_read_rec[b] = false;
    c->fan_writer[b] = c->fan_reader[b] = nullptr;
    c->fan_read_slots[b] = 0;
}

// The slot whose event tracks the context's work on stream s
// (geo_ctx::render_done): the caller's next kernel on s records it as its stop
// event (hipExtLaunchKernelGGL), which rides on the dispatch's own completion
// signal instead of a marker packet after it (a marker per frame cost ~1 % of
// the event-timed 4K kernel).  With every slot taken, the least recently
// claimed one is evicted after a HOST wait for its event (a
// device-side wait would tie the caller's stream to an unrelated stream's
// work, which may sit behind a collective); that wait is the only blocking
// step, and only a context rendering on more than kRenderStreams streams
// reaches it.  -1 on a HIP error.
static int render_slot(geo_ctx* c, hipStream_t s) {
    int i = 0;
    while (i < c->n_render_streams && c->render_stream[i] != s) ++i;
    if (i == c->n_render_streams) {
        if (c->n_render_streams < geo_ctx::kRenderStreams) {
            ++c->n_render_streams;
        } else {
            i = c->render_next;
            c->render_next = (i + 1) % geo_ctx::kRenderStreams;
            if (hipEventSynchronize(c->render_done[i]) != hipSuccess) return -1;
            // the evicted stream's draws are done: no fan buffer waits for them
            for (int b = 0; b < 2; ++b) c->fan_read_slots[b] &= ~(1u << i);
        }
        c->render_stream[i] = s;
    }
    return i;
}

static hipEvent_t render_event(geo_ctx* c, hipStream_t s) {
    const int i = render_slot(c, s);
    return i < 0 ? nullptr : c->render_done[i];
}

void geo_ctx_destroy(geo_ctx* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    // work in flight may still read the buffers or record the events: the
    // context's own work, not the device's (no device-wide wait, see geo_ctx)
    (void)wait_renders(c);
    for (int b = 0; b < 2; ++b) (void)wait_fan(c, b);
    for (int i = 0; i < geo_ctx::kStepCallSets; ++i)
        if (c->step_set_rec[i]) (void)hipEventSynchronize(c->step_set_free[i]);
    if (c->sky) (void)hipFree(c->sky);
    if (c->disk_tex) (void)hipFree(c->disk_tex);
    if (c->emit_ramp) (void)hipFree(c->emit_ramp);
    for (int i = 0; i < geo_ctx::kRenderStreams; ++i)
        if (c->band_table[i]) (void)hipFree(c->band_table[i]);
    for (int b = 0; b < 2; ++b) {
        if (c->fan[b]) (void)hipFree(c->fan[b]);
        (void)hipEventDestroy(c->fan_written[b]);
        (void)hipEventDestroy(c->fan_read[b]);
    }
    for (int i = 0; i < geo_ctx::kStepCallSets; ++i) (void)hipEventDestroy(c->step_set_free[i]);
    for (int i = 0; i < geo_ctx::kRenderStreams; ++i) (void)hipEventDestroy(c->render_done[i]);
    if (c->step_slots) (void)hipFree(c->step_slots);
    if (c->learn_valid || c->tile_cap) (void)hipEventSynchronize(c->order_written);
    if (c->learn_stream) (void)hipStreamDestroy(c->learn_stream);
    for (int b = 0; b < 2; ++b)
        if (c->order[b]) (void)hipFree(c->order[b]);
    if (c->tile_cost) (void)hipFree(c->tile_cost);
    if (c->class_hist) (void)hipFree(c->class_hist);
    (void)hipEventDestroy(c->order_written);
    delete c;
}

int geo_set_sky(geo_ctx* c, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    static_assert(geo_ctx::kSkyLevels == geo::kSkyMipLevels, "one mip chain");
    if (!c || !rgba8 || w == 0 || h == 0 || w > (1u << 20) || h > (1u << 20)) return GEO_EINVAL;
    // the padded chain must stay below 2^31 bytes (32-bit buffer offsets, PaddedSkyQuad / LevelQuad)
    uint32_t lw[geo_ctx::kSkyLevels], lh[geo_ctx::kSkyLevels], loff[geo_ctx::kSkyLevels];
    uint64_t total = 0;
    for (int l = 0; l < geo_ctx::kSkyLevels; ++l) {
        lw[l] = geo::mip_dim(w, l);
        lh[l] = geo::mip_dim(h, l);
        loff[l] = (uint32_t)total;
        total += ((uint64_t)lw[l] + 2u) * ((uint64_t)lh[l] + 2u) * 4u;
        if (total >= (1ull << 31)) return GEO_EINVAL;
    }
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    // the chain on the host: level 0 = the texture, level l + 1 = the 2 x 2
    // box mean of level l (geo::mip_down), each padded for wrap/clamp
    std::vector<uint32_t> lvl((size_t)w * h), next;
    std::memcpy(lvl.data(), rgba8, (size_t)w * h * 4);
    std::vector<uint32_t> pad(total / 4u);
    for (int l = 0; l < geo_ctx::kSkyLevels; ++l) {
        if (l > 0) {
            next.resize((size_t)lw[l] * lh[l]);
            geo::mip_down(lvl.data(), lw[l - 1], lh[l - 1], next.data());
            lvl.swap(next);
        }
        geo::pad_sky(reinterpret_cast<const uint8_t*>(lvl.data()), lw[l], lh[l], pad.data() + loff[l] / 4u);
    }
    // Renders of this context still running on any of the caller's streams
    // (non-blocking ones do not order against a blocking copy) may be reading
    // the current sky: let them finish before it is overwritten or freed.  A
    // sky change is a set-up call (the reference builds its texture once,
    // basic_sphere_buffer.rs:29-36), so the wait costs nothing per frame.
    if (wait_renders(c) != GEO_OK) return GEO_EHIP;
    if (c->sky && c->sky_total_bytes != (uint32_t)total) {
        (void)hipFree(c->sky);
        c->sky = nullptr;
        c->sky_w = c->sky_h = 0;
    }
    if (!c->sky && hipMalloc(&c->sky, total) != hipSuccess) {
        c->sky = nullptr;
        c->sky_w = c->sky_h = 0;
        return GEO_ENOMEM;
    }
    if (hipMemcpy(c->sky, pad.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        // the buffer's contents are unknown now: no sky (renders return GEO_ESTATE until the next upload)
        (void)hipFree(c->sky);
        c->sky = nullptr;
        c->sky_w = c->sky_h = 0;
        return GEO_EHIP;
    }
    c->sky_w = w;
    c->sky_h = h;
    c->sky_total_bytes = (uint32_t)total;
    for (int l = 0; l < geo_ctx::kSkyLevels; ++l) {
        c->sky_lvl_w[l] = lw[l];
        c->sky_lvl_h[l] = lh[l];
        c->sky_lvl_off[l] = loff[l];
    }
    bool opaque = true;
    const size_t bytes = (size_t)w * h * 4;
    for (size_t i = 3; i < bytes && opaque; i += 4) opaque = rgba8[i] == 255;
    c->sky_opaque = opaque;  // the means of opaque texels are opaque: every level
    return GEO_OK;
}

int geo_clear_disk(geo_ctx* c) {
    if (!c) return GEO_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    if (c->disk_tex) {
        if (wait_renders(c) != GEO_OK) return GEO_EHIP;
        (void)hipFree(c->disk_tex);
    }
    c->disk_tex = nullptr;
    c->disk_set = false;
    c->shift_set = false;
    c->emit_set = false;
    c->disk_ring = false;
    return GEO_OK;
}

int geo_set_disk(geo_ctx* c, const geo_disk* disk, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    if (!c || !disk || !rgba8 || w == 0 || h == 0 || w > (1u << 20) || h > (1u << 20)) return GEO_EINVAL;
    const uint64_t total = ((uint64_t)w + 2u) * ((uint64_t)h + 2u) * 4u;  // padded, 32-bit buffer offsets
    if (total >= (1ull << 31)) return GEO_EINVAL;
    if (!(disk->r_in > 0.0f) || !(disk->r_in < disk->r_out) || !(disk->r_out < 3.0e38f)) return GEO_EINVAL;
    {
        // the normal and the axis, checked as every render will derive them
        // (any frame: the identity stands in for central_to_uv)
        const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        geo::DiskConsts dk;
        if (!geo::disk_consts(id, disk->normal, disk->axis, disk->r_in, disk->r_out,
                              geo::make_consts(0.0f, 2.0f * disk->r_out, disk->r_out, 0.03125f, 1u), &dk))
            return GEO_EINVAL;
    }
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    std::vector<uint32_t> pad(total / 4u);
    geo::pad_sky(rgba8, w, h, pad.data());
    // renders in flight may sample the current disk texture (geo_set_sky's rule)
    if (wait_renders(c) != GEO_OK) return GEO_EHIP;
    c->disk_set = false;
    if (c->disk_tex && c->disk_bytes != (uint32_t)total) {
        (void)hipFree(c->disk_tex);
        c->disk_tex = nullptr;
    }
    if (!c->disk_tex && hipMalloc(&c->disk_tex, total) != hipSuccess) {
        c->disk_tex = nullptr;
        return GEO_ENOMEM;
    }
    if (hipMemcpy(c->disk_tex, pad.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(c->disk_tex);
        c->disk_tex = nullptr;
        return GEO_EHIP;
    }
    c->disk_bytes = (uint32_t)total;
    c->disk_w = w;
    c->disk_h = h;
    c->disk = *disk;
    c->disk_set = true;
    return GEO_OK;
}

int geo_set_disk_ring_f64(geo_ctx* c, int on) {
    if (!c) return GEO_EINVAL;
    c->disk_ring = on != 0;
    return GEO_OK;
}

int geo_disk_hits_next_render(geo_ctx* c, float* out_hits) {
    if (!c || !out_hits) return GEO_EINVAL;
    c->hits_next = out_hits;
    return GEO_OK;
}

int geo_set_disk_shift(geo_ctx* c, const geo_disk_shift* shift) {
    if (!c) return GEO_EINVAL;
    if (!shift) {
        c->shift_set = false;
        return GEO_OK;
    }
    if ((shift->spin != 1 && shift->spin != -1) || shift->exponent > 4u || !(shift->gain > 0.0f) ||
        !(shift->gain <= 3.4028234e38f))
        return GEO_EINVAL;
    c->shift = *shift;
    c->shift_set = true;
    return GEO_OK;
}

int geo_disk_shift_next_render(geo_ctx* c, float* out_g) {
    if (!c || !out_g) return GEO_EINVAL;
    c->g_next = out_g;
    return GEO_OK;
}

int geo_set_disk_emission(geo_ctx* c, const geo_disk_emission* e, const uint8_t* ramp_rgba8, uint32_t n) {
    if (!c) return GEO_EINVAL;
    if (!e) {
        c->emit_set = false;
        return GEO_OK;
    }
    const auto pos = [](float v) { return v > 0.0f && v <= 3.4028234e38f; };  // finite, > 0
    if ((e->spin != 1 && e->spin != -1) || (e->profile != GEO_DISK_PROFILE_POWER && e->profile != GEO_DISK_PROFILE_THIN) ||
        !pos(e->t_ref) || !pos(e->t_lo) || !pos(e->t_hi) || !pos(e->exposure) || !(e->t_lo < e->t_hi) || !ramp_rgba8 ||
        n < 2u || n > GEO_DISK_RAMP_MAX)
        return GEO_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    // renders in flight may read the current ramp (geo_set_disk's rule)
    if (wait_renders(c) != GEO_OK) return GEO_EHIP;
    if (!c->emit_ramp && hipMalloc(&c->emit_ramp, GEO_DISK_RAMP_MAX * sizeof(uint32_t)) != hipSuccess) {
        c->emit_ramp = nullptr;
        return GEO_ENOMEM;
    }
    if (hipMemcpy(c->emit_ramp, ramp_rgba8, (size_t)n * 4u, hipMemcpyHostToDevice) != hipSuccess) {
        c->emit_set = false;  // the buffer's contents are unknown now: no emission
        return GEO_EHIP;
    }
    c->emit = *e;
    c->emit_n = n;
    c->emit_set = true;
    return GEO_OK;
}

int geo_disk_emission_next_render(geo_ctx* c, float* out_q) {
    if (!c || !out_q) return GEO_EINVAL;
    c->q_next = out_q;
    return GEO_OK;
}

// Both fan buffers hold at least n nodes.  Growing them waits for the device
// (renders in flight may read the old buffers); 400-node fans never regrow.
static int ensure_fan(geo_ctx* c, uint32_t n) {
    if (c->fan[0] && c->fan_cap >= n) return GEO_OK;
    for (int b = 0; b < 2; ++b)
        if (wait_fan(c, b) != GEO_OK) return GEO_EHIP;
    for (int b = 0; b < 2; ++b) {
        if (c->fan[b]) (void)hipFree(c->fan[b]);
        c->fan[b] = nullptr;
        c->n_fan[b] = 0;
        fan_forget(c, b);
    }
    c->fan_cap = 0;
    c->fan_cur = -1;
    if (hipMalloc(&c->fan[0], sizeof(float) * n) != hipSuccess) return GEO_ENOMEM;
    if (hipMalloc(&c->fan[1], sizeof(float) * n) != hipSuccess) {
        (void)hipFree(c->fan[0]);
        c->fan[0] = nullptr;
        return GEO_ENOMEM;
    }
    c->fan_cap = n;
    return GEO_OK;
}

// The buffer a new fan goes to (the one the current fan is not in), ordered
// on stream s after its previous writer and readers (on s itself by stream
// order).
static int fan_next(geo_ctx* c, hipStream_t s) {
    const int b = c->fan_cur < 0 ? 0 : 1 - c->fan_cur;
    if (c->fan_written_rec[b] && c->fan_writer[b] != s && hipStreamWaitEvent(s, c->fan_written[b], 0) != hipSuccess)
        return -1;
    if (c->fan_read_rec[b] && c->fan_reader[b] != s && hipStreamWaitEvent(s, c->fan_read[b], 0) != hipSuccess)
        return -1;
    for (int i = 0; i < c->n_render_streams; ++i)
        if ((c->fan_read_slots[b] >> i & 1u) && c->render_stream[i] != s &&
            hipStreamWaitEvent(s, c->render_done[i], 0) != hipSuccess)
            return -1;
    return b;
}

int geo_set_fan(geo_ctx* c, const float* fan, uint32_t n) {
    if (!c || !fan || n < 2 || n > kMaxFan) return GEO_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    int st = ensure_fan(c, n);
    if (st) return st;
    // a synchronous upload: into the free buffer once its last solve and
    // draws are done
    const int b = c->fan_cur < 0 ? 0 : 1 - c->fan_cur;
    if (wait_fan(c, b) != GEO_OK) return GEO_EHIP;
    if (hipMemcpy(c->fan[b], fan, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess) return GEO_EHIP;
    fan_forget(c, b);  // written and read by nothing in flight
    c->n_fan[b] = n;
    c->fan_cur = b;
    return GEO_OK;
}

int geo_solve_ray_fan(geo_ctx* c, double sphere_r, double schwarz_r, uint32_t max_iter, double step,
                      uint32_t nr_nodes, double r, float* fan_out, void* stream) {
    if (!c || nr_nodes < 2 || nr_nodes > kMaxFan || !(step > 0.)) return GEO_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    int st = ensure_fan(c, nr_nodes);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    const int b = fan_next(c, s);
    if (b < 0) return GEO_EHIP;
    hipLaunchKernelGGL(geo_fan_kernel, dim3((nr_nodes + 63) / 64), dim3(64), 0, s, sphere_r,
                       schwarz_r, max_iter, step, nr_nodes, r, c->fan[b]);
    if (hipGetLastError() != hipSuccess) return GEO_EHIP;
    if (hipEventRecord(c->fan_written[b], s) != hipSuccess) return GEO_EHIP;
    // the solve is ordered after every earlier reader of b: later waits for
    // b's readers start afresh, and a wait for the solve covers the old ones
    fan_forget(c, b);
    c->fan_written_rec[b] = true;
    c->fan_writer[b] = s;
    c->n_fan[b] = nr_nodes;
    c->fan_cur = b;
    if (fan_out) {
        if (hipMemcpyAsync(fan_out, c->fan[b], sizeof(float) * nr_nodes, hipMemcpyDeviceToHost, s) !=
            hipSuccess)
            return GEO_EHIP;
        if (hipStreamSynchronize(s) != hipSuccess) return GEO_EHIP;
    }
    return GEO_OK;
}

// floor(lr / d) == umulhi(lr, m) for every local row lr < 2^20: d a power of
// two, m = 2^32 / d exactly; otherwise m = floor(2^32 / d) + 1, whose error
// lr (m - 2^32/d) / 2^32 < lr / 2^32 stays below 1/d while lr d < 2^32
// (d <= 4096, checked by the caller).
static uint32_t band_rows_magic(uint32_t d) {
    return (d & (d - 1u)) == 0u ? (uint32_t)((1ull << 32) / d) : (uint32_t)((1ull << 32) / d + 1u);
}

// One frame's tiles: grid.y is limited to 65535, so a taller tile grid (more
// than 524280 rows; the C-ABI takes 2^20) goes out as several launches, each
// with its first tile row in tile_y0.  The kernel's mapping is the same.
constexpr uint32_t kMaxGridY = 65535;
// rows of tiles per launch on WB's 1-D grid (wave_blocks): its limit too
static uint32_t wave_block_max_ny(uint32_t tiles_x) { return std::min(kMaxGridY, kMaxWaveBlockTiles / tiles_x); }

// Where a render's launches go: the frame's tile grid, the stream, the
// context's event for that stream (render_event) and the caller's timing
// pair (geo_time_next_render; null otherwise).
struct LaunchPlan {
    uint32_t tiles_x, tiles_y;
    hipStream_t s;
    hipEvent_t done, t_start, t_stop;
};

extern "C++" {
// f(std::integral_constant<int, K>{}) for the frame's integration kind K
// (geo::geodesic_kind): the kind as a template argument of what f launches.
template <typename F>
static int with_kind(int kind, F&& f) {
    switch (kind) {
        case geo::kCurvedOut: return f(std::integral_constant<int, geo::kCurvedOut>{});
        case geo::kCurvedIn: return f(std::integral_constant<int, geo::kCurvedIn>{});
        default: return f(std::integral_constant<int, geo::kFlat>{});
    }
}

// The launches of one render: the tile grid in slices of at most max_ny tile
// rows, each issued by launch_one(a, ny, start, stop) with its slice in
// a.tile_y0 and a.launch_tiles.  The last launch records `done` as its stop
// event; a timed render puts the caller's start event on the first launch's
// dispatch and its stop event on the last one's, and records `done` after it.
template <typename F>
static int launch_split(RenderArgs a, const LaunchPlan& p, uint32_t max_ny, F&& launch_one) {
    a.tiles_x = p.tiles_x;
    for (uint32_t y0 = 0; y0 < p.tiles_y; y0 += max_ny) {
        a.tile_y0 = y0;
        const uint32_t ny = std::min(p.tiles_y - y0, max_ny);
        a.launch_tiles = p.tiles_x * ny;
        const bool last = y0 + ny >= p.tiles_y;
        launch_one(a, ny, y0 == 0 ? p.t_start : nullptr, last ? (p.t_stop ? p.t_stop : p.done) : nullptr);
        if (hipGetLastError() != hipSuccess) return GEO_EHIP;
    }
    if (p.t_stop && hipEventRecord(p.done, p.s) != hipSuccess) return GEO_EHIP;
    return GEO_OK;
}

// A render of nframes frames on WB's 1-D grid (wave_blocks): one wave per
// workgroup, the frame in grid.z; the kernel takes RenderArgs and then args.
template <typename K, typename... Args>
static int launch_wave_blocks(const RenderArgs& a, const LaunchPlan& p, uint32_t nframes, K kernel,
                              const Args&... args) {
    return launch_split(a, p, wave_block_max_ny(p.tiles_x),
                        [&](const RenderArgs& la, uint32_t, hipEvent_t start, hipEvent_t stop) {
        const dim3 grid(wave_block_count(la.launch_tiles), 1, nframes), block(64);
        hipExtLaunchKernelGGL(kernel, grid, block, 0, p.s, start, stop, 0, la, args...);
    });
}

// The launch of geo_render_kernel's instantiation for NF frames.  band:
// GEO_FLAG_RING_F64's constants, or null; the ring kernels exist out of fan
// mode and for the curved kinds only (kFlat has no capture orbit), and with
// the level-0 sampler.
template <int MODE, int KIND, uint32_t NF>
static int launch_tiles(const RenderArgs& a, const FrameBatch<NF>& fb, uint32_t nframes, bool mips,
                        const LaunchPlan& p, const geo::BandConsts* band) {
    // wb: one wave per workgroup on WB's 1-D grid (wave_blocks); otherwise the
    // tile's four waves as one workgroup on the 2-D grid, the frame in grid.z
    const auto run = [&](auto kernel, bool wb, const auto& bk) {
        return launch_split(a, p, wb ? wave_block_max_ny(p.tiles_x) : kMaxGridY,
                            [&](const RenderArgs& la, uint32_t ny, hipEvent_t start, hipEvent_t stop) {
            dim3 grid(p.tiles_x, ny, nframes), block(kBlock);
            if (wb) grid = dim3(wave_block_count(la.launch_tiles)), block = dim3(64);
            hipExtLaunchKernelGGL(kernel, grid, block, 0, p.s, start, stop, 0, la, fb, bk);
        });
    };
    if constexpr (MODE != GEO_MODE_FAN && KIND != geo::kFlat) {
        if (band) {
            if constexpr (NF == 1) {
                BandArg<true> bk;
                bk.k = *band;
                return run(geo_render_kernel<MODE, KIND, false, 1, true>, wave_blocks(MODE, false, 1, true), bk);
            } else {  // fb.ring_kx, the constants derived per wave
                return run(geo_render_kernel<MODE, KIND, false, NF, true>, false, BandArg<false>{});
            }
        }
    }
    if constexpr (NF == 1) {
        if (mips) return run(geo_render_kernel<MODE, KIND, true, 1, false>, false, BandArg<false>{});
        return run(geo_render_kernel<MODE, KIND, false, 1, false>, wave_blocks(MODE, false, 1, false),
                   BandArg<false>{});
    } else {
        return run(geo_render_kernel<MODE, KIND, false, NF, false>, false, BandArg<false>{});
    }
}

// One frame (FrameBatch<1>, the kernel arguments as before batching), or a
// batch of 2 .. kMaxBatchFrames in one launch (FrameBatch<kMaxBatchFrames>,
// the frame in blockIdx.z; no mip-mapped sampler).  band: GEO_FLAG_RING_F64's
// constants (frame 0), or null; a batch carries each frame's band factor
// (ring_kx, 0 where the frame has no capture orbit) and its kernel derives
// the constants per wave from the frame and its scene constants.
static_assert(sizeof(RenderArgs) + sizeof(FrameBatch<kMaxBatchFrames>) <= 4096, "kernel arguments fit 4 KiB");
static_assert(sizeof(RenderArgs) + sizeof(FrameBatch<1>) + sizeof(BandArg<true>) <= 4096,
              "kernel arguments fit 4 KiB");
template <int MODE, int KIND>
static int launch_frames(const RenderArgs& a, const FrameK* fk, const geo::PixelConsts* pk, uint32_t nframes,
                         bool mips, const LaunchPlan& p, const geo::BandConsts* band) {
    if (nframes == 1) {
        FrameBatch<1> fb;
        fb.f[0] = fk[0];
        return launch_tiles<MODE, KIND, 1>(a, fb, 1, mips, p, band);
    }
    FrameBatch<kMaxBatchFrames> fb;
    std::memset(&fb, 0, sizeof(fb));
    for (uint32_t i = 0; i < nframes; ++i) {
        fb.f[i] = fk[i];
        fb.k[i] = pk[i];
        fb.ring_kx[i] = (band && pk[i].rs > 0.0f && pk[i].r > pk[i].rs) ? geo::band_kx(pk[i].rs, pk[i].r) : 0.0f;
    }
    return launch_tiles<MODE, KIND, kMaxBatchFrames>(a, fb, nframes, false, p, band);
}

// The disk texture's fields of DiskArgs and DiskBatchArgs.
template <typename D>
static void fill_disk_tex(const geo_ctx* c, D& d) {
    d.tex = c->disk_tex;
    d.tex_w256 = (float)c->disk_w * 256.0f;
    d.tex_h256 = (float)c->disk_h * 256.0f;
    d.tex_pitch_b = (c->disk_w + 2u) * 4u;
    d.tex_bytes = c->disk_bytes;
}

// f(std::integral_constant<Shade, S>{}) for what a disk render shades, decided
// here once per call: the emission where it is set (it takes the shift's
// place), else the shift, else the plain disk.
template <typename F>
static int with_shade(bool emit, bool shift, F&& f) {
    if (emit) return f(std::integral_constant<Shade, Shade::kDiskEmit>{});
    if (shift) return f(std::integral_constant<Shade, Shade::kDiskShift>{});
    return f(std::integral_constant<Shade, Shade::kDisk>{});
}

// f(std::true_type{}) or f(std::false_type{}): a render's property as a template argument.
template <typename F>
static int with_flag(bool on, F&& f) {
    return on ? f(std::true_type{}) : f(std::false_type{});
}

// The emission batch's further kernel argument, or none.
template <Shade SHADE>
static ShadeBatchArg<SHADE> shade_batch_arg(const DiskEmitBatchArgs& eb) {
    if constexpr (SHADE == Shade::kDiskEmit)
        return eb;
    else
        return NoArgs{};
}
}

// The order buffers hold at least n tiles (both orders, the costs, the class
// histograms).  Growing them waits for the context's renders and rebuilds,
// and forgets the learned order.
static int ensure_tiles(geo_ctx* c, uint32_t n) {
    if (c->tile_cap >= n) return GEO_OK;
    if (wait_renders(c) != GEO_OK || hipEventSynchronize(c->order_written) != hipSuccess) return GEO_EHIP;
    for (int b = 0; b < 2; ++b) {
        if (c->order[b]) (void)hipFree(c->order[b]);
        c->order[b] = nullptr;
    }
    if (c->tile_cost) (void)hipFree(c->tile_cost);
    if (c->class_hist) (void)hipFree(c->class_hist);
    c->tile_cost = c->class_hist = nullptr;
    c->tile_cap = 0;
    c->order_cur = -1;
    c->learn_valid = false;
    c->rebuild_pending = false;  // order_written synchronised above
    const size_t chunks = (n + kOrderChunk - 1) / kOrderChunk;
    if (hipMalloc(&c->order[0], n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&c->order[1], n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&c->tile_cost, n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&c->class_hist, chunks * kCostClasses * sizeof(uint32_t)) != hipSuccess) {
        for (int b = 0; b < 2; ++b)
            if (c->order[b]) (void)hipFree(c->order[b]);
        if (c->tile_cost) (void)hipFree(c->tile_cost);
        if (c->class_hist) (void)hipFree(c->class_hist);
        c->order[0] = c->order[1] = c->tile_cost = c->class_hist = nullptr;
        return GEO_ENOMEM;
    }
    if (hipMemset(c->tile_cost, 0, n * sizeof(uint32_t)) != hipSuccess) return GEO_EHIP;
    c->tile_cap = n;
    return GEO_OK;
}

// A render call refused before render_impl: the timing pair of
// geo_time_next_render is dropped too (it belongs to that call alone).
static int invalid_call(geo_ctx* c) {
    if (c) {
        c->time_start = c->time_stop = nullptr;
        c->hits_next = nullptr;
        c->g_next = nullptr;
        c->q_next = nullptr;
    }
    return GEO_EINVAL;
}

// What the stages of a render call (render_impl) hand on: what the rules
// decided (geo_render_rules.h) and what the launch needs.
struct RenderWork : RenderRules {
    FrameK fk[kMaxBatchFrames];
    geo::PixelConsts pk[kMaxBatchFrames];
    RenderArgs a;
    LaunchPlan p;
    int call_set;  // the per-call step-counter set (-1: none)
    int slot;      // p.s's render slot
    bool record;   // this render records its tiles' costs
};

// What the rules read of the context.
static RuleState rule_state(const geo_ctx* c) {
    RuleState s;
    s.sky = c->sky != nullptr;
    s.n_fan = c->fan_cur < 0 ? 0u : c->n_fan[c->fan_cur];
    s.disk_set = c->disk_set;
    s.shift_set = c->shift_set;
    s.emit_set = c->emit_set;
    s.disk_ring = c->disk_ring;
    s.r_in = c->disk.r_in;
    s.r_out = c->disk.r_out;
    return s;
}

// Stage 1, per frame: its camera and scene constants, and the rules by which
// the frames of a batch must agree (check_frames).
static int fill_frames(const RenderCall& rc, RenderWork& w) {
    for (uint32_t i = 0; i < rc.nframes; ++i) {
        const geo_frame& fr = rc.frames[i];
        std::memcpy(&w.fk[i].frame, &fr, sizeof(geo_frame));
        // (GEO_FLAG_SS4: the camera of the 2W x 2H sample frame; it takes the frame and the size only)
        const uint32_t ssf = w.ss ? 2u : 1u;
        w.fk[i].cam = geo::camera_consts(fr.display_to_movement, fr.movement_to_central, ssf * rc.width,
                                         ssf * rc.height);
        w.fk[i].kt = geo::aberration_kt(fr.psi_factor_and_position[0]);
    }
    return check_frames(rc, w, w.pk);
}

// Stage 2: the kernels' arguments (the sky and its mip chain, the fan, the
// outputs, the band mapping) and the frame's tile grid.
static void fill_args(const geo_ctx* c, const RenderCall& rc, RenderWork& w) {
    RenderArgs& a = w.a;
    a.out_frame_px = rc.out_frame_stride / 4u;
#if defined(GEO_WAVE_LOG)
    a.wave_log = c->wave_log;
#endif
    a.k = w.pk[0];
    // GEO_FLAG_SS4: the sample frame's sizes and rows (twice the call's; the
    // output's pitch rides in SsPitch).  band_magic stays the call's
    // band_rows': the SS kernels take the band index on output rows, where
    // band_rows_magic is exact.
    const uint32_t ssf = w.ss ? 2u : 1u;
    a.width = ssf * rc.width;
    a.height = ssf * rc.height;
    a.row0 = ssf * rc.row0;
    a.nrows = ssf * rc.nrows;
    a.band_rows = ssf * rc.band_rows;
    a.band_magic = band_rows_magic(rc.band_rows);
    a.band_stride = ssf * rc.band_stride;
    a.sky_opaque = c->sky_opaque ? 1u : 0u;
    a.composite = (rc.scene->flags & GEO_FLAG_COMPOSITE) ? 1u : 0u;
    w.p.tiles_x = (a.width + kTileW - 1) / kTileW;
    const uint32_t tile_h = kTileH * lane_rows(rc.scene->mode, w.mips);
    w.p.tiles_y = (a.nrows + tile_h - 1) / tile_h;
    a.sky = c->sky;
    a.sky_w = c->sky_w;
    a.sky_h = c->sky_h;
    a.sky_w256 = (float)c->sky_w * 256.0f;
    a.sky_h256 = (float)c->sky_h * 256.0f;
    a.sky_pitch_b = (c->sky_w + 2u) * 4u;
    a.sky_bytes = a.sky_pitch_b * (c->sky_h + 2u);
    for (int l = 0; l < geo::kSkyMipLevels; ++l) {
        a.mip_off[l] = c->sky_lvl_off[l];
        a.mip_pitch[l] = (c->sky_lvl_w[l] + 2u) * 4u;
        a.mip_w256[l] = (float)c->sky_lvl_w[l] * 256.0f;
        a.mip_h256[l] = (float)c->sky_lvl_h[l] * 256.0f;
    }
    a.sky_wf = (float)c->sky_w;
    a.sky_hf = (float)c->sky_h;
    a.sky_total_bytes = c->sky_total_bytes;
    a.tile_order = nullptr;
    a.tile_cost = nullptr;
    a.cost_overhead = w.adaptive ? kCostOverheadAdaptive : kCostOverheadDirect;
    const int fb = c->fan_cur;
    a.fan = fb < 0 ? nullptr : c->fan[fb];
    a.n_fan = fb < 0 ? 0u : c->n_fan[fb];
    a.out_rgba = reinterpret_cast<uint32_t*>(rc.out_rgba8);
    a.out_mask = rc.out_mask;
    a.out_uv = reinterpret_cast<float2*>(rc.out_uv);
    a.out_steps = rc.out_steps;
}

// Stage 3: the step counters: the context's accumulator (DEFER), or a per-call
// set free of any earlier call's fold (steps_total; not in fan mode, which
// has none).
static int take_step_set(geo_ctx* c, const RenderCall& rc, RenderWork& w) {
    w.call_set = -1;
    w.a.step_slots = w.defer ? c->step_slots : nullptr;
    if (rc.steps_total && rc.scene->mode != GEO_MODE_FAN) {
        w.call_set = c->step_set_next;
        c->step_set_next = (w.call_set + 1) % geo_ctx::kStepCallSets;
        if (c->step_set_rec[w.call_set] && hipStreamWaitEvent(w.p.s, c->step_set_free[w.call_set], 0) != hipSuccess)
            return GEO_EHIP;
        w.a.step_slots = c->step_slots + (size_t)(1 + w.call_set) * kSlotSetU64;
    }
    return GEO_OK;
}

// Stage 4: the dispatch order (geo_ctx): a learned or explicit order for
// exactly this grid, one launch, not in fan mode (its tiles all cost the
// same); and whether this render records its tiles' costs for the next order.
static int choose_order(geo_ctx* c, const RenderCall& rc, RenderWork& w) {
    const uint32_t tiles_x = w.p.tiles_x, tiles_y = w.p.tiles_y;
    w.record = false;
    // (one launch for the whole grid: the 2-D grid's y limit, and WB's tile count)
    if (rc.scene->mode == GEO_MODE_FAN || tiles_y > kMaxGridY || (uint64_t)tiles_x * tiles_y > kMaxWaveBlockTiles)
        return GEO_OK;
    if (c->dispatch_mode == GEO_DISPATCH_EXPLICIT) {
        if (c->order_cur >= 0 && tiles_x == c->explicit_x && tiles_y == c->explicit_y)
            w.a.tile_order = c->order[c->order_cur];
        return GEO_OK;
    }
    if (c->dispatch_mode != GEO_DISPATCH_LONGEST_FIRST) return GEO_OK;
    // (a GEO_FLAG_RING_F64 render learns its own order: its band's tiles cost
    // more; a GEO_FLAG_SS4 render too: its grid is the sample frame's; an
    // emission render has a key of its own, as the disk render has, and a
    // disk render with geo_set_disk_ring_f64 on, for its band's tiles, one
    // frame or geo_render_disk_ring_batch's, whose frame 0 records them;
    // geo_render_disk_adaptive_ring and geo_render_disk_adaptive_ring_batch
    // share a key with neither the adaptive disk renders, which have no
    // disk_ring bit, nor the direct ring renders, whose mode differs)
    const uint32_t key[9] = {rc.width, rc.height, rc.row0, rc.nrows, rc.band_rows, rc.band_stride, rc.scene->mode,
                             (w.mips ? 1u : 0u) | (w.ring ? 2u : 0u) | (w.disk ? 4u : 0u) | (w.ss ? 8u : 0u) |
                                 (w.emit ? 16u : 0u) | (w.disk_ring ? 32u : 0u),
                             tiles_x * tiles_y};
    if (!c->learn_valid || std::memcmp(key, c->learn_key, sizeof(key)) != 0) {
        std::memcpy(c->learn_key, key, sizeof(key));
        c->learn_valid = true;
        c->order_cur = -1;
        c->rebuild_keep = false;  // a rebuild still running learned another grid
        c->since_learn = c->dispatch_period;
    }
    // adopt a finished rebuild: a host query, never a wait
    if (c->rebuild_pending) {
        const hipError_t q = hipEventQuery(c->order_written);
        if (q == hipSuccess) {
            c->rebuild_pending = false;
            if (c->rebuild_keep) {
                c->order_cur = c->rebuild_nb;
                ++c->orders_adopted;
            }
        } else if (q != hipErrorNotReady) {
            return GEO_EHIP;
        }
    }
    // every period-th render of the grid records (period 1: every render), or
    // the first one after that whose predecessor's rebuild has been adopted
    if (c->since_learn < c->dispatch_period) ++c->since_learn;
    w.record = c->since_learn >= c->dispatch_period && !c->rebuild_pending;
    if (w.record) {
        c->since_learn = 0u;
        int est = ensure_tiles(c, tiles_x * tiles_y);
        if (est) return est;
        if (!c->learn_valid) {  // the growth forgot the key: this render learns it again
            std::memcpy(c->learn_key, key, sizeof(key));
            c->learn_valid = true;
        }
        w.a.tile_cost = c->tile_cost;
    }
    if (c->order_cur >= 0) w.a.tile_order = c->order[c->order_cur];
    return GEO_OK;
}

// Stage 5, fan mode: the draw after the solve that wrote the buffer (geo_ctx:
// on the solve's own stream by stream order, with no event work: the reader
// is its slot's bit); on another stream this render then joins the buffer's
// chain of readers (the wait is queued after the launch, so it holds back
// only later work on s, never this render).
// (a buffer uploaded by geo_set_fan has no writer in flight: its next writer
// waits for its readers on the host, so they need no event)
static int launch_fan(geo_ctx* c, const RenderCall& rc, const RenderWork& w) {
    const int fb = c->fan_cur;
    hipStream_t s = w.p.s;
    const bool by_slot = !c->fan_written_rec[fb] || c->fan_writer[fb] == s;
    if (!by_slot && hipStreamWaitEvent(s, c->fan_written[fb], 0) != hipSuccess) return GEO_EHIP;
    const int st = launch_frames<GEO_MODE_FAN, geo::kCurvedOut>(w.a, w.fk, w.pk, rc.nframes, w.mips, w.p, nullptr);
    if (st) return st;
    if (by_slot) {
        c->fan_read_slots[fb] |= 1u << w.slot;
    } else {
        if (c->fan_read_rec[fb] && c->fan_reader[fb] != s && hipStreamWaitEvent(s, c->fan_read[fb], 0) != hipSuccess)
            return GEO_EHIP;
        if (hipEventRecord(c->fan_read[fb], s) != hipSuccess) return GEO_EHIP;
        c->fan_read_rec[fb] = true;
        c->fan_reader[fb] = s;
    }
    return GEO_OK;
}

// The emission's kernel argument for frame 0 of the call (the emission takes
// the shift's place: geo_set_disk_shift's state is not read).
static DiskEmitArgs emit_args(const geo_ctx* c, const RenderCall& rc, const RenderWork& w) {
    DiskEmitArgs em;
    em.k = geo::disk_emission_consts(rc.frames[0].central_to_uv, rc.scene->rs, rc.scene->r_obs, c->emit.spin,
                                     c->emit.profile, c->emit.t_ref, c->emit.t_lo, c->emit.t_hi, c->emit.exposure,
                                     c->emit_n);
    em.ramp = c->emit_ramp;
    em.out_g = w.out_g;
    em.out_q = w.out_q;
    return em;
}

// Stage 5, a GEO_FLAG_DISK frame drawn alone (geo_render_disk_frame_kernel):
// direct, adaptive (geo_render_disk_adaptive) or GEO_FLAG_SS4
// (geo_render_ss_disk_frame_kernel; colour only: the rules left no per-pixel
// buffer armed; the disk's constants do not depend on the resolution), or
// with geo_set_disk_ring_f64 on (geo_render_disk_ring_kernel:
// the band's constants ride as a further argument; the curved kinds only, a
// capture orbit needs rs > 0), direct or adaptive
// (geo_render_disk_adaptive_ring: the same kernel's GEO_MODE_ADAPTIVE, the
// same arguments).  The rules let no adaptive SS4 frame through.
static int launch_disk_frame(const geo_ctx* c, const RenderCall& rc, const RenderWork& w) {
    DiskArgs d;
    if (!geo::disk_consts(rc.frames[0].central_to_uv, c->disk.normal, c->disk.axis, c->disk.r_in, c->disk.r_out, w.a.k,
                          &d.k))
        return GEO_EINVAL;
    fill_disk_tex(c, d);
    d.out_hits = w.out_hits;
    FrameBatch<1> fb;
    fb.f[0] = w.fk[0];
    BandArg<true> bk;
    if (w.disk_ring) bk.k = geo::band_consts(rc.frames[0], *rc.scene, rc.width, rc.height);
    return with_kind(geo::geodesic_kind(w.a.k), [&](auto kind) {
        return with_shade(w.emit, c->shift_set, [&](auto shade) {
            constexpr int KIND = decltype(kind)::value;
            constexpr Shade SHADE = decltype(shade)::value;
            ShadeFrameArg<SHADE> x;
            if constexpr (SHADE == Shade::kDiskEmit) x = emit_args(c, rc, w);
            if constexpr (SHADE == Shade::kDiskShift) {
                x.k = geo::disk_shift_consts(rc.frames[0].central_to_uv, rc.scene->rs, rc.scene->r_obs, c->shift.spin,
                                             c->shift.exponent, c->shift.gain);
                x.out_g = w.out_g;
            }
            if (w.disk_ring) {
                if constexpr (KIND != geo::kFlat) {
                    // (adaptive: geo_render_disk_adaptive_ring alone; the rules refuse the older calls)
                    const auto direct = geo_render_disk_ring_kernel<KIND, SHADE, GEO_MODE_DIRECT>;
                    const auto adaptive = geo_render_disk_ring_kernel<KIND, SHADE, GEO_MODE_ADAPTIVE>;
                    return launch_wave_blocks(w.a, w.p, 1, w.adaptive ? adaptive : direct, fb, d, x, bk);
                }
                return (int)GEO_EINVAL;  // (never reached: the state is ignored for rs = 0)
            }
            if (w.ss)
                return launch_wave_blocks(w.a, w.p, 1, geo_render_ss_disk_frame_kernel<KIND, SHADE>, fb,
                                          SsDiskArgs<SHADE>{rc.width, d, x});
            if (w.adaptive)
                return launch_wave_blocks(w.a, w.p, 1, geo_render_disk_frame_kernel<KIND, SHADE, GEO_MODE_ADAPTIVE>, fb,
                                          d, x);
            return launch_wave_blocks(w.a, w.p, 1, geo_render_disk_frame_kernel<KIND, SHADE, GEO_MODE_DIRECT>, fb, d,
                                      x);
        });
    });
}

// Stage 5, a GEO_FLAG_SS4 render without a disk (geo_render_ss_sky_kernel): the
// frame drawn alone, or geo_render_ss_batch's frames in grid.z on the disk
// batch's geometry.  w.fk holds each frame's camera at 2W x 2H and w.pk its
// scene constants (fill_frames).
static int launch_ss_sky(const RenderCall& rc, const RenderWork& w, bool batch) {
    const SsPitch<true> o{rc.width};
    return with_kind(geo::geodesic_kind(w.a.k), [&](auto kind) {
        constexpr int KIND = decltype(kind)::value;
        if (!batch) {
            FrameBatch<1> fb;
            fb.f[0] = w.fk[0];
            return launch_wave_blocks(w.a, w.p, 1, geo_render_ss_sky_kernel<KIND, 1>, fb, o);
        }
        FrameBatch<kMaxBatchFrames> fb;
        std::memset(&fb, 0, sizeof(fb));
        for (uint32_t i = 0; i < rc.nframes; ++i) {
            fb.f[i] = w.fk[i];
            fb.k[i] = w.pk[i];
        }
        return launch_wave_blocks(w.a, w.p, rc.nframes, geo_render_ss_sky_kernel<KIND, kMaxBatchFrames>, fb, o);
    });
}

// A batch's DiskBatchArgs: every frame's constants by the one-frame launch's
// own functions (launch_disk_frame; under GEO_FLAG_SS4 w.fk holds the sample
// frame's camera).  eb (an emission batch): the emission's batch-uniform
// argument, filled too; the frames' sb and ih are then the emission's.
static int fill_disk_batch(const geo_ctx* c, const RenderCall& rc, const RenderWork& w, DiskBatchArgs& db,
                           DiskEmitBatchArgs* eb) {
    std::memset(&db, 0, sizeof(db));
    if (eb) std::memset(eb, 0, sizeof(*eb));
    for (uint32_t i = 0; i < rc.nframes; ++i) {
        const geo_scene& si = traits(rc.entry).scene_per_frame ? rc.scene[i] : *rc.scene;
        DiskFrameK& f = db.f[i];
        geo::DiskConsts dk;
        if (!geo::disk_consts(rc.frames[i].central_to_uv, c->disk.normal, c->disk.axis, c->disk.r_in, c->disk.r_out,
                              w.pk[i], &dk))
            return GEO_EINVAL;
        std::memcpy(f.movement_to_central, w.fk[i].frame.movement_to_central, sizeof(f.movement_to_central));
        std::memcpy(f.central_to_uv, w.fk[i].frame.central_to_uv, sizeof(f.central_to_uv));
        f.psi = w.fk[i].frame.psi_factor_and_position[0];
        f.cam = w.fk[i].cam;
        f.kt = w.fk[i].kt;
        f.k = w.pk[i];
        for (int j = 0; j < 3; ++j) {
            f.N[j] = dk.N[j];
            f.ex[j] = dk.ex[j];
            f.ey[j] = dk.ey[j];
        }
        f.u_lo = dk.u_lo;
        f.u_hi = dk.u_hi;
        if (eb) {
            // the emission takes the shift's place (geo_set_disk_shift's state
            // is not read): sb and ih with the emission's spin, by the
            // one-frame launch's function (emit_args); the rest of it is the
            // same for every frame
            const geo::DiskEmission ek =
                geo::disk_emission_consts(rc.frames[i].central_to_uv, si.rs, si.r_obs, c->emit.spin, c->emit.profile,
                                          c->emit.t_ref, c->emit.t_lo, c->emit.t_hi, c->emit.exposure, c->emit_n);
            f.sb = ek.s.sb;
            f.ih = ek.s.ih;
            eb->inv_fmax = ek.inv_fmax;
            eb->ka = ek.ka;
            eb->kb = ek.kb;
            eb->n1 = ek.n1;
            eb->exposure = ek.exposure;
            eb->profile = ek.profile;
            eb->n2 = ek.n2;
            eb->ramp = c->emit_ramp;
        } else if (c->shift_set) {
            const geo::DiskShift sk = geo::disk_shift_consts(rc.frames[i].central_to_uv, si.rs, si.r_obs,
                                                             c->shift.spin, c->shift.exponent, c->shift.gain);
            f.sb = sk.sb;
            f.ih = sk.ih;
            db.gain = sk.gain;
            db.exponent = sk.exponent;
        }
        if (i == 0) {  // (the same for every frame: the disk, and the scenes' step)
            db.r_in = dk.r_in;
            db.r_out = dk.r_out;
            db.inv_dr = dk.inv_dr;
            db.inv_step = dk.inv_step;
        }
    }
    fill_disk_tex(c, db);
    return GEO_OK;
}

// Stage 5, a batch of GEO_FLAG_DISK frames (geo_render_disk_batch,
// geo_render_ss_batch's disk frames, geo_render_emission_batch,
// geo_render_disk_adaptive_batch, and geo_render_disk_ring_batch and
// geo_render_disk_adaptive_ring_batch with or without a capture orbit to
// draw): geo_render_disk_batch_kernel with the frames in
// grid.z, on the one-frame disk render's wave-block grid, not the plain batch's
// 32 x 8-pixel workgroups: a disk wave holds more registers than a plain one,
// and its frames are compared with one-frame launches wave for wave.
// With a capture orbit, the ring kernels, in the scenes' mode: each frame's
// band constants come from
// the one-frame launch's geo::band_consts (launch_disk_frame), at the sample
// frame's size under GEO_FLAG_SS4, and reach the kernel through the device table
// of the call's render-stream slot (geo_ctx::band_table), written on the call's
// stream by geo_band_table_kernel just before the render launch: no host copy,
// no wait.
static int launch_disk_frames(geo_ctx* c, const RenderCall& rc, const RenderWork& w) {
    DiskBatchArgs db;
    DiskEmitBatchArgs eb;
    if (const int st = fill_disk_batch(c, rc, w, db, w.emit ? &eb : nullptr)) return st;
    const geo::BandConsts* bands = nullptr;
    if (w.disk_ring) {
        BandTable bt;
        std::memset(&bt, 0, sizeof(bt));
        const uint32_t ssf = w.ss ? 2u : 1u;
        for (uint32_t i = 0; i < rc.nframes; ++i)
            bt.k[i] = geo::band_consts(rc.frames[i], traits(rc.entry).scene_per_frame ? rc.scene[i] : *rc.scene,
                                       ssf * rc.width, ssf * rc.height);
        void*& table = c->band_table[w.slot];
        if (!table && hipMalloc(&table, sizeof(BandTable)) != hipSuccess) {
            table = nullptr;
            return GEO_ENOMEM;
        }
        bands = static_cast<const geo::BandConsts*>(table);
        hipLaunchKernelGGL(geo_band_table_kernel, dim3(rc.nframes), dim3(64), 0, w.p.s, bt,
                           static_cast<geo::BandConsts*>(table));
        if (hipGetLastError() != hipSuccess) return GEO_EHIP;
    }
    return with_kind(geo::geodesic_kind(w.a.k), [&](auto kind) {
        return with_shade(w.emit, c->shift_set, [&](auto shade) {
            constexpr int KIND = decltype(kind)::value;
            constexpr Shade SHADE = decltype(shade)::value;
            const ShadeBatchArg<SHADE> x = shade_batch_arg<SHADE>(eb);
            return with_flag(w.ss, [&](auto ss) {
                constexpr bool SS = decltype(ss)::value;
                SsPitch<SS> o;
                if constexpr (SS) o.out_width = rc.width;
                return with_flag(w.adaptive, [&](auto adaptive) {
                    constexpr int MODE = decltype(adaptive)::value ? GEO_MODE_ADAPTIVE : GEO_MODE_DIRECT;
                    if (w.disk_ring) {
                        // (adaptive: geo_render_disk_adaptive_ring_batch alone; the rules refuse the older calls)
                        if constexpr (KIND != geo::kFlat)
                            return launch_wave_blocks(w.a, w.p, rc.nframes,
                                                      geo_render_disk_ring_batch_kernel<KIND, SHADE, SS, MODE>, db,
                                                      bands, x, o);
                        return (int)GEO_EINVAL;  // (never reached: the state is ignored for rs = 0)
                    }
                    return launch_wave_blocks(w.a, w.p, rc.nframes, geo_render_disk_batch_kernel<KIND, SHADE, SS, MODE>,
                                              db, x, o);
                });
            });
        });
    });
}

// Stage 5: the launch.
static int launch_render(geo_ctx* c, const RenderCall& rc, const RenderWork& w) {
    switch (choose_launcher(rc, w)) {
        // (what the batched disk launchers differ in, the launch reads from w:
        // the shade, SS4, the integrator and whether there is a band to draw)
        case Launcher::kAdaptiveFrames:
        case Launcher::kRingFrames:
        case Launcher::kEmitFrames:
        case Launcher::kDiskFrames: return launch_disk_frames(c, rc, w);
        case Launcher::kSsFrames: return w.disk ? launch_disk_frames(c, rc, w) : launch_ss_sky(rc, w, true);
        case Launcher::kSsFrame: return w.disk ? launch_disk_frame(c, rc, w) : launch_ss_sky(rc, w, false);
        case Launcher::kDiskFrame: return launch_disk_frame(c, rc, w);
        case Launcher::kFan: return launch_fan(c, rc, w);
        case Launcher::kFrames: break;
    }
    geo::BandConsts band_k;  // (one frame; a batch derives its frames' constants on the device)
    if (w.ring && rc.nframes == 1) band_k = geo::band_consts(rc.frames[0], *rc.scene, rc.width, rc.height);
    return with_kind(geo::geodesic_kind(w.a.k), [&](auto kind) {
        constexpr int KIND = decltype(kind)::value;
        // (kFlat has no capture orbit: its launch takes no band)
        const geo::BandConsts* band = w.ring && KIND != geo::kFlat ? &band_k : nullptr;
        return w.adaptive
                   ? launch_frames<GEO_MODE_ADAPTIVE, KIND>(w.a, w.fk, w.pk, rc.nframes, w.mips, w.p, band)
                   : launch_frames<GEO_MODE_DIRECT, KIND>(w.a, w.fk, w.pk, rc.nframes, w.mips, w.p, band);
    });
}

// Stage 6: a recording render's order rebuild, and the fold of a per-call
// step-counter set into the caller's total.
static int finish_render(geo_ctx* c, const RenderCall& rc, const RenderWork& w) {
    if (w.record) {
        // rebuild the order into the buffer not in use, on the context's
        // learn stream, after every render of the context issued so far (this
        // one included: its launch recorded render_done[slot]); earlier
        // renders on any stream may still read that buffer
        ++c->costs_recorded;
        if (!c->learn_stream && hipStreamCreateWithFlags(&c->learn_stream, hipStreamNonBlocking) != hipSuccess) {
            c->learn_stream = nullptr;
            return GEO_EHIP;
        }
        hipStream_t ls = c->learn_stream;
        const int nb = c->order_cur < 0 ? 0 : 1 - c->order_cur;
        for (int i = 0; i < c->n_render_streams; ++i)
            if (hipStreamWaitEvent(ls, c->render_done[i], 0) != hipSuccess) return GEO_EHIP;
        const uint32_t n = w.p.tiles_x * w.p.tiles_y;
        const uint32_t chunks = (n + kOrderChunk - 1) / kOrderChunk;
        hipLaunchKernelGGL(geo_order_hist, dim3(chunks), dim3(256), 0, ls, c->tile_cost, n, c->class_hist);
        hipLaunchKernelGGL(geo_order_scatter, dim3(chunks), dim3(256), 0, ls, c->tile_cost, n, c->class_hist,
                           w.p.tiles_x, c->order[nb]);
        if (hipGetLastError() != hipSuccess) return GEO_EHIP;
        if (hipEventRecord(c->order_written, ls) != hipSuccess) return GEO_EHIP;
        c->rebuild_pending = true;
        c->rebuild_keep = true;
        c->rebuild_nb = nb;
    }
    if (w.call_set >= 0) {
        hipLaunchKernelGGL(geo_steps_finalize, dim3(1), dim3(kStepSlots), 0, w.p.s, w.a.step_slots, rc.steps_total);
        if (hipGetLastError() != hipSuccess) return GEO_EHIP;
        if (hipEventRecord(c->step_set_free[w.call_set], w.p.s) != hipSuccess) return GEO_EHIP;
        c->step_set_rec[w.call_set] = true;
    }
    return GEO_OK;
}

static int render_impl(geo_ctx* c, const RenderCall& rc) {
    RenderWork w;
    // geo_time_next_render's events belong to this render alone, on every
    // exit path: a call that fails validation drops them (a later render
    // must not record the caller's pair)
    w.p.t_start = c->time_start;
    w.p.t_stop = c->time_stop;
    c->time_start = c->time_stop = nullptr;
    // geo_disk_hits_next_render's buffer likewise, and geo_disk_shift_next_render's
    w.out_hits = c->hits_next;
    c->hits_next = nullptr;
    w.out_g = c->g_next;
    c->g_next = nullptr;
    w.out_q = c->q_next;
    c->q_next = nullptr;
    int st = check_scene(rule_state(c), rc, w);
    if (st) return st;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    if ((st = fill_frames(rc, w))) return st;
    fill_args(c, rc, w);
    w.p.s = (hipStream_t)rc.stream;
    if ((st = take_step_set(c, rc, w))) return st;
    w.slot = render_slot(c, w.p.s);
    if (w.slot < 0) return GEO_EHIP;
    w.p.done = c->render_done[w.slot];
    if ((st = choose_order(c, rc, w))) return st;
    if ((st = launch_render(c, rc, w))) return st;
    return finish_render(c, rc, w);
}

int geo_assemble_bands(geo_ctx* c, const uint8_t* src, size_t rank_stride, size_t frame_stride, uint32_t world,
                       uint32_t band_rows, uint32_t width, uint32_t height, uint32_t nframes, uint32_t src_bpp,
                       uint8_t* dst, void* stream) {
    if (!c || !src || !dst || world == 0 || band_rows == 0 || width == 0 || height == 0 || nframes == 0 ||
        height > 65535u || nframes > 65535u || (src_bpp != 3u && src_bpp != 4u))
        return GEO_EINVAL;
    if (src_bpp == 3u && (width % 4u != 0 || rank_stride % 4u != 0 || frame_stride % 4u != 0 ||
                          (uintptr_t)src % 4u != 0 || (uintptr_t)dst % 16u != 0))
        return GEO_EINVAL;
    const size_t row_bytes = (size_t)width * src_bpp;
    const size_t nb_max = ((size_t)(height + band_rows - 1) / band_rows + world - 1) / world;
    if (frame_stride < nb_max * band_rows * row_bytes || rank_stride < (size_t)nframes * frame_stride)
        return GEO_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    hipStream_t s = (hipStream_t)stream;
    if (src_bpp == 3u) {
        const uint32_t quads = width / 4u;
        hipLaunchKernelGGL(geo_assemble_rgb_kernel, dim3((quads + 255u) / 256u, height, nframes), dim3(256), 0, s,
                           src, rank_stride, frame_stride, world, band_rows, quads, height, dst);
        return hipGetLastError() == hipSuccess ? GEO_OK : GEO_EHIP;
    }
    const bool wide = (width % 4u) == 0 && (rank_stride % 16u) == 0 && (frame_stride % 16u) == 0 &&
                      ((uintptr_t)src % 16u) == 0 && ((uintptr_t)dst % 16u) == 0;
    const uint32_t units = wide ? width / 4u : width;
    const dim3 grid((units + 255u) / 256u, height, nframes);
    if (wide)
        hipLaunchKernelGGL(geo_assemble_kernel<uint4>, grid, dim3(256), 0, s, src, rank_stride, frame_stride, world,
                           band_rows, units, height, dst);
    else
        hipLaunchKernelGGL(geo_assemble_kernel<uint32_t>, grid, dim3(256), 0, s, src, rank_stride, frame_stride,
                           world, band_rows, units, height, dst);
    return hipGetLastError() == hipSuccess ? GEO_OK : GEO_EHIP;
}

int geo_assemble_shares(geo_ctx* c, const uint8_t* lead_src, size_t lead_frame_stride, uint32_t lead_rows,
                        const uint8_t* src, size_t rank_stride, size_t frame_stride, uint32_t world,
                        uint32_t band_rows, uint32_t width, uint32_t height, uint32_t nframes, uint32_t src_bpp,
                        uint8_t* dst, void* stream) {
    if (!c || !lead_src || !dst || world == 0 || lead_rows == 0 || band_rows == 0 || width == 0 || height == 0 ||
        nframes == 0 || height > 65535u || nframes > 65535u || (src_bpp != 3u && src_bpp != 4u))
        return GEO_EINVAL;
    // 16-B units need width % 4 == 0 and aligned buffers; RGB24 peers need them
    const size_t lead_align = width % 4u == 0 ? 16u : 4u;
    if (src_bpp == 3u && width % 4u != 0) return GEO_EINVAL;
    if ((uint64_t)lead_rows + (uint64_t)(world - 1u) * band_rows > (1u << 20)) return GEO_EINVAL;
    const uint32_t cycle = lead_rows + (world - 1u) * band_rows;
    // rank 0 has ceil(H / cycle) bands; rank 1, the first peer, the most of the peers
    const size_t nb0 = (height + cycle - 1u) / cycle;
    const size_t nb1 = height > lead_rows ? (height - lead_rows + cycle - 1u) / cycle : 0;
    if (lead_frame_stride < nb0 * lead_rows * (size_t)width * 4u) return GEO_EINVAL;
    if (lead_frame_stride % lead_align != 0 || (uintptr_t)lead_src % lead_align != 0 ||
        (uintptr_t)dst % lead_align != 0)
        return GEO_EINVAL;
    if (world > 1u) {
        if ((nb1 > 0 && !src) || frame_stride < nb1 * band_rows * (size_t)width * src_bpp ||
            rank_stride < (size_t)nframes * frame_stride)
            return GEO_EINVAL;
        const size_t align = src_bpp == 4u ? lead_align : 4u;
        if (rank_stride % align != 0 || frame_stride % align != 0 || (uintptr_t)src % align != 0) return GEO_EINVAL;
    }
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    hipStream_t s = (hipStream_t)stream;
    if (width % 4u == 0) {
        const uint32_t quads = width / 4u;
        hipLaunchKernelGGL(geo_assemble_lead_kernel<true>, dim3((quads + 255u) / 256u, height, nframes), dim3(256),
                           0, s, lead_src, lead_frame_stride, lead_rows, src, rank_stride, frame_stride, world,
                           band_rows, quads, height, src_bpp, dst);
    } else {
        hipLaunchKernelGGL(geo_assemble_lead_kernel<false>, dim3((width + 255u) / 256u, height, nframes), dim3(256),
                           0, s, lead_src, lead_frame_stride, lead_rows, src, rank_stride, frame_stride, world,
                           band_rows, width, height, src_bpp, dst);
    }
    return hipGetLastError() == hipSuccess ? GEO_OK : GEO_EHIP;
}

int geo_assemble_lead(geo_ctx* c, const uint8_t* lead_src, size_t lead_frame_stride, uint32_t lead,
                      const uint8_t* src, size_t rank_stride, size_t frame_stride, uint32_t world,
                      uint32_t band_rows, uint32_t width, uint32_t height, uint32_t nframes, uint32_t src_bpp,
                      uint8_t* dst, void* stream) {
    if (lead == 0 || (uint64_t)lead * band_rows > (1u << 20)) return GEO_EINVAL;
    return geo_assemble_shares(c, lead_src, lead_frame_stride, lead * band_rows, src, rank_stride, frame_stride,
                               world, band_rows, width, height, nframes, src_bpp, dst, stream);
}

int geo_pack_rgb(geo_ctx* c, const uint8_t* rgba, uint64_t npixels, uint8_t* rgb, void* stream) {
    if (!c || !rgba || !rgb || npixels == 0 || npixels % 4u != 0 || (uintptr_t)rgba % 16u != 0 ||
        (uintptr_t)rgb % 4u != 0)
        return GEO_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    const uint64_t quads = npixels / 4u;
    hipLaunchKernelGGL(geo_pack_rgb_kernel, dim3((unsigned)((quads + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(rgba), quads, reinterpret_cast<uint32_t*>(rgb));
    return hipGetLastError() == hipSuccess ? GEO_OK : GEO_EHIP;
}

int geo_steps_flush(geo_ctx* c, unsigned long long* steps_total, void* stream) {
    if (!c || !steps_total) return GEO_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    const hipEvent_t done = render_event(c, (hipStream_t)stream);
    if (!done) return GEO_EHIP;
    hipExtLaunchKernelGGL(geo_steps_finalize, dim3(1), dim3(kStepSlots), 0, (hipStream_t)stream, nullptr, done, 0,
                          c->step_slots, steps_total);
    return hipGetLastError() == hipSuccess ? GEO_OK : GEO_EHIP;
}

int geo_time_next_render(geo_ctx* c, void* start_event, void* stop_event) {
    if (!c || !start_event || !stop_event) return GEO_EINVAL;
    c->time_start = (hipEvent_t)start_event;
    c->time_stop = (hipEvent_t)stop_event;
    return GEO_OK;
}

int geo_set_dispatch(geo_ctx* c, int mode, uint32_t period) {
    if (!c || (mode != GEO_DISPATCH_ROW_MAJOR && mode != GEO_DISPATCH_LONGEST_FIRST) || period == 0 ||
        period > (1u << 20))
        return GEO_EINVAL;
    c->dispatch_mode = mode;
    c->dispatch_period = period;
    c->learn_valid = false;  // learn again from the next render
    c->order_cur = -1;
    c->rebuild_keep = false;
    return GEO_OK;
}

#if defined(GEO_WAVE_LOG)
// Diagnostic build only: renders log every wave's span into `log` (4 u64 per
// wave of the launch's grid, device memory; NULL stops logging).
int geo_debug_set_wave_log(geo_ctx* c, void* log) {
    if (!c) return GEO_EINVAL;
    c->wave_log = (unsigned long long*)log;
    return GEO_OK;
}

// Diagnostic build only: out[0], out[1] = the waves that took the kTestLow and
// the kTestEnd loop since the last call (after a device synchronisation).
extern "C" int geo_debug_loop_waves(geo_ctx* c, unsigned long long* out) {
    if (!c || !out) return GEO_EINVAL;
    const unsigned long long zero[2] = {0, 0};
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_waves), sizeof zero) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_loop_waves), zero, sizeof zero) != hipSuccess)
        return GEO_EINVAL;
    return GEO_OK;
}
#endif

int geo_dispatch_stats(geo_ctx* c, unsigned long long* costs_recorded, unsigned long long* orders_adopted) {
    if (!c) return GEO_EINVAL;
    if (costs_recorded) *costs_recorded = c->costs_recorded;
    if (orders_adopted) *orders_adopted = c->orders_adopted;
    return GEO_OK;
}

int geo_set_tile_order(geo_ctx* c, uint32_t tiles_x, uint32_t tiles_y, const uint32_t* order) {
    if (!c) return GEO_EINVAL;
    DeviceGuard g(c->device);
    if (!g.ok) return GEO_EHIP;
    if (!order) {  // row-major
        c->dispatch_mode = GEO_DISPATCH_ROW_MAJOR;
        c->learn_valid = false;
        c->order_cur = -1;
        c->rebuild_keep = false;
        return GEO_OK;
    }
    if (tiles_x == 0 || tiles_y == 0 || tiles_x > 0xFFFFu || tiles_y > kMaxGridY) return GEO_EINVAL;
    const size_t n = (size_t)tiles_x * tiles_y;
    if (n > 0xFFFFFFFFu) return GEO_EINVAL;
    std::vector<uint8_t> seen(n, 0);  // a permutation of the grid's tiles
    for (size_t i = 0; i < n; ++i) {
        const uint32_t x = order[i] & 0xFFFFu, y = order[i] >> 16;
        if (x >= tiles_x || y >= tiles_y || seen[(size_t)y * tiles_x + x]) return GEO_EINVAL;
        seen[(size_t)y * tiles_x + x] = 1;
    }
    int st = ensure_tiles(c, (uint32_t)n);
    if (st) return st;
    // renders in flight may read either buffer, a rebuild may write one
    if (wait_renders(c) != GEO_OK || hipEventSynchronize(c->order_written) != hipSuccess) return GEO_EHIP;
    c->rebuild_pending = false;
    if (hipMemcpy(c->order[0], order, n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        c->order_cur = -1;
        return GEO_EHIP;
    }
    c->dispatch_mode = GEO_DISPATCH_EXPLICIT;
    c->explicit_x = tiles_x;
    c->explicit_y = tiles_y;
    c->order_cur = 0;
    c->learn_valid = false;
    return GEO_OK;
}

// The one-frame entry points: the argument stage (frame_call; g0 .. g3 are the
// entry point's own row arguments), then the render.
static int render_frame(Entry e, geo_ctx* c, const geo_frame* frame, const geo_scene* scene, uint32_t width,
                        uint32_t height, uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3, uint8_t* out_rgba8,
                        uint8_t* out_mask, float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                        void* stream) {
    RenderCall rc;
    if (!frame_call(rc, e, c, frame, scene, width, height, g0, g1, g2, g3, out_rgba8, out_mask, out_uv, out_steps,
                    steps_total, stream))
        return invalid_call(c);
    return render_impl(c, rc);
}

// The batched entry points likewise (batch_call).
static int render_batch(Entry e, geo_ctx* c, const geo_frame* frames, const geo_scene* scenes, uint32_t nframes,
                        uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0, uint32_t row_stride,
                        uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride, unsigned long long* steps_total,
                        void* stream) {
    RenderCall rc;
    if (!batch_call(rc, e, c, frames, scenes, nframes, width, height, band_rows, row0, row_stride, nbands, out_rgba8,
                    out_frame_stride, steps_total, stream))
        return invalid_call(c);
    return render_impl(c, rc);
}

int geo_render_rows(geo_ctx* c, const geo_frame* frame, const geo_scene* scene, uint32_t width, uint32_t height,
                    uint32_t row0, uint32_t nrows, uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv,
                    uint32_t* out_steps, unsigned long long* steps_total, void* stream) {
    return render_frame(Entry::kRows, c, frame, scene, width, height, row0, nrows, 0, 0, out_rgba8, out_mask, out_uv,
                        out_steps, steps_total, stream);
}

int geo_render_bands(geo_ctx* c, const geo_frame* frame, const geo_scene* scene, uint32_t width, uint32_t height,
                     uint32_t band_rows, uint32_t band0, uint32_t band_step, uint32_t nbands, uint8_t* out_rgba8,
                     uint8_t* out_mask, float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                     void* stream) {
    return render_frame(Entry::kBands, c, frame, scene, width, height, band_rows, band0, band_step, nbands, out_rgba8,
                        out_mask, out_uv, out_steps, steps_total, stream);
}

int geo_render_band_set(geo_ctx* c, const geo_frame* frame, const geo_scene* scene, uint32_t width, uint32_t height,
                        uint32_t band_rows, uint32_t row0, uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8,
                        uint8_t* out_mask, float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                        void* stream) {
    return render_frame(Entry::kBandSet, c, frame, scene, width, height, band_rows, row0, row_stride, nbands,
                        out_rgba8, out_mask, out_uv, out_steps, steps_total, stream);
}

int geo_render_disk_adaptive(geo_ctx* c, const geo_frame* frame, const geo_scene* scene, uint32_t width,
                             uint32_t height, uint32_t band_rows, uint32_t row0, uint32_t row_stride, uint32_t nbands,
                             uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv, uint32_t* out_steps,
                             unsigned long long* steps_total, void* stream) {
    return render_frame(Entry::kDiskAdaptive, c, frame, scene, width, height, band_rows, row0, row_stride, nbands,
                        out_rgba8, out_mask, out_uv, out_steps, steps_total, stream);
}

int geo_render_disk_adaptive_ring(geo_ctx* c, const geo_frame* frame, const geo_scene* scene, uint32_t width,
                                  uint32_t height, uint32_t band_rows, uint32_t row0, uint32_t row_stride,
                                  uint32_t nbands, uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv,
                                  uint32_t* out_steps, unsigned long long* steps_total, void* stream) {
    return render_frame(Entry::kDiskAdaptiveRing, c, frame, scene, width, height, band_rows, row0, row_stride, nbands,
                        out_rgba8, out_mask, out_uv, out_steps, steps_total, stream);
}

int geo_render_band_set_frames(geo_ctx* c, const geo_frame* frames, uint32_t nframes, const geo_scene* scene,
                               uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0, uint32_t row_stride,
                               uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                               unsigned long long* steps_total, void* stream) {
    return render_batch(Entry::kBandSetFrames, c, frames, scene, nframes, width, height, band_rows, row0, row_stride,
                        nbands, out_rgba8, out_frame_stride, steps_total, stream);
}

// The batched entry points of geo_render_band_set_batch's prototype: scenes[f] belongs to frames[f].
#define GEO_BATCH_ENTRY(name, entry)                                                                                 \
    int name(geo_ctx* c, const geo_frame* frames, const geo_scene* scenes, uint32_t nframes, uint32_t width,        \
             uint32_t height, uint32_t band_rows, uint32_t row0, uint32_t row_stride, uint32_t nbands,              \
             uint8_t* out_rgba8, size_t out_frame_stride, unsigned long long* steps_total, void* stream) {          \
        return render_batch(entry, c, frames, scenes, nframes, width, height, band_rows, row0, row_stride, nbands,  \
                            out_rgba8, out_frame_stride, steps_total, stream);                                      \
    }
GEO_BATCH_ENTRY(geo_render_band_set_batch, Entry::kBandSetBatch)
GEO_BATCH_ENTRY(geo_render_disk_batch, Entry::kDiskBatch)
GEO_BATCH_ENTRY(geo_render_ss_batch, Entry::kSsBatch)
GEO_BATCH_ENTRY(geo_render_emission_batch, Entry::kEmissionBatch)
GEO_BATCH_ENTRY(geo_render_disk_ring_batch, Entry::kDiskRingBatch)
GEO_BATCH_ENTRY(geo_render_disk_adaptive_batch, Entry::kDiskAdaptiveBatch)
GEO_BATCH_ENTRY(geo_render_disk_adaptive_ring_batch, Entry::kDiskAdaptiveRingBatch)
#undef GEO_BATCH_ENTRY

}  // extern "C"
