// geo_render_kernels.h — the gfx950 kernels of geo_render.hip (its device half;
// the C ABI and the launchers are there).
//
//   geo_render_kernel<MODE>  per-pixel fs_main + solve_geodesic (fixed RK4, fan lerp,
//                            or error-controlled RK5(4): GEO_MODE_ADAPTIVE)
//                            (SR/schwarzschild_sphere_shader/shader.wgsl:57-106,
//                             SR/simulation/sphere_ray_tracer.rs:35-193)
//   geo_fan_kernel           SphereRayTracer::solve_ray_fan in f64, one lane per node
//                            (sphere_ray_tracer.rs:35-193)
//   geo_steps_finalize       folds the sharded step counters into the caller's u64
//
// Work decomposition: one 256-thread workgroup per 32x8 pixel tile, each
// wave64 a 16x4 block (compact 2-D footprint = coherent step counts), 2 x 2
// of them (a tile row spans one 128-B sky line);
// the frame uniform rides in the kernarg segment (SGPRs, wave-uniform), the
// ray fan (fan mode) is read from its cache-resident device copy; per-lane
// ray state lives in VGPRs.  The hot loop
// is pure FP32 VALU — no MFMA, no LDS, no memory traffic.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/geo/geo.h"
#if defined(GEO_WAVE_LOG)
// Diagnostic build only: waves of the direct-mode loop by the exit test they
// take ([0] kTestLow, [1] kTestEnd; geo_pixel.h), counted by each wave's first
// live lane (geo_debug_loop_waves reads and clears them).
static __device__ unsigned long long g_loop_waves[2];
#define GEO_LOOP_COUNT(end_test)                                                              \
    do {                                                                                      \
        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) ==             \
            (unsigned)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true)))                     \
            atomicAdd(&g_loop_waves[(end_test) ? 1 : 0], 1ull);                               \
    } while (0)
#endif
#include "geo_ctx.h"
#include "geo_band.h"
#include "geo_disk.h"
#include "geo_pixel.h"

static_assert(geo::kDiskGMax == GEO_DISK_G_MAX, "geo.h announces the header's clamp");

// Work decomposition (measured): 32 x 8-pixel workgroup tiles
// of 2 x 2 waves of 16 x 4 pixels.  A tile row spans 32 sky texels = one
// 128-B line, so neighbouring waves share their sky lines in one CU instead of
// fetching them on up to 4 XCDs' L2s (102.8 -> 59.5 MB of L2 fabric reads per
// 4K frame against 8 x 32 tiles; config 3 -2 to -5 %, config 5 -2 %, config 2
// -1.5 %; 16 x 16, 64 x 8 and 32 x 16 in between); the 16 x 4 wave shape is
// -0.5 % on config 3 against 8 x 8, 32 x 2 is +2.5 % (steps diverge more
// within a wave).  Tiles keep the hardware's round-robin placement over the
// XCDs: runs of consecutive tiles per XCD were slower on every config.  The
// fan (fan mode) is read from its cache-resident device copy: staging it in
// LDS per workgroup put a load and a barrier before every block's pixel work
// (+6 % per 4K fan-mode frame).

namespace {

constexpr int kWaveW = 16;             // a wave64 covers a compact 16x4 block (few divergent
constexpr int kWaveRows = 64 / kWaveW;  // steps per wave; tools/ubench/loop_ab.hip at 3cd1aa2)
constexpr int kWavesX = 2;              // waves side by side in a tile
constexpr int kTileW = kWaveW * kWavesX;
constexpr int kTileH = 8;               // a block kTileW x kTileH
constexpr int kBlock = kTileW * kTileH;  // 256 threads = 4 waves (32 x 8, 2 x 2 waves of 16 x 4;
                                         // twice as tall with two pixels per lane, lane_rows)
static_assert(kTileH % kWaveRows == 0 && kBlock % 64 == 0, "tile of whole waves");
// band heights are multiples of 8 (the C-ABI's contract, geo.h), so a wave's
// rows never straddle a band for any wave shape up to 8 rows
constexpr uint32_t kBandRowAlign = 8;
static_assert(kBandRowAlign % kWaveRows == 0, "a wave's rows lie in one band");
constexpr uint32_t kMaxFan = 4096;       // fan nodes (16 KiB)
constexpr uint32_t kDefaultDispatchPeriod = 16;  // renders of a grid per re-learned order
// a tile's out-of-loop work in steps of its mode's loop (the set-up, Newton
// crossing and sky epilogue: ~330 VALU against 14 per RK4 step, ~420 against
// ~57 per RK5(4) attempt), added to each wave's recorded cost
constexpr uint32_t kCostOverheadDirect = 24, kCostOverheadAdaptive = 8;
constexpr int kStepSlots = 256;          // sharded step counters (one per 128-B line)
constexpr int kSlotStride = 16;          // u64 per slot = 128 B (own cache line)
constexpr size_t kSlotSetU64 = (size_t)kStepSlots * kSlotStride;  // one set of sharded counters
constexpr int kSlotSets = 1 + geo_ctx::kStepCallSets;            // the DEFER accumulator + per-call sets

// The per-frame part of a launch: the uniform and the camera constants the
// host derives from it (a second kernel argument, FrameBatch, one per frame
// of a batched launch, geo_render_band_set_frames).
struct FrameK {
    geo_frame frame;
    geo::CameraConsts cam;  // the pixel's camera ray (geo::camera_consts)
    float kt;               // geo::aberration_kt
};
constexpr uint32_t kMaxBatchFrames = GEO_MAX_BATCH_FRAMES;
// A batch's frames may each have their own observer radius (their scenes
// differ in r_obs only, geo_render_band_set_batch): the scene constants of
// each frame ride along (the integration kind is shared); a single-frame
// launch reads RenderArgs::k.
template <uint32_t NF>
struct FrameBatch {
    FrameK f[NF];
    geo::PixelConsts k[NF];
    float ring_kx[NF];  // GEO_FLAG_RING_F64: frame z's band factor (geo::band_kx; 0: no band)
};
template <>
struct FrameBatch<1> {
    FrameK f[1];
};

struct RenderArgs {
    geo::PixelConsts k;  // scene constants, evaluated once on the host (IEEE f32, same bits)
    uint32_t width, height, row0, nrows;
    uint32_t tile_y0;  // first tile row of this launch (launch_tiles)
    uint32_t tiles_x, launch_tiles;  // the frame's tiles per row; the tiles of this launch (wave_blocks)
    // dispatch order (geo_ctx): workgroup i draws tile
    // (order[i] & 0xFFFF, order[i] >> 16); null = row-major
    const uint32_t* tile_order;
    // a cost-recording render: each wave adds its largest step count plus
    // cost_overhead (its out-of-loop work, in steps) into its tile's entry
    unsigned int* tile_cost;
    uint32_t cost_overhead;
    // local row lr -> row0 + b*band_stride + (lr - b*band_rows), b = lr / band_rows
    // = umulhi(lr, band_magic) (band_rows_magic)
    uint32_t band_rows, band_magic, band_stride;
    uint32_t sky_opaque;
    uint32_t composite;  // GEO_FLAG_COMPOSITE
    const uint32_t* sky;  // padded (geo::pad_sky): (sky_w + 2) x (sky_h + 2) texels
    uint32_t sky_w, sky_h;
    float sky_w256, sky_h256;  // sky_w * 256, sky_h * 256 (exact; geo::sample_sky_quad_f)
    uint32_t sky_pitch_b, sky_bytes;
    // GEO_FLAG_MIPS: level l's byte offset, pitch and sizes * 256; level 0's
    // size for the footprint; the whole chain's bytes
    uint32_t mip_off[geo::kSkyMipLevels], mip_pitch[geo::kSkyMipLevels];
    float mip_w256[geo::kSkyMipLevels], mip_h256[geo::kSkyMipLevels];
    float sky_wf, sky_hf;
    uint32_t sky_total_bytes;
    const float* fan;
    uint32_t n_fan;
    uint32_t* out_rgba;
    uint8_t* out_mask;
    float2* out_uv;
    uint32_t* out_steps;
    unsigned long long* step_slots;
    uint64_t out_frame_px;  // batched launch: pixels from one frame's output to the next (colour only)
#if defined(GEO_WAVE_LOG)
    // diagnostic build only (tools/wave_timeline.py): per wave, in launch
    // order, {start, end} (s_memrealtime, 100 MHz), {HW_ID, XCC_ID}, {tile,
    // the wave's largest step count}
    unsigned long long* wave_log;
#endif
};

// MODE: GEO_MODE_DIRECT / GEO_MODE_FAN / GEO_MODE_ADAPTIVE; KIND: geo::kCurvedOut/kCurvedIn/kFlat
// (frame-uniform integration kind, geo::geodesic_kind; ignored in fan mode).
// Max of v over the 64 lanes of a fully active wave (the same DPP scan).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Sum of v over the 64 lanes of a fully active wave (DPP inclusive scan:
// row_shr 1/2/4/8 within rows of 16, then row_bcast 15/31; lane 63 holds it).
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The texel quad from the context's padded sky (geo::pad_sky): the 2 x 2 block
// at padded texel (ix0 + 1, iy0 + 1), by four buffer loads from one 32-bit
// byte offset (one v_mad_u32_u24): +4 B for the right column as the immediate
// offset, +pitch for the lower row as the scalar offset.  Against the wrap/clamp
// quad on the unpadded texture this drops the wrap and clamp selects, the
// quarter-rate v_mul_lo_u32 row products and the 64-bit address adds; the
// texels are the same (geo_set_sky limits the padded sky to < 2^31 bytes).
constexpr int kBufferRsrcWord3 = 0x00020000;  // gfx9 buffer resource: raw 32-bit dwords
struct PaddedSkyQuad {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t pitch_b;  // bytes per padded row, (sky_w + 2) * 4
    __device__ __forceinline__ void operator()(int ix0, int iy0, uint32_t (&t)[4]) const {
        const uint32_t off = __umul24((uint32_t)(iy0 + 1), pitch_b) + ((uint32_t)(ix0 + 1) << 2);
        t[0] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0);
        t[1] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 4u, 0, 0);
        t[2] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, (int)pitch_b, 0);
        t[3] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 4u, (int)pitch_b, 0);
    }
};

// Tried: level 0 also stored as row pairs (geo::pair_sky_rows), a quad in one
// 16-byte load.  The fan draw -0.5 to -1 %, config 3 +0.2 to +0.8 %, the ring
// overhead up by half a point, for a second copy of level 0: not kept
// (profiles/r06zk_sky_pairs_ab.txt, profiles/r06zl_sky_pairs_ab.txt).
__device__ __forceinline__ PaddedSkyQuad level0_quad(const RenderArgs& a) {
    return PaddedSkyQuad{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.sky), 0, (int)a.sky_bytes,
                                                           kBufferRsrcWord3),
                         a.sky_pitch_b};
}

// The texel quad of one mip level of the padded chain (geo_ctx::sky): like
// PaddedSkyQuad at a per-lane level, so base and pitch are vector values.
struct LevelQuad {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t base, pitch_b;
    __device__ __forceinline__ void operator()(int ix0, int iy0, uint32_t (&t)[4]) const {
        const uint32_t off = base + __umul24((uint32_t)(iy0 + 1), pitch_b) + ((uint32_t)(ix0 + 1) << 2);
        t[0] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0);
        t[1] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 4u, 0, 0);
        t[2] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + pitch_b, 0, 0);
        t[3] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + pitch_b + 4u, 0, 0);
    }
};

template <typename T>
__device__ __forceinline__ T level_sel(const T (&v)[geo::kSkyMipLevels], uint32_t l) {
    static_assert(geo::kSkyMipLevels == 4, "four levels");
    return l == 0u ? v[0] : (l == 1u ? v[1] : (l == 2u ? v[2] : v[3]));
}

// The trilinear sample (GEO_FLAG_MIPS, geo_pixel.h): levels floor(lambda) and
// the next, blended with frac(lambda) in 8 bits.  A zero weight returns
// level floor(lambda) alone: mip_blend(s0, s1, 0) == s0 bit for bit (each
// channel (256 s0 + 128) >> 8), so the second level is fetched only under the
// lanes that blend.  A wave magnified everywhere (rho2 <= 1, so lambda = 0,
// on every active lane: most of a 4K frame of a 4096 x 2048 sky) skips the
// level of detail and samples level 0 with its base and pitch as scalars, as
// the level-0 path does.
__device__ __forceinline__ uint32_t sample_trilinear(const RenderArgs& a, float rho2, float U, float V) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.sky), 0,
                                                                           (int)a.sky_total_bytes, kBufferRsrcWord3);
    if (geo::ballot_(rho2 > 1.0f) == 0)  // lod_q8 is 0 unless rho2 > 1
        return geo::sample_sky_quad_f(LevelQuad{rsrc, a.mip_off[0], a.mip_pitch[0]}, a.mip_w256[0], a.mip_h256[0], U,
                                      V);
    const uint32_t q = geo::lod_q8(rho2);
    const uint32_t l0 = q >> 8, f = q & 255u;
    const uint32_t s0 = geo::sample_sky_quad_f(LevelQuad{rsrc, level_sel(a.mip_off, l0), level_sel(a.mip_pitch, l0)},
                                               level_sel(a.mip_w256, l0), level_sel(a.mip_h256, l0), U, V);
    if (f == 0u) return s0;
    const uint32_t l1 = l0 + 1u < (uint32_t)geo::kSkyMipLevels ? l0 + 1u : l0;
    const uint32_t s1 = geo::sample_sky_quad_f(LevelQuad{rsrc, level_sel(a.mip_off, l1), level_sel(a.mip_pitch, l1)},
                                               level_sel(a.mip_w256, l1), level_sel(a.mip_h256, l1), U, V);
    return geo::mip_blend(s0, s1, f);
}

// The value of v in lane ^ 1 (DPP quad_perm [1, 0, 3, 2]) and in lane ^ 16
// (ds_swizzle, bit mode: and 0x1F, xor 0x10, within 32-lane halves): the
// x and y partners of the pixel's 2 x 2 quad in the 16 x 4 wave.
__device__ __forceinline__ float lane_xor1(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_xor16(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));
}

// Epilogue of one pixel (shader.wgsl:88-105): black-hole test, sky UV,
// bilinear sample, blend and the optional outputs at index o.
// bh: the mask (lam < -7, or the band's f64 decision, GEO_FLAG_RING_F64).
__device__ __forceinline__ void shade_pixel_bh(const RenderArgs& a, const float* central_to_uv, float c2x, float c2y,
                                               float ct, float rct, float lam, bool bh, uint32_t steps, size_t o) {
    // A black-hole pixel is discarded (shader.wgsl:88): it needs its UV
    // only when the caller asks for it, so a wave inside the shadow skips
    // the sincos/atan2/asin and the sample (config 3 -0.3 %, config 5 -4.4 %)
    float U = 0.0f, V = 0.0f;
    if (!bh || a.out_uv)
        geo::sky_uv(central_to_uv, c2x, c2y, ct, rct, lam, &U, &V);
    const auto quad = level0_quad(a);
    if (a.composite) {
        // over the previous spheres; a discarded pixel keeps the target
        if (!bh) {
            const uint32_t s = geo::sample_sky_quad_f(quad, a.sky_w256, a.sky_h256, U, V);
            a.out_rgba[o] = a.sky_opaque ? s : geo::composite_(s, a.out_rgba[o]);
        }
    } else {
        a.out_rgba[o] = bh ? geo::kBlackRGBA : geo::sample_sky_qf(quad, a.sky_w256, a.sky_h256, a.sky_opaque != 0, U, V);
    }
    if (a.out_mask) a.out_mask[o] = bh ? 1 : 0;
    if (a.out_uv) a.out_uv[o] = make_float2(U, V);
    if (a.out_steps) a.out_steps[o] = steps;
}
__device__ __forceinline__ void shade_pixel(const RenderArgs& a, const float* central_to_uv, float c2x, float c2y,
                                            float ct, float rct, float lam, uint32_t steps, size_t o) {
    shade_pixel_bh(a, central_to_uv, c2x, c2y, ct, rct, lam, lam < geo::kBlackHoleLambda, steps, o);
}

// GEO_FLAG_RING_F64's kernel argument: the band's f64 constants (geo_band.h);
// empty in the other instantiations.
template <bool RING>
struct BandArg {};
template <>
struct BandArg<true> {
    geo::BandConsts k;
};
// The band's constants reach the band's lanes through LDS: the kernel copies
// them there from its argument segment at its start (one dword per thread,
// one barrier).  Kernel arguments are loaded at the kernel's entry and held
// in SGPRs to their last use: read in the band branch they took the kernel
// to 106 SGPRs (6 waves per SIMD instead of 8); from LDS they are loaded
// where the band's lanes use them.
constexpr uint32_t kBandDwords = (uint32_t)(sizeof(geo::BandConsts) / 4u);
// A ring render launches one wave per workgroup (the tile's four waves as
// four workgroups): a wave with band lanes lives two to three times as long
// as its tile's others, and a 4-wave workgroup keeps its finished waves'
// slots from the next workgroup until it ends (config 3 +8.4 -> +7.4 %,
// config 2 +15.0 -> +13.1 % over the plain frame, profiles/r06e_ring_wave_blocks_ab.txt).
// The same for a plain one-frame direct-mode render (tiles differ ~30x in
// cost, and its waves' lifetimes within a tile differ too): config 3
// -0.7 %, config 2 -1 % per frame; the adaptive mode measured +0.8 % and
// keeps 4-wave workgroups (profiles/r06h_all_wave_blocks_ab.txt)
__host__ __device__ constexpr bool wave_blocks(int mode, bool mips, uint32_t nf, bool ring) {
    return nf == 1 && (ring || (!mips && mode == GEO_MODE_DIRECT));
}
// WB's 1-D grid for a launch of n tiles (n <= kMaxWaveBlockTiles: at most 2^31
// workgroups): whole groups of 8 tiles, the four waves of a tile 8 workgroups
// apart and so on one XCD (its L2 holds the tile's sky lines).  Against four
// consecutive workgroups (on four XCDs), config 3 -0.6 to -0.8 %, config 2
// -0.8 % (profiles/r06k_wave_block_layout_ab.txt)
constexpr uint32_t kMaxWaveBlockTiles = 1u << 26;
inline uint32_t wave_block_count(uint32_t n) { return (n + 7u) / 8u * 32u; }
static_assert(sizeof(geo::BandConsts) % 8u == 0 && kBandDwords / 2u <= 64u, "one 8-byte word per thread");

// GEO_FLAG_MIPS epilogue: the pixel's UV and its quad footprint rho2 are
// known; the trilinear sample in place of the level-0 one.
__device__ __forceinline__ void shade_pixel_mips(const RenderArgs& a, float lam, float U, float V, float rho2,
                                                 uint32_t steps, size_t o) {
    const bool bh = lam < geo::kBlackHoleLambda;
    if (a.composite) {
        if (!bh) {
            const uint32_t s = sample_trilinear(a, rho2, U, V);
            a.out_rgba[o] = a.sky_opaque ? s : geo::composite_(s, a.out_rgba[o]);
        }
    } else {
        a.out_rgba[o] = bh ? geo::kBlackRGBA : geo::over_clear(sample_trilinear(a, rho2, U, V), a.sky_opaque != 0);
    }
    if (a.out_mask) a.out_mask[o] = bh ? 1 : 0;
    if (a.out_uv) a.out_uv[o] = make_float2(U, V);
    if (a.out_steps) a.out_steps[o] = steps;
}

// The pixel's traveled-angle result lambda' (pi/2 - angle) by mode.
template <int MODE, int KIND>
__device__ __forceinline__ float pixel_lambda(const RenderArgs& a, const geo::PixelConsts& k, float st, float ct,
                                              float rct, uint32_t* steps) {
    if constexpr (MODE == GEO_MODE_FAN) {
        *steps = 0;
        return geo::fan_lerp(a.fan, a.n_fan, st);
    } else if constexpr (MODE == GEO_MODE_ADAPTIVE) {
        return geo::kPi2 - geo::geodesic_angle_adaptive<KIND>(k, st, ct, rct, steps);
    } else {
        return geo::kPi2 - geo::geodesic_angle_v<KIND>(k, st, ct, rct, steps);
    }
}

// The scene constants of frame z of the launch.
template <uint32_t NF>
__device__ __forceinline__ const geo::PixelConsts& frame_consts(const RenderArgs& a, const FrameBatch<NF>& fb,
                                                                uint32_t z) {
    if constexpr (NF > 1)
        return fb.k[z];
    else
        return a.k;
}

// Pixels per lane: a fan-mode lane (level-0 sampler) draws two, rows
// kWaveRows apart, so one wave covers 16 x 8 pixels and each lane's loads of
// the second pixel overlap the first's (the fan lerp and the texel quads are
// the kernel's latency; its VALU work is short).  The mip-mapped fan draw
// measured the same either way (profiles/r03v_fan_mips_ab.txt) and keeps one.
// Four pixels per lane (a 32 x 32 tile, 47 VGPRs) measured the same as two
// (4K draw 0.0373 vs 0.0370 ms, 3 x 3 interleaved, profiles/r04g_fan_lr_ab.txt):
// the draw's waves are not short of independent work.
constexpr uint32_t kFanLaneRows = 2;
__host__ __device__ constexpr uint32_t lane_rows(int mode, bool mips) {
    return mode == GEO_MODE_FAN && !mips ? kFanLaneRows : 1u;
}

// The fan-mode draw of one 32 x (8 LR) tile, LR pixels per lane (lane_rows)
// kWaveRows rows apart: every pixel's ray, then every fan lerp (2 LR loads in
// flight), then every epilogue.  Pixels k and k + 1 (k even) lie in one
// 8-row-aligned group of the wave's rows, so in one band (band heights are
// multiples of 8): the band mapping is per group, in scalar ops.
template <uint32_t LR>
__device__ __forceinline__ void fan_tile(const RenderArgs& a, const FrameK& f, size_t obase, uint2 tile, uint32_t wave,
                                         uint32_t lane) {
    static_assert(LR % 2 == 0 && LR * kWaveRows % 8 == 0, "pixel pairs fill 8-row groups");
    const uint32_t px = tile.x * kTileW + (wave % kWavesX) * kWaveW + lane % kWaveW;
    const uint32_t wl0 = tile.y * (kTileH * LR) + (wave / kWavesX) * (kWaveRows * LR);
    const uint32_t r = lane / kWaveW;
    uint32_t ly[LR], py[LR];
#pragma unroll
    for (uint32_t k = 0; k < LR; k += 2) {
        const uint32_t g0 = wl0 + (k / 2) * 8u;  // 8-row-aligned local row of pixels k, k + 1
        const uint32_t band = __umulhi(g0, a.band_magic);
        const uint32_t p0 = a.row0 + band * a.band_stride + (g0 - band * a.band_rows) + r;
        ly[k] = g0 + r;
        ly[k + 1] = g0 + r + kWaveRows;
        py[k] = p0;
        py[k + 1] = p0 + kWaveRows;
    }
    float c2x[LR], c2y[LR], st[LR], ct[LR], rct[LR], lam[LR];
#pragma unroll
    for (uint32_t k = 0; k < LR; ++k) {
        float c2z;
        geo::pixel_central_dir(f.cam, f.frame.movement_to_central, f.frame.psi_factor_and_position[0], f.kt, px,
                               py[k], &c2x[k], &c2y[k], &c2z);
        st[k] = geo::central_sin(c2z);
        ct[k] = geo::central_rho(c2x[k], c2y[k]);
        rct[k] = geo::rcpf_(ct[k]);
    }
    geo::FanPos fp[LR];
#pragma unroll
    for (uint32_t k = 0; k < LR; ++k) fp[k] = geo::fan_pos(a.n_fan, st[k]);
#pragma unroll
    for (uint32_t k = 0; k < LR; ++k) lam[k] = geo::fan_at(a.fan, fp[k]);
    bool in[LR], bh[LR];
    bool all_bh = true;
#pragma unroll
    for (uint32_t k = 0; k < LR; ++k) {
        in[k] = px < a.width && ly[k] < a.nrows && py[k] < a.height;
        bh[k] = lam[k] < geo::kBlackHoleLambda;
        all_bh = all_bh && bh[k];
    }
    if (!a.composite && !a.out_uv && !a.out_mask && !a.out_steps) {
        // the plain draw: every UV, then every texel quad (4 LR loads in
        // flight), then the stores; a wave with no sky pixel stores the
        // clear colour only
        uint32_t rgba[LR];
#pragma unroll
        for (uint32_t k = 0; k < LR; ++k) rgba[k] = geo::kBlackRGBA;
        if (geo::ballot_(!all_bh) != 0) {
            float U[LR], V[LR];
#pragma unroll
            for (uint32_t k = 0; k < LR; ++k)
                geo::sky_uv(f.frame.central_to_uv, c2x[k], c2y[k], ct[k], rct[k], lam[k], &U[k], &V[k]);
            const auto quad = level0_quad(a);
            uint32_t smp[LR];
#pragma unroll
            for (uint32_t k = 0; k < LR; ++k)
                smp[k] = geo::sample_sky_quad_f(quad, a.sky_w256, a.sky_h256, U[k], V[k]);
#pragma unroll
            for (uint32_t k = 0; k < LR; ++k)
                rgba[k] = bh[k] ? geo::kBlackRGBA : geo::over_clear(smp[k], a.sky_opaque != 0);
        }
#pragma unroll
        for (uint32_t k = 0; k < LR; ++k)
            if (in[k]) a.out_rgba[obase + (size_t)ly[k] * a.width + px] = rgba[k];
    } else {
#pragma unroll
        for (uint32_t k = 0; k < LR; ++k)
            if (in[k])
                shade_pixel(a, f.frame.central_to_uv, c2x[k], c2y[k], ct[k], rct[k], lam[k], 0u,
                            obase + (size_t)ly[k] * a.width + px);
    }
}

// NF: frames of the launch (FrameBatch; 1, or up to kMaxBatchFrames with the
// frame in blockIdx.z and its output a.out_frame_px pixels after the last's).
// RING: GEO_FLAG_RING_F64 (geo_band.h): the lanes of the capture-orbit band
// take their traveled angle from the f64 path instead of the f32 one.
template <int MODE, int KIND, bool MIPS, uint32_t NF, bool RING>
__global__ __launch_bounds__(kBlock) void geo_render_kernel(const RenderArgs a, const FrameBatch<NF> fb,
                                                            const BandArg<RING && NF == 1> bk) {
#if defined(GEO_WAVE_LOG)
    const unsigned long long t_wave0 = __builtin_amdgcn_s_memrealtime();
#endif
    constexpr uint32_t LR = lane_rows(MODE, MIPS);
    const uint32_t z = NF > 1 ? blockIdx.z : 0u;
    const FrameK& f = fb.f[z];
    const size_t obase = NF > 1 ? (size_t)z * a.out_frame_px : 0;
    // WB (wave_blocks): one wave per workgroup, on a 1-D grid: workgroup L
    // draws wave w of the tile at dispatch position p (p indexes the order,
    // or the launch's tiles row-major).  The hardware deals workgroups to
    // the 8 XCDs round-robin (L mod 8), so the four waves of a tile are put 8
    // apart (p = 8 (L / 32) + L mod 8, w = (L / 8) mod 4) and share their
    // XCD's L2 for the tile's sky lines; the grid is padded to whole groups
    // of 8 tiles (wave_block_count).
    constexpr bool WB = wave_blocks(MODE, MIPS, NF, RING);
    uint32_t pos, wave;
    if constexpr (WB) {
        const uint32_t L = blockIdx.x;
        pos = ((L >> 5) << 3) + (L & 7u);
        wave = (L >> 3) & 3u;
        if (pos >= a.launch_tiles) return;  // the padding of the last group (a whole workgroup)
    } else {
        pos = blockIdx.y * gridDim.x + blockIdx.x;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x) >> 6;
    }
    const uint32_t tiles_x = WB ? a.tiles_x : gridDim.x;
    uint2 tile;
    if (a.tile_order) {
        const uint32_t t = a.tile_order[pos];  // one scalar load
        tile = make_uint2(t & 0xFFFFu, t >> 16);
    } else if constexpr (WB) {
        tile = make_uint2(pos % tiles_x, a.tile_y0 + pos / tiles_x);
    } else {
        tile = make_uint2(blockIdx.x, a.tile_y0 + blockIdx.y);
    }
    const uint32_t lane = threadIdx.x & 63u;
    // RING: the band's constants in LDS (kBandDwords): a one-frame launch
    // copies them from its kernel arguments; a batched launch (RB) derives
    // frame z's in a wave's own slot when the wave has band lanes
    constexpr bool RB = RING && NF > 1;
    __shared__ double band_lds[RING ? (RB ? kBlock / 64u : 1u) * (kBandDwords / 2u) : 1u];
    if constexpr (RING && NF == 1) {
        // one 8-byte word per thread (kBandDwords / 2 <= 64)
        if (threadIdx.x < kBandDwords / 2u)
            reinterpret_cast<uint2*>(band_lds)[threadIdx.x] = reinterpret_cast<const uint2*>(&bk.k)[threadIdx.x];
        __syncthreads();
    }
    const uint32_t px = tile.x * kTileW + (wave % kWavesX) * kWaveW + lane % kWaveW;
    // local row -> frame row.  band_rows is a multiple of 8 (checked on the
    // host): each wave's rows (at most 8) lie in one band and the mapping is
    // wave-uniform (scalar ops; the band index by a multiply-high,
    // band_rows_magic).
    const uint32_t wl0 = tile.y * (kTileH * LR) + (wave / kWavesX) * (kWaveRows * LR);
    const uint32_t ly = wl0 + lane / kWaveW;
    const uint32_t band = __umulhi(wl0, a.band_magic);
    const uint32_t py = a.row0 + band * a.band_stride + (wl0 - band * a.band_rows) + (ly - wl0);
    uint32_t steps = 0;
    uint32_t cost_scale = 1u;  // RING: 2 on the band's lanes (their steps are f64)
    (void)cost_scale;
    const bool in_frame = px < a.width && ly < a.nrows && py < a.height;
    if constexpr (LR > 1) {
        fan_tile<LR>(a, f, obase, tile, wave, lane);
    } else if constexpr (!MIPS) {
        if (in_frame) {
            float c2x, c2y, c2z;
            geo::pixel_central_dir(f.cam, f.frame.movement_to_central, f.frame.psi_factor_and_position[0], f.kt, px,
                                   py, &c2x, &c2y, &c2z);
            const float st = geo::central_sin(c2z);
            const float ct = geo::central_rho(c2x, c2y);
            const float rct = geo::rcpf_(ct);  // shared by the ray's 1/b^2 and its sky direction
            if constexpr (RING) {
                // the band's lanes skip the f32 integration (its loop runs on
                // the other lanes) and take lambda' and the mask from the f64
                // path; both then draw the sky from the f32 ray
                double* const bslot = band_lds + (RB ? wave * (kBandDwords / 2u) : 0u);
                const geo::BandConsts& bkl = *reinterpret_cast<const geo::BandConsts*>(bslot);
                float kx;
                if constexpr (RB)
                    kx = fb.ring_kx[z];
                else
                    kx = bkl.kx;
                const bool band = geo::in_band(kx, ct);
                float lam = 0.0f;
                bool bh = false;
                if (!band) {
                    lam = pixel_lambda<MODE, KIND>(a, frame_consts(a, fb, z), st, ct, rct, &steps);
                    bh = lam < geo::kBlackHoleLambda;
                }
                if (geo::ballot_(band) != 0) {
                    if constexpr (RB) {
                        // frame z's constants, written by the wave's first
                        // active lane (lanes outside the frame are off here)
                        // into the wave's slot (the same f64 operations as the
                        // host's geo::band_consts), then read by the band's lanes
                        if (lane == (uint32_t)__builtin_amdgcn_readfirstlane((int)lane)) {
                            const geo::PixelConsts& kz = fb.k[z];
                            geo::band_consts_into(*reinterpret_cast<geo::BandConsts*>(bslot), f.frame, kz.rs,
                                                  kz.sphere_r, kz.r, kz.step, kz.max_steps, a.width, a.height);
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
                    if (band) {
                        GEO_COLD_ARM();
                        const double l = geo::band_lambda(bkl, px, py, &steps);
                        lam = (float)l;
                        bh = l < (double)geo::kBlackHoleLambda;
                        cost_scale = 2u;  // an f64 step issues as two f32 ones
                    }
                }
                shade_pixel_bh(a, f.frame.central_to_uv, c2x, c2y, ct, rct, lam, bh, steps,
                               obase + (size_t)ly * a.width + px);
            } else {
                const float lam = pixel_lambda<MODE, KIND>(a, frame_consts(a, fb, z), st, ct, rct, &steps);
                shade_pixel(a, f.frame.central_to_uv, c2x, c2y, ct, rct, lam, steps,
                            obase + (size_t)ly * a.width + px);
            }
        }
    } else {
        // Every lane traces its pixel, the ones outside the frame or the
        // requested rows too (the helpers of the frame-aligned 2 x 2 quads,
        // as a fragment shader's): the footprint needs all four UVs of a quad.
        // Black-hole pixels keep their UV as well (textureSample runs before
        // the discard, shader.wgsl:101-104).
        float c2x, c2y, c2z;
        geo::pixel_central_dir(f.cam, f.frame.movement_to_central, f.frame.psi_factor_and_position[0], f.kt, px, py,
                               &c2x, &c2y, &c2z);
        const float st = geo::central_sin(c2z);
        const float ct = geo::central_rho(c2x, c2y);
        const float rct = geo::rcpf_(ct);
        const float lam = pixel_lambda<MODE, KIND>(a, frame_consts(a, fb, z), st, ct, rct, &steps);
        // A pixel's UV is read by its own sample and by its quad partners'
        // footprints, all in this wave: a wave wholly inside the shadow reads
        // none (unless the caller asks for UV) and skips the UV and the
        // footprint (a wave-uniform branch)
        float U = 0.0f, V = 0.0f, rho2 = 0.0f;
        if (geo::ballot_(!(lam < geo::kBlackHoleLambda)) != 0 || a.out_uv) {
            geo::sky_uv(f.frame.central_to_uv, c2x, c2y, ct, rct, lam, &U, &V);
            const float ux = lane_xor1(U), vx = lane_xor1(V), uy = lane_xor16(U), vy = lane_xor16(V);
            rho2 = geo::mip_rho2(U - ux, V - vx, U - uy, V - vy, a.sky_wf, a.sky_hf);
        }
        if (in_frame)
            shade_pixel_mips(a, lam, U, V, rho2, steps, obase + (size_t)ly * a.width + px);
        else
            steps = 0;
    }
    if constexpr (MODE != GEO_MODE_FAN) {
        if (a.step_slots) {
            // One atomic per wave (all 64 lanes active here; a wave's sum fits
            // u32: 64 x 2^20 steps at most) into one of kStepSlots sharded
            // slots.  No block barrier, so a wave that finishes early frees
            // its slot at once.
            const uint32_t total = wave_sum_u32(steps);
            const uint32_t slot = (tile.x * (kBlock / 64) + wave) % kStepSlots;
            if ((threadIdx.x & 63) == 0 && total)
                atomicAdd(&a.step_slots[slot * kSlotStride], (unsigned long long)total);
        }
        if (a.tile_cost && z == 0u) {
            // a wave holds its slot until its slowest lane stops: the tile's
            // cost is the sum of its waves' largest step counts (frame 0's
            // of a batch: the order is per tile)
            // (RING: a wave runs its f32 lanes' loop, then its band lanes'
            // f64 loop at about twice the cost per step)
            const uint32_t wmax = RING ? wave_max_u32(cost_scale == 1u ? steps : 0u) +
                                             2u * wave_max_u32(cost_scale == 1u ? 0u : steps)
                                       : wave_max_u32(steps);
            if ((threadIdx.x & 63) == 0)
                atomicAdd(&a.tile_cost[tile.y * tiles_x + tile.x], wmax + a.cost_overhead);
        }
    }
#if defined(GEO_WAVE_LOG)
    if (a.wave_log) {
        const uint32_t wmax = wave_max_u32(steps);
        const unsigned long long t_wave1 = __builtin_amdgcn_s_memrealtime();
        if ((threadIdx.x & 63) == 0) {
            const size_t wg = (size_t)blockIdx.z * (WB ? a.launch_tiles : gridDim.x * gridDim.y) + pos;  // the tile, in launch order
            unsigned long long* p = a.wave_log + (wg * (kBlock / 64) + wave) * 4;
            const uint32_t hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_REG_HW_ID
            const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);    // HW_REG_XCC_ID[3:0]
            p[0] = t_wave0;
            p[1] = t_wave1;
            p[2] = hw_id | ((unsigned long long)xcc << 32);
            p[3] = (tile.x | (tile.y << 16)) | ((unsigned long long)wmax << 32);
        }
    }
#endif
}

// ---- GEO_FLAG_DISK: the thin accretion disk (geo_disk.h) ----------------
// The disk renders are kernels of their own beside geo_render_kernel, whose
// instantiations carry no disk branch, argument or register: GEO_MODE_DIRECT
// (GEO_MODE_ADAPTIVE in the kernels of geo_render_disk_adaptive and
// geo_render_disk_adaptive_batch),
// level-0 sampler, one wave per workgroup on the 1-D grid of the plain
// direct-mode render (wave_blocks), the same tile mapping, step counting and
// tile-cost recording.  The argument structs come first, then the ring
// kernels, then the one body of all the others (wave_block_body) and its
// __global__ wrappers.
struct DiskArgs {
    geo::DiskConsts k;
    const uint32_t* tex;  // padded (geo::pad_sky): (tex_w + 2) x (tex_h + 2) texels
    float tex_w256, tex_h256;
    uint32_t tex_pitch_b, tex_bytes;
    float* out_hits;  // optional: 3 x (r, U) per pixel
};

// The shifted render (geo_set_disk_shift): the ray's shift terms are computed
// once per lane and the per-hit ones in the hit arm of
// geo::disk_shade_shift_slot_; the RK4 loop is the plain render's.
struct DiskShiftArgs {
    geo::DiskShift k;
    float* out_g;  // optional: 3 x g per pixel
};

// The emission render (geo_set_disk_emission): the shifted render with
// geo::disk_shade_emit_slot_'s hit arm, which turns g and r into
// q = T_obs / t_ref, reads the ramp's two neighbouring entries (two dword
// loads, inside the arm only) and scales the texture sample.
struct DiskEmitArgs {
    geo::DiskEmission k;
    const uint32_t* ramp;  // k.n2 + 2 RGBA8 entries
    float* out_g;          // optional: 3 x g per pixel
    float* out_q;          // optional: 3 x q per pixel
};

// What a wave-block kernel shades: the sky alone, or the disk plain, shifted or
// with its emission.  The host decides it once per call (geo_render.hip).
enum class Shade { kSky, kDisk, kDiskShift, kDiskEmit };
// A kernel argument that an instantiation does not have: the shade's own
// (ShadeFrameArg, ShadeBatchArg below) of an unshaded render, the output pitch
// (SsPitch) of a one-sample one.
struct NoArgs {};
// They fit the 4 KiB argument segment (each padded to 8 bytes at most).
template <typename... A>
constexpr bool kKernargsFit = (((sizeof(A) + 7u) / 8u * 8u) + ...) <= 4096u;
template <Shade SHADE>
using ShadeFrameArg = std::conditional_t<SHADE == Shade::kDiskEmit, DiskEmitArgs,
                                         std::conditional_t<SHADE == Shade::kDiskShift, DiskShiftArgs, NoArgs>>;
// GEO_FLAG_SS4: the output's pitch in pixels (RenderArgs::width is then the
// sample frame's, twice it).
template <bool SS>
struct SsPitch {
    __device__ __forceinline__ uint32_t width() const { return 0u; }
};
template <>
struct SsPitch<true> {
    uint32_t out_width;
    __device__ __forceinline__ uint32_t width() const { return out_width; }
};


// ---- geo_set_disk_ring_f64: the disk's capture band in f64 ----------------
// The three one-frame disk renders (SHADE: unshaded, shifted, emission)
// with the band's lanes (geo::in_band on the f32 ray, GEO_FLAG_RING_F64's
// test) taken through the f64 path of geo_band.h, probes included
// (geo::disk_hits_band).  Kernels with their own body on the same launch
// geometry, not a property of wave_block_body below: the band's constants are a
// kernel argument copied to LDS, as in geo_render_kernel<..., RING>, a wave's
// f32 lanes run their loop first and its band lanes, if it has any, the f64
// loop in a cold arm behind one ballot, and a band lane's steps count twice in
// its tile's cost.  Both kinds of lane hand their crossings on as
// geo::DiskHits, and one geo::disk_shade_hits follows (which the three
// geo::disk_shade* forms of wave_block_body are not yet expressed through).  No thread returns
// before the barrier except by the workgroup-uniform padding exit.  rs > 0 and
// r_obs > rs (a capture orbit): the curved kinds only.
//   MODE   the f32 lanes' integrator: GEO_MODE_DIRECT (geo::disk_ray,
//          geo::geodesic_angle_disk), or GEO_MODE_ADAPTIVE
//          (geo_render_disk_adaptive_ring, and disk_ring_body's frames of
//          geo_render_disk_adaptive_ring_batch: geo::disk_ray_adaptive makes every
//          lane's DiskRay, of which the band's f64 path reads only ak[0] and
//          "no crossing", and geo::geodesic_angle_adaptive_disk; the band's
//          lanes take the scene's step and max_steps as the f64 loop's fixed
//          step and budget).  The step slots then mix units, as the plain
//          adaptive GEO_FLAG_RING_F64 render's do: attempted adaptive steps of
//          the f32 lanes, fixed f64 steps of the band's.  So does the tile
//          cost: the wave's largest count of RK5(4) attempts (~57 VALU each;
//          a.cost_overhead is the adaptive mode's, in attempts) plus twice its
//          largest count of f64 RK4 steps, where the unit beside it in the
//          direct mode is the cheaper f32 RK4 step.  The cost only orders the
//          tiles of this render's own grid key.
template <int KIND, Shade SHADE, int MODE>
__global__ __launch_bounds__(64) void geo_render_disk_ring_kernel(const RenderArgs a, const FrameBatch<1> fb,
                                                                  const DiskArgs d, const ShadeFrameArg<SHADE> x,
                                                                  const BandArg<true> bk) {
    static_assert(KIND != geo::kFlat && SHADE != Shade::kSky, "no capture orbit without a black hole; a disk render");
    static_assert(MODE == GEO_MODE_DIRECT || MODE == GEO_MODE_ADAPTIVE, "the f32 lanes' integrator");
    static_assert(kKernargsFit<RenderArgs, FrameBatch<1>, DiskArgs, ShadeFrameArg<SHADE>, BandArg<true>>);
    const FrameK& f = fb.f[0];
    const uint32_t L = blockIdx.x;
    const uint32_t pos = ((L >> 5) << 3) + (L & 7u);
    const uint32_t wave = (L >> 3) & 3u;
    if (pos >= a.launch_tiles) return;  // the padding of the last group (a whole workgroup)
    const uint32_t tiles_x = a.tiles_x;
    uint2 tile;
    if (a.tile_order) {
        const uint32_t t = a.tile_order[pos];
        tile = make_uint2(t & 0xFFFFu, t >> 16);
    } else {
        tile = make_uint2(pos % tiles_x, a.tile_y0 + pos / tiles_x);
    }
    const uint32_t lane = threadIdx.x & 63u;
    // the band's constants in LDS: one 8-byte word per thread (kBandDwords / 2 <= 64)
    __shared__ double band_lds[kBandDwords / 2u];
    if (threadIdx.x < kBandDwords / 2u)
        reinterpret_cast<uint2*>(band_lds)[threadIdx.x] = reinterpret_cast<const uint2*>(&bk.k)[threadIdx.x];
    __syncthreads();
    const geo::BandConsts& bkl = *reinterpret_cast<const geo::BandConsts*>(band_lds);
    const uint32_t px = tile.x * kTileW + (wave % kWavesX) * kWaveW + lane % kWaveW;
    const uint32_t wl0 = tile.y * kTileH + (wave / kWavesX) * kWaveRows;
    const uint32_t ly = wl0 + lane / kWaveW;
    const uint32_t band = __umulhi(wl0, a.band_magic);
    const uint32_t py = a.row0 + band * a.band_stride + (wl0 - band * a.band_rows) + (ly - wl0);
    uint32_t steps = 0;
    bool f64_lane = false;
    if (px < a.width && ly < a.nrows && py < a.height) {
        float c2x, c2y, c2z, g_obs = 1.0f;
        if constexpr (SHADE == Shade::kDisk)
            geo::pixel_central_dir(f.cam, f.frame.movement_to_central, f.frame.psi_factor_and_position[0], f.kt, px,
                                   py, &c2x, &c2y, &c2z);
        else
            geo::pixel_central_dir_g(f.cam, f.frame.movement_to_central, f.frame.psi_factor_and_position[0], f.kt, px,
                                     py, &c2x, &c2y, &c2z, &g_obs);
        const float st = geo::central_sin(c2z);
        const float ct = geo::central_rho(c2x, c2y);
        const float rct = geo::rcpf_(ct);
        geo::DiskRay dr;
        if constexpr (MODE == GEO_MODE_ADAPTIVE)
            geo::disk_ray_adaptive(d.k, a.k, c2x, c2y, ct, rct, &dr);
        else
            geo::disk_ray(d.k, a.k, c2x, c2y, ct, rct, &dr);
        f64_lane = geo::in_band(bkl.kx, ct);
        float lam = 0.0f;
        bool bh = false;
        geo::DiskHits h;
#pragma unroll
        for (int c = 0; c < geo::kDiskMaxCrossings; ++c) {
            h.hit[c] = false;
            h.r[c] = 0.0f;
        }
        if (!f64_lane) {
            float Uk[geo::kDiskMaxCrossings];
            float ang;
            if constexpr (MODE == GEO_MODE_ADAPTIVE)
                ang = geo::geodesic_angle_adaptive_disk<KIND>(a.k, st, ct, rct, dr, &steps, Uk);
            else
                ang = geo::geodesic_angle_disk<KIND>(a.k, st, ct, rct, dr, &steps, Uk);
            lam = geo::kPi2 - ang;
            bh = lam < geo::kBlackHoleLambda;
            geo::disk_hits_f32(d.k, a.k, dr, Uk, steps, ang, &h);
        }
        if (geo::ballot_(f64_lane) != 0) {
            if (f64_lane) {
                GEO_COLD_ARM();
                const double l = geo::disk_hits_band(bkl, d.k, dr, px, py, &steps, &h);
                lam = (float)l;
                bh = l < (double)geo::kBlackHoleLambda;
            }
        }
        float U = 0.0f, V = 0.0f;
        if (!bh || a.out_uv) geo::sky_uv(f.frame.central_to_uv, c2x, c2y, ct, rct, lam, &U, &V);
        const size_t o = (size_t)ly * a.width + px;
        const uint32_t base =
            bh ? geo::kBlackRGBA : geo::sample_sky_qf(level0_quad(a), a.sky_w256, a.sky_h256, a.sky_opaque != 0, U, V);
        const PaddedSkyQuad dquad{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(d.tex), 0, (int)d.tex_bytes,
                                                                    kBufferRsrcWord3),
                                  d.tex_pitch_b};
        const auto dsample = [&](float Ud, float Vd) {
            return geo::sample_sky_quad_f(dquad, d.tex_w256, d.tex_h256, Ud, Vd);
        };
        float* const hits = d.out_hits ? d.out_hits + o * (2u * geo::kDiskMaxCrossings) : nullptr;
        if constexpr (SHADE == Shade::kDiskEmit) {
            const DiskEmitArgs& em = x;
            const auto rfetch = [ramp = em.ramp](uint32_t i) { return ramp[i]; };
            geo::DiskShiftRay sr;
            geo::disk_shift_ray(d.k, em.k.s, dr, ct, g_obs, &sr);
            a.out_rgba[o] = geo::disk_shade_hits(d.k, dr, h, base,
                                                 geo::disk_colour_emit(d.k, a.k, em.k, sr, dsample, rfetch), hits,
                                                 em.out_g ? em.out_g + o * geo::kDiskMaxCrossings : nullptr,
                                                 em.out_q ? em.out_q + o * geo::kDiskMaxCrossings : nullptr);
        } else if constexpr (SHADE == Shade::kDiskShift) {
            const DiskShiftArgs& sh = x;
            geo::DiskShiftRay sr;
            geo::disk_shift_ray(d.k, sh.k, dr, ct, g_obs, &sr);
            a.out_rgba[o] = geo::disk_shade_hits(d.k, dr, h, base, geo::disk_colour_shift(a.k, sh.k, sr, dsample),
                                                 hits, sh.out_g ? sh.out_g + o * geo::kDiskMaxCrossings : nullptr,
                                                 nullptr);
        } else {
            a.out_rgba[o] = geo::disk_shade_hits(d.k, dr, h, base, geo::disk_colour_plain(dsample), hits, nullptr,
                                                 nullptr);
        }
        if (a.out_mask) a.out_mask[o] = bh ? 1 : 0;
        if (a.out_uv) a.out_uv[o] = make_float2(U, V);
        if (a.out_steps) a.out_steps[o] = steps;
    }
    // wave_block_body's epilogue with the ring kernel's tile cost: the wave runs its
    // f32 lanes' loop, then its band lanes' f64 loop at about twice the cost
    // per step (every lane of the wave is active again here)
    if (a.step_slots) {
        const uint32_t total = wave_sum_u32(steps);
        const uint32_t slot = (tile.x * (kBlock / 64) + wave) % kStepSlots;
        if (lane == 0 && total) atomicAdd(&a.step_slots[slot * kSlotStride], (unsigned long long)total);
    }
    if (a.tile_cost) {
        const uint32_t wmax = wave_max_u32(f64_lane ? 0u : steps) + 2u * wave_max_u32(f64_lane ? steps : 0u);
        if (lane == 0) atomicAdd(&a.tile_cost[tile.y * tiles_x + tile.x], wmax + a.cost_overhead);
    }
}

// ---- geo_render_disk_batch: up to kMaxBatchFrames disk frames in one launch --
// The plain and the shifted disk render with the frame in blockIdx.z (its output
// a.out_frame_px pixels after the last frame's), colour only, on the same
// wave-block grid.
// RenderArgs and FrameBatch<kMaxBatchFrames> leave no room in the 4 KiB of
// kernel arguments for eight frames' disk constants, so the batch has a
// per-frame struct of its own: FrameK without what no disk kernel reads
// (display_to_movement, which only geo::camera_consts reads on the host, and
// three of psi_factor_and_position's four floats), the frame's scene constants,
// and the parts of geo::DiskConsts and geo::DiskShift that change with the
// frame: N, ex and ey with its central_to_uv, u_lo and u_hi with its scale, sb
// and ih with its r_obs and det M2.  The host fills them with the one-frame
// launch's geo::disk_consts and geo::disk_shift_consts, so a batch frame is the
// one-frame render of that frame bit for bit.
struct DiskFrameK {
    float movement_to_central[16];
    float central_to_uv[16];
    float psi;  // psi_factor_and_position[0]
    geo::CameraConsts cam;
    float kt;
    geo::PixelConsts k;
    float N[3], ex[3], ey[3];
    float u_lo, u_hi;
    float sb, ih;  // shaded batches (zero otherwise)
};
struct DiskBatchArgs {
    DiskFrameK f[kMaxBatchFrames];
    float r_in, r_out, inv_dr, inv_step;  // geo::DiskConsts, batch-uniform
    const uint32_t* tex;
    float tex_w256, tex_h256;
    uint32_t tex_pitch_b, tex_bytes;
    float gain;  // geo::DiskShift, batch-uniform
    uint32_t exponent;
};

// Launch geometry: the one-frame disk render's, one wave per workgroup on the
// 1-D wave-block grid, with the frame in grid.z.  The plain batch's 32 x 8-pixel
// workgroups of four waves on a 2-D grid were measured against it.

// ---- GEO_FLAG_SS4: 2 x 2 supersampling, resolved in the kernel -----------
// The one-frame direct-mode renders with a lane per SAMPLE: RenderArgs
// describes the sample frame (width, height, row0, nrows, band_rows and
// band_stride are twice the call's; f.cam is geo::camera_consts at twice the
// size), so a lane traces and shades pixel (px, py) of the 2W x 2H render
// exactly as its one-sample sibling does, keeps the colour in a register, and
// the wave's 16 x 4 samples are resolved to 8 x 2 output pixels across its
// lanes.  The output's pitch rides in SsPitch<true>.

// lane_xor1 / lane_xor16 on integers: a sample's x and y partners in its
// output pixel's 2 x 2 quad.
__device__ __forceinline__ uint32_t lane_xor1_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t lane_xor16_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);
}

// The box resolve of an output pixel's four samples (lanes l, l ^ 1, l ^ 16,
// l ^ 17), each 8-bit channel on its own: (s00 + s01 + s10 + s11 + 2) >> 2.
// Two channels per register: c & 0x00FF00FF holds R and B, (c >> 8) &
// 0x00FF00FF G and A, in 16-bit fields; a field's sum over four samples is at
// most 1020 (1022 with the rounding term), so it never carries into its
// neighbour.  Every lane of the wave must be active: a cross-lane read from an
// inactive lane returns nothing useful.
__device__ __forceinline__ uint32_t ss_resolve(uint32_t c) {
    uint32_t rb = c & 0x00FF00FFu, ga = (c >> 8) & 0x00FF00FFu;
    rb += lane_xor1_u32(rb);
    ga += lane_xor1_u32(ga);
    rb += lane_xor16_u32(rb);
    ga += lane_xor16_u32(ga);
    rb = ((rb + 0x00020002u) >> 2) & 0x00FF00FFu;
    ga = ((ga + 0x00020002u) >> 2) & 0x00FF00FFu;
    return rb | (ga << 8);
}

// ---- geo_render_ss_batch: up to kMaxBatchFrames GEO_FLAG_SS4 frames in one launch --
// The one-frame SS4 renders with the frame in blockIdx.z, on the disk batch's
// geometry: one wave per workgroup on the 1-D wave-block grid, grid.z frames.
// Frame z's constants come from the batched kernels' own argument structs,
// indexed by z (uniform: scalar loads): the sky-only render reads
// FrameBatch<kMaxBatchFrames> (f[z], k[z]), the disk renders DiskBatchArgs
// (DiskFrameK, assembled into geo::DiskConsts and geo::DiskShift by
// DiskBatchFrame below).  The host fills both with the one-frame
// SS launch's functions at the sample frame's size, so a batch frame is its
// one-frame render bit for bit.  Frame z's output starts a.out_frame_px output
// pixels after frame z - 1's.

// ---- geo_render_emission_batch: up to kMaxBatchFrames emission frames in one launch --
// The shaded disk batch and the SS batch's disk frames with
// geo::disk_shade_emit as the hit arm (null per-pixel outputs: a batch draws
// colour only).  DiskBatchArgs is reused unchanged: of a
// geo::DiskEmission only sb and ih change with the frame (its r_obs and
// det M2), and DiskFrameK carries them, filled by geo::disk_emission_consts
// with the emission's spin; the batch-uniform rest and the ramp ride in one
// further argument.  Everything read here per frame or per batch is
// wave-uniform (scalar loads); the ramp's two entries are loaded inside the hit
// arm only, as in the one-frame emission render.
struct DiskEmitBatchArgs {
    float inv_fmax, ka, kb, n1, exposure;  // geo::DiskEmission, batch-uniform
    uint32_t profile, n2;
    const uint32_t* ramp;  // n2 + 2 RGBA8 entries
};
template <Shade SHADE>
using ShadeBatchArg = std::conditional_t<SHADE == Shade::kDiskEmit, DiskEmitBatchArgs, NoArgs>;

// ---- the one body of the disk and SS4 kernels on the wave-block grid ------
// The four kernels below (all of this file's wave-block kernels but
// geo_render_kernel and the ring kernels) are one wrapper per argument layout:
// the sky-only SS4 render, one disk frame, that frame with SS4, a disk batch.
// Each names its frame source and calls wave_block_body, which holds what they
// share: the tile mapping, the camera ray, geo::disk_ray and
// geo::geodesic_angle_disk, the sky sample, the disk texture quad, the shading
// call, the SS4 resolve, and the step-slot and tile-cost epilogue.  (The ring
// bodies spell the mapping and the epilogue again: as shared __forceinline__
// helpers they changed the instruction selection of every kernel here, a
// handful of scalar instructions each, and are not kept;
// profiles/wave_block_wrappers_isa.txt.)  It varies along five properties of
// the render, not of the caller:
//   SHADE  what is shaded: the sky alone (pixel_lambda), or the disk plain,
//          shifted or with its emission (geo::disk_shade, _shift, _emit)
//   SS     one sample per pixel, or GEO_FLAG_SS4: a lane per sample, the band
//          index on output rows, the colour kept in a register, ss_resolve
//          and one store per 2 x 2 quad
//   SIDE   the per-pixel side outputs of the one-frame one-sample renders
//          (mask, uv, steps, hits, g, q; the sky UV also where only a.out_uv
//          asks for it); every other render is colour only
//   MODE   the integrator: GEO_MODE_DIRECT (geo::geodesic_angle_disk), or
//          GEO_MODE_ADAPTIVE (geo::geodesic_angle_adaptive_disk: the one-frame
//          one-sample disk renders of geo_render_disk_adaptive with their side
//          outputs, and the colour-only frames of
//          geo_render_disk_adaptive_batch on DiskBatchFrame, one sample or SS4;
//          a tile's cost is then in attempts).  The adaptive loop's lanes
//          leave it one by one; they rejoin at the end of the in_frame arm, as
//          the direct loop's do, before the SS4 resolve reads across lanes
//   SRC    the frame source: what frame z of the launch reads its camera,
//          scene, disk, texture, shift or emission constants and ramp from,
//          where its output starts and whether it records tile costs, one
//          struct per argument layout (SkyFrame<1>, SkyFrame<kMaxBatchFrames>,
//          DiskFrame, DiskBatchFrame)
// A new variant is a new value of a property, which the wrappers take as a
// template argument and the host's launchers pass on (geo_render.hip): not a
// wrapper, an argument struct or a launcher of its own, and not a copy of the
// body.  An argument that an instantiation lacks is NoArgs.  One body on the
// CPU path too (run_rows_disk, cpu_render.cpp), which every instantiation is
// tested against bit for bit (tests/test_gpu_wave_block_matrix.py: one cell
// each).

// FrameBatch<NF> and the scene constants of frame_consts: the sky-only renders
// (and, as DiskFrame's base, the one-frame disk renders).
template <uint32_t NF>
struct SkyFrame {
    const RenderArgs& a;
    const FrameBatch<NF>& fb;
    uint32_t z;  // the frame of the launch (0 of one)
    static constexpr bool kOneFrame = NF == 1;
    __device__ __forceinline__ const FrameK& f() const { return fb.f[NF > 1 ? z : 0u]; }
    __device__ __forceinline__ const geo::CameraConsts& cam() const { return f().cam; }
    __device__ __forceinline__ const float* movement_to_central() const { return f().frame.movement_to_central; }
    __device__ __forceinline__ const float* central_to_uv() const { return f().frame.central_to_uv; }
    __device__ __forceinline__ float psi() const { return f().frame.psi_factor_and_position[0]; }
    __device__ __forceinline__ float kt() const { return f().kt; }
    __device__ __forceinline__ const geo::PixelConsts& consts() const { return frame_consts(a, fb, z); }
    __device__ __forceinline__ size_t out_base() const { return NF > 1 ? (size_t)z * a.out_frame_px : 0; }
    // (frame 0's of a batch: the order is per tile)
    __device__ __forceinline__ bool records_cost() const { return NF == 1 || z == 0u; }
};

// FrameBatch<1>, RenderArgs::k and DiskArgs, with the shaded renders' further
// argument X (DiskShiftArgs or DiskEmitArgs): the constants by reference.
template <typename X>
struct DiskFrame : SkyFrame<1> {
    const DiskArgs& d;
    const X& x;
    __device__ __forceinline__ const geo::DiskConsts& disk() const { return d.k; }
    __device__ __forceinline__ const DiskArgs& tex() const { return d; }
    __device__ __forceinline__ const geo::DiskShift& shift() const { return x.k; }
    __device__ __forceinline__ const geo::DiskEmission& emission() const { return x.k; }
    __device__ __forceinline__ const uint32_t* ramp() const { return x.ramp; }
};

// DiskBatchArgs, with the emission batch's further argument E: frame z's
// geo::DiskConsts, geo::DiskShift and geo::DiskEmission assembled by value
// from its DiskFrameK and the batch's part (wave-uniform: they stay scalars).
template <typename E>
struct DiskBatchFrame {
    const RenderArgs& a;
    const DiskBatchArgs& db;
    const E& eb;
    uint32_t z;
    static constexpr bool kOneFrame = false;
    __device__ __forceinline__ const DiskFrameK& f() const { return db.f[z]; }
    __device__ __forceinline__ const geo::CameraConsts& cam() const { return f().cam; }
    __device__ __forceinline__ const float* movement_to_central() const { return f().movement_to_central; }
    __device__ __forceinline__ const float* central_to_uv() const { return f().central_to_uv; }
    __device__ __forceinline__ float psi() const { return f().psi; }
    __device__ __forceinline__ float kt() const { return f().kt; }
    __device__ __forceinline__ const geo::PixelConsts& consts() const { return f().k; }
    __device__ __forceinline__ size_t out_base() const { return (size_t)z * a.out_frame_px; }
    __device__ __forceinline__ bool records_cost() const { return z == 0u; }  // frame 0's: the order is per tile
    __device__ __forceinline__ geo::DiskConsts disk() const {
        geo::DiskConsts dk;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dk.N[i] = f().N[i];
            dk.ex[i] = f().ex[i];
            dk.ey[i] = f().ey[i];
        }
        dk.r_in = db.r_in;
        dk.r_out = db.r_out;
        dk.inv_dr = db.inv_dr;
        dk.u_lo = f().u_lo;
        dk.u_hi = f().u_hi;
        dk.inv_step = db.inv_step;
        return dk;
    }
    __device__ __forceinline__ const DiskBatchArgs& tex() const { return db; }
    __device__ __forceinline__ geo::DiskShift shift() const {
        geo::DiskShift sk;
        sk.sb = f().sb;
        sk.ih = f().ih;
        sk.gain = db.gain;
        sk.exponent = db.exponent;
        return sk;
    }
    __device__ __forceinline__ geo::DiskEmission emission() const {  // (its gain and exponent are not read)
        geo::DiskEmission ek;
        ek.s.sb = f().sb;
        ek.s.ih = f().ih;
        ek.s.gain = 1.0f;
        ek.s.exponent = 0u;
        ek.inv_fmax = eb.inv_fmax;
        ek.ka = eb.ka;
        ek.kb = eb.kb;
        ek.n1 = eb.n1;
        ek.exposure = eb.exposure;
        ek.profile = eb.profile;
        ek.n2 = eb.n2;
        return ek;
    }
    __device__ __forceinline__ const uint32_t* ramp() const { return eb.ramp; }
};

// out_width (SS): the output's pitch in pixels; RenderArgs then describes the
// sample frame.
template <int KIND, Shade SHADE, bool SS, bool SIDE, int MODE = GEO_MODE_DIRECT, typename SRC>
__device__ __forceinline__ void wave_block_body(const RenderArgs& a, const SRC& src, uint32_t out_width) {
    static_assert(!(SS && SIDE) && !(SIDE && SHADE == Shade::kSky), "side outputs: the one-sample disk renders'");
    static_assert(MODE == GEO_MODE_DIRECT ||
                      (MODE == GEO_MODE_ADAPTIVE && SHADE != Shade::kSky && (SIDE ? !SS : !SRC::kOneFrame)),
                  "the adaptive integrator: the one-frame one-sample disk renders', and the disk batch's frames'");
    // geo_render_kernel's WB mapping: workgroup L draws wave `wave` of the tile
    // at dispatch position pos.  The padding of the last group (a whole
    // workgroup) leaves here: the body's only early exit, and a wave-uniform
    // one, because ss_resolve below needs every lane of the wave.
    const uint32_t L = blockIdx.x;
    const uint32_t pos = ((L >> 5) << 3) + (L & 7u);
    const uint32_t wave = (L >> 3) & 3u;
    if (pos >= a.launch_tiles) return;
    const uint32_t tiles_x = a.tiles_x;
    uint2 tile;
    if (a.tile_order) {
        const uint32_t t = a.tile_order[pos];
        tile = make_uint2(t & 0xFFFFu, t >> 16);
    } else {
        tile = make_uint2(pos % tiles_x, a.tile_y0 + pos / tiles_x);
    }
    const uint32_t lane = threadIdx.x & 63u;
    // SS: (px, ly) is the lane's sample in the 2W x 2 nrows grid; py its row of
    // the 2H sample frame.  The band index is taken on output rows (wl0 / 2
    // over the call's band_rows: band_magic is that divisor's, within the range
    // band_rows_magic is exact on); a.band_rows, a.band_stride and a.row0 are
    // in sample rows.  Bands are multiples of 16 sample rows, so the wave's
    // four rows lie in one.
    const uint32_t px = tile.x * kTileW + (wave % kWavesX) * kWaveW + lane % kWaveW;
    const uint32_t wl0 = tile.y * kTileH + (wave / kWavesX) * kWaveRows;
    const uint32_t ly = wl0 + lane / kWaveW;
    const uint32_t band = __umulhi(SS ? wl0 >> 1 : wl0, a.band_magic);
    const uint32_t py = a.row0 + band * a.band_stride + (wl0 - band * a.band_rows) + (ly - wl0);
    // SS: in the frame or out of it, the four samples of an output pixel go
    // together: a.width, a.nrows and a.height are even (twice the call's),
    // px and px ^ 1 differ in bit 0 only, and so do ly and ly ^ 1 and, with
    // them, py and its partner (wl0 is a multiple of 4; a.row0, a.band_stride
    // and a.band_rows are even, so py - (ly - wl0) is even and py's bit 0 is
    // ly's).  Lanes l ^ 1 and l ^ 16 hold samples (px ^ 1, ly) and (px, ly ^ 1).
    const bool in_frame = px < a.width && ly < a.nrows && py < a.height;
    uint32_t steps = 0;
    uint32_t colour = 0;  // SS: the sample's colour, kept in a register
    if (in_frame) {
        float c2x, c2y, c2z, g_obs = 0.0f;
        if constexpr (SHADE == Shade::kDiskShift || SHADE == Shade::kDiskEmit)
            geo::pixel_central_dir_g(src.cam(), src.movement_to_central(), src.psi(), src.kt(), px, py, &c2x, &c2y,
                                     &c2z, &g_obs);
        else
            geo::pixel_central_dir(src.cam(), src.movement_to_central(), src.psi(), src.kt(), px, py, &c2x, &c2y, &c2z);
        const float st = geo::central_sin(c2z);
        const float ct = geo::central_rho(c2x, c2y);
        const float rct = geo::rcpf_(ct);
        const geo::PixelConsts& k = src.consts();
        const size_t o = src.out_base() + (size_t)ly * a.width + px;  // (one sample per pixel)
        if constexpr (SHADE == Shade::kSky) {
            const float lam = pixel_lambda<GEO_MODE_DIRECT, KIND>(a, k, st, ct, rct, &steps);
            const bool bh = lam < geo::kBlackHoleLambda;
            float U = 0.0f, V = 0.0f;
            if (!bh) geo::sky_uv(src.central_to_uv(), c2x, c2y, ct, rct, lam, &U, &V);
            colour = bh ? geo::kBlackRGBA
                        : geo::sample_sky_qf(level0_quad(a), a.sky_w256, a.sky_h256, a.sky_opaque != 0, U, V);
            if constexpr (!SS) a.out_rgba[o] = colour;
        } else {
            const auto& dk = src.disk();
            geo::DiskRay dr;
            float Uk[geo::kDiskMaxCrossings];
            float ang;
            if constexpr (MODE == GEO_MODE_ADAPTIVE) {
                geo::disk_ray_adaptive(dk, k, c2x, c2y, ct, rct, &dr);
                ang = geo::geodesic_angle_adaptive_disk<KIND>(k, st, ct, rct, dr, &steps, Uk);
            } else {
                geo::disk_ray(dk, k, c2x, c2y, ct, rct, &dr);
                ang = geo::geodesic_angle_disk<KIND>(k, st, ct, rct, dr, &steps, Uk);
            }
            const float lam = geo::kPi2 - ang;
            const bool bh = lam < geo::kBlackHoleLambda;
            float U = 0.0f, V = 0.0f;
            if (!bh || (SIDE && a.out_uv)) geo::sky_uv(src.central_to_uv(), c2x, c2y, ct, rct, lam, &U, &V);
            const uint32_t base =
                bh ? geo::kBlackRGBA
                   : geo::sample_sky_qf(level0_quad(a), a.sky_w256, a.sky_h256, a.sky_opaque != 0, U, V);
            const auto& t = src.tex();
            const PaddedSkyQuad dquad{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(t.tex), 0,
                                                                        (int)t.tex_bytes, kBufferRsrcWord3),
                                      t.tex_pitch_b};
            const auto dsample = [&](float Ud, float Vd) {
                return geo::sample_sky_quad_f(dquad, t.tex_w256, t.tex_h256, Ud, Vd);
            };
            float *hits = nullptr, *gs = nullptr, *qs = nullptr;
            if constexpr (SIDE) {
                hits = src.d.out_hits ? src.d.out_hits + o * (2u * geo::kDiskMaxCrossings) : nullptr;
                if constexpr (SHADE != Shade::kDisk)
                    gs = src.x.out_g ? src.x.out_g + o * geo::kDiskMaxCrossings : nullptr;
                if constexpr (SHADE == Shade::kDiskEmit)
                    qs = src.x.out_q ? src.x.out_q + o * geo::kDiskMaxCrossings : nullptr;
            }
            if constexpr (SHADE == Shade::kDiskEmit) {
                const auto rfetch = [ramp = src.ramp()](uint32_t i) { return ramp[i]; };
                const auto& ek = src.emission();
                geo::DiskShiftRay sr;
                geo::disk_shift_ray(dk, ek.s, dr, ct, g_obs, &sr);
                colour = geo::disk_shade_emit(dk, k, dr, ek, sr, Uk, steps, ang, base, dsample, rfetch, hits, gs, qs);
            } else if constexpr (SHADE == Shade::kDiskShift) {
                const auto& sk = src.shift();
                geo::DiskShiftRay sr;
                geo::disk_shift_ray(dk, sk, dr, ct, g_obs, &sr);
                colour = geo::disk_shade_shift(dk, k, dr, sk, sr, Uk, steps, ang, base, dsample, hits, gs);
            } else {
                colour = geo::disk_shade(dk, k, dr, Uk, steps, ang, base, dsample, hits);
            }
            if constexpr (!SS) a.out_rgba[o] = colour;
            if constexpr (SIDE) {
                if (a.out_mask) a.out_mask[o] = bh ? 1 : 0;
                if (a.out_uv) a.out_uv[o] = make_float2(U, V);
                if (a.out_steps) a.out_steps[o] = steps;
            }
        }
    }
    // Every per-lane arm (out of frame, black hole, disk hits, shading) has
    // rejoined: all 64 lanes are active, as the resolve's exchange and the
    // wave reductions need.
    if constexpr (SS) {
        // a pixel out of the frame resolves four zeros and is not stored
        const uint32_t resolved = ss_resolve(colour);
        if (in_frame && (lane & 0x11u) == 0u)
            a.out_rgba[src.out_base() + (size_t)(ly >> 1) * out_width + (px >> 1)] = resolved;
    }
    // geo_render_kernel's step counting and tile-cost recording: the wave's
    // steps into its sharded slot and, where the launch records costs, its
    // largest step count into its tile's
    if (a.step_slots) {
        const uint32_t total = wave_sum_u32(steps);
        const uint32_t slot = (tile.x * (kBlock / 64) + wave) % kStepSlots;
        if (lane == 0 && total) atomicAdd(&a.step_slots[slot * kSlotStride], (unsigned long long)total);
    }
    if (a.tile_cost && src.records_cost()) {
        const uint32_t wmax = wave_max_u32(steps);
        if (lane == 0) atomicAdd(&a.tile_cost[tile.y * tiles_x + tile.x], wmax + a.cost_overhead);
    }
}

// The sky-only GEO_FLAG_SS4 render: one frame (NF = 1), or geo_render_ss_batch's
// frames (NF = kMaxBatchFrames, the frame in blockIdx.z).
template <int KIND, uint32_t NF>
__global__ __launch_bounds__(64) void geo_render_ss_sky_kernel(const RenderArgs a, const FrameBatch<NF> fb,
                                                               const SsPitch<true> o) {
    static_assert(kKernargsFit<RenderArgs, FrameBatch<NF>, SsPitch<true>>);
    wave_block_body<KIND, Shade::kSky, true, false>(a, SkyFrame<NF>{a, fb, NF > 1 ? blockIdx.z : 0u}, o.width());
}

// One disk frame, one sample per pixel, with the side outputs: plain, shifted
// (geo_set_disk_shift) or with its emission (geo_set_disk_emission), x being
// the shade's own argument; direct or adaptive (geo_render_disk_adaptive).
template <int KIND, Shade SHADE, int MODE>
__global__ __launch_bounds__(64) void geo_render_disk_frame_kernel(const RenderArgs a, const FrameBatch<1> fb,
                                                                   const DiskArgs d, const ShadeFrameArg<SHADE> x) {
    static_assert(kKernargsFit<RenderArgs, FrameBatch<1>, DiskArgs, ShadeFrameArg<SHADE>>);
    wave_block_body<KIND, SHADE, false, true, MODE>(a, DiskFrame<ShadeFrameArg<SHADE>>{{a, fb, 0u}, d, x}, 0u);
}

// The same frame with GEO_FLAG_SS4, colour only.  Its arguments stay one
// struct, the output's pitch first: a small argument of its own (the pitch, a
// shift's 24 bytes) is loaded at the kernel's entry, a member of a large one
// where it is used, and as three arguments these nine kernels came out with
// their scalar loads moved and their registers renumbered
// (profiles/wave_block_wrappers_isa.txt).
template <Shade SHADE>
struct SsDiskArgs {
    uint32_t out_width;  // SsPitch<true>'s
    DiskArgs d;
    ShadeFrameArg<SHADE> x;
};
template <int KIND, Shade SHADE>
__global__ __launch_bounds__(64) void geo_render_ss_disk_frame_kernel(const RenderArgs a, const FrameBatch<1> fb,
                                                                      const SsDiskArgs<SHADE> s) {
    static_assert(kKernargsFit<RenderArgs, FrameBatch<1>, SsDiskArgs<SHADE>>);
    wave_block_body<KIND, SHADE, true, false>(a, DiskFrame<ShadeFrameArg<SHADE>>{{a, fb, 0u}, s.d, s.x}, s.out_width);
}

// A disk batch (geo_render_disk_batch, geo_render_ss_batch's disk frames,
// geo_render_emission_batch, geo_render_disk_adaptive_batch): the frame in
// blockIdx.z, colour only; eb is the emission's batch-uniform argument.
template <int KIND, Shade SHADE, bool SS, int MODE>
__global__ __launch_bounds__(64) void geo_render_disk_batch_kernel(const RenderArgs a, const DiskBatchArgs db,
                                                                   const ShadeBatchArg<SHADE> eb,
                                                                   const SsPitch<SS> o) {
    static_assert(kKernargsFit<RenderArgs, DiskBatchArgs, ShadeBatchArg<SHADE>, SsPitch<SS>>);
    wave_block_body<KIND, SHADE, SS, false, MODE>(a, DiskBatchFrame<ShadeBatchArg<SHADE>>{a, db, eb, blockIdx.z},
                                                  o.width());
}

// ---- the one body of the batched disk kernels with the f64 band -----------
// geo_render_disk_ring_kernel's lanes (f32 lanes through MODE's integrator and
// geo::disk_hits_f32, band lanes through geo::disk_hits_band in a cold arm
// behind one ballot, then one geo::disk_shade_hits) with wave_block_body's
// frame source, colour-only output and SS4 resolve.  It varies along
//   SHADE  the shading: Shade::kDisk, kDiskShift, kDiskEmit
//   MODE   the f32 lanes' integrator, as geo_render_disk_ring_kernel's MODE
//          (there: what the band reads of an adaptive DiskRay, the band's step
//          and budget, and the units the step slots and the tile cost then
//          mix); GEO_MODE_ADAPTIVE: geo_render_disk_adaptive_ring_batch
//   SS     GEO_FLAG_SS4, as in wave_block_body (the band's constants are then
//          the sample frame's, and px, py the sample's)
//   SRC    the frame source (DiskBatchFrame)
// band_words: the frame's geo::BandConsts as 8-byte words in the context's
// device table (geo_band_table_kernel); every workgroup copies them to LDS, one
// word per thread, behind the wave-uniform padding return and one barrier.
// The one-frame kernel above (geo_render_disk_ring_kernel, both of its modes)
// keeps the body it has: routed through this one (with DiskFrame as its source
// and its side outputs and its mode as properties) its shaded instantiations
// came out with 81 VGPRs instead of 80, five waves per SIMD instead of six.
template <int KIND, Shade SHADE, bool SS, int MODE, typename SRC>
__device__ __forceinline__ void disk_ring_body(const RenderArgs& a, const SRC& src, const uint2* band_words,
                                               uint32_t out_width) {
    static_assert(KIND != geo::kFlat && SHADE != Shade::kSky, "no capture orbit without a black hole; a disk render");
    static_assert(MODE == GEO_MODE_DIRECT || MODE == GEO_MODE_ADAPTIVE, "the f32 lanes' integrator");
    const uint32_t L = blockIdx.x;
    const uint32_t pos = ((L >> 5) << 3) + (L & 7u);
    const uint32_t wave = (L >> 3) & 3u;
    if (pos >= a.launch_tiles) return;  // the padding of the last group (a whole workgroup)
    const uint32_t tiles_x = a.tiles_x;
    uint2 tile;
    if (a.tile_order) {
        const uint32_t t = a.tile_order[pos];
        tile = make_uint2(t & 0xFFFFu, t >> 16);
    } else {
        tile = make_uint2(pos % tiles_x, a.tile_y0 + pos / tiles_x);
    }
    const uint32_t lane = threadIdx.x & 63u;
    // the band's constants in LDS: one 8-byte word per thread (kBandDwords / 2 <= 64)
    __shared__ double band_lds[kBandDwords / 2u];
    if (threadIdx.x < kBandDwords / 2u) reinterpret_cast<uint2*>(band_lds)[threadIdx.x] = band_words[threadIdx.x];
    __syncthreads();
    const geo::BandConsts& bkl = *reinterpret_cast<const geo::BandConsts*>(band_lds);
    const uint32_t px = tile.x * kTileW + (wave % kWavesX) * kWaveW + lane % kWaveW;
    const uint32_t wl0 = tile.y * kTileH + (wave / kWavesX) * kWaveRows;
    const uint32_t ly = wl0 + lane / kWaveW;
    const uint32_t band = __umulhi(SS ? wl0 >> 1 : wl0, a.band_magic);  // (SS: on output rows, wave_block_body)
    const uint32_t py = a.row0 + band * a.band_stride + (wl0 - band * a.band_rows) + (ly - wl0);
    const bool in_frame = px < a.width && ly < a.nrows && py < a.height;
    uint32_t steps = 0;
    uint32_t colour = 0;  // SS: the sample's colour, kept in a register (a sample out of the frame does not return)
    bool f64_lane = false;
    if (in_frame) {
        float c2x, c2y, c2z, g_obs = 1.0f;
        if constexpr (SHADE == Shade::kDisk)
            geo::pixel_central_dir(src.cam(), src.movement_to_central(), src.psi(), src.kt(), px, py, &c2x, &c2y, &c2z);
        else
            geo::pixel_central_dir_g(src.cam(), src.movement_to_central(), src.psi(), src.kt(), px, py, &c2x, &c2y,
                                     &c2z, &g_obs);
        const float st = geo::central_sin(c2z);
        const float ct = geo::central_rho(c2x, c2y);
        const float rct = geo::rcpf_(ct);
        const geo::PixelConsts& k = src.consts();
        const auto& dk = src.disk();
        geo::DiskRay dr;
        if constexpr (MODE == GEO_MODE_ADAPTIVE)
            geo::disk_ray_adaptive(dk, k, c2x, c2y, ct, rct, &dr);
        else
            geo::disk_ray(dk, k, c2x, c2y, ct, rct, &dr);
        f64_lane = geo::in_band(bkl.kx, ct);
        float lam = 0.0f;
        bool bh = false;
        geo::DiskHits h;
#pragma unroll
        for (int c = 0; c < geo::kDiskMaxCrossings; ++c) {
            h.hit[c] = false;
            h.r[c] = 0.0f;
        }
        if (!f64_lane) {
            float Uk[geo::kDiskMaxCrossings];
            float ang;
            if constexpr (MODE == GEO_MODE_ADAPTIVE)
                ang = geo::geodesic_angle_adaptive_disk<KIND>(k, st, ct, rct, dr, &steps, Uk);
            else
                ang = geo::geodesic_angle_disk<KIND>(k, st, ct, rct, dr, &steps, Uk);
            lam = geo::kPi2 - ang;
            bh = lam < geo::kBlackHoleLambda;
            geo::disk_hits_f32(dk, k, dr, Uk, steps, ang, &h);
        }
        if (geo::ballot_(f64_lane) != 0) {
            if (f64_lane) {
                GEO_COLD_ARM();
                const double l = geo::disk_hits_band(bkl, dk, dr, px, py, &steps, &h);
                lam = (float)l;
                bh = l < (double)geo::kBlackHoleLambda;
            }
        }
        float U = 0.0f, V = 0.0f;
        if (!bh) geo::sky_uv(src.central_to_uv(), c2x, c2y, ct, rct, lam, &U, &V);
        const uint32_t base =
            bh ? geo::kBlackRGBA : geo::sample_sky_qf(level0_quad(a), a.sky_w256, a.sky_h256, a.sky_opaque != 0, U, V);
        const auto& t = src.tex();
        const PaddedSkyQuad dquad{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(t.tex), 0, (int)t.tex_bytes,
                                                                    kBufferRsrcWord3),
                                  t.tex_pitch_b};
        const auto dsample = [&](float Ud, float Vd) {
            return geo::sample_sky_quad_f(dquad, t.tex_w256, t.tex_h256, Ud, Vd);
        };
        float* const none = nullptr;  // a batch draws colour only: no hits, g or q
        if constexpr (SHADE == Shade::kDiskEmit) {
            const auto rfetch = [ramp = src.ramp()](uint32_t i) { return ramp[i]; };
            const auto& ek = src.emission();
            geo::DiskShiftRay sr;
            geo::disk_shift_ray(dk, ek.s, dr, ct, g_obs, &sr);
            colour = geo::disk_shade_hits(dk, dr, h, base, geo::disk_colour_emit(dk, k, ek, sr, dsample, rfetch), none,
                                          none, none);
        } else if constexpr (SHADE == Shade::kDiskShift) {
            const auto& sk = src.shift();
            geo::DiskShiftRay sr;
            geo::disk_shift_ray(dk, sk, dr, ct, g_obs, &sr);
            colour = geo::disk_shade_hits(dk, dr, h, base, geo::disk_colour_shift(k, sk, sr, dsample), none, none, none);
        } else {
            colour = geo::disk_shade_hits(dk, dr, h, base, geo::disk_colour_plain(dsample), none, none, none);
        }
        if constexpr (!SS) a.out_rgba[src.out_base() + (size_t)ly * a.width + px] = colour;
    }
    // every per-lane arm has rejoined: all 64 lanes are active, as the
    // resolve's exchange and the wave reductions need
    if constexpr (SS) {
        const uint32_t resolved = ss_resolve(colour);
        if (in_frame && (lane & 0x11u) == 0u)
            a.out_rgba[src.out_base() + (size_t)(ly >> 1) * out_width + (px >> 1)] = resolved;
    }
    // wave_block_body's epilogue with the ring kernel's tile cost: the wave runs its
    // f32 lanes' loop, then its band lanes' f64 loop at about twice the cost
    // per step
    if (a.step_slots) {
        const uint32_t total = wave_sum_u32(steps);
        const uint32_t slot = (tile.x * (kBlock / 64) + wave) % kStepSlots;
        if (lane == 0 && total) atomicAdd(&a.step_slots[slot * kSlotStride], (unsigned long long)total);
    }
    if (a.tile_cost && src.records_cost()) {
        const uint32_t wmax = wave_max_u32(f64_lane ? 0u : steps) + 2u * wave_max_u32(f64_lane ? steps : 0u);
        if (lane == 0) atomicAdd(&a.tile_cost[tile.y * tiles_x + tile.x], wmax + a.cost_overhead);
    }
}

// ---- geo_render_disk_ring_batch: up to kMaxBatchFrames ring frames in one launch --
// The disk batch, the SS batch's disk frames and the emission batch (SHADE) with
// the band's lanes in f64: disk_ring_body on DiskBatchFrame, the frame in
// blockIdx.z.  MODE: GEO_MODE_DIRECT, or the adaptive disk batch's frames
// likewise (geo_render_disk_adaptive_ring_batch: GEO_MODE_ADAPTIVE).  The argument segment has no room for eight frames'
// geo::BandConsts (8 x 344 bytes beside DiskBatchArgs' 3312), nor for the
// display_to_movement rows they are derived from, so the host computes them
// with the one-frame launch's geo::band_consts (at twice the size under SS4) and
// geo_band_table_kernel, which takes them by value, writes them to the
// context's device table of the call's render-stream slot just before the
// render launch on the same stream; workgroups of frame z copy table[z] to LDS.
struct BandTable {
    geo::BandConsts k[kMaxBatchFrames];
};
static_assert(sizeof(BandTable) == kMaxBatchFrames * 344u && sizeof(BandTable) <= 4096 - 16, "the table by value");
__global__ __launch_bounds__(64) void geo_band_table_kernel(const BandTable t, geo::BandConsts* out) {
    // one workgroup per frame, one 8-byte word per thread
    if (threadIdx.x < kBandDwords / 2u)
        reinterpret_cast<uint2*>(out + blockIdx.x)[threadIdx.x] =
            reinterpret_cast<const uint2*>(&t.k[blockIdx.x])[threadIdx.x];
}

// bands: the table, frame z's constants at bands[z]; eb: the emission's
// batch-uniform argument.
template <int KIND, Shade SHADE, bool SS, int MODE>
__device__ __forceinline__ void disk_ring_batch(const RenderArgs& a, const DiskBatchArgs& db,
                                                const geo::BandConsts* bands, const ShadeBatchArg<SHADE>& eb,
                                                uint32_t out_width) {
    static_assert(kKernargsFit<RenderArgs, DiskBatchArgs, const geo::BandConsts*, ShadeBatchArg<SHADE>, SsPitch<SS>>);
    disk_ring_body<KIND, SHADE, SS, MODE>(a, DiskBatchFrame<ShadeBatchArg<SHADE>>{a, db, eb, blockIdx.z},
                                    reinterpret_cast<const uint2*>(bands + blockIdx.z), out_width);
}

// (amdgpu_waves_per_eu: the one-frame ring kernels' six waves per SIMD as the
// allocator's target of the one-sample instantiations.  Left to itself it gave
// their emission ones 81 VGPRs, one over the class, for the lanes of an SGPR it
// moved to a VGPR: a batch reads its frame's constants through db.f[z] and
// holds more scalars (106) than the one-frame kernel (100).  With the target
// they take 80, the others are unchanged, and none uses scratch;
// profiles/disk_ring_batch_isa.txt.  The GEO_FLAG_SS4 instantiations, a lane
// per sample of the 2W x 2H ring render, have no target: 0.  The
// GEO_MODE_ADAPTIVE instantiations came out in the class with the same
// targets, 76 / 80 / 80 VGPRs one sample and SS4 alike, no scratch;
// profiles/disk_adaptive_ring_batch_isa.txt.)
template <int KIND, Shade SHADE, bool SS, int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SS ? 0 : 6))) void geo_render_disk_ring_batch_kernel(
    const RenderArgs a, const DiskBatchArgs db, const geo::BandConsts* bands, const ShadeBatchArg<SHADE> eb,
    const SsPitch<SS> o) {
    disk_ring_batch<KIND, SHADE, SS, MODE>(a, db, bands, eb, o.width());
}


// ---- longest-first dispatch: the order from recorded tile costs ---------
// Cost classes of an eighth of an octave (the octave and the next three
// bits of the cost, 256 classes), dispatched from the highest class down;
// within a class, tile order.  Two
// kernels: per-chunk class histograms, then each chunk's tiles scattered to
// their positions (and their costs cleared for the next recording).
// eighth-octave classes: on an 8-rank share of the 4K frame the learned
// order runs 0.0316 ms against 0.0325 with half octaves and 0.0314 for the
// exact LPT order (profiles/r04e_cost_class_ab.txt)
constexpr uint32_t kSubOctaveBits = 3;
constexpr int kCostClasses = 32 << kSubOctaveBits;
constexpr uint32_t kOrderChunk = 1024;  // tiles per workgroup

// class = (octave << bits) + the top `bits` mantissa bits below the leading one
__device__ __forceinline__ uint32_t cost_class(uint32_t c) {
    if (c == 0u) return 0u;
    const uint32_t o = 31u - (uint32_t)__clz(c);
    const uint32_t m = (c << (31u - o)) >> (31u - kSubOctaveBits) & ((1u << kSubOctaveBits) - 1u);
    return (o << kSubOctaveBits) + m;
}

__global__ __launch_bounds__(256) void geo_order_hist(const uint32_t* __restrict__ cost, uint32_t n,
                                                      uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kCostClasses];
    if (threadIdx.x < kCostClasses) h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lo = blockIdx.x * kOrderChunk, hi = min(n, lo + kOrderChunk);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256u) atomicAdd(&h[cost_class(cost[i])], 1u);
    __syncthreads();
    if (threadIdx.x < kCostClasses) hist[blockIdx.x * kCostClasses + threadIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(256) void geo_order_scatter(uint32_t* __restrict__ cost, uint32_t n,
                                                         const uint32_t* __restrict__ hist, uint32_t tiles_x,
                                                         uint32_t* __restrict__ order) {
    __shared__ uint32_t tot[kCostClasses], base[kCostClasses];
    const uint32_t c = threadIdx.x;
    if (c < kCostClasses) {
        uint32_t t = 0u, mine = 0u;
        for (uint32_t g = 0; g < gridDim.x; ++g) {
            const uint32_t v = hist[g * kCostClasses + c];
            t += v;
            if (g < blockIdx.x) mine += v;
        }
        tot[c] = t;
        base[c] = mine;
    }
    __syncthreads();
    if (c < kCostClasses) {
        uint32_t above = 0u;  // tiles of the higher classes, dispatched first
        for (uint32_t k = c + 1u; k < (uint32_t)kCostClasses; ++k) above += tot[k];
        base[c] += above;
    }
    __syncthreads();
    const uint32_t lo = blockIdx.x * kOrderChunk, hi = min(n, lo + kOrderChunk);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256u) {
        const uint32_t pos = atomicAdd(&base[cost_class(cost[i])], 1u);
        order[pos] = ((i / tiles_x) << 16) | (i % tiles_x);
        cost[i] = 0u;
    }
}

// Frame row y of frame f comes from rank r = (y / band_rows) % world, local
// row ((y / band_rows) / world) * band_rows + y % band_rows of that rank's
// packed bands (geo_render_bands' layout).  One thread per 16 B (W % 4 == 0)
// or per pixel.
template <typename T>
__global__ __launch_bounds__(256) void geo_assemble_kernel(const uint8_t* __restrict__ src, size_t rank_stride,
                                                           size_t frame_stride, uint32_t world, uint32_t band_rows,
                                                           uint32_t row_units, uint32_t height,
                                                           uint8_t* __restrict__ dst) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const uint32_t y = blockIdx.y;
    const uint32_t f = blockIdx.z;
    if (x >= row_units) return;
    const uint32_t b = y / band_rows;
    const uint32_t r = b % world;
    const size_t lrow = (size_t)(b / world) * band_rows + y % band_rows;
    const size_t row_bytes = (size_t)row_units * sizeof(T);
    const T* s = reinterpret_cast<const T*>(src + r * rank_stride + f * frame_stride + lrow * row_bytes);
    T* d = reinterpret_cast<T*>(dst + ((size_t)f * height + y) * row_bytes);
    d[x] = s[x];
}

// The same from RGB24-packed bands (geo_pack_rgb; alpha restored to 255):
// one thread per 4 pixels (12 B in, 16 B out), W % 4 == 0.
__global__ __launch_bounds__(256) void geo_assemble_rgb_kernel(const uint8_t* __restrict__ src, size_t rank_stride,
                                                               size_t frame_stride, uint32_t world,
                                                               uint32_t band_rows, uint32_t quads, uint32_t height,
                                                               uint8_t* __restrict__ dst) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const uint32_t y = blockIdx.y;
    const uint32_t f = blockIdx.z;
    if (x >= quads) return;
    const uint32_t b = y / band_rows;
    const uint32_t r = b % world;
    const size_t lrow = (size_t)(b / world) * band_rows + y % band_rows;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src + r * rank_stride + f * frame_stride +
                                                         lrow * (size_t)quads * 12u) + 3u * x;
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    uint4 o;
    o.x = (w0 & 0x00FFFFFFu) | 0xFF000000u;
    o.y = (w0 >> 24) | ((w1 & 0xFFFFu) << 8) | 0xFF000000u;
    o.z = (w1 >> 16) | ((w2 & 0xFFu) << 16) | 0xFF000000u;
    o.w = (w2 >> 8) | 0xFF000000u;
    reinterpret_cast<uint4*>(dst + ((size_t)f * height + y) * (size_t)quads * 16u)[x] = o;
}

// The lead layout (geo_assemble_lead): cycles of lead*band_rows rows of rank 0
// followed by one band_rows band per peer.  QUAD: one thread per 4 pixels
// (16 B out; peers' rows RGBA8 or RGB24), else one per pixel (RGBA8 only).
// The row's source (rank 0's own bands or a peer's) is block-uniform.
template <bool QUAD>
__global__ __launch_bounds__(256) void geo_assemble_lead_kernel(
    const uint8_t* __restrict__ lead_src, size_t lead_frame_stride, uint32_t lead_rows,
    const uint8_t* __restrict__ src, size_t rank_stride, size_t frame_stride, uint32_t world, uint32_t band_rows,
    uint32_t units, uint32_t height, uint32_t src_bpp, uint8_t* __restrict__ dst) {
    using T = typename std::conditional<QUAD, uint4, uint32_t>::type;
    constexpr uint32_t kPix = QUAD ? 4u : 1u;  // pixels per unit
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const uint32_t y = blockIdx.y;
    const uint32_t f = blockIdx.z;
    if (x >= units) return;
    const uint32_t cycle = lead_rows + (world - 1u) * band_rows;
    const uint32_t c = y / cycle, off = y % cycle;
    const size_t rgba_row = (size_t)units * sizeof(T);
    T* d = reinterpret_cast<T*>(dst + ((size_t)f * height + y) * rgba_row);
    if (off < lead_rows) {
        const size_t lrow = (size_t)c * lead_rows + off;
        d[x] = reinterpret_cast<const T*>(lead_src + f * lead_frame_stride + lrow * rgba_row)[x];
        return;
    }
    const uint32_t o2 = off - lead_rows;
    const uint32_t r = 1u + o2 / band_rows;
    const size_t lrow = (size_t)c * band_rows + o2 % band_rows;
    const uint8_t* row = src + r * rank_stride + f * frame_stride + lrow * (size_t)units * kPix * src_bpp;
    if constexpr (QUAD) {
        if (src_bpp == 3u) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(row) + 3u * x;
            const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            uint4 o;
            o.x = (w0 & 0x00FFFFFFu) | 0xFF000000u;
            o.y = (w0 >> 24) | ((w1 & 0xFFFFu) << 8) | 0xFF000000u;
            o.z = (w1 >> 16) | ((w2 & 0xFFu) << 16) | 0xFF000000u;
            o.w = (w2 >> 8) | 0xFF000000u;
            d[x] = o;
            return;
        }
    }
    d[x] = reinterpret_cast<const T*>(row)[x];
}

// RGBA8 -> RGB24 (alpha dropped: every frame pixel is opaque after the clear),
// 4 pixels per thread.
__global__ __launch_bounds__(256) void geo_pack_rgb_kernel(const uint4* __restrict__ src, uint64_t quads,
                                                           uint32_t* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= quads) return;
    const uint4 p = src[i];
    uint32_t* d = dst + 3u * i;
    d[0] = (p.x & 0x00FFFFFFu) | (p.y << 24);
    d[1] = ((p.y >> 8) & 0xFFFFu) | (p.z << 16);
    d[2] = ((p.z >> 16) & 0xFFu) | (p.w << 8);
}

__global__ __launch_bounds__(kStepSlots) void geo_steps_finalize(unsigned long long* slots,
                                                                  unsigned long long* total) {
    __shared__ unsigned long long s[kStepSlots / 64];
    const int i = threadIdx.x;
    unsigned long long v = slots[i * kSlotStride];
    slots[i * kSlotStride] = 0;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((i & 63) == 0) s[i >> 6] = v;
    __syncthreads();
    if (i == 0) {
        unsigned long long t = 0;
        for (int j = 0; j < kStepSlots / 64; ++j) t += s[j];
        *total += t;
    }
}

// f64 restatement of SphereRayTracer::solve_geodesic (sphere_ray_tracer.rs:60-193),
// operation for operation (no contraction).  The radial cases and
// pre-filters (:60-119): false with the result in *early, else the initial
// u' (:123).
__device__ bool solve_geodesic_f64_init(double sphere_r, double schwarz_r, double r, double energy, double rotation,
                                        bool r_falling, double* early, double* u_bar0) {
    const double NO_VALUE = GEO_NO_VALUE;
    const double PI = 3.14159265358979323846;
    const double b = rotation / energy;
    const bool outside = r > schwarz_r;
    const bool sphere_outside = sphere_r > schwarz_r;
    const bool inside_sphere = r < sphere_r;
    if (rotation < 1e-10) {
        if (inside_sphere) {
            if (outside)
                *early = r_falling ? (schwarz_r == 0. ? PI : NO_VALUE) : 0.;
            else
                *early = sphere_outside ? (energy > 0. ? 0. : NO_VALUE) : 0.;
        } else {
            *early = (sphere_outside && r_falling) ? 0. : NO_VALUE;
        }
        return false;
    }
    const bool barrier_3r_2 = (schwarz_r > 0.) && 1. / (b * b) < 4. / (27. * schwarz_r * schwarz_r);
    const double r3_2 = 3. * schwarz_r / 2.;
    const bool different_sides_3r_2 = ((r < r3_2) != (sphere_r < r3_2)) && fabs(r - r3_2) > 1e-10;
    if ((inside_sphere && !sphere_outside) || (!outside && sphere_outside && energy < 0.) ||
        (barrier_3r_2 && different_sides_3r_2) || (r < r3_2 && inside_sphere && r_falling) ||
        (r > r3_2 && !inside_sphere && !r_falling)) {
        *early = NO_VALUE;
        return false;
    }
    *u_bar0 = (r_falling ? 1. : -1.) * sqrt(1. / (b * b) - (1. - schwarz_r / r) / (r * r));
    return true;
}

// The f64 solve (sphere_ray_tracer.rs:121-193), restructured for latency.
// A fan is one lane per node, 400 lanes = 7 waves, so its time is
// the longest node's dependent chain: the literal loop spends ~60 f64
// instructions per step (two f64 divisions by 6 among them), this one the
// scaled 14-op RK4 of the f32 kernel (geo_pixel.h rk4_step) in f64 --
// U = c u, c = 3 rs/2 (1 for rs = 0), F(U) = U(U - 1) (-U in flat space),
// the thresholds scaled alike, Newton's ratio scale-free.  It is the same
// algorithm (stages, tests, Newton) with a different rounding of the f64
// intermediates: the fan agrees with the literal f64 restatement to within
// one f32 ulp (tests/test_gpu_parity.py, the fan tolerance).
template <bool FLAT>
__device__ __forceinline__ double fan_F(double U) {
    return FLAT ? -U : __builtin_fma(U, U, -U);
}
template <bool FLAT>
__device__ __forceinline__ void fan_rk4(double U, double V, double h, double hh, double hh2, double hhh, double h6,
                                        double h2_6, double* NU, double* NV) {
    const double fu = fan_F<FLAT>(U);
    const double au = __builtin_fma(hh, V, U);
    const double uh = __builtin_fma(h, V, U);
    const double fa = fan_F<FLAT>(au);
    const double bu = __builtin_fma(hh2, fu, au);
    const double fb = fan_F<FLAT>(bu);
    const double cu = __builtin_fma(hhh, fa, uh);
    const double fc = fan_F<FLAT>(cu);
    const double fab = fa + fb;
    *NU = __builtin_fma(h2_6, fu + fab, uh);
    *NV = __builtin_fma(h6, __builtin_fma(2.0, fab, fu) + fc, V);
}
// One step of the literal loop's tests (:134, :150, :184) from (U, V) to
// (NU, NV): 0 continue, 1 crossing (Newton), 2 stop without a value.
template <bool FLAT>
__device__ __forceinline__ int fan_test(double U, double V, double NU, double SU, double BD, double HU) {
    if (!FLAT && U > HU && V > 0.) return 2;  // the loop test on the pre-step state (:134)
    if ((NU > SU) != (U > SU)) return 1;
    if (NU < BD) return 2;
    return 0;
}
// A lane's chain of RK4 steps is the fan's critical path, so the exit branch
// (which waits for the newest state's compares) is taken once per kFanGroup
// steps: the group's flags are formed without branches, and a group that
// stops is replayed step by step from its start (the same arithmetic, so the
// same result as testing every step).  Groups of 8 and 16 are +-4 % and up
// to +22 %.
constexpr int kFanGroup = 4;
template <bool FLAT>
__device__ double fan_integrate(double sphere_r, double schwarz_r, uint32_t max_iter, double step, double r,
                                double u_bar0) {
    const double NO_VALUE = GEO_NO_VALUE;
    const double r3_2 = 3. * schwarz_r / 2.;
    const double c = FLAT ? 1. : r3_2;
    const double u0 = 1. / r;
    const double SU = c / sphere_r;                                      // sphere_u
    const double BD = c * (0.9 * fmin(u0, 1. / fmax(sphere_r, r3_2)));  // bound
    const double HU = FLAT ? __builtin_inf() : c / schwarz_r;           // schwarz_u
    const double h = step, hh = step / 2., hh2 = step * step / 4., hhh = step * step / 2., h6 = step / 6.,
                 h2_6 = step * step / 6.;
    double U = c * u0, V = c * u_bar0;
    if (!(U > 0.)) return NO_VALUE;
    double angle = 0.;
    uint32_t it = 0;
    // whole groups while the budget allows; a stopping group falls through
    // to the per-step loop below from its start state
    while (it + kFanGroup <= max_iter) {
        double su[kFanGroup + 1], sv[kFanGroup + 1];
        su[0] = U;
        sv[0] = V;
        bool stop = false;
#pragma unroll
        for (int j = 0; j < kFanGroup; ++j) {
            fan_rk4<FLAT>(su[j], sv[j], h, hh, hh2, hhh, h6, h2_6, &su[j + 1], &sv[j + 1]);
            stop |= fan_test<FLAT>(su[j], sv[j], su[j + 1], SU, BD, HU) != 0;
        }
        if (stop) break;
        U = su[kFanGroup];
        V = sv[kFanGroup];
#pragma unroll
        for (int j = 0; j < kFanGroup; ++j) angle += step;  // the literal accumulation (:190)
        it += kFanGroup;
    }
    for (; it < max_iter; ++it) {
        double NU, NV;
        fan_rk4<FLAT>(U, V, h, hh, hh2, hhh, h6, h2_6, &NU, &NV);
        const int t = fan_test<FLAT>(U, V, NU, SU, BD, HU);
        if (t == 2) return NO_VALUE;
        if (t == 1) {
            // Newton on the step length from the steeper end (:150-182)
            double ns, wu, wv;
            if (fabs(V) > fabs(NV)) {
                ns = 0.;
                wu = U;
                wv = V;
            } else {
                ns = h;
                wu = NU;
                wv = NV;
            }
            for (int n = 0; n < 3; ++n) {
                ns -= (wu - SU) / wv;
                const double n2 = ns * ns;
                fan_rk4<FLAT>(U, V, ns, ns / 2., n2 / 4., n2 / 2., ns / 6., n2 / 6., &wu, &wv);
            }
            return angle + ns;
        }
        U = NU;
        V = NV;
        angle += step;
    }
    // budget exhausted; the literal loop re-tests the final state only
    // against :134 and `u > 0`, both of which end without a value too
    return NO_VALUE;
}

__global__ void geo_fan_kernel(double sphere_r, double schwarz_r, uint32_t max_iter, double step,
                               uint32_t n, double r, float* fan) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double PI = 3.14159265358979323846;
    const double FRAC_PI_2 = 1.57079632679489661923;
    // solve_ray_fan (sphere_ray_tracer.rs:37-53)
    const double theta = FRAC_PI_2 - PI * (double)i / ((double)n - 1.);
    const double rotation = r * cos(theta);
    bool r_falling;
    double energy;
    if (r < schwarz_r) {
        r_falling = false;
        energy = sin(-theta) * sqrt(-1. + schwarz_r / r);
    } else {
        r_falling = theta > 0.;
        energy = sqrt(1. - schwarz_r / r);
    }
    double angle, u_bar0;
    if (solve_geodesic_f64_init(sphere_r, schwarz_r, r, energy, rotation, r_falling, &angle, &u_bar0)) {
        angle = schwarz_r == 0. ? fan_integrate<true>(sphere_r, schwarz_r, max_iter, step, r, u_bar0)
                                : fan_integrate<false>(sphere_r, schwarz_r, max_iter, step, r, u_bar0);
    }
    fan[i] = (float)(FRAC_PI_2 - angle);
}

// The template kernels of the code object, in the order it holds them.  A
// template kernel is instantiated, and laid out after the plain kernels above,
// at its first use in the translation unit; these uses come before any host
// code, so this list, not the order in which launchers happen to be written,
// fixes the kernels' set and order, and the host code may be arranged for its
// readers.  (Explicit instantiation definitions do not serve: they are emitted
// where they stand, ahead of the plain kernels.)  tools/isa.sh on a commit and
// its parent shows a kernel added, dropped or moved.
[[maybe_unused]] void kernel_order() {  // never called
    (void)geo_render_kernel<GEO_MODE_FAN, geo::kCurvedOut, true, 1, false>;
    (void)geo_render_kernel<GEO_MODE_FAN, geo::kCurvedOut, false, 1, false>;
    (void)geo_render_kernel<GEO_MODE_FAN, geo::kCurvedOut, false, kMaxBatchFrames, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedOut, false, 1, true>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedOut, true, 1, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedOut, false, 1, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedOut, false, kMaxBatchFrames, true>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedOut, false, kMaxBatchFrames, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedIn, false, 1, true>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedIn, true, 1, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedIn, false, 1, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedIn, false, kMaxBatchFrames, true>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kCurvedIn, false, kMaxBatchFrames, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kFlat, true, 1, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kFlat, false, 1, false>;
    (void)geo_render_kernel<GEO_MODE_ADAPTIVE, geo::kFlat, false, kMaxBatchFrames, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedOut, false, 1, true>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedOut, true, 1, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedOut, false, 1, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedOut, false, kMaxBatchFrames, true>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedOut, false, kMaxBatchFrames, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedIn, false, 1, true>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedIn, true, 1, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedIn, false, 1, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedIn, false, kMaxBatchFrames, true>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kCurvedIn, false, kMaxBatchFrames, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kFlat, true, 1, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kFlat, false, 1, false>;
    (void)geo_render_kernel<GEO_MODE_DIRECT, geo::kFlat, false, kMaxBatchFrames, false>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedOut, Shade::kDisk, GEO_MODE_DIRECT>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedIn, Shade::kDisk, GEO_MODE_DIRECT>;
    (void)geo_render_disk_frame_kernel<geo::kFlat, Shade::kDisk, GEO_MODE_DIRECT>;
    (void)geo_assemble_kernel<uint4>;
    (void)geo_assemble_kernel<uint32_t>;
    (void)geo_assemble_lead_kernel<true>;
    (void)geo_assemble_lead_kernel<false>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedOut, Shade::kDiskShift, GEO_MODE_DIRECT>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedIn, Shade::kDiskShift, GEO_MODE_DIRECT>;
    (void)geo_render_disk_frame_kernel<geo::kFlat, Shade::kDiskShift, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDiskShift, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDiskShift, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDiskShift, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDisk, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDisk, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDisk, false, GEO_MODE_DIRECT>;
    (void)geo_render_ss_sky_kernel<geo::kCurvedOut, 1>;
    (void)geo_render_ss_sky_kernel<geo::kCurvedIn, 1>;
    (void)geo_render_ss_sky_kernel<geo::kFlat, 1>;
    (void)geo_render_ss_disk_frame_kernel<geo::kCurvedOut, Shade::kDisk>;
    (void)geo_render_ss_disk_frame_kernel<geo::kCurvedIn, Shade::kDisk>;
    (void)geo_render_ss_disk_frame_kernel<geo::kFlat, Shade::kDisk>;
    (void)geo_render_ss_disk_frame_kernel<geo::kCurvedOut, Shade::kDiskShift>;
    (void)geo_render_ss_disk_frame_kernel<geo::kCurvedIn, Shade::kDiskShift>;
    (void)geo_render_ss_disk_frame_kernel<geo::kFlat, Shade::kDiskShift>;
    (void)geo_render_ss_sky_kernel<geo::kCurvedOut, kMaxBatchFrames>;
    (void)geo_render_ss_sky_kernel<geo::kCurvedIn, kMaxBatchFrames>;
    (void)geo_render_ss_sky_kernel<geo::kFlat, kMaxBatchFrames>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDisk, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDisk, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDisk, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDiskShift, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDiskShift, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDiskShift, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedOut, Shade::kDiskEmit, GEO_MODE_DIRECT>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedIn, Shade::kDiskEmit, GEO_MODE_DIRECT>;
    (void)geo_render_disk_frame_kernel<geo::kFlat, Shade::kDiskEmit, GEO_MODE_DIRECT>;
    (void)geo_render_ss_disk_frame_kernel<geo::kCurvedOut, Shade::kDiskEmit>;
    (void)geo_render_ss_disk_frame_kernel<geo::kCurvedIn, Shade::kDiskEmit>;
    (void)geo_render_ss_disk_frame_kernel<geo::kFlat, Shade::kDiskEmit>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDiskEmit, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDiskEmit, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDiskEmit, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDiskEmit, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDiskEmit, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDiskEmit, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedOut, Shade::kDisk, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedIn, Shade::kDisk, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedOut, Shade::kDiskShift, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedIn, Shade::kDiskShift, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedOut, Shade::kDiskEmit, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedIn, Shade::kDiskEmit, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDisk, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDisk, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDiskShift, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDiskShift, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDiskEmit, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDiskEmit, false, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDisk, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDisk, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDiskShift, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDiskShift, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDiskEmit, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDiskEmit, true, GEO_MODE_DIRECT>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedOut, Shade::kDiskEmit, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedOut, Shade::kDiskShift, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedOut, Shade::kDisk, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedIn, Shade::kDiskEmit, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedIn, Shade::kDiskShift, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_frame_kernel<geo::kCurvedIn, Shade::kDisk, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_frame_kernel<geo::kFlat, Shade::kDiskEmit, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_frame_kernel<geo::kFlat, Shade::kDiskShift, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_frame_kernel<geo::kFlat, Shade::kDisk, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDiskEmit, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDiskEmit, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDiskShift, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDiskShift, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDisk, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedOut, Shade::kDisk, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDiskEmit, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDiskEmit, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDiskShift, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDiskShift, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDisk, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kCurvedIn, Shade::kDisk, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDiskEmit, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDiskEmit, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDiskShift, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDiskShift, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDisk, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_batch_kernel<geo::kFlat, Shade::kDisk, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedOut, Shade::kDisk, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedIn, Shade::kDisk, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedOut, Shade::kDiskShift, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedIn, Shade::kDiskShift, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedOut, Shade::kDiskEmit, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_kernel<geo::kCurvedIn, Shade::kDiskEmit, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDisk, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDisk, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDiskShift, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDiskShift, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDiskEmit, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDiskEmit, false, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDisk, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDisk, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDiskShift, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDiskShift, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedOut, Shade::kDiskEmit, true, GEO_MODE_ADAPTIVE>;
    (void)geo_render_disk_ring_batch_kernel<geo::kCurvedIn, Shade::kDiskEmit, true, GEO_MODE_ADAPTIVE>;
}

}  // namespace
