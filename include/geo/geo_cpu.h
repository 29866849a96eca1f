/*
 * geo_cpu.h — the CPU baseline path (libgeo_cpu.so), SURVEY.md §8b's
 * geo_render_cpu: the product's per-pixel header (geo_pixel.h, the same f32
 * operation sequence the gfx950 kernel runs) compiled for the host, scalar,
 * over std::thread row blocks ("the same FP32 integrator
 * header, scalar, run over std::thread row blocks").
 *
 * It is the reported-but-not-optimised baseline bench.py times beside the
 * GPU (north_star: "a CPU reference path ... timed in the same run").  It is
 * a separate library: libgeo.so and the Python package never load it, so the
 * product has no CPU fallback (geo_ctx_create fails without a HIP device).
 * Output equals geo_render_rows' bit for bit (tests/test_cpu_baseline.py).
 * GEO_FLAG_MIPS builds the same 4-level chain as geo_set_sky and takes each
 * pixel's level of detail from its frame-aligned 2 x 2 quad, tracing the
 * quad partners outside the frame or the requested rows as the kernel's
 * helper lanes do; any row0 and row_step are accepted.
 * GEO_FLAG_SS4 (geo.h) is taken by all three entry points under the device's
 * rules (GEO_MODE_DIRECT, GEO_FLAG_DISK and GEO_FLAG_DEFER_STEPS at most, width
 * and height at most 2^19; out_mask, out_uv, out_steps, out_hits and out_g must
 * be NULL): output row i is frame row row0 + i row_step, its samples are rows
 * 2 (row0 + i row_step) and the next of the 2 width x 2 height frame, traced
 * through the same header and resolved with the kernel's integer rule;
 * steps_total counts every sample's steps.
 */
#ifndef GEO_GEO_CPU_H
#define GEO_GEO_CPU_H

#include <stdint.h>

#include "geo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows row0, row0 + row_step, ... (nrows of them) of a width x height frame,
 * in the layout of geo_render_rows' outputs (row i of the outputs = frame row
 * row0 + i row_step).  sky_rgba8: the sky texture (row-major RGBA8, host);
 * fan/n_fan: the ray fan (GEO_MODE_FAN only).  out_rgba8 is required (read
 * too under GEO_FLAG_COMPOSITE); out_mask, out_uv, out_steps and steps_total
 * may be NULL.  threads <= 0: std::thread::hardware_concurrency().  Returns
 * GEO_OK or GEO_EINVAL.  Scenes and skies geo_render_rows or geo_set_sky
 * reject are rejected here too (max_steps > 2^24, a sky side > 2^20, a
 * padded mip chain of 2^31 bytes or more), so the bit-for-bit equality holds
 * for every scene and sky either path accepts; row0 and row_step are free
 * (the device's GEO_FLAG_MIPS even-row rule does not apply).  Blocking;
 * reentrant. */
int geo_render_cpu(const geo_frame* frame, const geo_scene* scene, const uint8_t* sky_rgba8, uint32_t sky_w,
                   uint32_t sky_h, const float* fan, uint32_t n_fan, uint32_t width, uint32_t height, uint32_t row0,
                   uint32_t nrows, uint32_t row_step, int threads, uint8_t* out_rgba8, uint8_t* out_mask,
                   float* out_uv, uint32_t* out_steps, unsigned long long* steps_total);

/* geo_render_cpu with the thin disk of GEO_FLAG_DISK (geo.h): scene->flags
 * must carry GEO_FLAG_DISK (geo_render_cpu itself rejects it), under the
 * rules of geo_render_rows and geo_set_disk.  disk_rgba8: the disk texture
 * (row-major RGBA8, host, disk_w x disk_h); out_hits (optional, host):
 * nrows*width*3*2 floats, the layout of geo_disk_hits_next_render.  Through
 * the kernel's header (csrc/geo_disk.h): output equal to the GPU's bit for
 * bit. */
int geo_render_cpu_disk(const geo_frame* frame, const geo_scene* scene, const uint8_t* sky_rgba8, uint32_t sky_w,
                        uint32_t sky_h, const float* fan, uint32_t n_fan, uint32_t width, uint32_t height,
                        uint32_t row0, uint32_t nrows, uint32_t row_step, int threads, uint8_t* out_rgba8,
                        uint8_t* out_mask, float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                        const geo_disk* disk, const uint8_t* disk_rgba8, uint32_t disk_w, uint32_t disk_h,
                        float* out_hits);

/* geo_render_cpu_disk with the shading of geo_set_disk_shift (geo.h): shift
 * NULL draws the unshaded disk; otherwise its fields and the r_in > 1.5 rs
 * rule are checked as the device checks them.  out_g (optional, host):
 * nrows*width*3 floats, the layout of geo_disk_shift_next_render, written
 * only when shift is given.  Output equal to the GPU's bit for bit. */
int geo_render_cpu_disk_shift(const geo_frame* frame, const geo_scene* scene, const uint8_t* sky_rgba8, uint32_t sky_w,
                              uint32_t sky_h, const float* fan, uint32_t n_fan, uint32_t width, uint32_t height,
                              uint32_t row0, uint32_t nrows, uint32_t row_step, int threads, uint8_t* out_rgba8,
                              uint8_t* out_mask, float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                              const geo_disk* disk, const uint8_t* disk_rgba8, uint32_t disk_w, uint32_t disk_h,
                              float* out_hits, const geo_disk_shift* shift, float* out_g);

/* geo_render_cpu_disk with the emission of geo_set_disk_emission (geo.h):
 * emission NULL draws the unshaded disk (ramp and n are then ignored);
 * otherwise its fields, the ramp (n RGBA8 entries, host), n and the
 * r_in > 1.5 rs rule are checked as the device checks them.  out_g and out_q
 * (optional, host): nrows*width*3 floats each, the layouts of
 * geo_disk_shift_next_render and geo_disk_emission_next_render, written only
 * when emission is given.  GEO_FLAG_SS4 under the device's rules (out_g and
 * out_q must then be NULL).  Output equal to the GPU's bit for bit. */
int geo_render_cpu_disk_emission(const geo_frame* frame, const geo_scene* scene, const uint8_t* sky_rgba8,
                                 uint32_t sky_w, uint32_t sky_h, const float* fan, uint32_t n_fan, uint32_t width,
                                 uint32_t height, uint32_t row0, uint32_t nrows, uint32_t row_step, int threads,
                                 uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv, uint32_t* out_steps,
                                 unsigned long long* steps_total, const geo_disk* disk, const uint8_t* disk_rgba8,
                                 uint32_t disk_w, uint32_t disk_h, float* out_hits, const geo_disk_emission* emission,
                                 const uint8_t* ramp_rgba8, uint32_t n, float* out_g, float* out_q);

/* geo_render_cpu_disk_emission with the state of geo_set_disk_ring_f64
 * (geo.h, GEO_HAS_DISK_RING_F64) as a trailing argument: ring_f64 != 0 takes
 * the disk's band lanes (|b/b_c - 1| < GEO_RING_X on the f32 ray) through the
 * f64 path of csrc/geo_band.h, under the device's rules: GEO_FLAG_SS4 with
 * ring_f64 != 0 is GEO_EINVAL, GEO_FLAG_DISK | GEO_FLAG_RING_F64 stays
 * GEO_EINVAL, and rs = 0 ignores it.  ring_f64 == 0 is
 * geo_render_cpu_disk_emission.  Output equal to the GPU's bit for bit. */
int geo_render_cpu_disk_ring_f64(const geo_frame* frame, const geo_scene* scene, const uint8_t* sky_rgba8,
                                 uint32_t sky_w, uint32_t sky_h, const float* fan, uint32_t n_fan, uint32_t width,
                                 uint32_t height, uint32_t row0, uint32_t nrows, uint32_t row_step, int threads,
                                 uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv, uint32_t* out_steps,
                                 unsigned long long* steps_total, const geo_disk* disk, const uint8_t* disk_rgba8,
                                 uint32_t disk_w, uint32_t disk_h, float* out_hits, const geo_disk_emission* emission,
                                 const uint8_t* ramp_rgba8, uint32_t n, float* out_g, float* out_q, int ring_f64);

/* The same for the shaded render: geo_render_cpu_disk_shift with a trailing
 * ring_f64 (ring_f64 == 0 is geo_render_cpu_disk_shift). */
int geo_render_cpu_disk_shift_ring_f64(const geo_frame* frame, const geo_scene* scene, const uint8_t* sky_rgba8,
                                       uint32_t sky_w, uint32_t sky_h, const float* fan, uint32_t n_fan,
                                       uint32_t width, uint32_t height, uint32_t row0, uint32_t nrows,
                                       uint32_t row_step, int threads, uint8_t* out_rgba8, uint8_t* out_mask,
                                       float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                                       const geo_disk* disk, const uint8_t* disk_rgba8, uint32_t disk_w,
                                       uint32_t disk_h, float* out_hits, const geo_disk_shift* shift, float* out_g,
                                       int ring_f64);

/* The disk frame in GEO_MODE_ADAPTIVE (geo.h, geo_render_disk_adaptive):
 * geo_render_cpu_disk_emission's arguments and a trailing shift.  emission
 * non-NULL draws the emission and takes the shift's place, as on the device
 * (shift is then not read); otherwise shift non-NULL draws the shifted disk;
 * both NULL, the unshaded one.  out_g is written with either, out_q with the
 * emission.  The scene carries GEO_MODE_ADAPTIVE and GEO_FLAG_DISK, with
 * GEO_FLAG_DEFER_STEPS at most, under the device's rules (GEO_EINVAL for a
 * GEO_MODE_DIRECT or GEO_MODE_FAN scene, for GEO_FLAG_SS4 and for a broken
 * disk, shift or emission rule); every other geo_render_cpu_disk* function
 * keeps refusing the adaptive mode.  It runs the kernels' header
 * (geo::geodesic_angle_adaptive_disk): output equal to the GPU's bit for bit. */
int geo_render_cpu_disk_adaptive(const geo_frame* frame, const geo_scene* scene, const uint8_t* sky_rgba8,
                                 uint32_t sky_w, uint32_t sky_h, const float* fan, uint32_t n_fan, uint32_t width,
                                 uint32_t height, uint32_t row0, uint32_t nrows, uint32_t row_step, int threads,
                                 uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv, uint32_t* out_steps,
                                 unsigned long long* steps_total, const geo_disk* disk, const uint8_t* disk_rgba8,
                                 uint32_t disk_w, uint32_t disk_h, float* out_hits, const geo_disk_emission* emission,
                                 const uint8_t* ramp_rgba8, uint32_t n, float* out_g, float* out_q,
                                 const geo_disk_shift* shift);

/* geo_render_cpu_disk_adaptive with the state of geo_set_disk_ring_f64 as a
 * trailing argument (geo.h, geo_render_disk_adaptive_ring,
 * GEO_HAS_DISK_ADAPTIVE_RING): ring_f64 != 0 takes the band's lanes
 * (|b/b_c - 1| < GEO_RING_X on the f32 ray) through the f64 path of
 * csrc/geo_band.h with the scene's step and max_steps as its fixed step and
 * budget, and every other lane through the adaptive integrator, under the
 * device's rules (rs = 0 ignores it).  ring_f64 == 0 is
 * geo_render_cpu_disk_adaptive.  Output equal to the GPU's bit for bit.  The
 * statuses differ from the device's where this path has no context: a NULL
 * disk is GEO_EINVAL here, as in every geo_render_cpu_disk* function (the
 * device call returns GEO_ESTATE while no disk is set), and ring_f64 == 0
 * draws the state-off frame where the device call returns GEO_ESTATE. */
int geo_render_cpu_disk_adaptive_ring_f64(const geo_frame* frame, const geo_scene* scene, const uint8_t* sky_rgba8,
                                          uint32_t sky_w, uint32_t sky_h, const float* fan, uint32_t n_fan,
                                          uint32_t width, uint32_t height, uint32_t row0, uint32_t nrows,
                                          uint32_t row_step, int threads, uint8_t* out_rgba8, uint8_t* out_mask,
                                          float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                                          const geo_disk* disk, const uint8_t* disk_rgba8, uint32_t disk_w,
                                          uint32_t disk_h, float* out_hits, const geo_disk_emission* emission,
                                          const uint8_t* ramp_rgba8, uint32_t n, float* out_g, float* out_q,
                                          const geo_disk_shift* shift, int ring_f64);

#ifdef __cplusplus
}
#endif

#endif /* GEO_GEO_CPU_H */
