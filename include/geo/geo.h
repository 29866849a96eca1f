/*
 * geo.h — C-ABI of libgeo.so, the MI355X-native per-pixel Schwarzschild
 * geodesic renderer (drop-in for the sky-sphere hot path of
 * FirePrincess01/schwarzschild_raytracer_wgpu).
 *
 * Plain C, plain pointers and sizes: no HIP, no torch types.  A HIP stream is
 * passed as `void*` (a hipStream_t; NULL = the legacy default stream).
 *
 * Reference interfaces replaced (paths relative to the reference repo,
 * `SR/` = schwarzschild_raytracer/src/):
 *
 *   geo_frame                  TransformationPipeline            SR/simulation/observer.rs:21-28
 *                              (WGSL twin ObserverTransformations SR/schwarzschild_sphere_shader/shader.wgsl:26-33)
 *   geo_observer_*             Observer::{new, calc_transformation_pipeline,
 *                              update_screen_format, move_camera, start_*}
 *                                                                SR/simulation/observer.rs:68-296
 *   geo_set_sky                Texture::new_with_mipmaps (group 2, 4 levels)
 *                                                                SR/schwarzschild_sphere_shader/sphere_buffer/basic_sphere_buffer.rs:29-36
 *   geo_solve_ray_fan          SphereRayTracer::solve_ray_fan + BasicSphereBuffer::update_ray_fan
 *                                                                SR/simulation/sphere_ray_tracer.rs:35-56,
 *                                                                .../basic_sphere_buffer.rs:85-88
 *   geo_set_fan                RayFanTexture::update             SR/schwarzschild_sphere_shader/ray_fan_texture.rs:65-90
 *   geo_rays_* / geo_points_*  RayConnector / PointCloud      SR/simulation/ray_connector.rs:6-157,
 *                                                                SR/schwarzschild_point_shader/point_cloud.rs:7-156
 *   geo_draw_points            point pipeline vs_main + fs_main  SR/schwarzschild_point_shader/shader.wgsl:36-74
 *   geo_render_rows            SchwarzschildSphereShaderDraw::draw + fs_main
 *                                                                SR/schwarzschild_sphere_shader/schwarzschild_sphere_shader_draw.rs:3-6,
 *                                                                .../basic_sphere_buffer.rs:92-100,
 *                                                                SR/schwarzschild_sphere_shader/shader.wgsl:57-106
 *
 * Conventions: every int-returning entry point returns GEO_OK (0) or a
 * negative geo_status.  All output buffers are caller-owned.  A geo_ctx is
 * bound to one device and is not thread-safe; calls that take a stream are
 * asynchronous on it unless documented otherwise.
 */
#ifndef GEO_GEO_H
#define GEO_GEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEO_ABI_VERSION 8  /* 4: geo_render_band_set_frames, geo_assemble_shares;
                                5: geo_render_band_set_batch, geo_dispatch_stats;
                                6: GEO_FLAG_RING_F64;
                                7: GEO_FLAG_RING_F64 inside the render kernel (any stream,
                                   no context memory), in GEO_MODE_ADAPTIVE too; steps_total
                                   counts the band's f64 steps;
                                8: GEO_RING_X 5e-3 (was 8e-3); GEO_FLAG_RING_F64 in batched
                                   launches (geo_render_band_set_frames / _batch);
                                   (still 8, additions only, announced by GEO_HAS_DISK:
                                   GEO_FLAG_DISK, geo_set_disk, geo_clear_disk,
                                   geo_disk_hits_next_render;
                                   announced by GEO_HAS_DISK_SHIFT: geo_disk_shift,
                                   geo_set_disk_shift, geo_disk_shift_next_render;
                                   announced by GEO_HAS_DISK_BATCH: geo_render_disk_batch;
                                   announced by GEO_HAS_SS4: GEO_FLAG_SS4;
                                   announced by GEO_HAS_SS4_BATCH: geo_render_ss_batch;
                                   announced by GEO_HAS_DISK_EMISSION: geo_disk_emission,
                                   geo_set_disk_emission, geo_disk_emission_next_render;
                                   announced by GEO_HAS_DISK_EMISSION_BATCH:
                                   geo_render_emission_batch;
                                   announced by GEO_HAS_DISK_RING_F64: geo_set_disk_ring_f64;
                                   announced by GEO_HAS_DISK_RING_BATCH:
                                   geo_render_disk_ring_batch;
                                   announced by GEO_HAS_DISK_ADAPTIVE:
                                   geo_render_disk_adaptive;
                                   announced by GEO_HAS_DISK_ADAPTIVE_BATCH:
                                   geo_render_disk_adaptive_batch;
                                   announced by GEO_HAS_DISK_ADAPTIVE_RING:
                                   geo_render_disk_adaptive_ring;
                                   announced by GEO_HAS_DISK_ADAPTIVE_RING_BATCH:
                                   geo_render_disk_adaptive_ring_batch) */
#define GEO_HAS_DISK 1
#define GEO_HAS_DISK_SHIFT 1
#define GEO_HAS_DISK_BATCH 1
#define GEO_HAS_SS4 1
#define GEO_HAS_SS4_BATCH 1
#define GEO_HAS_DISK_EMISSION 1
#define GEO_HAS_DISK_EMISSION_BATCH 1
#define GEO_HAS_DISK_RING_F64 1
#define GEO_HAS_DISK_RING_BATCH 1
#define GEO_HAS_DISK_ADAPTIVE 1
#define GEO_HAS_DISK_ADAPTIVE_BATCH 1
#define GEO_HAS_DISK_ADAPTIVE_RING 1
#define GEO_HAS_DISK_ADAPTIVE_RING_BATCH 1

typedef enum geo_status {
    GEO_OK = 0,
    GEO_EINVAL = -1,  /* bad argument (null pointer, zero size, out-of-range rows) */
    GEO_EHIP = -2,    /* a HIP runtime call failed */
    GEO_ENOMEM = -3,  /* device or host allocation failed */
    GEO_ENODEV = -4,  /* no such HIP device */
    GEO_ESTATE = -5   /* call out of order (e.g. render before geo_set_sky) */
} geo_status;

/* Render modes (geo_scene.mode). */
#define GEO_MODE_DIRECT 0u /* per-pixel RK4 of the null geodesic at the pixel's own angle */
#define GEO_MODE_FAN 1u    /* reference-exact: lerp into the ray fan (shader.wgsl:77-84) */
#define GEO_MODE_ADAPTIVE 2u /* per-pixel, error-controlled Dormand-Prince RK5(4) steps (config 5;
                                a build extension, not in the reference): geo_scene.step is the
                                initial step, max_steps the budget of step ATTEMPTS, tol the
                                local error tolerance in u */

/* geo_scene.flags */
#define GEO_FLAG_DEFER_STEPS 1u /* executed steps accumulate in the context (no per-call
                                   fold); read them with geo_steps_flush.  steps_total
                                   must then be NULL. */
#define GEO_FLAG_COMPOSITE 2u   /* draw OVER the current contents of out_rgba8 with the
                                   reference's alpha blending (BlendState::ALPHA_BLENDING,
                                   pipeline.rs:49) and leave discarded (black-hole / no-hit)
                                   pixels untouched: the 2nd, 3rd... sphere of a frame
                                   (lib.rs:67-89).  Without it a sphere is drawn over the
                                   cleared target (0,0,0,1). */
#define GEO_FLAG_MIPS 4u        /* (parity unpinned: the reference's mip generator and sampler
                                   are in its absent wgpu_renderer submodule; this is the
                                   repo's own specification of them)
                                   sample the sky through its 4-level mip chain, trilinear,
                                   with the level of detail from the UV differences across
                                   each 2x2 pixel quad, as textureSample does
                                   (basic_sphere_buffer.rs:31-36, shader.wgsl:101; the
                                   level-0 bilinear sample otherwise).  Quads are frame-
                                   aligned, so row0 must be even (GEO_EINVAL otherwise);
                                   band layouts keep bands 8-row aligned. */
#define GEO_FLAG_RING_F64 8u    /* (off on the benchmarked path) GEO_MODE_DIRECT or
                                   GEO_MODE_ADAPTIVE: the pixels next to the capture orbit,
                                   |b/b_c - 1| < GEO_RING_X by the f32 ray (b = r_obs
                                   cos(theta) / sqrt(1 - rs/r_obs), b_c = 3 sqrt(3) rs / 2;
                                   rs > 0, r_obs > rs), take their traveled angle from an
                                   f64 path inside the render kernel: the camera ray, the
                                   reference's set-up and fixed-step RK4 loop at
                                   geo_scene.step (with its exits, step count and Newton,
                                   sphere_ray_tracer.rs:38-191) in f64; the mask is decided
                                   in f64, the sky drawn from the f32 ray with lambda'
                                   rounded to f32 (geo_band.h).  There the orbit amplifies
                                   the f32 roundings (and, in the adaptive mode, its
                                   tolerance) past the 1e-4 UV bar.  The
                                   band's out_steps and steps_total are its f64 steps.  A
                                   one-frame ring render launches one wave per workgroup; a
                                   batch (geo_render_band_set_frames / _batch) carries each
                                   frame's band factor and derives its constants on the
                                   device; no state is kept in the context.  Not with
                                   GEO_MODE_FAN, GEO_FLAG_COMPOSITE or GEO_FLAG_MIPS
                                   (GEO_EINVAL). */
#define GEO_RING_X 5e-3f  /* (8e-3 before ABI 8; tools/ring_width_margin.py) */
#define GEO_FLAG_DISK 16u       /* (a build extension, not in the reference) draw the context's
                                   thin accretion disk (geo_set_disk) over the frame: a ray
                                   meets the disk plane at the traveled angles a_0 + k pi,
                                   k < GEO_DISK_MAX_CROSSINGS (the direct image, the secondary
                                   image over the shadow, the third one at the photon ring);
                                   crossing k is a hit when the main loop integrated that far
                                   (before its exit by crossing, escape, horizon or budget)
                                   and r_in <= r <= r_out there.  "That far" is decided on
                                   what the loop returns: the crossing's node floor(a_k / step)
                                   lies below the step count and a_k below the returned
                                   traveled angle (NO_VALUE = 15 for a ray that never crosses
                                   the sphere).  For a step above about 2.2 the reference's
                                   three Newton iterations need not converge, and the returned
                                   angle can lie before a crossing the loop has passed: such
                                   a crossing is no hit.  The hits' level-0 samples
                                   of the disk texture are blended far to near (k = 2, 1, 0)
                                   with the reference's 8-bit alpha blend over what the plain
                                   render writes; mask, UV, steps and steps_total are the
                                   plain render's (csrc/geo_disk.h).
                                   geo_render_rows / _bands / _band_set for one frame and
                                   geo_render_disk_batch for up to GEO_MAX_BATCH_FRAMES in
                                   one launch (the multi-GPU pipeline's batches, a moving
                                   observer's frames); geo_render_band_set_frames / _batch
                                   refuse the flag.  GEO_MODE_DIRECT (GEO_MODE_ADAPTIVE
                                   through geo_render_disk_adaptive, whose comment states
                                   the crossing rule of that mode,
                                   geo_render_disk_adaptive_ring,
                                   geo_render_disk_adaptive_batch and
                                   geo_render_disk_adaptive_ring_batch alone),
                                   with GEO_FLAG_DEFER_STEPS at most; rs == 0, or r_obs > rs
                                   and rs < r_in; r_out < sphere_r and r_obs < sphere_r
                                   (GEO_EINVAL otherwise; GEO_ESTATE when no disk is set).
                                   A ray the reference ends before its loop (its pre-filters
                                   and radial cases: an observer inside the photon sphere)
                                   draws no disk.  The flag stays refused together with
                                   GEO_FLAG_RING_F64; the capture band of a disk frame goes
                                   through f64 by the context state geo_set_disk_ring_f64
                                   (mask, UV, steps and steps_total are then the plain
                                   GEO_FLAG_RING_F64 render's).  Follow-ups, not in this ABI:
                                   GEO_FLAG_MIPS / _COMPOSITE.
                                   With geo_set_disk_shift the hits are shaded by their
                                   Doppler and redshift factor. */
#define GEO_FLAG_SS4 32u        /* (a build extension, not in the reference) 2 x 2 supersampling,
                                   resolved in the render kernel: output pixel (x, y) of the
                                   width x height render is drawn from four samples, sample
                                   (i, j), i, j in {0, 1}, being pixel (2x + i, 2y + j) of the
                                   2 width x 2 height render of the same geo_frame and the same
                                   scene without this flag, bit for bit (the camera takes the
                                   frame and the frame size only, so the samples sit a quarter
                                   of a pixel from the centre).  Each of R, G, B, A on its own
                                   is (s00 + s01 + s10 + s11 + 2) >> 2 of the 8-bit values that
                                   render writes.  steps_total (or the context's accumulator,
                                   GEO_FLAG_DEFER_STEPS) receives the steps of every sample:
                                   the 2 width x 2 height render's over sample rows 2r, 2r + 1
                                   of the requested rows r.  Colour only: out_mask, out_uv and
                                   out_steps must be NULL, and a buffer armed by
                                   geo_disk_hits_next_render or geo_disk_shift_next_render is
                                   consumed and refuses the call (GEO_EINVAL).
                                   geo_render_rows / _bands / _band_set, GEO_MODE_DIRECT, the
                                   level-0 sampler, with GEO_FLAG_DISK (shaded by
                                   geo_set_disk_shift or not) and GEO_FLAG_DEFER_STEPS at most.
                                   GEO_EINVAL with GEO_MODE_FAN, GEO_MODE_ADAPTIVE (but
                                   through geo_render_disk_adaptive_batch, the only call
                                   that supersamples an adaptive disk frame),
                                   GEO_FLAG_MIPS, GEO_FLAG_COMPOSITE or GEO_FLAG_RING_F64,
                                   through geo_render_band_set_frames / _batch and
                                   geo_render_disk_batch, and where 2 width or 2 height
                                   (or twice the rows of a band layout) exceeds what the call
                                   takes as width, height and rows (2^20).  Rows and bands are
                                   in output pixels; the tile grid (geo_set_tile_order, the
                                   learned order, which is the supersampled render's own) is
                                   the sample frame's, ceil(2 width / 32) x ceil(2 nrows / 8).
                                   No buffer of samples is kept: a wave's 16 x 4 samples are
                                   8 x 2 output pixels, resolved across its lanes
                                   (DESIGN.md §3).  Up to GEO_MAX_BATCH_FRAMES supersampled
                                   frames in one launch go through geo_render_ss_batch
                                   (GEO_HAS_SS4_BATCH); with the emission set through
                                   geo_render_emission_batch, and with geo_set_disk_ring_f64
                                   on through geo_render_disk_ring_batch, the only call
                                   that draws a supersampled disk frame with its f64 band. */
#define GEO_DISK_MAX_CROSSINGS 3
#define GEO_DISK_G_MAX 16.0f    /* the largest frequency ratio a shaded hit reports
                                   (geo_set_disk_shift; csrc/geo_disk.h) */

/* Observer motion states, ObserverState (SR/simulation/observer.rs:12-16). */
#define GEO_OBSERVER_UNMOVING 0
#define GEO_OBSERVER_FROZEN_FALL 1
#define GEO_OBSERVER_ORBITING 2

/* GEO_MODE_ADAPTIVE step control (geo_pixel.h, geodesic_angle_adaptive). */
#define GEO_ADAPTIVE_DEFAULT_TOL 1e-6f
#define GEO_ADAPTIVE_MAX_GROWTH 16u /* largest step = 16 x geo_scene.step */

/* Sentinel for a ray that never reaches the sphere, SphereRayTracer::NO_VALUE
 * (sphere_ray_tracer.rs:22).  Fan / traveled-angle space. */
#define GEO_NO_VALUE 15.0

/* Byte-for-byte TransformationPipeline (observer.rs:21-28): three column-major
 * 4x4 f32 matrices and [sqrt((psi-1)/psi), x, y, z].  208 bytes. */
typedef struct geo_frame {
    float display_to_movement[16]; /* camera rotation; column 3 = FOV scale (observer.rs:253-254) */
    float movement_to_central[16];
    float central_to_uv[16];
    float psi_factor_and_position[4];
} geo_frame;

/* Per-draw scene constants.  The reference fixes these per sphere
 * (basic_sphere_buffer.rs:42-51, lib.rs:72, renderer.rs:83). */
typedef struct geo_scene {
    float rs;           /* Schwarzschild radius */
    float sphere_r;     /* radius of the textured sky sphere */
    float r_obs;        /* observer radial position |pos| (lib.rs:292) */
    float step;         /* RK4 step in traveled angle (PI/100 in the reference);
                           GEO_MODE_ADAPTIVE: the initial step */
    uint32_t max_steps; /* RK4 budget per ray (1000 in the reference), <= 2^24;
                           GEO_MODE_ADAPTIVE: budget of step attempts */
    uint32_t mode;      /* GEO_MODE_* */
    uint32_t flags;     /* GEO_FLAG_* */
    float tol;          /* GEO_MODE_ADAPTIVE: local error tolerance in u (0 = 1e-6);
                           must be 0 in the other modes */
} geo_scene;

typedef struct geo_ctx geo_ctx;
typedef struct geo_observer geo_observer;

/* ---- library ---------------------------------------------------------- */
/* Every call that launches device work first clears the calling thread's HIP
 * last-error state (hipGetLastError), so that an earlier, unrelated failure
 * of the caller is not reported as the call's: a caller that checks its own
 * launches with hipGetLastError must do so before calling into libgeo. */
int geo_abi_version(void);
const char* geo_status_str(int status);

/* ---- device context --------------------------------------------------- */
/* Creates a context on HIP device `device`.  Fails with GEO_ENODEV when the
 * device does not exist (there is no CPU fallback). */
int geo_ctx_create(int device, geo_ctx** out);
void geo_ctx_destroy(geo_ctx* ctx);

/* Uploads an equirect RGBA8 sky (row-major, w*h*4 bytes, host memory; the
 * bytes are copied, synchronously, after this context's renders in flight on
 * any stream have finished, so no frame samples a half-written sky; other
 * contexts' work and collectives are not waited for).  On failure the
 * context has no sky (renders return GEO_ESTATE).  U wraps, V clamps,
 * bilinear with 8-bit sub-texel weights: level 0, or with GEO_FLAG_MIPS the
 * 4-level mip chain built here (box filter; Texture::new_with_mipmaps(..., 4),
 * basic_sphere_buffer.rs:31-36).  The device keeps every level padded by one
 * texel on every side, which must stay below 2^31 bytes in all:
 * sum over l < 4 of (max(1, w >> l) + 2) * (max(1, h >> l) + 2) * 4 < 2^31,
 * w, h <= 2^20 (GEO_EINVAL otherwise). */
int geo_set_sky(geo_ctx* ctx, const uint8_t* rgba8, uint32_t w, uint32_t h);

/* The thin accretion disk of GEO_FLAG_DISK renders: the annulus r_in..r_out
 * of the plane through the centre with normal `normal`, in the sky texture's
 * frame (the frame central_to_uv maps to; the observer sits at r_obs times
 * central_to_uv's third column there).  Texture coordinates: U = the azimuth
 * in turns from `axis` (projected into the plane) towards normal x axis,
 * V = (r - r_in) / (r_out - r_in). */
typedef struct geo_disk {
    float r_in, r_out;
    float normal[3];
    float axis[3];
} geo_disk;

/* Sets the context's disk and uploads its RGBA8 texture (row-major, w*h*4
 * bytes, host memory; copied synchronously after this context's renders in
 * flight, as geo_set_sky does; sampled at level 0: U wraps, V clamps, 8-bit
 * sub-texel weights; a texture with alpha gives a translucent disk).
 * w, h <= 2^20 and (w + 2) * (h + 2) * 4 < 2^31.  GEO_EINVAL for
 * !(0 < r_in < r_out), a zero normal, or an axis parallel to the normal (or
 * zero); a refused call leaves the context's disk as it was.  After a failed
 * upload (GEO_EHIP, GEO_ENOMEM) the context has no disk. */
int geo_set_disk(geo_ctx* ctx, const geo_disk* disk, const uint8_t* rgba8, uint32_t w, uint32_t h);
/* Removes the disk (GEO_FLAG_DISK renders return GEO_ESTATE again). */
int geo_clear_disk(geo_ctx* ctx);
/* The next render of this context writes its disk hits to out_hits (device,
 * nrows*width*3*2 floats, laid out as the render's rows): slot k of a pixel
 * holds (r, U) of crossing k, or (0, 0) when that crossing is not a hit.
 * Consumed by the next render call whether it succeeds or not (the idiom of
 * geo_time_next_render); a render without GEO_FLAG_DISK writes nothing. */
int geo_disk_hits_next_render(geo_ctx* ctx, float* out_hits);

/* (GEO_HAS_DISK_RING_F64) The disk's capture band in f64: while on (on != 0),
 * a GEO_FLAG_DISK render through geo_render_rows / _bands / _band_set
 * (unshaded, shaded by geo_set_disk_shift, or the emission of
 * geo_set_disk_emission; GEO_FLAG_DEFER_STEPS at most, as before) takes the
 * pixels of the band |b/b_c - 1| < GEO_RING_X, GEO_FLAG_RING_F64's band decided
 * on the f32 ray, through the f64 path: their traveled angle, mask, step count
 * and the disk's crossing probes (csrc/geo_band.h band_lambda_disk states the
 * rules).  A band pixel's hit radius is the f64 integrator's, rounded once to
 * f32; everything after it (U, g, q, the samples, the blend) is the f32 code.
 * Every other pixel is drawn as without the state, bit for bit.  mask, UV,
 * steps and steps_total (or the deferred accumulator) are those of the plain
 * GEO_FLAG_RING_F64 render: the same scene with GEO_FLAG_RING_F64 in place of
 * GEO_FLAG_DISK.  All per-pixel outputs work (out_mask, out_uv, out_steps and
 * the buffers of geo_disk_hits_next_render, geo_disk_shift_next_render and
 * geo_disk_emission_next_render), as do geo_time_next_render, geo_set_dispatch
 * (the learned order has a grid key of its own; a band pixel's steps count
 * twice in a tile's cost, as in a GEO_FLAG_RING_F64 render) and
 * geo_set_tile_order.  With rs == 0 there is no capture orbit: the state is
 * ignored and the frame is the plain disk frame.  While on, what is colour-only
 * or batched returns GEO_EINVAL for a disk scene, launches nothing and writes
 * nothing (an armed per-pixel buffer is still consumed): GEO_FLAG_SS4 disk
 * renders, geo_render_disk_batch, geo_render_ss_batch and
 * geo_render_emission_batch (such a frame would come out without its band);
 * geo_render_disk_ring_batch (GEO_HAS_DISK_RING_BATCH) draws batched and
 * GEO_FLAG_SS4 disk frames with the band, and geo_render_disk_adaptive_ring
 * (GEO_HAS_DISK_ADAPTIVE_RING) one GEO_MODE_ADAPTIVE disk frame with it, and
 * geo_render_disk_adaptive_ring_batch (GEO_HAS_DISK_ADAPTIVE_RING_BATCH)
 * batched and GEO_FLAG_SS4 GEO_MODE_ADAPTIVE disk frames.
 * Renders without GEO_FLAG_DISK are untouched, and GEO_FLAG_DISK |
 * GEO_FLAG_RING_F64 stays GEO_EINVAL everywhere.  Off by default; kept across
 * geo_set_disk, cleared by geo_clear_disk.  GEO_EINVAL for a NULL ctx. */
int geo_set_disk_ring_f64(geo_ctx* ctx, int on);

/* Doppler and redshift shading of the disk (csrc/geo_disk.h).  The disk's
 * matter moves on circular geodesics about spin * normal (spin = +1: the
 * sense in which the disk's azimuth U grows; -1: the other), and a hit at
 * radius r is seen at the frequency ratio (received / emitted, c = 1)
 *   g = sqrt(1 - 1.5 rs/r) / sqrt(1 - rs/r_obs)
 *       / (1 + spin sqrt(rs / (2 r^3)) b w) * g_obs,  clamped to 0..GEO_DISK_G_MAX,
 * b the ray's impact parameter, b w its angular momentum about the disk axis
 * and g_obs the moving observer's own Doppler factor.  The hit's texture
 * sample has R, G and B multiplied by min(gain * g^exponent, 65536), rounded
 * and saturated at 255, before it is blended; alpha is kept (exponent 4:
 * bolometric intensity; 3: specific intensity; 0 with gain 1: the unshaded
 * bytes). */
typedef struct geo_disk_shift {
    int32_t spin;      /* +1 or -1 */
    uint32_t exponent; /* 0..4 */
    float gain;        /* finite, > 0 */
} geo_disk_shift;

/* Turns the shading on for this context's GEO_FLAG_DISK renders, or off with
 * NULL (they are then byte for byte the unshaded ones).  GEO_EINVAL for a spin
 * other than +1 or -1, exponent > 4 or a gain that is not finite and
 * positive; a refused call leaves the state as it was.  The state is kept
 * across geo_set_disk (a texture can be swapped under it) and cleared by
 * geo_clear_disk.  While it is set a GEO_FLAG_DISK render needs circular
 * orbits down to the inner edge: rs == 0 or r_in > 1.5 rs (GEO_EINVAL
 * otherwise, at render time).  The combinations GEO_FLAG_DISK refuses stay
 * refused. */
int geo_set_disk_shift(geo_ctx* ctx, const geo_disk_shift* shift);
/* The next render of this context writes its hits' frequency ratios to out_g
 * (device, nrows*width*3 floats, laid out as the render's rows): element k of
 * a pixel is the g of crossing k, or 0 when that crossing is not a hit.
 * Armed and consumed as geo_disk_hits_next_render's buffer is; written only
 * by a shaded GEO_FLAG_DISK render. */
int geo_disk_shift_next_render(geo_ctx* ctx, float* out_g);

/* Blackbody emission of the disk (csrc/geo_disk.h): the disk's colour comes
 * from a temperature instead of the texture alone.  The emitted temperature is
 * T(r) = t_ref tau(r) with the radial profile tau below, the observed one
 * T_obs = g T(r) with the frequency ratio g of geo_disk_shift (this struct's
 * own spin), and q = T_obs / t_ref = g tau(r), in 0..GEO_DISK_G_MAX.  A hit is
 * coloured by the ramp at
 *   (n - 1) (1/t_lo - 1/T_obs) / (1/t_lo - 1/t_hi), clamped to 0..n-1
 * (q = 0 or a NaN: entry 0), the two neighbouring entries blended per 8-bit
 * channel with the weight w = floor(frac * 256): (a (256 - w) + b w + 128) >> 8.
 * Each of R, G and B of the hit's disk-texture sample t and the ramp colour e
 * becomes min(255, floor(t e m / 255 + 0.5)) with the bolometric multiplier
 * m = min(exposure q^4, 65536), which holds the g^4 beaming; the texture's
 * alpha is kept, and that colour is what is blended, far to near, as ever.  A
 * white opaque texture draws the pure ramp; a patterned or translucent one
 * modulates it. */
#define GEO_DISK_PROFILE_POWER 0u  /* tau(r) = (r_in/r)^(3/4) */
#define GEO_DISK_PROFILE_THIN  1u  /* zero-torque inner edge: tau(r) = f(r_in/r) / f_max,
                                      f(x) = x^(3/4) (1 - sqrt x)^(1/4), f_max = f(36/49) = 0.487871339...;
                                      tau = 0 at r_in, 1 at r = 49/36 r_in */
#define GEO_DISK_RAMP_MAX 1024u
typedef struct geo_disk_emission {
    int32_t  spin;      /* +1 or -1, as geo_disk_shift.spin */
    uint32_t profile;   /* GEO_DISK_PROFILE_* */
    float    t_ref;     /* the profile's hottest emitted temperature: T(r) = t_ref tau(r) */
    float    t_lo, t_hi;/* the ramp's ends, 0 < t_lo < t_hi: entry 0 is the colour of T_obs <= t_lo,
                           entry n-1 of T_obs >= t_hi, the entries evenly spaced in 1/T (mired) */
    float    exposure;  /* finite, > 0: colour multiplier m = min(exposure q^4, 65536), q = T_obs / t_ref */
} geo_disk_emission;

/* Turns the emission on for this context's GEO_FLAG_DISK renders and uploads
 * its ramp (n RGBA8 entries, host memory; copied synchronously after this
 * context's renders in flight, as geo_set_disk copies its texture), or turns it
 * off with NULL (ramp and n are then ignored).  While it is set the state of
 * geo_set_disk_shift is neither read nor changed; it takes effect again once
 * the emission is cleared.  GEO_EINVAL for a spin other than +1 or -1, an
 * unknown profile, a t_ref, t_lo, t_hi or exposure that is not finite and
 * positive, t_lo >= t_hi, a NULL ramp, or n outside 2..GEO_DISK_RAMP_MAX; a
 * refused call leaves the state as it was.  The state is kept across
 * geo_set_disk and cleared by geo_clear_disk.  At render time the shift's rule
 * holds: rs == 0 or r_in > 1.5 rs (GEO_EINVAL otherwise).
 * Entry points: geo_render_rows, geo_render_bands and geo_render_band_set with
 * all the per-pixel outputs (out_g of geo_disk_shift_next_render is written
 * too), and GEO_FLAG_SS4 on those three, colour only.  geo_render_disk_batch,
 * and geo_render_ss_batch for a GEO_FLAG_DISK scene, return GEO_EINVAL while an
 * emission is set, launch nothing and write nothing: a batched disk frame
 * would come out without its emission.  Batched emission frames go through
 * geo_render_emission_batch (GEO_HAS_DISK_EMISSION_BATCH). */
int geo_set_disk_emission(geo_ctx* ctx, const geo_disk_emission* emission, const uint8_t* ramp_rgba8, uint32_t n);
/* The next render of this context writes its hits' q = T_obs / t_ref to out_q
 * (device, nrows*width*3 floats, laid out as the render's rows): element k of
 * a pixel is the q of crossing k, or 0 when that crossing is not a hit.  Armed
 * and consumed as geo_disk_hits_next_render's buffer is (an armed buffer
 * refuses a GEO_FLAG_SS4 or a batched call); written only by an emission
 * render. */
int geo_disk_emission_next_render(geo_ctx* ctx, float* out_q);

/* Uploads a ray fan of n >= 2 nodes (host memory, copied synchronously after
 * the last solve and draws of the buffer it goes to; geo_solve_ray_fan
 * replaces it stream-ordered):
 * node i is PI/2 - traveled angle of the ray at theta_i = PI/2 - PI*i/(n-1). */
int geo_set_fan(geo_ctx* ctx, const float* fan, uint32_t n);

/* Computes the ray fan on the GPU in f64 (SphereRayTracer::solve_ray_fan,
 * sphere_ray_tracer.rs:35-193) for nr_nodes nodes at observer radius r and
 * makes it the context's fan: fan-mode renders issued after this call read
 * it.  Asynchronous on `stream`; the context keeps two fan buffers and
 * orders them itself, so the stream need not be the renders' stream: the
 * solve waits for the renders that read the buffer it overwrites (issued
 * before the previous solve), and a render waits for the solve of the fan it
 * reads.  A fan solved on a side stream thus overlaps the previous frame's
 * draws.  When fan_out (host) is non-NULL the call synchronises `stream` and
 * copies the nr_nodes f32 values there. */
int geo_solve_ray_fan(geo_ctx* ctx, double sphere_r, double schwarz_r, uint32_t max_iter,
                      double step, uint32_t nr_nodes, double r, float* fan_out, void* stream);

/* Renders rows [row0, row0+nrows) of a width x height frame (fs_main,
 * shader.wgsl:57-106, composited onto the clear colour (0,0,0,1) with the
 * reference's alpha blend, pipeline.rs:49 / renderer.rs:233-238).
 * Outputs are DEVICE pointers laid out row-major relative to row0:
 *   out_rgba8    nrows*width*4 bytes (required)
 *   out_mask     nrows*width bytes, 1 = black hole / discard (optional)
 *   out_uv       nrows*width*2 floats, sky-sphere (U,V) (optional)
 *   out_steps    nrows*width u32, executed RK4 main-loop steps (optional)
 *   steps_total  one u64 that the executed steps of this call are ADDED to (optional;
 *                exactly this call's steps, also while other renders of the context
 *                run on other streams: the call counts into a counter set of its own,
 *                reused only after that set's previous fold)
 * Asynchronous on `stream`. */
int geo_render_rows(geo_ctx* ctx, const geo_frame* frame, const geo_scene* scene,
                    uint32_t width, uint32_t height, uint32_t row0, uint32_t nrows,
                    uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv,
                    uint32_t* out_steps, unsigned long long* steps_total, void* stream);

/* Renders an interleaved set of row bands (balanced multi-GPU sharding): bands
 * band0, band0+band_step, ..., nbands of them, each band_rows tall (a
 * power of two >= 8, the pixel rows of one wave); band b
 * covers rows [b*band_rows, (b+1)*band_rows) clipped to height.  Outputs are
 * packed band after band (nbands*band_rows rows; clipped rows are not
 * written).  geo_render_rows(row0, nrows) is the single-band case. */
int geo_render_bands(geo_ctx* ctx, const geo_frame* frame, const geo_scene* scene,
                     uint32_t width, uint32_t height, uint32_t band_rows, uint32_t band0,
                     uint32_t band_step, uint32_t nbands, uint8_t* out_rgba8, uint8_t* out_mask,
                     float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                     void* stream);

/* Rank 0's reassembly after gathering every rank's geo_render_bands output
 * (multi-GPU present): `src` (device) holds `world` rank blocks
 * of rank_stride bytes, rank r's block being its packed bands (bands r,
 * r+world, r+2*world, ... of band_rows rows) for nframes frames at
 * frame_stride bytes apart, src_bpp bytes per pixel (4: RGBA8 as rendered,
 * 3: RGB24 from geo_pack_rgb, width % 4 == 0).  Writes nframes width x height
 * RGBA8 frames back to back to `dst` (device).  Asynchronous on `stream`. */
int geo_assemble_bands(geo_ctx* ctx, const uint8_t* src, size_t rank_stride, size_t frame_stride, uint32_t world,
                       uint32_t band_rows, uint32_t width, uint32_t height, uint32_t nframes, uint32_t src_bpp,
                       uint8_t* dst, void* stream);

/* The general strided band set: bands starting at rows row0, row0+row_stride,
 * ..., nbands of them, each band_rows tall (a multiple of 8; at most 4096
 * unless a power of two) and clipped
 * to height; row_stride >= band_rows.  Outputs packed band after band as in
 * geo_render_bands (which is the case row0 = band0*band_rows,
 * row_stride = band_step*band_rows).  Used for the lead layout below, where
 * rank 0 renders taller bands than its peers. */
int geo_render_band_set(geo_ctx* ctx, const geo_frame* frame, const geo_scene* scene,
                        uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                        uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, uint8_t* out_mask,
                        float* out_uv, uint32_t* out_steps, unsigned long long* steps_total,
                        void* stream);

/* A batch of nframes (1 .. GEO_MAX_BATCH_FRAMES) frames of one scene in ONE
 * launch: frame f's uniform is frames[f], its packed bands (the layout of
 * geo_render_band_set) go to out_rgba8 + f*out_frame_stride bytes
 * (out_frame_stride a multiple of 4, at least the packed bands' bytes).  The
 * frames share the scene (observer radius, step, budget, mode): frames of an
 * observer at one radius (a camera pan, or the same pose drawn again); a
 * moving observer's frames go through geo_render_band_set_batch below.  Fan
 * mode reads the context's current fan for every frame.
 * Colour only (no mask, UV or per-pixel steps; no GEO_FLAG_MIPS); the
 * executed steps of all frames go to steps_total or, with
 * GEO_FLAG_DEFER_STEPS, to the context's accumulator.  One launch pays the
 * dispatch, ramp and drain of a render once for the whole batch: a rank's
 * share of a 4K frame at N = 8 (about two waves per slot) draws 10-12 %
 * faster per frame.  Asynchronous on `stream`. */
#define GEO_MAX_BATCH_FRAMES 8
int geo_render_band_set_frames(geo_ctx* ctx, const geo_frame* frames, uint32_t nframes, const geo_scene* scene,
                               uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                               uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                               unsigned long long* steps_total, void* stream);

/* geo_render_band_set_frames with a scene per frame (scenes[f] for frames[f]):
 * a moving observer's frames, whose radius r_obs changes every frame, in one
 * launch.  The scenes may differ in r_obs only (every other field equal, the
 * same integration kind: all outside or all inside the horizon; a fan-mode
 * batch draws one fan, so r_obs must agree too), else GEO_EINVAL. */
int geo_render_band_set_batch(geo_ctx* ctx, const geo_frame* frames, const geo_scene* scenes, uint32_t nframes,
                              uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                              uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                              unsigned long long* steps_total, void* stream);

/* geo_render_band_set_batch for GEO_FLAG_DISK scenes (GEO_HAS_DISK_BATCH): nframes
 * (1 .. GEO_MAX_BATCH_FRAMES) frames of the context's thin disk in ONE launch,
 * scenes[f] for frames[f], the band-set layout and out_frame_stride rules of
 * geo_render_band_set_frames.  Frame f's bytes are those of geo_render_band_set
 * with frames[f] and scenes[f]; with geo_set_disk_shift the hits are shaded.
 * Every scene carries GEO_FLAG_DISK and GEO_MODE_DIRECT, with
 * GEO_FLAG_DEFER_STEPS at most, and the scenes may differ in r_obs only (the
 * same integration kind), else GEO_EINVAL.  GEO_FLAG_DISK's rules hold for
 * every frame's scene: rs == 0, or r_obs > rs and rs < r_in; r_out < sphere_r
 * and r_obs < sphere_r; with the shift set and rs > 0, r_in > 1.5 rs
 * (GEO_EINVAL; GEO_ESTATE when no disk is set).  Colour only: a buffer armed by
 * geo_disk_hits_next_render, geo_disk_shift_next_render or
 * geo_disk_emission_next_render is consumed and the call returns GEO_EINVAL.
 * While geo_set_disk_emission is set the call returns GEO_EINVAL (batched
 * emission frames go through geo_render_emission_batch; the one-frame entry
 * points draw them too).  A refused call launches nothing and writes nothing.
 * The executed steps of all frames go to steps_total or, with
 * GEO_FLAG_DEFER_STEPS, to the context's accumulator; geo_time_next_render and
 * the dispatch order work as for the other batches (frame 0 records the tile
 * costs).  One scene for every frame: pass copies.  Asynchronous on `stream`. */
int geo_render_disk_batch(geo_ctx* ctx, const geo_frame* frames, const geo_scene* scenes, uint32_t nframes,
                          uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                          uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                          unsigned long long* steps_total, void* stream);

/* geo_render_band_set_batch for GEO_FLAG_SS4 scenes (GEO_HAS_SS4_BATCH): nframes
 * (1 .. GEO_MAX_BATCH_FRAMES) 2 x 2 supersampled frames in ONE launch, scenes[f]
 * for frames[f]: the plain frame, the GEO_FLAG_DISK frame and, with
 * geo_set_disk_shift, the shaded disk frame.  width, height, rows and bands are
 * in output pixels, as for the one-frame supersampled render; frame f's packed
 * bands go to out_rgba8 + f*out_frame_stride bytes (out_frame_stride a multiple
 * of 4, at least nbands*band_rows*width*4).  Frame f's bytes are those of
 * geo_render_band_set with frames[f] and scenes[f] (the same flags), bit for
 * bit, and so, by GEO_FLAG_SS4's definition, the box resolve of the one-sample
 * render at twice the size.
 * Every scene carries GEO_FLAG_SS4 and GEO_MODE_DIRECT, with GEO_FLAG_DISK and
 * GEO_FLAG_DEFER_STEPS at most; a scene without GEO_FLAG_SS4 is GEO_EINVAL (the
 * other batched calls draw those).  The scenes may differ in r_obs only and
 * share the integration kind (geo_render_band_set_batch's rules), else
 * GEO_EINVAL.  With GEO_FLAG_DISK, geo_render_disk_batch's rules hold for every
 * frame's scene.  GEO_ESTATE when no sky, or no disk for a disk scene, is set.
 * Colour only: a buffer armed by geo_disk_hits_next_render,
 * geo_disk_shift_next_render or geo_disk_emission_next_render is consumed and
 * the call returns GEO_EINVAL.  A GEO_FLAG_DISK scene is GEO_EINVAL while
 * geo_set_disk_emission is set (as for geo_render_disk_batch).  The
 * one-frame supersampled render's size limits apply: width and height at most
 * 2^19 (and twice a band layout's rows within what the call takes as rows).  A
 * refused call launches nothing and writes nothing; ctx, frames, scenes or
 * out_rgba8 NULL and nframes out of range are refused before any device work.
 * The steps of every sample of every frame go to steps_total or, with
 * GEO_FLAG_DEFER_STEPS, to the context's accumulator.  geo_time_next_render
 * works as for the other batches.  The tile grid, for the learned order and
 * for geo_set_tile_order alike, is the sample frame's, ceil(2 width / 32) x
 * ceil(2 nrows / 8); frame 0 records the tile costs, the learned order is per
 * tile and is the one-frame supersampled render's own for the same grid.
 * geo_render_band_set_frames / _batch and geo_render_disk_batch keep refusing
 * the flag.  One scene for every frame: pass copies.  Asynchronous on `stream`. */
int geo_render_ss_batch(geo_ctx* ctx, const geo_frame* frames, const geo_scene* scenes, uint32_t nframes,
                        uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                        uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                        unsigned long long* steps_total, void* stream);

/* geo_render_band_set_batch for the blackbody disk (GEO_HAS_DISK_EMISSION_BATCH):
 * nframes (1 .. GEO_MAX_BATCH_FRAMES) frames of the context's thin disk with
 * geo_set_disk_emission set, in ONE launch, scenes[f] for frames[f], the
 * band-set layout and the out_frame_stride rules of the other batches.  Frame
 * f's bytes are those of geo_render_band_set with frames[f], scenes[f] and the
 * same context state, bit for bit (and so geo_render_cpu_disk_emission's).
 * Every scene carries GEO_FLAG_DISK and GEO_MODE_DIRECT; GEO_FLAG_SS4 on all of
 * them or on none (width, height, rows and bands are then in output pixels, as
 * for geo_render_ss_batch, with its size limits); GEO_FLAG_DEFER_STEPS is
 * allowed and nothing else.  The scenes may differ in r_obs only and share the
 * integration kind.  geo_render_disk_batch's disk rules and the emission's
 * r_in > 1.5 rs rule hold for every frame's scene, else GEO_EINVAL.
 * GEO_ESTATE when no sky, no disk or no emission is set.  While
 * geo_set_disk_shift is set too, the emission takes its place (its own spin),
 * as in the one-frame render.  Colour only: a buffer armed by
 * geo_disk_hits_next_render, geo_disk_shift_next_render or
 * geo_disk_emission_next_render is consumed and the call returns GEO_EINVAL.
 * A refused call launches nothing and writes nothing; ctx, frames, scenes or
 * out_rgba8 NULL and nframes out of range are refused before any device work.
 * steps_total and the deferred accumulator, geo_time_next_render,
 * geo_set_dispatch and geo_set_tile_order work as for the other batches (frame
 * 0 records the tile costs; under GEO_FLAG_SS4 the grid is the sample frame's).
 * geo_render_disk_batch, geo_render_ss_batch and geo_render_band_set_frames /
 * _batch keep refusing what they refuse.  One scene for every frame: pass
 * copies.  Asynchronous on `stream`. */
int geo_render_emission_batch(geo_ctx* ctx, const geo_frame* frames, const geo_scene* scenes, uint32_t nframes,
                              uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                              uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                              unsigned long long* steps_total, void* stream);

/* geo_render_band_set_batch for the thin disk with its capture band in f64
 * (GEO_HAS_DISK_RING_BATCH): nframes (1 .. GEO_MAX_BATCH_FRAMES) GEO_FLAG_DISK
 * frames of a context with geo_set_disk_ring_f64 on, in ONE render launch,
 * scenes[f] for frames[f], the band-set layout and the out_frame_stride rules
 * of the other batches.  The shading is what the context has set: none,
 * geo_set_disk_shift, or geo_set_disk_emission (which takes the shift's place,
 * as everywhere else).
 * One-sample frames: frame f's bytes are those of geo_render_band_set with
 * frames[f], scenes[f] and the same context state (the ring state on), bit for
 * bit, and so geo_render_cpu_disk_ring_f64's / _shift_ring_f64's; steps_total
 * (or the deferred accumulator) is the sum of those renders' steps, the band's
 * f64 steps included.
 * GEO_FLAG_SS4 on every scene or on none (width, height, rows and bands are
 * then in output pixels, as for geo_render_ss_batch, with its size limits).  No
 * one-frame supersampled render exists while the state is on (it stays
 * refused), so the flag's own definition fixes frame f: output pixel (x, y) is
 * the per-channel (s00 + s01 + s10 + s11 + 2) >> 2 of pixels (2x + i, 2y + j)
 * of the one-sample ring-on render at 2 width x 2 height with the same uniform
 * and scene; the steps are those of every sample over sample rows 2r, 2r + 1.
 * Every scene carries GEO_FLAG_DISK and GEO_MODE_DIRECT, with
 * GEO_FLAG_DEFER_STEPS and GEO_FLAG_SS4 at most; the scenes may differ in r_obs
 * only and share the integration kind.  geo_render_disk_batch's disk rules
 * hold, and with a shift or an emission set so does r_in > 1.5 rs; anything
 * else is GEO_EINVAL.  GEO_ESTATE when no sky or no disk is set, or when the
 * ring state is off.  Colour only: a buffer armed by geo_disk_hits_next_render,
 * geo_disk_shift_next_render or geo_disk_emission_next_render is consumed and
 * the call returns GEO_EINVAL.  A refused call launches nothing and writes
 * nothing; ctx, frames, scenes or out_rgba8 NULL and nframes out of range are
 * refused before any device work.  With rs == 0 there is no capture orbit: the
 * state is ignored and the frames are geo_render_disk_batch's, _ss_batch's or
 * _emission_batch's.  steps_total and the deferred accumulator,
 * geo_time_next_render (the render launch; a small kernel that writes the
 * frames' band constants to a context-owned table runs on `stream` before it),
 * geo_set_dispatch and geo_set_tile_order work as for the other batches (frame
 * 0 records the tile costs, a band pixel's steps counting twice; the learned
 * order has a grid key of its own; under GEO_FLAG_SS4 the grid is the sample
 * frame's).  Every older call keeps every refusal it has.  One scene for every
 * frame: pass copies.  Asynchronous on `stream`. */
int geo_render_disk_ring_batch(geo_ctx* ctx, const geo_frame* frames, const geo_scene* scenes, uint32_t nframes,
                               uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                               uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                               unsigned long long* steps_total, void* stream);

/* The thin disk in GEO_MODE_ADAPTIVE (GEO_HAS_DISK_ADAPTIVE): one GEO_FLAG_DISK
 * frame of the context's disk drawn by the error-controlled integrator,
 * unshaded, with geo_set_disk_shift or with geo_set_disk_emission (which takes
 * the shift's place, as everywhere else).  The layout and the output rules are
 * geo_render_band_set's; a row range is the one-band case: with nbands == 1,
 * band_rows is any number of rows from 1 to 2^20 (clipped to height; row_stride
 * is not read).  All per-pixel outputs work, and the buffers armed by
 * geo_disk_hits_next_render, geo_disk_shift_next_render and
 * geo_disk_emission_next_render are written as in the one-frame direct render.
 * mask, UV, steps and steps_total (or the deferred accumulator) are those of
 * the plain GEO_MODE_ADAPTIVE render of the same scene without GEO_FLAG_DISK,
 * bit for bit: the integration is that render's, attempt for attempt.
 * The crossings are GEO_FLAG_DISK's, a_k = a_0 + k pi.  The integrator's
 * accepted steps tile the traveled angle; crossing k is probed in the accepted
 * attempt whose span [ang, ang + h) holds a_k, while the ray is still
 * integrating (its stopping attempt counts; a rejected attempt probes nothing),
 * by one RK5 step of length a_k - ang from the attempt's start state.  A probed
 * crossing is a hit when a_k lies before the returned traveled angle and
 * r_in <= r <= r_out there; everything after r is the direct mode's
 * (csrc/geo_disk.h).
 * Accuracy next to the capture orbit: the radii carry the integrator's local
 * error at `tol`, which the capture orbit amplifies like 1/|b/b_c - 1|.  At the
 * default tol (1e-6) and step pi/100, against an f64 integration over fuzzed
 * scenes (tests/disk_truth.py): relative radius within 3.6e-5 for
 * |b/b_c - 1| >= 0.05 where a_0 is well conditioned (the f32 floor the direct
 * mode has too), up to 1.95e-4 for 0.02 <= |b/b_c - 1| < 0.05 (a third-image
 * pixel; the direct mode: 6.4e-5 there).  tol = 1e-7 brings that band down to
 * 8.8e-5 at most, for 20 to 30 % more attempts.
 * The scene carries GEO_MODE_ADAPTIVE and GEO_FLAG_DISK, with
 * GEO_FLAG_DEFER_STEPS at most, and tol under the adaptive mode's rules;
 * GEO_EINVAL for a GEO_MODE_DIRECT or GEO_MODE_FAN scene (the older calls draw
 * those) and wherever a GEO_FLAG_DISK rule is broken (rs == 0, or r_obs > rs
 * and rs < r_in; r_out < sphere_r; r_obs < sphere_r; with a shift or an
 * emission set and rs > 0, r_in > 1.5 rs).  GEO_ESTATE without a sky or a disk.
 * GEO_EINVAL while geo_set_disk_ring_f64 is on and rs > 0: the frame would come
 * out without its band (with rs == 0 the state is ignored).  A refused call
 * launches nothing, writes nothing and consumes the armed buffers and the
 * timing pair.  geo_time_next_render, geo_set_dispatch (the learned order has
 * a grid key of its own; a tile's cost is in attempts) and geo_set_tile_order
 * work as for the one-frame direct render.  Batched adaptive disk frames, the
 * multi-GPU pipeline's and GEO_FLAG_SS4 with the adaptive disk go through
 * geo_render_disk_adaptive_batch (this call keeps refusing the flag); one
 * adaptive disk frame with its f64 capture band goes through
 * geo_render_disk_adaptive_ring (this call keeps refusing that state).  Every
 * older call keeps every refusal it has.  Asynchronous on `stream`. */
int geo_render_disk_adaptive(geo_ctx* ctx, const geo_frame* frame, const geo_scene* scene, uint32_t width,
                             uint32_t height, uint32_t band_rows, uint32_t row0, uint32_t row_stride,
                             uint32_t nbands, uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv,
                             uint32_t* out_steps, unsigned long long* steps_total, void* stream);

/* The adaptive disk with its capture band in f64 (GEO_HAS_DISK_ADAPTIVE_RING):
 * one GEO_MODE_ADAPTIVE | GEO_FLAG_DISK frame (GEO_FLAG_DEFER_STEPS at most
 * beside it) of the context's disk, unshaded, with geo_set_disk_shift or with
 * geo_set_disk_emission as the context has it, with the state of
 * geo_set_disk_ring_f64 on.  The prototype, the layouts (a band set, or a row
 * range as the one-band case) and the output rules are
 * geo_render_disk_adaptive's; all per-pixel outputs are written: colour, mask,
 * UV, steps, and the buffers armed by geo_disk_hits_next_render,
 * geo_disk_shift_next_render and geo_disk_emission_next_render.
 * Per pixel: a pixel of the band |b/b_c - 1| < GEO_RING_X (GEO_FLAG_RING_F64's
 * band, decided on the f32 ray as in every ring render) skips the adaptive
 * loop and takes its traveled angle, mask, step count and the three crossing
 * probes from the f64 path of geo_set_disk_ring_f64 (csrc/geo_band.h
 * band_lambda_disk), with the scene's step and max_steps as that loop's fixed
 * step and budget, as in a plain GEO_MODE_ADAPTIVE | GEO_FLAG_RING_F64 render;
 * tol is not read there.  Every other pixel is geo_render_disk_adaptive's.
 * Three properties follow, and the tests hold the call to them:
 *   1. outside the band every output of a pixel equals that of
 *      geo_render_disk_adaptive for the same call with the state off, bit for
 *      bit;
 *   2. inside the band every output of a pixel, steps included, equals that of
 *      the GEO_MODE_DIRECT ring render of the same scene (geo_render_band_set
 *      with the state on, the same rs, sphere_r, r_obs, step and max_steps),
 *      bit for bit: the band's arithmetic does not depend on the mode;
 *   3. mask, UV, steps and steps_total of the frame equal those of the plain
 *      GEO_MODE_ADAPTIVE render of the scene with GEO_FLAG_RING_F64 in place
 *      of GEO_FLAG_DISK.
 * steps_total (or the deferred accumulator) therefore mixes units, as that
 * plain render's does: adaptive attempts outside the band, fixed f64 steps
 * inside it.  On the 96 x 54 test pose whose band holds 2212 pixels the frame
 * counts 663738 against 161635 attempts with the state off.
 * Accuracy: in the band the hit radii are the f64 integrator's rounded once to
 * f32, the direct ring render's: on that pose the largest relative radius error
 * against the f64 integration of tests/disk_ref.py falls from 9.1e-4 (the
 * adaptive disk, state off, in the band; 1.25e-3 for the direct disk with the
 * state off) to 2.11e-6.  Outside the band the radii stay
 * geo_render_disk_adaptive's: up to 1.95e-4 just outside it on the fuzzed
 * scenes (0.02 <= |b/b_c - 1| < 0.05, tol 1e-6).  On the MI355X the kernels'
 * own buffers on 18 fuzzed scenes (472 in-band slots, none dropped) differ
 * from the f64 answer by at most: radius 9.71e-07 (0.23 of its bar), azimuth
 * 7.15e-08 turns (0.13), g 1.06e-06 (0.14), q 4.85e-06 (0.16)
 * (tests/disk_band_truth.py's bars; profiles/disk_adaptive_ring_truth_gpu.txt).
 * GEO_ESTATE with the state off (the call has nothing to draw that
 * geo_render_disk_adaptive does not), without a sky or a disk.  With rs == 0
 * there is no capture orbit: the state is ignored and the frame is
 * geo_render_disk_adaptive's, kernel and bytes.  GEO_EINVAL for a
 * GEO_MODE_DIRECT or GEO_MODE_FAN scene, for any flag beside GEO_FLAG_DISK and
 * GEO_FLAG_DEFER_STEPS (GEO_FLAG_SS4, _MIPS, _COMPOSITE and _RING_F64
 * included), and wherever geo_render_disk_adaptive's disk, shift, emission or
 * tol rules are broken.  A refused call launches nothing, writes nothing and
 * consumes the armed buffers and the timing pair.  geo_time_next_render,
 * geo_set_dispatch (the learned order has a grid key of its own: the mode and
 * the band bit; a tile's cost is its waves' largest count of attempts plus
 * twice their largest count of f64 steps) and geo_set_tile_order work as for
 * geo_render_disk_adaptive.  Batched frames, GEO_FLAG_SS4 with the adaptive
 * band and the multi-GPU pipeline's route for such a scene go through
 * geo_render_disk_adaptive_ring_batch (this call keeps refusing the flag).
 * Every older call keeps every refusal it has.  Asynchronous on `stream`. */
int geo_render_disk_adaptive_ring(geo_ctx* ctx, const geo_frame* frame, const geo_scene* scene, uint32_t width,
                                  uint32_t height, uint32_t band_rows, uint32_t row0, uint32_t row_stride,
                                  uint32_t nbands, uint8_t* out_rgba8, uint8_t* out_mask, float* out_uv,
                                  uint32_t* out_steps, unsigned long long* steps_total, void* stream);

/* geo_render_band_set_batch for the thin disk in GEO_MODE_ADAPTIVE
 * (GEO_HAS_DISK_ADAPTIVE_BATCH): nframes (1 .. GEO_MAX_BATCH_FRAMES)
 * GEO_MODE_ADAPTIVE | GEO_FLAG_DISK frames of the context's disk in ONE render
 * launch, scenes[f] for frames[f], the band-set layout and the
 * out_frame_stride rules of the other batches.  The shading is what the
 * context has set: none, geo_set_disk_shift, or geo_set_disk_emission (which
 * takes the shift's place, as everywhere else).
 * One-sample frames: frame f's bytes are those of geo_render_disk_adaptive with
 * frames[f], scenes[f], the same layout and the same context state, bit for
 * bit, and so geo_render_cpu_disk_adaptive's; steps_total (or the deferred
 * accumulator) is the sum of those renders' attempts.
 * GEO_FLAG_SS4 on every scene or on none (width, height, rows and bands are
 * then in output pixels, with geo_render_ss_batch's size limits of 2^19).  No
 * one-frame supersampled adaptive render exists (geo_render_disk_adaptive keeps
 * refusing the flag), so the flag's own definition fixes frame f: output pixel
 * (x, y) is the per-channel (s00 + s01 + s10 + s11 + 2) >> 2 of pixels
 * (2x + i, 2y + j) of the one-sample geo_render_disk_adaptive render at
 * 2 width x 2 height with the same uniform and scene; the steps are those of
 * every sample over sample rows 2r, 2r + 1.
 * Every scene carries GEO_MODE_ADAPTIVE and GEO_FLAG_DISK, with
 * GEO_FLAG_DEFER_STEPS and GEO_FLAG_SS4 at most, and tol under the adaptive
 * mode's rules; the scenes may differ in r_obs only (tol, step and the budget
 * are equal across the batch) and share the integration kind.
 * geo_render_disk_adaptive's disk rules hold for every frame's scene, r_in >
 * 1.5 rs with a shift or an emission set included; anything else is
 * GEO_EINVAL.  GEO_ESTATE when no sky or no disk is set.  GEO_EINVAL while
 * geo_set_disk_ring_f64 is on and rs > 0: the frames would come out without
 * their band (with rs == 0 the state is ignored).  Colour only: a buffer armed
 * by geo_disk_hits_next_render, geo_disk_shift_next_render or
 * geo_disk_emission_next_render is consumed and the call returns GEO_EINVAL.
 * A refused call launches nothing, writes nothing and drops the timing pair;
 * ctx, frames, scenes or out_rgba8 NULL and nframes out of range are refused
 * before any device work.  geo_time_next_render, geo_set_dispatch and
 * geo_set_tile_order work as for the other batches (frame 0 records the tile
 * costs, a tile's cost being in attempts; the learned order's key holds the
 * mode beside the disk, SS and emission bits; under GEO_FLAG_SS4 the grid is
 * the sample frame's).  Not in this ABI: per-pixel outputs from a batch.  The
 * f64 capture band in a batch of adaptive disk frames or under GEO_FLAG_SS4
 * goes through geo_render_disk_adaptive_ring_batch (this call keeps refusing
 * that state).  Every older call keeps every refusal it has.  One scene for
 * every frame: pass copies.  Asynchronous on `stream`. */
int geo_render_disk_adaptive_batch(geo_ctx* ctx, const geo_frame* frames, const geo_scene* scenes, uint32_t nframes,
                                   uint32_t width, uint32_t height, uint32_t band_rows, uint32_t row0,
                                   uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8, size_t out_frame_stride,
                                   unsigned long long* steps_total, void* stream);

/* geo_render_band_set_batch for the adaptive disk with its capture band in f64
 * (GEO_HAS_DISK_ADAPTIVE_RING_BATCH): nframes (1 .. GEO_MAX_BATCH_FRAMES)
 * GEO_MODE_ADAPTIVE | GEO_FLAG_DISK frames of a context with
 * geo_set_disk_ring_f64 on, in ONE render launch, scenes[f] for frames[f], the
 * band-set layout and the out_frame_stride rules of the other batches.  The
 * shading is what the context has set: none, geo_set_disk_shift, or
 * geo_set_disk_emission (which takes the shift's place, as everywhere else).
 * One-sample frames: frame f's bytes are those of
 * geo_render_disk_adaptive_ring with frames[f], scenes[f], the same layout and
 * the same context state, bit for bit, and so
 * geo_render_cpu_disk_adaptive_ring_f64's; steps_total (or the deferred
 * accumulator) is the sum of those renders' counts, in their mixed units:
 * adaptive attempts outside the band, fixed f64 steps inside it.
 * GEO_FLAG_SS4 on every scene or on none (width, height, rows and bands are
 * then in output pixels, with geo_render_ss_batch's size limits of 2^19).  No
 * one-frame supersampled adaptive ring render exists
 * (geo_render_disk_adaptive_ring keeps refusing the flag), so the flag's own
 * definition fixes frame f: output pixel (x, y) is the per-channel
 * (s00 + s01 + s10 + s11 + 2) >> 2 of pixels (2x + i, 2y + j) of the one-sample
 * geo_render_disk_adaptive_ring render at 2 width x 2 height with the same
 * uniform and scene; the steps are those of every sample over sample rows 2r,
 * 2r + 1.
 * Every scene carries GEO_MODE_ADAPTIVE and GEO_FLAG_DISK, with
 * GEO_FLAG_DEFER_STEPS and GEO_FLAG_SS4 at most, and tol under the adaptive
 * mode's rules; the scenes may differ in r_obs only (tol, step and the budget
 * are equal across the batch; the band's lanes take step and max_steps as
 * their f64 loop's fixed step and budget) and share the integration kind.
 * GEO_EINVAL for GEO_MODE_DIRECT and GEO_MODE_FAN scenes (geo_render_disk_ring_batch
 * draws the direct ones), for any other flag (GEO_FLAG_RING_F64, _MIPS and
 * _COMPOSITE included), and wherever a rule of geo_render_disk_adaptive_batch
 * is broken.  GEO_ESTATE with the ring state off (the call has nothing to draw
 * that geo_render_disk_adaptive_batch does not), or without a sky or a disk.
 * With rs == 0 there is no capture orbit: the state is ignored and the frames
 * are geo_render_disk_adaptive_batch's, kernels and bytes.  Colour only: a
 * buffer armed by geo_disk_hits_next_render, geo_disk_shift_next_render or
 * geo_disk_emission_next_render is consumed and the call returns GEO_EINVAL.
 * A refused call launches nothing, writes nothing and drops the timing pair;
 * ctx, frames, scenes or out_rgba8 NULL and nframes out of range are refused
 * before any device work.  geo_time_next_render (the render launch; a small
 * kernel that writes the frames' band constants to a context-owned table runs
 * on `stream` before it), geo_set_dispatch and geo_set_tile_order work as for
 * the other batches (frame 0 records the tile costs, a tile's cost being its
 * waves' largest count of attempts plus twice their largest count of f64
 * steps; the learned order's key holds the mode and the band bit, so it
 * differs from geo_render_disk_ring_batch's and from
 * geo_render_disk_adaptive_batch's; under GEO_FLAG_SS4 the grid is the sample
 * frame's).  Not in this ABI: per-pixel outputs from a batch.  Every older call
 * keeps every refusal it has: geo_render_disk_adaptive_batch stays GEO_EINVAL
 * with the state on and rs > 0, geo_render_disk_ring_batch for adaptive scenes.
 * One scene for every frame: pass copies.  Asynchronous on `stream`. */
int geo_render_disk_adaptive_ring_batch(geo_ctx* ctx, const geo_frame* frames, const geo_scene* scenes,
                                        uint32_t nframes, uint32_t width, uint32_t height, uint32_t band_rows,
                                        uint32_t row0, uint32_t row_stride, uint32_t nbands, uint8_t* out_rgba8,
                                        size_t out_frame_stride, unsigned long long* steps_total, void* stream);

/* Rank 0's reassembly for the LEAD layout (multi-GPU present with rank 0
 * taking a larger share: it renders but never sends its rows, while the peers'
 * rows cross the xGMI links).  The frame is cut into cycles of
 * (lead + world - 1) * band_rows rows: the first lead*band_rows rows of each
 * cycle are rank 0's (one band of that height), then one band_rows band per
 * peer r = 1..world-1 in order.  lead = 1 is geo_assemble_bands' layout.
 *   lead_src  rank 0's packed RGBA8 bands (geo_render_band_set output), nframes
 *             frames lead_frame_stride bytes apart
 *   src       the gathered peer blocks: rank r's packed bands at
 *             src + r*rank_stride + f*frame_stride, src_bpp bytes per pixel
 *             (4 or 3 = RGB24 from geo_pack_rgb); block 0 is not read
 * Writes nframes RGBA8 frames back to back to dst.  width % 4 == 0 and
 * 16-byte aligned device buffers (4-byte for src with src_bpp 3).
 * Asynchronous on `stream`. */
int geo_assemble_lead(geo_ctx* ctx, const uint8_t* lead_src, size_t lead_frame_stride, uint32_t lead,
                      const uint8_t* src, size_t rank_stride, size_t frame_stride, uint32_t world,
                      uint32_t band_rows, uint32_t width, uint32_t height, uint32_t nframes, uint32_t src_bpp,
                      uint8_t* dst, void* stream);

/* geo_assemble_lead with rank 0's rows per cycle given directly: cycles of
 * lead_rows + (world - 1) * band_rows rows, rank 0's first (one lead_rows
 * band), then one band_rows band per peer.  Any lead_rows, so rank 0's share
 * need not be a whole number of peer bands (e.g. 24 rows against peers' 16:
 * bench.py --rank0-lead 3:2).  geo_assemble_lead(lead) is
 * geo_assemble_shares(lead * band_rows).  Same buffers and alignment rules. */
int geo_assemble_shares(geo_ctx* ctx, const uint8_t* lead_src, size_t lead_frame_stride, uint32_t lead_rows,
                        const uint8_t* src, size_t rank_stride, size_t frame_stride, uint32_t world,
                        uint32_t band_rows, uint32_t width, uint32_t height, uint32_t nframes, uint32_t src_bpp,
                        uint8_t* dst, void* stream);

/* RGBA8 -> RGB24 (the alpha byte dropped: frames are opaque after the clear,
 * renderer.rs:233-238) of npixels (a multiple of 4) device pixels: 25 % fewer
 * bytes on the links for the multi-GPU present.  Asynchronous on `stream`. */
int geo_pack_rgb(geo_ctx* ctx, const uint8_t* rgba, uint64_t npixels, uint8_t* rgb, void* stream);

/* The workgroup dispatch order of this context's renders.
 * A frame's tiles differ ~30x in cost (steps per pixel peak at the photon
 * ring), and the hardware dispatches workgroups in launch order, so a long
 * tile dispatched late stretches the kernel's tail.
 *   GEO_DISPATCH_LONGEST_FIRST (the default): every period-th render of a grid
 *     (period 1: every render; 16: renders 1, 17, 33, ...)
 *     (same width, height, rows, bands, mode and sampler) records each 32 x 8
 *     tile's cost on the device, and two small kernels after it build the
 *     order, most expensive tile first, for the renders that follow; the
 *     first render of a new grid records and uses row-major order.  Nothing
 *     is read back to the host.
 *   GEO_DISPATCH_ROW_MAJOR: the launch order.
 * Fan-mode renders (uniform cost) and frames of more than 65 535 tile rows
 * always use row-major order.  The output is the same in any order.
 * period: 1 .. 2^20 (default 16). */
#define GEO_DISPATCH_ROW_MAJOR 0
#define GEO_DISPATCH_LONGEST_FIRST 1
#define GEO_DISPATCH_EXPLICIT 2 /* set by geo_set_tile_order */
int geo_set_dispatch(geo_ctx* ctx, int mode, uint32_t period);

/* GEO_DISPATCH_LONGEST_FIRST's counters since the context was created: the
 * renders that recorded tile costs, and the rebuilt orders renders have
 * adopted.  A rebuild runs on the context's own stream after every render
 * issued before it; renders adopt its order once the host sees it complete
 * (an event query, never a wait), so a recording render due while the last
 * rebuild is still running is deferred to the next render.  Either pointer
 * may be NULL. */
int geo_dispatch_stats(geo_ctx* ctx, unsigned long long* costs_recorded, unsigned long long* orders_adopted);

/* Times the next render of this context (geo_render_rows/bands/band_set, on
 * any stream): its kernel dispatch carries start_event and stop_event
 * (hipEvent_t created with timing), so hipEventElapsedTime gives the
 * kernel's own execution time, as a profiler's dispatch timestamps do, with
 * no marker packets around it.  (A frame of more than 65 535 tile rows: from
 * the first launch's start to the last one's end.)  Consumed by the next
 * render call whether it succeeds or not: a refused call (GEO_EINVAL,
 * GEO_ESTATE, ...) records neither event and drops the pair. */
int geo_time_next_render(geo_ctx* ctx, void* start_event, void* stop_event);

/* An explicit dispatch order (GEO_DISPATCH_EXPLICIT): workgroup i draws tile
 * (order[i] & 0xFFFF, order[i] >> 16) of a tiles_x x tiles_y grid of
 * 32 x 8-pixel tiles over the rendered rows; order (host) must be a
 * permutation of the grid's tiles.  Renders whose grid is exactly
 * tiles_x x tiles_y use it, others row-major order.  order = NULL selects
 * GEO_DISPATCH_ROW_MAJOR.  Waits for the context's renders in flight. */
int geo_set_tile_order(geo_ctx* ctx, uint32_t tiles_x, uint32_t tiles_y, const uint32_t* order);

/* Adds the steps accumulated under GEO_FLAG_DEFER_STEPS to *steps_total
 * (device u64) and clears the context's counter.  Asynchronous on `stream`. */
int geo_steps_flush(geo_ctx* ctx, unsigned long long* steps_total, void* stream);

/* ---- accretion-disk points ------------------------- */
/* A batch of RayConnectors (SR/simulation/ray_connector.rs:6-25) on n points:
 * per point a near-side connector (less_than_180 = true) and/or a far-side one
 * (false).  Connector order: the n near-side ones, then the n far-side ones.
 * State (48 node values per connector, needs_reset) stays on the device. */
#define GEO_RAYS_NEAR 1u
#define GEO_RAYS_FAR 2u
typedef struct geo_rays geo_rays;
typedef struct geo_points geo_points;

/* RayConnector::new for every (point, side); pos_xyz: host, 3 floats per point. */
int geo_rays_create(geo_ctx* ctx, float schwarz_r, uint32_t n_points, uint32_t sides, const float* pos_xyz,
                    geo_rays** out);
void geo_rays_destroy(geo_rays* rays);
/* number of connectors */
int geo_rays_count(const geo_rays* rays);
/* RayConnector::set_position (:134-136) for every point (host, 3 floats per
 * point).  Synchronous: waits for the batch's last update first. */
int geo_rays_set_positions(geo_rays* rays, const float* pos_xyz);
/* update_ray(other, iterations) (ray_connector.rs:48-132) for every connector,
 * or reset_ray(other) (:27-44) when reset != 0.  other_xyz (host): 3 floats
 * (one other end for all) or 3 per point when per_point != 0 (then the call
 * synchronises `stream` after uploading them).  out_vertices: device, 4 floats
 * per connector [x, y, z, incoming angle], or NULL for the batch's own buffer
 * (geo_rays_vertices).  Asynchronous on `stream`; it waits for the batch's
 * previous update, whichever stream that ran on.  Readers of the vertices
 * (geo_draw_points) are the caller's to order: an update overwrites them. */
int geo_rays_update(geo_rays* rays, const float* other_xyz, int per_point, uint32_t iterations, int reset,
                    float* out_vertices, void* stream);
const float* geo_rays_vertices(const geo_rays* rays);

/* PointCloud::new (SR/schwarzschild_point_shader/point_cloud.rs:20-65): one
 * near-side RayConnector per model vertex (host, 3 floats each), plus a
 * far-side one when farside != 0, all reset against observer_xyz; with
 * orbits != 0 every vertex also becomes a particle on an Orbit (f64,
 * orbit.rs) with direction (-y, x, 0) and rotation 18 + 2 rand.  seed: the
 * per-point random streams (wyrand) for those rotations and for respawns.
 * Synchronous. */
int geo_points_create(geo_ctx* ctx, float schwarz_r, const float* model_xyz, uint32_t n,
                      const float* observer_xyz, int farside, int orbits, unsigned long long seed,
                      geo_points** out);
void geo_points_destroy(geo_points* pts);
int geo_points_count(const geo_points* pts);
/* PointCloud::update (point_cloud.rs:117-148): orbit step by dt seconds and
 * respawn (orbits), then update_ray(observer, 1) for every connector, in
 * one kernel launch (two, orbit step then rays, from 131072 connectors on).
 * Asynchronous on `stream`; it waits for the cloud's
 * previous update and for every geo_points_draw before it, whichever streams
 * they ran on. */
int geo_points_update(geo_points* pts, const float* observer_xyz, double dt, void* stream);
/* get_vertices / get_vertices_farside: device pointer, 4 floats per point
 * (NULL for the far side of a cloud without one). */
const float* geo_points_vertices(const geo_points* pts, int farside);
/* current point positions (host, 3 floats per point); `stream` waits for the
 * last update, then the call synchronises it. */
int geo_points_positions(const geo_points* pts, float* out_xyz, void* stream);

/* The point pipeline (SR/schwarzschild_point_shader/shader.wgsl:36-74,
 * pipeline.rs:55-74: PointList, colour (1,0,0,1), REPLACE) drawn over rows
 * [row0, row0+nrows) of an RGBA8 frame (device, laid out as geo_render_rows'
 * out_rgba8).  vertices: device, 4 floats each.  out_xy (device, optional):
 * the pixel (x, y) of every vertex, (-1, -1) when clipped.  Async on `stream`. */
int geo_draw_points(geo_ctx* ctx, const geo_frame* frame, const float* vertices, uint32_t n, uint32_t width,
                    uint32_t height, uint32_t row0, uint32_t nrows, uint8_t* out_rgba8, int* out_xy,
                    void* stream);

/* The point meshes of a PointCloud (the near-side vertices, then the
 * far-side ones; lib.rs:415-418, renderer.rs:256-264) drawn as by
 * geo_draw_points, both in one launch (every point writes the same colour,
 * so their order cannot show).  out_xy (device, optional): 2 ints per
 * connector, near side first.  Stream order: the draw waits for the cloud's last
 * geo_points_update and the next update waits for this draw and every draw
 * before it (events owned by the cloud), whichever streams they run on, so a caller may put the update
 * on a side stream where it overlaps the sphere draws.  Async on `stream`. */
int geo_points_draw(geo_points* pts, const geo_frame* frame, uint32_t width, uint32_t height, uint32_t row0,
                    uint32_t nrows, uint8_t* out_rgba8, int* out_xy, void* stream);

/* ---- observer (host, f64; SR/simulation/observer.rs) ----------------- */
/* Observer::new (observer.rs:68-87): pos (25,0,1), camera (PI,0), FrozenFall,
 * energy 1, fov scale (tan(fov/2), tan(fov/2)*w/h, 1, 1). */
int geo_observer_create(double schwarz_r, double fov, double width, double height,
                        geo_observer** out);
void geo_observer_destroy(geo_observer* obs);
int geo_observer_set_position(geo_observer* obs, double x, double y, double z);
int geo_observer_get_position(const geo_observer* obs, double* xyz3);
int geo_observer_set_camera(geo_observer* obs, double phi, double theta);
int geo_observer_set_energy(geo_observer* obs, double energy);
/* GEO_OBSERVER_UNMOVING / GEO_OBSERVER_FROZEN_FALL (start_unmoving / start_frozen_fall,
 * observer.rs:173-181). */
int geo_observer_set_state(geo_observer* obs, int state);
/* Observer::start_orbit (observer.rs:162-169); returns GEO_ESTATE when no orbit
 * can start there (inside the horizon, orbit.rs:33-35). */
int geo_observer_start_orbit(geo_observer* obs, double rotation);
int geo_observer_get_state(const geo_observer* obs);
double geo_observer_radial_position(const geo_observer* obs);
/* Observer::update_position (observer.rs:105-125); dir = (forward, left, up). */
int geo_observer_update_position(geo_observer* obs, double fwd, double left, double up, double dt);
int geo_observer_move_camera(geo_observer* obs, double dx_pixels, double dy_pixels);
int geo_observer_update_screen_format(geo_observer* obs, double width, double height);
int geo_observer_is_singular(const geo_observer* obs);
/* Observer::calc_transformation_pipeline (observer.rs:197-262). */
int geo_observer_calc_transformation_pipeline(geo_observer* obs, geo_frame* out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* GEO_GEO_H */
