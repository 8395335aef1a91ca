/*
 * bzr_debug.h -- test hooks of libbzr.so (not part of the drop-in boundary).
 */
#ifndef BZR_DEBUG_H
#define BZR_DEBUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The culling boxes the BVH is built from, by patch index: boxes[6*i] = lo.xyz, hi.xyz of the region
 * where patch i's planar gate can pass for ray origins with |s|_inf <= *s_max.  Returns 0 on success. */
int32_t bzr_debug_gate_boxes(const void *patches, uint32_t n, uint32_t stride, float *boxes, float *s_max);
/* The same for one BVH tier: 0 = far (as above), 1 = near (bvh.hpp kTierNear; tighter boxes, valid for
 * origins |s|_inf <= *s_max, which is 8x the mesh's control-point span). */
int32_t bzr_debug_gate_boxes_tier(const void *patches, uint32_t n, uint32_t stride, int32_t tier, float *boxes,
                                  float *s_max);
/* Patches without a proven gate region (rounding-dominated, or non-finite records): they are not in the
 * tier's tree and every wave-segment gate-tests them (bvh.hpp Bvh::always).  *count = their number; out
 * (optional, *count words) = their indices, ascending.  Their gate boxes above are the always-hit box.
 * Returns 0 on success. */
int32_t bzr_debug_always_list(const void *patches, uint32_t n, uint32_t stride, int32_t tier, uint32_t *out,
                              uint32_t *count);
/* The always list's wedge pre-test (bvh.cpp always_wedge), 8 floats per always-listed patch in list order:
 * w.xyz, L, H, B, C, 0.  A lane whose float plane point p~ = s + d (num x rcp(cs)) has w.p~ outside
 * [L - B|p~| - C(|s|+|p~|), H + B|p~| + C(|s|+|p~|)] cannot pass that patch's gate. */
int32_t bzr_debug_always_wedges(const void *patches, uint32_t n, uint32_t stride, int32_t tier, float *out);
/* The oriented gate-region boxes of one tier's wide-patch subtree (bvh.hpp Bvh4ObbNode), by patch index:
 * out[16*i] = centre xyz, axes u v w (xyz each), half extents (3), then 1.0f if patch i is a wide patch
 * (its parent node tests this box) or 0.0f (16 zeros: the patch is AABB-culled).  Returns 0 on success. */
int32_t bzr_debug_gate_obbs(const void *patches, uint32_t n, uint32_t stride, int32_t tier, float *out);
/* The bounding sphere bzr_illuminate culls with (Ritter over the gate boxes): centre xyz, radius. */
int32_t bzr_debug_bounding_sphere(const void *patches, uint32_t n, uint32_t stride, float out[4]);
/* Host replay of the device BVH walk (same 4-wide trees and wave-uniform tier choice, same float slab and
 * oriented-box tests -- 1/x where the device uses v_rcp_f32) over `nr` rays in SoA
 * [6, nr], grouped in waves of 64 consecutive rays.  hits (optional, nr x n bytes): hits[r*n + b] = 1
 * when ray r reaches patch b's leaf box -- a superset of the patches whose planar gate it passes.
 * stats[0] node visits (per wave), [1] leaf records fetched (per wave), [2] leaf-box hits (per ray),
 * [3] waves.  Returns 0 on success. */
int32_t bzr_debug_traverse(const void *patches, uint32_t n, uint32_t stride, const float *rays, uint32_t nr,
                           uint8_t *hits, uint64_t stats[4]);
/* Host replay of the wave-bundle walk (trace.hip BZR_TRACE_BUNDLE: batches of up to 16 nodes tested against
 * the wave's ray bundle) beside the per-lane walk, waves of 64 consecutive rays; waves whose direction spread
 * exceeds max_spread take the per-lane walk.  stats[0] waves, [1] bundle batches, [2] leaves (bundle or
 * per-lane walk), [3] per-lane node visits, [4] per-lane leaves, [5] per-lane leaves the bundle walk missed
 * (0: conservative), [6] child slots tested, [7] deepest work stack, [8] waves on the per-lane walk, [9]
 * batches after which the work stack exceeded 64, [10] bundle-walk leaves the leaf pre-test keeps, [11] leaves it
 * rejected although some lane's exact planar gate passes (0: conservative).  Returns 0 on success. */
int32_t bzr_debug_traverse_bundle(const void *patches, uint32_t n, uint32_t stride, const float *rays, uint32_t nr,
                                  float max_spread, uint64_t stats[12]);
/* The same replay on trees built with `split` cells per barycentric axis of each narrow patch's gate region
 * (bvh.hpp build_bvh; < 1: the split the fused refract and chain kernels walk).  A split tree names a leaf slot once per
 * cell box: [2] and [4] count distinct slots per wave, as the device's per-wave slot set queues them.  Four more
 * words: [12] leaf references the bundle walk reached, [13] nodes it visited, [14] / [15] the near / far tree's
 * leaf references.  slots (optional, two words per wave): the distinct slots this walk queued, and the distinct
 * slots the device's two-level walk queues (an inner child's own box skipped, its four children tested in its
 * place: a superset; 0xFFFFFFFF with oriented-box nodes) -- the wave's leaf fetches in k_trace's counters. */
int32_t bzr_debug_traverse_bundle_split(const void *patches, uint32_t n, uint32_t stride, const float *rays, uint32_t nr,
                                        float max_spread, int32_t split, uint64_t stats[16], uint32_t *slots);
/* The leaf references of one tier's device tree built with `split`: count, and per reference the patch it names
 * (mesh order) and its box (lo xyz, hi xyz) when patch / boxes are not null; also Bvh::order (n words) and
 * Bvh::patch_box (8 floats per slot) when not null. */
int32_t bzr_debug_split_boxes(const void *patches, uint32_t n, uint32_t stride, int32_t tier, int32_t split,
                              uint32_t *patch, float *boxes, uint32_t *count, uint32_t *order, float *patch_box);
/* The extreme points (double) of every proven finite gate region of one tier: count, and per point its patch
 * (mesh order) and xyz when patch / pts are not null. */
int32_t bzr_debug_region_points(const void *patches, uint32_t n, uint32_t stride, int32_t tier, uint32_t *patch,
                                double *pts, uint32_t *count);
/* One tier's device tree (128-byte Bvh4Node records) built with `split`: count, and the nodes when out is not null. */
int32_t bzr_debug_nodes4(const void *patches, uint32_t n, uint32_t stride, int32_t tier, int32_t split, void *out,
                         uint32_t *count);
/* Device check of the exact normalized() (Eigen a / sqrt(a.a)): `a` is device memory [3][n], `out` device
 * memory [6][n]: rows 0-2 the product's normalized(a), rows 3-5 the same with the compiler's correctly
 * rounded sqrt and one division per component.  Asynchronous on the context's stream.  ctx is a
 * bzr_ctx* (bzr.h). */
int32_t bzr_debug_unit(void *ctx, const float *a, uint32_t n, float *out);
/* Device check of newton_tail's bracket quotients hIn / cos, hOut / cos (patch_math.hpp div_heights: one shared
 * reciprocal where proven): `a` device memory [3][n] (hIn, hOut, cos), `out` device memory [4][n]: rows 0-1 the
 * product's quotients, rows 2-3 one correctly rounded division each.  Asynchronous on the context's stream. */
int32_t bzr_debug_div_heights(void *ctx, const float *a, uint32_t n, float *out);
/* Device check of the trace kernels' per-segment bundle setup (trace.hip bundle_setup_swap) on waves of 64
 * consecutive rays: `rays` device memory [6][n] (origin xyz, direction xyz), `active` device memory [n] bytes (0: the
 * lane is idle), n a multiple of 64, `out` device memory [n / 64][23]: per wave the 22 bundle words (origin box lo,
 * hi; direction box lo, hi; finite flag; 1 / Dl', 1 / Dh'; mixed flags) and the returned direction spread.
 * Asynchronous on the context's stream. */
int32_t bzr_debug_bundle_setup(void *ctx, const float *rays, const uint8_t *active, uint32_t n, float *out);
/* Device check of the fused pass loop's near-first order (trace.hip batch_append / batch_store over pass_order.hpp:
 * the insertion the trace kernels run while they collect a batch of leaves).  n key sequences, one wave each: `keys`
 * device memory [n][16], `len` device memory [n] (<= 16 entries used), `out` device memory [n][16][3].  Entry e of a
 * sequence carries patch index e and the ballot 0x9E3779B97F4A7C15 * (e + 1); out[w][p] = the index and the ballot
 * (low, high word) of the entry at place p of the list the passes read -- the stable ascending order of the keys --
 * and 0xFFFFFFFF words at and past len[w].  Asynchronous on the context's stream. */
int32_t bzr_debug_pass_order(void *ctx, const uint32_t *keys, const uint32_t *len, uint32_t n, uint32_t *out);
/* Device check of BZR_MODE_FAST's primitives (patch_math.hpp namespace fast): `a` device memory [3][n], `out`
 * device memory [5][n]: row 0 fast::div_rn(a0, a1), row 1 fast::sqrt_rn(|a0|), rows 2-4 fast::normalized(a).
 * Asynchronous on the context's stream. */
int32_t bzr_debug_fast_unit(void *ctx, const float *a, uint32_t n, float *out);
/* The staged path's chunking rule as pure host arithmetic (no device): *cap = the rays-per-chunk cap for a device with
 * `free_bytes` free (whole waves, at least 64, at most 2^23 = 8 M; a quarter of the free memory at the
 * workspace's bytes per ray; free_bytes == 0 means unknown and gives the ceiling), *chunk = the chunk length for a
 * batch of n rays under that cap (n itself when it fits, else equal pieces rounded up to whole waves, never above
 * the cap; the last chunk is ragged). */
int32_t bzr_debug_chunk_plan(uint64_t free_bytes, uint64_t n, uint32_t *cap, uint32_t *chunk);
/* Lowers the context's chunk cap for the following calls (staged calls and bzr_illuminate's batches): the cap in
 * force becomes `rays` rounded down to whole waves, at least 64, and never above the cap the context derives itself
 * (free memory at its first staged call, 8 M).  rays == 0 restores the automatic cap.  *effective (optional) = the
 * cap now in force (asking for it sizes the automatic cap now if no staged call has yet).  ctx is a bzr_ctx* (bzr.h). */
int32_t bzr_debug_chunk_cap(void *ctx, uint32_t rays, uint32_t *effective);
/* Per-wave timing of the fused kernel: while set, every fused call (k_trace, one 64-ray wave per 64
 * consecutive rays) of `n` <= 64 * waves rays writes clock[2w] = the wave's start (s_memtime ticks) and
 * clock[2w+1] = its duration, for wave w = ray index / 64.  `clock` is device memory; NULL turns it off.
 * ctx is a bzr_ctx* (bzr.h). */
int32_t bzr_debug_wave_clock(void *ctx, unsigned long long *clock, uint32_t waves);
/* The same with the constant 100 MHz clock beside it (a diagnostic of the shader clock the chip holds,
 * MI355X_MICROARCH.md "DVFS give-back" item 6): clock[4w] = start, [4w+1] = duration (s_memtime ticks),
 * [4w+2] = start, [4w+3] = duration (s_memrealtime ticks); the wave's clock is [4w+1] / [4w+3] x 100 MHz. */
int32_t bzr_debug_wave_clock_rate(void *ctx, unsigned long long *clock, uint32_t waves);
/* Host check of the short Newton pass (patch_math_body.inc newton_tail's hook; trace.hip BZR_TRACE_SHORT): for
 * each of m triples (patch[i] < n, ray i of `rays` in SoA [6, m], limit[i]: 0 = cThis, 1 = cNone) the host's
 * BezierTriangle::intersect twice -- `full` as always, `skipped` with the hook answering "not needed", so the last
 * iteration's normal is not evaluated.  12 words per triple each: t, point xyz, cos, barycentrics, normal xyz,
 * what (uint32).  In `skipped` the normal and cos words are unspecified; every other word must equal `full`'s.
 * No device.  Returns 0 on success. */
int32_t bzr_debug_newton_short(const void *patches, uint32_t n, uint32_t stride, const uint32_t *patch,
                               const float *rays, const uint8_t *limit, uint32_t m, float *full, float *skipped);
/* Host evaluation of the Fresnel transmittance the kernels run (patch_math_body.inc fresnel_t, the text
 * bzr_trace_chain_power documents in bzr.h): for each of n pairs (eta[i], cs[i]), s2 = eta^2 (1 - cs^2) as Snell's
 * step computes it and t_out[i] = T, or 0 where s2 >= 0.99 (no refraction).  No device.  Returns 0 on success. */
int32_t bzr_debug_fresnel(const float *eta, const float *cs, uint32_t n, float *t_out);
/* The chain's Beer-Lambert term (patch_math_body.inc att, the text bzr_trace_chain_absorb documents in bzr.h):
 * out[i] = att(x[i]) for x[i] >= 0 (or NaN).  x and out are host memory.  With ctx == NULL the host's compilation of
 * the text evaluates it (no device); otherwise ctx is a bzr_ctx* (bzr.h) and one small kernel on its device does,
 * synchronously.  The two agree bit for bit.  Returns 0 on success. */
int32_t bzr_debug_attenuation(void *ctx, const float *x, uint32_t n, float *out);
/* bzr_coat_transmittance (bzr.h) over n cosines at once: out[i] = coat_t(row, mu[i]), row [BZR_COAT_SAMPLES], the same
 * compilation of patch_math_body.inc coat_t.  A NULL pointer with n > 0, or a mu[i] that is not >= 0, returns
 * BZR_ERR_INVALID_ARGUMENT with nothing written.  No device.  Returns 0 on success. */
int32_t bzr_debug_coat_transmittance(const float *row, const float *mu, uint32_t n, float *out);
/* A/B hook of k_land_far's wave combine (bzr_farfield_bin, bzr_illuminate_farfield): the following calls on this
 * context run at most `rounds` leader-election rounds per wave before the lanes left over issue their own atomics
 * (0: plain per-lane atomics, 64: unbounded); a negative value restores the default.  The maps' bits do not depend
 * on it.  ctx is a bzr_ctx* (bzr.h). */
int32_t bzr_debug_farfield_rounds(void *ctx, int32_t rounds);
/* bzr_farfield_cell (bzr.h) over n directions at once: far is a bzr_farfield*, d_xyz [n][3], cell [n] (-1: not
 * binned).  No device.  Returns 0 on success. */
int32_t bzr_debug_farfield_cells(const void *far, const float *d_xyz, uint32_t n, int32_t *cell);
#ifdef __cplusplus
}
#endif
#endif
