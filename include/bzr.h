/*
 * bzr.h -- C ABI of the MI355X-native Bezier-triangle ray tracer (libbzr.so).
 *
 * The reference (balazs-bamer/cuda-bezier-triangle-raytracer @ v1) has no FFI;
 * its boundary is the C++ class API it exports for this path:
 *   BezierMesh::intersect(Ray)          reference/bezierMesh.h:37, bezierMesh.cpp:206-227
 *   BezierTriangle::intersect(Ray, lim) reference/bezierTriangle.h:105, bezierTriangle.cpp:123-195
 *   BezierLens::refract(Ray, expected)  reference/bezierLens.h:27, bezierLens.cpp:4-34
 *   the refraction-chain driver loop    reference/test.cpp:376-401
 * plus the host preprocessing that produces the patch records
 *   Mesh                                reference/mesh.h:18-133
 *   BezierMesh::BezierMesh(Mesh)        reference/bezierMesh.cpp:4-51
 * Every entry point below is the batch form of one of those, with plain
 * pointers and sizes.  The C++ drop-in classes in include/bzr/bzr.hpp forward
 * to it; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *   - Every call returns bzr_status (0 = ok).  Nothing throws across the ABI.
 *     bzr_last_error() returns the calling thread's last error text.
 *   - Rays are SoA: rays_soa[k*n + i], k = 0..5 -> ox, oy, oz, dx, dy, dz.
 *     Directions are used as given (the reference's Ray ctor normalises;
 *     normalise on the caller side exactly as Ray(start, dir) does).
 *   - Hits are SoA, 13 words per ray: hits_soa[k*n + i] with k =
 *       0 t   1 px  2 py  3 pz  4 cos  5 b0  6 b1  7 b2  8 nx  9 ny  10 nz
 *       11 what (uint32: 0..2 follow side, 3 none, 4 intersect)
 *       12 patch (uint32: index of the patch hit, 0xFFFFFFFF on a miss)
 *     On a miss t = FLT_MAX and fields 1..10 are 0 (the reference leaves them
 *     uninitialised).
 *   - Pointer residency is selected per call by BZR_DEVICE_PTRS; host-pointer
 *     calls are synchronous, device-pointer calls are asynchronous on the
 *     context's stream until bzr_sync().
 *   - Numerics: BZR_MODE_PARITY (default) is IEEE binary32 with the
 *     reference's operation order and no contraction, bit-identical to the CPU
 *     oracle.  BZR_MODE_FAST keeps the planar gate exact (same candidate
 *     patches as the reference) and runs the Newton stage with FMA contraction
 *     and the hardware's approximate reciprocal / square root; it meets the
 *     SURVEY 8c fast-mode gates (hit/miss >= 99.5 %, t within 1e-5 relative on
 *     >= 99 % of same-patch hits) but is not bit-exact.  FAST needs the culled
 *     path: FAST | BZR_ACCEL_NONE returns BZR_ERR_INVALID_ARGUMENT.
 *   - Scan strategy: by default each lens mesh carries a BVH over the regions
 *     where each patch's planar gate can pass, and only those patches reach
 *     the Newton stage -- the output bits are the brute-force scan's.
 *     BZR_ACCEL_NONE runs the reference's brute-force scan itself (A/B testing).
 *     Patches with no proven bound on where their float gate can pass (planes
 *     through ~the origin whose M is rounding-dominated, non-finite records)
 *     are not in the BVH: every wave tests them (the always list).
 *   - Flags are checked first: unknown bits, BZR_PIPELINE_STAGED together with
 *     BZR_PIPELINE_FUSED, or FAST | ACCEL_NONE return BZR_ERR_INVALID_ARGUMENT.
 */
#ifndef BZR_H
#define BZR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BZR_ABI_VERSION 2

typedef int32_t bzr_status;
enum {
  BZR_OK = 0,
  BZR_ERR_INVALID_ARGUMENT = 1,
  BZR_ERR_HIP = 2,
  BZR_ERR_OUT_OF_MEMORY = 3,
  BZR_ERR_PREPROCESS = 4,   /* a reference preprocessing "throw" (e.g. "Vertex on edge detected.") */
  BZR_ERR_NO_DEVICE = 5,
  BZR_ERR_CAPACITY = 6      /* a compact multi-GPU gather had more survivors than its capacity (bzr_tiled_sync) */
};

enum {
  BZR_HOST_PTRS = 0u,
  BZR_DEVICE_PTRS = 1u,
  BZR_MODE_PARITY = 0u,
  BZR_MODE_FAST = 2u,
  BZR_ACCEL_NONE = 4u,  /* brute-force patch scan instead of the (bit-identical) BVH-culled path */
  /* Culled-path pipeline (same output bits either way; neither flag = automatic choice):
   *   fused   one kernel per call (k_trace): each wave walks the BVH and runs the Newton stage for its own
   *           rays with patch-uniform records -- no per-pair HBM traffic; best when a wave's rays meet
   *           few distinct patches (dense ray grids, many rays per patch)
   *   staged  traverse -> bucket pairs by patch -> Newton -> resolve -> finish per segment; full-wave
   *           Newton passes whatever the ray coherence, at 3-12x the algorithmic HBM bytes
   * automatic: fused when n >= 256 x the largest lens's patch count (and always for meshes of 2^25 patches
   * or more, which the staged encoding cannot hold), else staged.  The 256 is tuned for callers that keep
   * two or three frames in flight (bench.py, bzr_tiled with several slots): there the fused path wins from
   * ~256 rays per patch up.  A caller that traces ONE frame at a time and waits for it sees the fused
   * frame's tail (its slowest waves) undiluted; the fused path dispatches a context's repeated same-size
   * calls longest-tile-first from the previous calls' costs, which shortens that tail (cfg2 lone frames
   * 0.62 -> 0.40 ms), and lone cfg2 frames now run as fast fused as staged (0.395 vs 0.392 ms, 341 rays per
   * patch).  The first call of a size, or calls of changing sizes, run in input order. */
  BZR_PIPELINE_STAGED = 8u,
  BZR_PIPELINE_FUSED = 16u,
  /* Ray records in the reference's layout: rays / out_rays are [n][6] (per ray start xyz, direction xyz --
   * `Ray` of reference/3dGeomUtil.h:168, 24 bytes) instead of [6][n].  Host or device pointers alike; the library
   * transposes on the device (48 bytes per ray each way, HBM-bound), so a C++ caller hands its std::vector<Ray>
   * over with no host-side conversion.  Accepted by bzr_intersect (rays), bzr_refract, bzr_trace_chain,
   * bzr_trace_chain_power, bzr_trace_tiled, bzr_tiled_set_rays (rays) and bzr_tiled_trace (out_rays); other calls reject it (the illumination calls and
   * bzr_farfield_bin, which reads rows only, among them).  Other
   * arrays (hits, status, segments, expected) keep their layouts. */
  BZR_RAYS_AOS = 32u
};

enum { BZR_WHAT_FOLLOW0 = 0, BZR_WHAT_FOLLOW1 = 1, BZR_WHAT_FOLLOW2 = 2, BZR_WHAT_NONE = 3, BZR_WHAT_INTERSECT = 4 };
enum { BZR_LIMIT_THIS = 0, BZR_LIMIT_NONE = 1 };                       /* BezierTriangle::LimitPlaneIntersection */
enum { BZR_RR_NONE = 0, BZR_RR_INSIDE = 1, BZR_RR_OUTSIDE = 2 };       /* RefractionResult */
/* bzr_trace_chain_bidir alone: the ray left the chain in front of its first lens.  (3 is kept free.) */
enum { BZR_RR_BACK = 4 };
enum { BZR_HIT_FIELDS = 13, BZR_RAY_FIELDS = 6 };

/* One cubic Bezier patch, byte-identical to the reference's BezierTriangle
 * (reference/bezierTriangle.h:64-80; Eigen column-major 3x3): 264 bytes. */
typedef struct bzr_patch {
  float    under_n[3], under_c;        /* mUnderlyingPlane                  @0   */
  float    divider[3][4];              /* mNeighbourDividerPlanes (n, c)    @16  */
  uint32_t neigh[3];                   /* mNeighbours                       @64  */
  float    cp[10][3];                  /* mControlPoints                    @76  */
  float    minv[9];                    /* mBarycentricInverse, col-major    @196 */
  float    h_in, h_out;                /* mHeightInside / mHeightOutside    @232 */
  float    dir_a[3], dir_b[3];         /* derivative direction vectors      @240 */
} bzr_patch;

typedef struct bzr_ctx bzr_ctx;         /* one HIP device + one stream; one host thread at a time */
typedef struct bzr_mesh bzr_mesh;       /* immutable device copy of a patch array */
typedef struct bzr_trimesh bzr_trimesh; /* host triangle mesh (reference Mesh) */

/* ---- library ---- */
int32_t     bzr_abi_version(void);
const char *bzr_last_error(void);
bzr_status  bzr_device_count(int32_t *count);

/* ---- context ---- */
bzr_status bzr_ctx_create(int32_t hip_device, bzr_ctx **out);
bzr_status bzr_ctx_destroy(bzr_ctx *ctx);
/* Launch on a caller-owned hipStream_t (NULL = the HIP null stream);
 * bzr_ctx_use_own_stream() goes back to the context's own non-blocking stream.  Work already queued
 * on the previous stream is ordered before later launches (an event hand-off, no host wait): the
 * hand-off records an event on the previous stream, so a caller stream must stay alive while it is
 * bound and until the next bzr_ctx_set_stream / bzr_ctx_use_own_stream / bzr_ctx_destroy returns.
 * Device-pointer calls launch on the bound stream and return before the kernels finish: inputs must
 * be ready on that stream, and outputs are valid on it (or after bzr_sync). */
bzr_status bzr_ctx_set_stream(bzr_ctx *ctx, void *hip_stream);
bzr_status bzr_ctx_use_own_stream(bzr_ctx *ctx);
bzr_status bzr_ctx_get_stream(bzr_ctx *ctx, void **hip_stream);
bzr_status bzr_sync(bzr_ctx *ctx);

/* ---- measurement: per-kernel HIP-event timing on the context's stream ---- */
enum {
  BZR_KERNEL_TRAVERSE = 0,        /* BVH walk + planar gate -> candidate pairs, per-patch histogram */
  BZR_KERNEL_BUCKET = 1,          /* prefix sum + scatter of the pairs into patch-major order */
  BZR_KERNEL_NEWTON = 2,          /* Newton stage per pair, patch-uniform waves */
  BZR_KERNEL_FOLLOW = 3,          /* k_resolve: follow-side neighbour retries + the overflow rays' full scans */
  BZR_KERNEL_FINISH = 4,          /* winner -> BezierIntersection / refraction */
  BZR_KERNEL_OVERFLOW = 5,        /* (unused since the full scans run inside k_resolve; id kept) */
  BZR_KERNEL_INTERSECT_SCAN = 6,  /* brute force (BZR_ACCEL_NONE) */
  BZR_KERNEL_REFRACT_SCAN = 7,
  BZR_KERNEL_CHAIN_SCAN = 8,
  BZR_KERNEL_PATCH = 9,
  BZR_KERNEL_NEWTON_LANE = 10,    /* Newton stage for fragmented pair chunks, one patch record per lane */
  BZR_KERNEL_TRACE = 11,          /* fused culled path: BVH walk + gate + Newton + winner (+ refraction chain) */
  BZR_KERNEL_COUNT = 12
};
/* While enabled, every launch is bracketed by hipEvents on the context's stream. */
bzr_status bzr_ctx_timing(bzr_ctx *ctx, int32_t enable);
/* Synchronises, returns the summed milliseconds and launch counts per kernel id since the last
 * report, and resets them. */
bzr_status bzr_ctx_timing_report(bzr_ctx *ctx, float ms[BZR_KERNEL_COUNT], uint32_t calls[BZR_KERNEL_COUNT]);

/* ---- measurement: work counters of the culled path (device-side, accumulated per segment) ---- */
enum {
  BZR_COUNTER_SEGMENTS = 0,      /* rays traced (one BezierMesh::intersect each) */
  BZR_COUNTER_PAIRS = 1,         /* (ray, patch) pairs that passed the planar gate: Newton runs */
  BZR_COUNTER_FOLLOWS = 2,       /* follow-side retries on a neighbour patch: Newton runs */
  BZR_COUNTER_OVERFLOW_RAYS = 3, /* rays resolved by the in-order full scan */
  BZR_COUNTER_LANE_CHUNKS = 4,   /* staged path: 64-pair chunks spanning many patches, one record per lane */
  BZR_COUNTER_NODE_VISITS = 5,   /* fused path: BVH nodes fetched (per wave, 128 B each) */
  BZR_COUNTER_LEAF_FETCHES = 6,  /* fused path: leaf gate records fetched (per wave, 64 B each) */
  BZR_COUNTER_GATE_TESTS = 7,    /* fused path: planar gates evaluated (per ray: lanes whose box test hit a fetched leaf) */
  BZR_COUNTER_NEWTON_ROUNDS = 8, /* fused path: patch-uniform Newton passes (per wave; cThis + follow-side) */
  BZR_COUNTER_ROUNDS_ODD = 9,    /* fused path: the passes of odd chain segments (refract(OUTSIDE): a lens's back surface) */
  BZR_COUNTER_RUNS_ODD = 10,     /* fused path: their Newton runs (pairs + follow retries) */
  BZR_COUNTER_SHORT_PASSES = 11, /* fused: Newton passes that skipped the last normal: no lane could win (BZR_TRACE_SHORT) */
  BZR_COUNTER_COUNT = 12
};
/* While enabled, each culled segment adds its counts on the device (one tiny kernel per segment). */
bzr_status bzr_ctx_counters(bzr_ctx *ctx, int32_t enable);
/* Synchronises, returns the counts accumulated since the last report, and resets them. */
bzr_status bzr_ctx_counters_report(bzr_ctx *ctx, uint64_t counts[BZR_COUNTER_COUNT]);

/* ---- device mesh: BezierMesh's patch vector (reference/bezierMesh.h:17) ---- */
/* Copies n records of `stride` bytes (stride >= sizeof(bzr_patch)) from host memory. */
bzr_status bzr_mesh_create(bzr_ctx *ctx, const void *patches, uint32_t n, uint32_t stride, bzr_mesh **out);
bzr_status bzr_mesh_destroy(bzr_mesh *mesh);
bzr_status bzr_mesh_size(const bzr_mesh *mesh, uint32_t *n);

/* ---- hot path ---- */
/* BezierMesh::intersect over a ray batch (reference/bezierMesh.cpp:206-227). */
bzr_status bzr_intersect(bzr_ctx *ctx, const bzr_mesh *mesh, const float *rays_soa, uint32_t n,
                         float *hits_soa, uint32_t flags);
/* One hit in the reference's BezierIntersection layout (reference/bezierTriangle.h:7-21 with
 * Intersection of reference/3dGeomUtil.h:209-214): 52 bytes, `valid` is the bool mValid in its first
 * byte (the other three bytes zero). */
typedef struct bzr_hit_record {
  uint32_t valid;             /* mIntersection.mValid (what == BZR_WHAT_INTERSECT)   @0  */
  float    point[3];          /* mIntersection.mPoint                                @4  */
  float    cos_incidence;     /* mIntersection.mCosIncidence                         @16 */
  float    distance;          /* mIntersection.mDistance (FLT_MAX on a miss)          @20 */
  float    bary[3];           /* mBarycentric                                        @24 */
  float    normal[3];         /* mNormal                                             @36 */
  uint32_t what;              /* mWhat (BZR_WHAT_*)                                  @48 */
} bzr_hit_record;
/* bzr_intersect with the hits written as n bzr_hit_record (the drop-in's BezierIntersection array, no
 * host-side conversion; the records are built on the device, 52 B per ray) and the hit patch indices in
 * patch_index [n] (may be NULL; 0xFFFFFFFF on a miss).  Same values as bzr_intersect's rows; flags as
 * bzr_intersect's, BZR_RAYS_AOS included. */
bzr_status bzr_intersect_records(bzr_ctx *ctx, const bzr_mesh *mesh, const float *rays, uint32_t n,
                                 bzr_hit_record *records, uint32_t *patch_index, uint32_t flags);
/* BezierTriangle::intersect for (patch, ray, limit) triples (reference/bezierTriangle.cpp:123-195).
 * The `patch` field of the output is the input patch index. */
bzr_status bzr_patch_intersect(bzr_ctx *ctx, const bzr_mesh *mesh, const uint32_t *patch_index,
                               const uint32_t *limit, const float *rays_soa, uint32_t n,
                               float *hits_soa, uint32_t flags);
/* BezierLens::refract (reference/bezierLens.cpp:4-34); expected may be NULL (then every ray expects
 * `expected_all`).  out_rays_soa: the refracted ray (start = hit point) when status != NONE,
 * the input ray otherwise. */
bzr_status bzr_refract(bzr_ctx *ctx, const bzr_mesh *mesh, float refractive_index, const float *rays_soa,
                       const uint32_t *expected, uint32_t expected_all, uint32_t n,
                       float *out_rays_soa, uint32_t *out_status, uint32_t flags);
/* The reference refraction chain (reference/test.cpp:376-401): for each lens, refract(INSIDE) then
 * refract(OUTSIDE); a NONE terminates the ray.  out_rays_soa: ray after the last successful
 * refraction (input ray if none); out_status: last status (OUTSIDE = passed every lens);
 * out_segments (may be NULL): BezierMesh::intersect calls made for the ray. */
bzr_status bzr_trace_chain(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *refractive_index,
                           uint32_t nlens, const float *rays_soa, uint32_t n, float *out_rays_soa,
                           uint32_t *out_status, uint32_t *out_segments, uint32_t flags);
/* bzr_trace_chain with the rays' power.  weight_in [n] (may be NULL: every ray starts at 1.0f) and out_weight [n]
 * are plain rows in either ray layout, host or device memory as the rays; weight_in == out_weight is allowed.
 * out_weight[i] = weight_in[i] times the unpolarised Fresnel transmittance T of each successful refraction of
 * ray i, multiplied in chain order.  With eta = 1/ri entering and ri leaving, cs the hit's cosine and
 * s2 = eta^2 (1 - cs^2) < 0.99 as Snell's step has them, in IEEE binary32 without contraction:
 *   c1 = |cs|   c2 = sqrt(1 - s2)   rs = (eta c1 - c2) / (eta c1 + c2)   rp = (eta c2 - c1) / (eta c2 + c1)
 *   T = 1 - 0.5 (rs rs + rp rp)
 * always in exact arithmetic (BZR_MODE_FAST too: the Fresnel term belongs to Snell's step).  A refraction that
 * returns NONE leaves the weight untouched, so a ray that never refracts keeps weight_in[i].  Everything else --
 * flags, BZR_RAYS_AOS for the ray arrays, pipeline choice, out_rays / out_status / out_segments bit for bit -- is
 * bzr_trace_chain's. */
bzr_status bzr_trace_chain_power(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *refractive_index,
                                 uint32_t nlens, const float *rays_soa, const float *weight_in, uint32_t n,
                                 float *out_rays_soa, float *out_weight, uint32_t *out_status, uint32_t *out_segments,
                                 uint32_t flags);
/* ---- spectral channels ----
 * A channel is an index c in [0, nchan), 1 <= nchan <= BZR_MAX_CHANNELS: one wavelength sample.
 * ri_table[nlens][nchan] (row-major float32, host memory always, like refractive_index) gives lens l's index
 * for channel c; bzr_dispersion_index fills a row from a glass's dispersion formula. */
#define BZR_MAX_CHANNELS 64
/* bzr_trace_chain_power with one refractive index per ray and lens.  channel [n], one uint8_t per ray, is a plain
 * row in either ray layout, host or device memory as the rays.  Ray i is traced exactly as bzr_trace_chain_power
 * traces it with refractive_index[l] = ri_table[l][channel[i]]: the same eta = 1/ri division on the device, the
 * same Fresnel term (exact under BZR_MODE_FAST too), the same bits in out_rays, out_weight, out_status and
 * out_segments.  weight_in may be NULL and may be out_weight; out_weight is required.  A ray whose channel[i] is at
 * or above nchan is handled like a ray with a non-finite component: status NONE, one segment, its ray and weight
 * unchanged, and no other ray is affected -- on every pipeline, for host rows as for device rows (which cannot be
 * validated), so it is no error.  nchan of 0 or above BZR_MAX_CHANNELS, a NULL ri_table, channel or out_weight and
 * bzr_trace_chain's nlens rules return BZR_ERR_INVALID_ARGUMENT before any output is touched.  Flags,
 * BZR_RAYS_AOS, the pipeline choice and chunking are bzr_trace_chain_power's.  The multi-GPU plan (bzr_trace_tiled,
 * bzr_tiled_*, bzr_pack_frame) takes no channels, and bzr_refract stays single-index. */
bzr_status bzr_trace_chain_spectral(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table, uint32_t nlens,
                                    uint32_t nchan, const float *rays_soa, const uint8_t *channel,
                                    const float *weight_in, uint32_t n, float *out_rays_soa, float *out_weight,
                                    uint32_t *out_status, uint32_t *out_segments, uint32_t flags);
/* ---- total internal reflection ----
 * bzr_trace_chain_spectral with reflections: a ray that cannot leave a lens is mirrored inside it and traced against
 * the same lens again, until it leaves or has reflected max_bounces times in that lens (max_bounces <=
 * BZR_MAX_BOUNCES).  In a refract(OUTSIDE) segment whose winning hit has cs >= 0, for a ray whose channel is in the
 * table, with s2 = ri^2 (1 - cs^2) as Snell's step has it:
 *   s2 < 0.99        the ray refracts out of the lens, with the Fresnel gain (bzr_trace_chain_power);
 *   0.99 <= s2 < 1   NONE, as in every other chain: the reference's grazing limit (T is near 0 there anyway);
 *   s2 >= 1          total internal reflection, if the ray has reflected fewer than max_bounces times in this lens:
 *                      k = 2 cs   r = d - normal k (per component: one multiply, one subtract)
 *                      direction = r / sqrt(r.r) (r.r = r0 r0 + (r1 r1 + r2 r2); r itself if r.r is not > 0)
 *                      origin = the hit's point
 *                    in IEEE binary32 without contraction, under BZR_MODE_FAST too (it belongs to Snell's step).  The
 *                    weight is not touched, the ray stays inside and meets the same lens again with expected OUTSIDE.
 *                    With the lens's budget spent it is NONE: ray and weight stay as the last reflection left them.
 * A NaN s2 is NONE, and a refract(INSIDE) segment never reflects.  out_status is OUTSIDE or NONE as before; out_rays is
 * the ray after its last successful refraction or reflection; out_segments counts every BezierMesh::intersect made for
 * the ray, bounce segments included (at most nlens (2 + max_bounces)); out_bounces [n] (may be NULL, a plain row like
 * out_segments) is the ray's reflections summed over the lenses.  channel may be NULL: every ray is channel 0 (with
 * nchan = 1 the single-index form).  With max_bounces = 0 every output is bzr_trace_chain_spectral's bit for bit and
 * out_bounces is all zero.  max_bounces above BZR_MAX_BOUNCES returns BZR_ERR_INVALID_ARGUMENT before any output is
 * touched; everything else -- the table and nlens rules, weight_in NULL or aliasing out_weight, out_weight required,
 * a channel at or above nchan and a non-finite ray (NONE after one segment, unchanged), flags, BZR_RAYS_AOS, host and
 * device pointers, the pipeline choice and chunking -- is bzr_trace_chain_spectral's.  bzr_illuminate_tir (below)
 * is the illumination entry point that reflects; bzr_illuminate, bzr_illuminate_power and bzr_illuminate_spectral,
 * the multi-GPU plan and bzr_refract do not reflect. */
#define BZR_MAX_BOUNCES 8
bzr_status bzr_trace_chain_tir(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table, uint32_t nlens,
                               uint32_t nchan, const float *rays_soa, const uint8_t *channel, const float *weight_in,
                               uint32_t n, uint32_t max_bounces, float *out_rays_soa, float *out_weight,
                               uint32_t *out_status, uint32_t *out_segments, uint32_t *out_bounces, uint32_t flags);
/* ---- optical path length ----
 * bzr_trace_chain_tir with two per-ray accumulators: out_opl [n], the optical path length sum n l over the ray's
 * legs, and out_glass [n] (may be NULL), the geometric length of the legs inside glass, summed over the lenses.
 * opl_in [n] (may be NULL: every ray starts at 0; may be out_opl) is the path the rays arrive with.  All three are
 * plain float rows like out_weight: host or device memory as the rays, in either ray layout.
 * For every segment that ends in a successful refraction or in a reflection, with s the segment's origin, p the
 * winning hit's point and ri the value Snell's step used (ri_table[l][channel]):
 *   e = p - s (per component)   z = e0 e0 + (e1 e1 + e2 e2)   len = sqrt(z)
 *   refract(INSIDE) segment  (the leg lies in air):     opl = opl + len
 *   refract(OUTSIDE) segment (the leg lies in glass,    glass = glass + len;  m = ri len;  opl = opl + m
 *                             bounce segments included)
 * in IEEE binary32 without contraction, the square root correctly rounded, under BZR_MODE_FAST too (it belongs to
 * the chain step, like the Fresnel term).  The leg is the distance between the points the chain continues from, not
 * the hit's t: t is BezierIntersection's value from before the last Newton step and differs from that distance by
 * up to 1e-3 relative, while the hit point lies on the surface, where the path length is stationary (Fermat).
 * A segment that ends NONE -- a miss, the wrong side, the grazing limit 0.99 <= s2 < 1, a refused reflection, a NaN
 * -- adds nothing: out_opl is the optical length of exactly the polyline from the input origin to out_rays' origin,
 * plus opl_in, and out_glass the part of that polyline inside glass.  A ray with a non-finite component and a ray
 * whose channel is at or above nchan keep opl_in and get glass 0.
 * out_rays, out_weight, out_status, out_segments and out_bounces are bzr_trace_chain_tir's bit for bit, for every
 * max_bounces including 0, and so are the argument rules; a NULL out_opl returns BZR_ERR_INVALID_ARGUMENT before any
 * output is touched.  The illumination entry points, the multi-GPU plan and bzr_refract carry no path length. */
bzr_status bzr_trace_chain_opl(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table, uint32_t nlens,
                               uint32_t nchan, const float *rays_soa, const uint8_t *channel, const float *weight_in,
                               const float *opl_in, uint32_t n, uint32_t max_bounces, float *out_rays_soa,
                               float *out_weight, uint32_t *out_status, uint32_t *out_segments, uint32_t *out_bounces,
                               float *out_opl, float *out_glass, uint32_t flags);
/* ---- surrounding media ----
 * bzr_trace_chain_opl with a medium in front of, between and behind the lenses: an immersed optic, an emitter under an
 * encapsulant, a cemented joint.  gap_table [nlens + 1][nchan] is row-major float32 and always host memory, like
 * ri_table: row l is the index of the medium in front of lens l, row nlens that of the medium behind the last lens;
 * NULL means every entry is 1.0f (vacuum).  For ray i with channel c in lens l let n0 = gap_table[l][c], n1 =
 * ri_table[l][c] and n2 = gap_table[l + 1][c].  Apart from the following the call is bzr_trace_chain_opl: the same
 * outputs, argument rules, flags, BZR_RAYS_AOS, host and device pointers, pipeline choice and chunking.
 *   refract(INSIDE) segment:   eta = n0 / n1, one correctly rounded binary32 division on the device (for 1 / ri);
 *   refract(OUTSIDE) segment:  eta = n1 / n2, one correctly rounded division (for ri), bounce segments included;
 *   everything derived from eta uses this eta: s2 = eta eta (1 - cs cs), the refraction limit s2 < 0.99, the
 *     reflection test s2 >= 1 of bzr_trace_chain_tir and the Fresnel term of bzr_trace_chain_power, in their operation
 *     order, without contraction and exact under BZR_MODE_FAST as there;
 *   per-leg step: a refract(INSIDE) leg adds m = n0 len; opl = opl + m (for opl + len); a refract(OUTSIDE) leg is
 *     unchanged, glass = glass + len; m = n1 len; opl = opl + m.  out_glass stays the geometric length inside lens
 *     glass: the gap media do not count;
 *   every used gap_table entry must be finite and > 0, else BZR_ERR_INVALID_ARGUMENT before any output is touched
 *     (ri_table is not validated, as in the other entry points).
 * Since x / 1 = x and 1 x = x exactly, a gap_table of ones or NULL gives bzr_trace_chain_opl's outputs bit for bit, in
 * every mode and on every pipeline.  The limits:
 *   The chain stays sequential.  A ray that leaves lens l is in medium l + 1 whichever surface it left through (only
 *     bounced rays can leave through the front).
 *   A front surface never reflects.  A refract(INSIDE) segment from a denser medium with s2 >= 0.99 is NONE (cfg2 with
 *     1.6 in front of 1.3: 102 more rays end NONE after one segment than in vacuum).
 *   bzr_illuminate, bzr_illuminate_power, bzr_illuminate_spectral, bzr_illuminate_tir, the multi-GPU plan and
 *     bzr_refract take no media; bzr_illuminate_media (below) is the illumination over this chain with absorption. */
bzr_status bzr_trace_chain_media(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                 const float *gap_table, uint32_t nlens, uint32_t nchan, const float *rays_soa,
                                 const uint8_t *channel, const float *weight_in, const float *opl_in, uint32_t n,
                                 uint32_t max_bounces, float *out_rays_soa, float *out_weight, uint32_t *out_status,
                                 uint32_t *out_segments, uint32_t *out_bounces, float *out_opl, float *out_glass,
                                 uint32_t flags);
/* ---- absorption ----
 * bzr_trace_chain_media with Beer-Lambert absorption along the legs.  Two tables follow gap_table, row-major float32
 * in host memory like ri_table: glass_absorb[nlens][nchan], the Napierian absorption coefficient of lens l's glass for
 * channel c per unit of the scene's length, and gap_absorb[nlens][nchan], the same for the medium in front of lens l
 * (gap_table's row l; the chain has no leg behind the last lens, so there is no row nlens).  Either may be NULL: all
 * zero.  Every used entry must be finite and >= 0, else BZR_ERR_INVALID_ARGUMENT before any output is touched.
 * The step runs for every segment that ends in a successful refraction or in a reflection -- the segments whose leg
 * enters out_opl -- with that leg's len, a = gap_absorb[l][c] on a refract(INSIDE) segment and glass_absorb[l][c] on a
 * refract(OUTSIDE) one, bounce segments included:
 *   x = a len;  A = a > 0 ? att(x) : 1.0f;  w = w A (the light travels the leg), then w = w T (it meets the surface:
 *   the Fresnel term as in bzr_trace_chain_power; a reflection has no T, and now applies A alone).
 * att(x) stands for exp(-x) and is defined by its operations, IEEE binary32 without contraction, exact under
 * BZR_MODE_FAST too (it belongs to the chain step):
 *   y = x * 0x3FB8AA3B (log2 e);  !(y < 125) -> 0 (a NaN too);  k = rint(y), ties to even;  f = y - k (exact);
 *   p = c7; for j = 6 .. 0: p = p * f; p = p + c_j;  att = p * 2^-k (exact),
 *   c_j = float((-ln 2)^j / j!) = 3f800000 bf317218 3e75fdf0 bd635847 3c1d955b baaec3ff 39218489 b77fe5fe.
 * att(0) = 1, every result is 0 or a normal number in (0, 1], the relative error against exp(-x) is at most
 * 2^-23 (1 + y) where exp(-x) > 1e-37, and the recipe is not monotone in the last bit.
 * A segment that ends NONE attenuates nothing; a ray with a non-finite component or a channel at or above nchan keeps
 * its weight.  A weight may reach 0: such a ray is traced on like any other.  out_rays, out_status, out_segments,
 * out_bounces, out_opl and out_glass never depend on the two tables, and with both NULL or zero every output is
 * bzr_trace_chain_media's bit for bit, in every mode and on every pipeline (the select on a > 0 keeps 0 x inf out of
 * the weight). */
bzr_status bzr_trace_chain_absorb(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                  const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                  uint32_t nlens, uint32_t nchan, const float *rays_soa, const uint8_t *channel,
                                  const float *weight_in, const float *opl_in, uint32_t n, uint32_t max_bounces,
                                  float *out_rays_soa, float *out_weight, uint32_t *out_status, uint32_t *out_segments,
                                  uint32_t *out_bounces, float *out_opl, float *out_glass, uint32_t flags);
/* ---- Fresnel ghost reflections: the roulette at glass exits ----
 * bzr_trace_chain_absorb plus two arguments behind max_bounces: ghost_seed, and first_ray -- ray i of the call has the
 * 64-bit ray number j = first_ray + i (mod 2^64).  Everything is bzr_trace_chain_absorb's except the following.
 * The draw happens in a segment expected OUTSIDE, for a ray whose channel is in the table, whose winning hit is an
 * intersection with cs >= 0 and s2 = eta^2 (1 - cs^2) < 0.99 -- exactly the rays Snell's step refracts out of the
 * glass -- and that has made k < max_bounces reflections in this lens l so far:
 *   T = fresnel_t(eta, cs, s2), the value the absorbing chain multiplies in (exact binary32 in both modes);
 *   u = G(ghost_seed, j, e) with e = 16 l + k (l <= 7, k <= 7);
 *   u >= T: the ray reflects -- the mirror step of a total reflection bit for bit (k2 = 2 cs, r = d - n k2 per
 *           component, normalised, origin at the hit's point); out_bounces goes up, the ray meets the same lens again
 *           expected OUTSIDE, and its weight gets the leg's attenuation A alone, like a total reflection;
 *   u <  T: the ray refracts as before, but its weight gets A alone: T is not multiplied in, the roulette already took
 *           the 1 - T share.
 * With k == max_bounces (the budget spent) there is no draw: the ray refracts with w = (w A) T as in
 * bzr_trace_chain_absorb, so no ray leaves a lens pending, and max_bounces = 0 is bzr_trace_chain_absorb bit for bit on
 * every pipeline and under BZR_MODE_FAST.  s2 >= 1 (total reflection), 0.99 <= s2 < 1, a NaN and a hit on the wrong
 * side are unchanged.  A segment expected INSIDE is unchanged: w = (w A) T, a front surface never reflects.  The
 * optical path and glass legs are unchanged; a reflected leg is a glass leg, as for a total reflection.
 * The uniform, in 64-bit unsigned arithmetic mod 2^64, mix64 being the splitmix64 finaliser
 * (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31):
 *   r = mix64((ghost_seed ^ 0x5851F42D4C957F2D) + 0x9E3779B97F4A7C15 * (j + 1))
 *   h = mix64(r + 0x9E3779B97F4A7C15 * (e + 1))
 *   u = (h >> 40) / 2^24        (a 24-bit uniform in [0, 1), exact in binary32)
 * The xor keeps it off the emitter's stream.  A ray's draws depend on nothing but (ghost_seed, j, l, k): the results do
 * not depend on the pipeline, the chunking, the batching or on which other rays are in the call -- a call over all rays
 * at first_ray = F equals the calls over [0, m) at F and [m, n) at F + m bit for bit.  The estimator is unbiased: the
 * expected weight of the rays that leave with no reflection is bzr_trace_chain_absorb's, and the reflected share now
 * travels on as rays instead of vanishing.  The argument checks are bzr_trace_chain_absorb's. */
bzr_status bzr_trace_chain_ghost(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                 const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                 uint32_t nlens, uint32_t nchan, const float *rays_soa, const uint8_t *channel,
                                 const float *weight_in, const float *opl_in, uint32_t n, uint32_t max_bounces,
                                 uint64_t ghost_seed, uint64_t first_ray,
                                 float *out_rays_soa, float *out_weight, uint32_t *out_status, uint32_t *out_segments,
                                 uint32_t *out_bounces, float *out_opl, float *out_glass, uint32_t flags);
/* The draw's host twin (no context, no device): *u = G(seed, ray, 16 lens + reflections).  lens above 7 or reflections
 * above 8, or a NULL u, return BZR_ERR_INVALID_ARGUMENT with nothing written. */
bzr_status bzr_ghost_uniform(uint64_t seed, uint64_t ray, uint32_t lens, uint32_t reflections, float *u);
/* ---- the bidirectional chain: front-surface reflections and ghosts between lenses ----
 * bzr_trace_chain_ghost's arguments with `axis` behind first_ray: the chain's forward direction.  Only the sign of one
 * dot product with it is used.  A zero or non-finite axis returns BZR_ERR_INVALID_ARGUMENT before any output is touched.
 * Every other chain call sends a ray that leaves lens l to lens l + 1.  Here a ray goes to the neighbour that the
 * surface it left faces, the roulette runs at every surface, and max_bounces (<= BZR_MAX_BOUNCES) is the ray's budget of
 * reflections for its whole path, not per lens.
 * Per-ray state: g in [0, nlens], the gap the ray is in (gap g is gap_table[g], in front of lens g); fwd: a ray in the
 * open heads for lens g when fwd, else for lens g - 1; k, the reflections so far on the whole path; q, the segments so
 * far.  Start: g = 0, fwd, k = q = 0.  c is the ray's channel; a channel outside the table ends the ray NONE in its
 * first segment, as before.  The walk is a loop over events:
 *   fwd && g == nlens: the ray ends, status BZR_RR_OUTSIDE.   !fwd && g == 0: it ends, status BZR_RR_BACK (4).
 *   Open segment.  Lens l = fwd ? g : g - 1, expected INSIDE; eta = gap_table[g][c] / ri_table[l][c], one correctly
 *     rounded division; q += 1.  The step applies where the winning hit is an intersection with cs < 0;
 *     s2 = eta^2 (1 - cs^2).
 *       s2 >= 1 with k < max_bounces: the mirror step of bzr_trace_chain_tir bit for bit (k2 = 2 cs, r = d - n k2 per
 *         component, normalised, origin at the hit's point); k += 1, fwd = !fwd, the weight gets the leg's A alone.
 *         With the budget spent the ray ends NONE.
 *       0.99 <= s2 < 1, a NaN, a miss, a hit with cs >= 0: NONE, as in every chain.
 *       s2 < 0.99 with k < max_bounces: T = fresnel_t(eta, cs, s2), u = G(ghost_seed, j, 256 + q - 1), G being
 *         bzr_trace_chain_ghost's function (the offset 256 keeps these draws off that call's e <= 135).
 *         u >= T: mirrored as above, k += 1, fwd = !fwd, w = w A.   u < T: refracted into lens l, w = w A (no T).
 *       s2 < 0.99 with the budget spent: refracted in with w = (w A) T, bzr_trace_chain_absorb's step.
 *     The leg lies in gap g: m = gap_table[g][c] len goes into out_opl, and A comes from gap_absorb[g][c].  Every such
 *     leg has g <= nlens - 1, so gap_absorb needs no row of its own for the space behind the last lens: a ray is in gap
 *     nlens only after it left lens nlens - 1 through a surface that faces forward, which sets fwd, and such a ray ends
 *     OUTSIDE before its next segment; a reflection in the open flips fwd but keeps g, and happens only in a gap with
 *     an open segment.
 *   Glass segment.  The ray is inside lens l, expected OUTSIDE; q += 1.  The step applies on an intersection with
 *     cs >= 0.  The side rule: back = n0 a0 + (n1 a1 + n2 a2) >= 0 with n the hit's normal and a the axis, in binary32
 *     without contraction (exact under BZR_MODE_FAST too); g' = back ? l + 1 : l.  eta = ri_table[l][c] /
 *     gap_table[g'][c]: the medium behind the surface the ray actually meets decides eta, s2, total reflection and T.
 *       s2 >= 1 with k < max_bounces: total reflection; the ray stays in lens l, k += 1, w = w A.
 *       s2 < 0.99 with k < max_bounces: the roulette of bzr_trace_chain_ghost with the draw G(ghost_seed, j, 256 + q - 1):
 *         u >= T reflects (k += 1, w = w A, the same lens again), u < T refracts out with w = w A.
 *       s2 < 0.99 with the budget spent: refracted out with w = (w A) T.   Everything else: NONE.
 *     After refracting out g = g', fwd = back.  The leg is a glass leg: len into out_glass, ri_table[l][c] len into
 *     out_opl, A from glass_absorb[l][c].
 * Outputs: out_status is NONE, OUTSIDE or BACK; out_rays_soa the ray after its last successful refraction or reflection
 * (the input ray if there was none); out_segments = q, out_bounces = k, out_opl and out_glass as the legs define them.
 * Termination: between two reflections a ray crosses each surface of the chain at most once in one direction, at most
 * 2 nlens segments, and one more ends in the reflection or the end; with at most max_bounces reflections
 * q <= (max_bounces + 1)(2 nlens + 1), 153 at the most.
 * Consequences.  A ray that ends with k < max_bounces under zero absorption tables has out_weight == weight_in bit for
 * bit: no step multiplied T in and every A was exactly 1.  A ray's results depend on nothing but its own inputs and
 * (ghost_seed, j): not on the pipeline, on the split of a call (first_ray moved along) or on which rays share its wave.
 * max_bounces = 0 is bzr_trace_chain_absorb bit for bit on every ray for which every surface it met from inside glass
 * faced forward (back true each time: the side rule then names the gap the forward chain assumes).
 * Limits.  The walk is ordered by neighbours: a ray that misses its neighbour lens is NONE even where a lens further
 * on would have met it; it is not a nearest-of-all-lenses search.  There is no staged pipeline: an explicit
 * BZR_PIPELINE_STAGED returns BZR_ERR_INVALID_ARGUMENT, the automatic choice is fused, BZR_ACCEL_NONE is the brute-force
 * scan.  The other argument checks are bzr_trace_chain_ghost's. */
bzr_status bzr_trace_chain_bidir(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                 const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                 uint32_t nlens, uint32_t nchan, const float *rays_soa, const uint8_t *channel,
                                 const float *weight_in, const float *opl_in, uint32_t n, uint32_t max_bounces,
                                 uint64_t ghost_seed, uint64_t first_ray, const float axis[3],
                                 float *out_rays_soa, float *out_weight, uint32_t *out_status, uint32_t *out_segments,
                                 uint32_t *out_bounces, float *out_opl, float *out_glass, uint32_t flags);
/* The walk's draw on the host (no context, no device): *u = G(seed, ray, 256 + segment), segment = q - 1 counting from
 * 0.  A segment above the bound (BZR_MAX_BOUNCES + 1)(2 * 8 + 1) = 153, or a NULL u, return BZR_ERR_INVALID_ARGUMENT
 * with nothing written. */
bzr_status bzr_bidir_uniform(uint64_t seed, uint64_t ray, uint32_t segment, float *u);
/* ---- surface coatings: tabulated reflectance in the bidirectional chain ----
 * Every surface above is bare glass: T = fresnel_t(eta, cs, s2).  A coating replaces that T, per surface and per
 * channel, by a table of the unpolarised power reflectance R against the cosine of incidence.
 * Surface numbering.  A surface is (l, side), side = back ? 1 : 0, where back is bzr_trace_chain_bidir's side rule
 * applied to the winning hit's normal n: n0 a0 + (n1 a1 + n2 a2) >= 0.  Here it is evaluated in open segments too, not
 * only in glass segments.  In both kinds of segment the normal of a hit that the step accepts points out of the glass,
 * so the rule names the same physical surface from either side: side 0 is the front of lens l, side 1 its back.
 * The row.  table[2 l + side][c][i] is R of that surface for channel c at the gap-side cosine mu_i = i / 128: the cosine
 * of the ray's angle to the normal in the medium outside the glass.  For a lossless stack R is the same from both sides
 * at Snell-linked angles, so one row serves both directions; the gap-side cosine is the smooth parametrisation (the
 * glass-side one has a square-root singularity at the critical angle).
 * The step.  On a surface whose mask bit is set, in an open segment whose winning hit has cs < 0 or a glass segment
 * whose hit has cs >= 0, with s2 < 0.99, T = coat_t(row, mu) stands where T = fresnel_t(eta, cs, s2) stood:
 *   mu = open segment ? |cs| : sqrt_rn(1 - s2)        (the c2 Snell's step has; s2 = eta eta (1 - cs cs))
 *   mu = min(mu, 1.0f)
 *   x  = mu * 128.0f                                   (exact)
 *   i  = min((int)x, 127)       f = x - (float)i       (exact)
 *   d  = row[i + 1] - row[i]    p = f * d              R = row[i] + p
 *   T  = 1.0f - R
 * in IEEE binary32 without contraction, exact under BZR_MODE_FAST too: it belongs to the chain step like fresnel_t.
 * With every entry in [0, 1], R and T stay in [0, 1] without a clamp: row[i] + fl(f d) lies between the two entries up
 * to one rounding, and 0 and 1 are representable.  T is used exactly where bzr_trace_chain_bidir uses it: as the
 * roulette's threshold (u >= T mirrors, u < T refracts with w = w A) and in the budget-spent step w = (w A) T.
 * Unchanged on every surface: total reflection (s2 >= 1) and the band 0.99 <= s2 < 1; the draw
 * G(ghost_seed, j, 256 + q - 1); the mirror step, the legs, A, the states and the termination bound.
 * Mask and validation.  A surface whose mask bit is clear uses fresnel_t exactly as before; rows of unmasked surfaces
 * are neither read nor validated.  With coat == NULL or mask == 0 every output is bzr_trace_chain_bidir's bit for bit,
 * in both modes, fused and on the brute-force scan.  A mask bit at or above 2 nlens, a non-zero mask with a NULL table,
 * an entry of a masked row that is not finite or lies outside [0, 1], and an explicit BZR_PIPELINE_STAGED return
 * BZR_ERR_INVALID_ARGUMENT before any output is touched.
 * Consequences.  A row of zeros is a perfect anti-reflection coating: no draw ever mirrors there, and the budget-spent
 * step keeps the weight.  A row of ones is a mirror: a ray with budget left always reflects there, and a ray whose
 * budget is spent refracts with weight exactly 0.
 * Out of scope: a coating that absorbs (R + T < 1: metals, absorbing filters), polarisation, and the coating's phase
 * in out_opl. */
#define BZR_COAT_SAMPLES 129
typedef struct bzr_coating {
  const float *table;   /* [2 nlens][nchan][BZR_COAT_SAMPLES], row-major float32, host memory like ri_table */
  uint32_t mask;        /* bit 2 l + side: surface (l, side) is coated; side 0 = front, 1 = back */
} bzr_coating;
/* bzr_trace_chain_bidir's arguments with `coat` behind axis (NULL: no surface is coated).  Fused, or BZR_ACCEL_NONE for
 * the brute-force scan; at max_bounces = 0 it is the plain coated forward chain. */
bzr_status bzr_trace_chain_coated(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                  const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                  uint32_t nlens, uint32_t nchan, const float *rays_soa, const uint8_t *channel,
                                  const float *weight_in, const float *opl_in, uint32_t n, uint32_t max_bounces,
                                  uint64_t ghost_seed, uint64_t first_ray, const float axis[3], const bzr_coating *coat,
                                  float *out_rays_soa, float *out_weight, uint32_t *out_status, uint32_t *out_segments,
                                  uint32_t *out_bounces, float *out_opl, float *out_glass, uint32_t flags);
/* The lookup's host twin (no context, no device), compiled from the text the kernels compile: *t = coat_t(row, mu).
 * A NULL pointer or a mu that is not >= 0 returns BZR_ERR_INVALID_ARGUMENT with nothing written. */
bzr_status bzr_coat_transmittance(const float row[BZR_COAT_SAMPLES], float mu, float *t);
/* One row on the host (no context, no device): the unpolarised reflectance (R_s + R_p) / 2 of a lossless dielectric
 * stack between a gap of index n_gap and glass of index n_glass by the characteristic-matrix method, evaluated in
 * binary64 at mu_i = i / 128 and rounded once to float.  Layers are listed from the gap side to the glass, thicknesses
 * and the wavelength in micrometres; nlayers = 0 is the bare Fresnel surface.  Cosines are complex: an evanescent
 * layer frustrates the reflection (however thick: its matrix is scaled, so cosh and sinh do not overflow, and R tends
 * to 1), a layer exactly at its critical angle takes its matrix's limit, and glass at or beyond its critical angle
 * gives R = 1 exactly.  out_row[0] = 1 by
 * definition (mu = 0 divides by zero in p).  Indices or thicknesses that are not finite and positive, a wavelength
 * that is not, nlayers above 8 and NULL pointers return BZR_ERR_INVALID_ARGUMENT with out_row untouched. */
bzr_status bzr_coating_reflectance(double n_gap, double n_glass, const double *layer_index,
                                   const double *layer_thickness_um, uint32_t nlayers, double wavelength_um,
                                   float out_row[BZR_COAT_SAMPLES]);
/* Absorption coefficients from a glass catalogue's internal transmittance, on the host (no context, no device):
 * out_a[i] = -ln(internal_transmittance[i]) / thickness, evaluated in binary64 and rounded once to float, per unit of
 * the length `thickness` is given in.  A transmittance outside (0, 1], a thickness that is not finite and positive or
 * a result that is not finite return BZR_ERR_INVALID_ARGUMENT with nothing written. */
bzr_status bzr_absorption_from_transmittance(const double *internal_transmittance, uint32_t n, double thickness,
                                             float *out_a);
/* Refractive index from a dispersion formula, on the host (no context, no device): evaluated in binary64 and
 * rounded once to float.  wavelength_um [n] in micrometres, out_ri [n].
 *   BZR_DISPERSION_CAUCHY     n = A + B / l^2 + C / l^4           coeff = A, B[, C]             ncoeff 2 or 3
 *   BZR_DISPERSION_SELLMEIER  n^2 = 1 + sum_k B_k l^2 / (l^2 - C_k)   coeff = B1, C1, B2, C2, ...  ncoeff 2, 4 or 6
 * An unknown model, another ncoeff, a wavelength that is not finite and positive, a result that is not finite or a
 * Sellmeier n^2 that is not positive return BZR_ERR_INVALID_ARGUMENT with nothing written. */
enum { BZR_DISPERSION_CAUCHY = 0, BZR_DISPERSION_SELLMEIER = 1 };
bzr_status bzr_dispersion_index(int32_t model, const double *coeff, uint32_t ncoeff, const double *wavelength_um,
                                uint32_t n, float *out_ri);
/* Multi-GPU refraction chain in ONE process (C/C++ hosts without torch.distributed):
 * image-plane tiles are dealt round-robin to the contexts, one per device.  Tile k is the rays
 * [k * tile_rays, (k + 1) * tile_rays) of the SoA input (callers order rays tile-major, e.g. 64x64-pixel
 * tiles of 4096 rays); context d traces tiles d, d + nctx, ... through its own copy of the lenses,
 * lenses[d * nlens + l] living on ctxs[d]'s device, and the results are gathered to ctxs[0]'s device on
 * the device side (RCCL when the contexts' devices are distinct, peer copies otherwise) and land in the
 * outputs in input order (same bits as one bzr_trace_chain over all rays).  A one-frame bzr_tiled plan
 * (below) created and destroyed per call: host pointers, or with BZR_DEVICE_PTRS rays and outputs on
 * ctxs[0]'s device.  Synchronous either way; the mode / pipeline flags pass through.  Callers tracing
 * many frames keep a plan instead (the RCCL communicator and the buffers are set up once). */
bzr_status bzr_trace_tiled(bzr_ctx *const *ctxs, uint32_t nctx, const bzr_mesh *const *lenses,
                           const float *refractive_index, uint32_t nlens, const float *rays_soa, uint32_t n,
                           uint32_t tile_rays, float *out_rays_soa, uint32_t *out_status,
                           uint32_t *out_segments, uint32_t flags);

/* ---- multi-GPU frames from one process, gathered on the device (one host thread drives
 * every device, ncclCommInitAll, grouped ncclSend / ncclRecv to device 0) ---- */
typedef struct bzr_tiled bzr_tiled;
enum { BZR_GATHER_AUTO = 0, BZR_GATHER_RCCL = 1, BZR_GATHER_PEER = 2, BZR_GATHER_DIRECT = 3 };
/* A frame plan over ndev devices and nslot frame slots: ctxs[s * ndev + d] is slot s's context on list
 * device d (every slot lists the same devices in the same order; all contexts distinct).  The frame is n
 * rays in tile-major order; device d traces tiles d, d + ndev, ... (its share).  The plan owns each
 * device's share buffers per slot and device 0's receive buffers.  transport: BZR_GATHER_RCCL (one RCCL
 * communicator per device, ncclCommInitAll; needs distinct devices), BZR_GATHER_PEER (hipMemcpyPeerAsync;
 * any device list, including several list entries on one device), BZR_GATHER_DIRECT (ndev == 1 only: the
 * one device traces straight into the caller's outputs -- no pack, no gather, no unpack, no share
 * buffers), BZR_GATHER_AUTO (DIRECT for one device, RCCL when several devices are distinct, PEER
 * otherwise).  Not thread-safe; the contexts must not be used by other threads meanwhile. */
bzr_status bzr_tiled_create(bzr_ctx *const *ctxs, uint32_t ndev, uint32_t nslot, uint32_t n, uint32_t tile_rays,
                            int32_t transport, bzr_tiled **out);
bzr_status bzr_tiled_destroy(bzr_tiled *plan);
/* transport chosen; share_rays[ndev] (may be NULL): rays per device; npad (may be NULL): columns of a
 * packed share (the largest share, in whole tiles) -- each device sends 28 * npad bytes per frame. */
bzr_status bzr_tiled_info(const bzr_tiled *plan, int32_t *transport, uint32_t *share_rays, uint32_t *npad);
/* The frame's input rays [6][n] (host memory, or with BZR_DEVICE_PTRS ctxs[0]'s device memory) into every
 * device's share.  Waits for the frames in flight first (they read the previous rays).  The frame lands on
 * device 0 once (host: one H2D copy, then the call waits for it so the host buffer may be reused; device:
 * one D2D copy, which must find the source complete and unchanged until bzr_tiled_sync); device 0 extracts
 * each device's share and sends it there (one peer copy per other device, (ndev - 1) / ndev of the frame
 * in all), queued on ctxs[0]'s stream and ordered before the next bzr_tiled_trace without a host wait.
 * With one device the frame is the share: one copy, nothing extracted.  The rays stay resident for every
 * following frame.  BZR_RAYS_AOS: the rays are [n][6] records, transposed on device 0 after the copy. */
bzr_status bzr_tiled_set_rays(bzr_tiled *plan, const float *rays_soa, uint32_t flags);
/* Device d's share input [6][share_rays[d]] (device memory on device d), for callers that generate rays
 * on the devices: write it (ordered before the next bzr_tiled_trace, e.g. then bzr_tiled_sync). */
bzr_status bzr_tiled_share_rays(bzr_tiled *plan, uint32_t device_index, float **rays_soa);
/* One frame on slot (frame number mod nslot): every device traces its share through
 * lenses[d * nlens + l] (refract(INSIDE) then refract(OUTSIDE) per lens, as bzr_trace_chain), packs it
 * (28 B per ray), the packed shares are gathered to device 0, which writes out_rays_soa [6][n],
 * out_status [n] and out_segments [n] (may be NULL) in input order.  BZR_DEVICE_PTRS: outputs on ctxs[0]'s
 * device; the call returns once the frame is queued (no host wait), frames on different slots overlap,
 * and the outputs are ready on bzr_tiled_stream's stream (or after bzr_tiled_sync) -- keep one set of
 * outputs per frame in flight.  Host pointers: synchronous, and a compact frame with more survivors than
 * the capacity returns BZR_ERR_CAPACITY at once.  Mode / pipeline flags pass through.  BZR_RAYS_AOS: out_rays
 * as [n][6] records (device 0 transposes the frame's rays on the stream that produced them, 48 B per ray). */
bzr_status bzr_tiled_trace(bzr_tiled *plan, const bzr_mesh *const *lenses, const float *refractive_index,
                           uint32_t nlens, float *out_rays_soa, uint32_t *out_status, uint32_t *out_segments,
                           uint32_t flags);
/* Device 0's gather stream: the outputs of the last bzr_tiled_trace are complete in its order. */
bzr_status bzr_tiled_stream(bzr_tiled *plan, void **hip_stream);
/* Waits for every frame queued; returns BZR_ERR_CAPACITY if a compact frame since the last sync had more
 * survivors than the capacity (that frame's outputs are incomplete). */
bzr_status bzr_tiled_sync(bzr_tiled *plan);
/* What each device sends per frame (bzr_pack_frame's layouts): BZR_PACK_RAYS (default; 28 B per ray of the
 * share, npad columns) or BZR_PACK_COMPACT: one status/segment byte per ray, the survivor count and the
 * final rays of at most `cap` survivors (the rays that refracted at least once; 0 < cap <= npad) -- device
 * 0 returns the others' primary rays from its copy of the frame, so the compact layout needs
 * bzr_tiled_set_rays.  Synchronises first.  A BZR_GATHER_DIRECT plan gathers nothing: it keeps the layout,
 * which has no effect on its frames. */
bzr_status bzr_tiled_set_layout(bzr_tiled *plan, int32_t layout, uint32_t cap);
/* Traces one frame (rays layout, synchronous), counts each device's survivors and switches to the compact
 * layout with cap = the largest count + 1/64 + 64 (at most npad); cap_out (may be NULL) gets it. */
bzr_status bzr_tiled_calibrate(bzr_tiled *plan, const bzr_mesh *const *lenses, const float *refractive_index,
                               uint32_t nlens, uint32_t flags, uint32_t *cap_out);
/* BezierMesh::interpolate(divisor) on the device (reference/bezierMesh.cpp:55-66): the tessellated
 * surface, divisor^2 sub-triangles of every patch, in the reference's order (sub-triangle outer,
 * patch inner).  out_xyz: divisor^2 * n_patches triangles x 3 vertices x 3 floats.  divisor >= 1.
 * Bit-identical to the host bzr_bezier_interpolate of the same patches. */
bzr_status bzr_mesh_interpolate(bzr_ctx *ctx, const bzr_mesh *mesh, int32_t divisor, float *out_xyz,
                                uint32_t flags);

/* ---- illumination: emitter -> lens chain -> target plane (reference README.md:159-194) ---- */
/* A rectangular emitter (origin + a*edge_u + b*edge_v, a, b in [0,1)) divided into parts_u x
 * parts_v parts; rays are numbered part by part, points_per_part points per part, rays_per_point
 * rays per point.  Directions are uniform over the hemisphere around +x, sampled as
 * UniformHemisphere::getRandom does (reference/hostUtil.cpp:16-29: cos(incidence) uniform in
 * [0,1), turn uniform in [0, 2*pi)) from a counter-based generator (splitmix64 of seed and ray
 * index), so any ray range can be generated independently; `belts` sets the hemisphere patch
 * numbering of UniformHemisphere(belts) (reference/hostUtil.cpp:3-14).
 *
 * Ray j (a 64-bit ray number, j = first + i in bzr_emit) in full, so that a caller can restate it on the host; the
 * device evaluates the real-valued steps in binary32, a restatement agrees with it to rounding:
 *   uniforms   U(key, stream) is a pair (u, v) of 24-bit uniforms in [0, 1).  With 64-bit unsigned arithmetic (mod 2^64)
 *                z = seed + 0x9E3779B97F4A7C15 * (2 * key + stream + 1)
 *                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  h = z ^ (z >> 31)
 *              (the splitmix64 finaliser), u = (h >> 40) / 2^24 (bits 40..63) and v = ((h >> 16) & 0xFFFFFF) / 2^24
 *              (bits 16..39).
 *   direction  (ci, tf) = U(j, 0): ci the cosine of the incidence, tf the turn as a fraction of a full turn.  With
 *              si = sqrt(1 - ci^2) the direction is (ci, si cos(2 pi tf), si sin(2 pi tf)), normalised.
 *   origin     the point number is j / rays_per_point (integer division) and (u, v) = U(point number, 1): all the
 *              rays of a point share one origin.  The part is (j / (points_per_part * rays_per_point)) mod
 *              (parts_u * parts_v), u fastest: pu = part mod parts_u, pv = part / parts_u.  Then a = (pu + u) / parts_u,
 *              b = (pv + v) / parts_v and the origin is origin + a * edge_u + b * edge_v.
 *   patch      belts is in 1..4096 (anything else: BZR_ERR_INVALID_ARGUMENT before anything is allocated or written).
 *              Belt i (0 <= i < belts) spans the incidences [i, i + 1) * (pi / 2) / belts and holds
 *              count[i] = ceil(4 * belts * sin((2 i + 1) pi / (4 * belts))) patches of equal turn width, numbered from
 *              first[i] = count[0] + ... + count[i - 1].  (As the reference evaluates it: the sine's argument is the
 *              binary32 value of (2 i + 1) / (4 belts) * pi, each of its steps rounded to binary32, the sine and the
 *              product are binary64.  A binary64 argument gives another count where the product lies within rounding
 *              of an integer: for one belt of 4096.)  The ray's belt is the one its incidence acos(ci) lies in
 *              (the last one at ci = 0), its patch number first[belt] + min(floor(tf * count[belt]), count[belt] - 1).
 *              A ray within rounding of a belt's or a patch's edge may be numbered on either side of it. */
typedef struct bzr_emitter {
  float origin[3], edge_u[3], edge_v[3];
  uint32_t parts_u, parts_v, points_per_part, rays_per_point, belts;
  uint64_t seed;
} bzr_emitter;
/* The illuminated rectangle: origin + a*axis_u + b*axis_v (unit, orthogonal axes), a in
 * [0, size_u), b in [0, size_v), bins_u x bins_v counting cells (row-major, u fastest).  A ray that
 * leaves the last lens (status OUTSIDE) lands where Plane::intersect (reference/3dGeomUtil.h:279-296)
 * meets the plane through origin with normal axis_u x axis_v.
 *
 * The cell rule: with n = axis_u x axis_v normalised, a ray (start s, direction d) meets the plane when
 * |d . n| >= 1e-5 and t = (n . origin - n . s) / (d . n) > 0, at p = s + t d.  Its coordinates are
 * a = (p - origin) . axis_u and b = (p - origin) . axis_v; it lands when 0 <= a < size_u and 0 <= b < size_v, in cell
 * iu = min(floor(a / cell_u), bins_u - 1), iv = min(floor(b / cell_v), bins_v - 1) with cell_u = size_u / bins_u and
 * cell_v = size_v / bins_v, and is counted in hist[iv][iu] (index iv * bins_u + iu).  All in binary32: a ray within
 * rounding of a cell's or the target's edge may fall on either side of it. */
typedef struct bzr_target {
  float origin[3], axis_u[3], axis_v[3];
  float size_u, size_v;
  uint32_t bins_u, bins_v;
} bzr_target;
enum { BZR_ILLUM_EMITTED = 0, BZR_ILLUM_CULLED = 1, BZR_ILLUM_EXITED = 2, BZR_ILLUM_LANDED = 3 };
/* Rays first .. first+n-1 of the emitter: rays_soa [6][n] (unit directions), hemisphere patch
 * index per ray (may be NULL). */
bzr_status bzr_emit(bzr_ctx *ctx, const bzr_emitter *em, uint64_t first, uint32_t n, float *rays_soa,
                    uint32_t *patch_index, uint32_t flags);
/* Emits `total_rays` rays, drops those that miss the first lens's bounding sphere (Ritter's sphere
 * over the gate-region boxes: a ray that misses it cannot pass any planar gate, so dropping it is
 * exact), traces the rest through the refraction chain and adds one count per landed ray to
 * hist[bins_v][bins_u] (accumulates: zero it first).  stats (may be NULL) gets the BZR_ILLUM_*
 * counts.  Synchronous; hist may be host or device memory per `flags`. */
bzr_status bzr_illuminate(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *refractive_index,
                          uint32_t nlens, const bzr_emitter *em, uint64_t total_rays, const bzr_target *target,
                          uint32_t *hist, uint64_t stats[4], uint32_t flags);
/* Radiometry of bzr_illuminate_power: each ray's initial power w0 and what a lens surface transmits. */
enum { BZR_EMISSION_UNIFORM = 0, BZR_EMISSION_LAMBERT = 1 };   /* w0 = 1  |  w0 = direction . (+x) = dx */
enum { BZR_SURFACE_LOSSLESS = 0, BZR_SURFACE_FRESNEL = 1 };    /* T = 1   |  T of bzr_trace_chain_power */
typedef struct bzr_radiometry { uint32_t emission, surface; } bzr_radiometry;
/* bzr_illuminate (same emitter stream, sphere cull, batching and pipelines) with ray power.  Power is summed as
 * unsigned 64-bit fixed point with 32 fraction bits, q(w) = (uint64) trunc(w x 2^32) for w in [0, 1]: integer sums
 * do not depend on the order of arrival, so every output is bit-reproducible.  Each landed ray adds q(w) to its
 * cell of flux_q32[bins_v][bins_u] (accumulates: zero it first) and, when hist is not NULL, one count to hist as
 * bzr_illuminate does.  stats (may be NULL): the BZR_ILLUM_* counts.  power_q32 (may be NULL), same fixed point:
 * [EMITTED] the sum of q(w0) over every emitted ray, [CULLED] over the culled ones, [EXITED] and [LANDED] the sums
 * of q(w).  total_rays >= 2^32 (the 64-bit sums could overflow), an unknown emission or surface, or a NULL rad or
 * flux_q32 return BZR_ERR_INVALID_ARGUMENT before any output is touched.  Synchronous; flux_q32 and hist are
 * host or device memory per `flags`. */
bzr_status bzr_illuminate_power(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *refractive_index,
                                uint32_t nlens, const bzr_emitter *em, uint64_t total_rays, const bzr_target *target,
                                const bzr_radiometry *rad, uint64_t *flux_q32, uint32_t *hist, uint64_t stats[4],
                                uint64_t power_q32[4], uint32_t flags);
/* bzr_illuminate_power per spectral channel: the same emitter stream, sphere cull, batching rule, 32.32 fixed point
 * and accumulation into the outputs, with global ray i (the emitter's 64-bit ray number) in channel i mod nchan and
 * refracted with ri_table[l][i mod nchan].  Kept per channel: flux_q32 [nchan][bins_v][bins_u], hist (may be NULL)
 * of the same shape, stats [nchan][4] and power_q32 [nchan][4] (each may be NULL).  Summed over the channels, the
 * EMITTED and CULLED counts and power sums do not depend on the table and equal bzr_illuminate_power's for the same
 * emitter (the cull happens before the first refraction).  rad->surface == BZR_SURFACE_LOSSLESS keeps the weights
 * as emitted; the rays still refract with their channel's index.  No source spectrum is taken: the maps are linear
 * in it, so a caller scales channel c's map by the source's power in that channel on the host.  The argument checks
 * are bzr_illuminate_power's, plus nchan in 1..BZR_MAX_CHANNELS and a non-NULL ri_table. */
bzr_status bzr_illuminate_spectral(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table, uint32_t nlens,
                                   uint32_t nchan, const bzr_emitter *em, uint64_t total_rays, const bzr_target *target,
                                   const bzr_radiometry *rad, uint64_t *flux_q32, uint32_t *hist, uint64_t *stats,
                                   uint64_t *power_q32, uint32_t flags);
/* bzr_illuminate_spectral with the chain of bzr_trace_chain_tir: the same emitter stream (global ray i in channel
 * i mod nchan), sphere cull, batching rule, 32.32 fixed point, accumulation into the maps and flags; every traced ray
 * goes through the refraction chain with up to max_bounces reflections per lens, exactly as bzr_trace_chain_tir
 * traces it (a reflection leaves the weight untouched; rad->surface == BZR_SURFACE_LOSSLESS keeps the weights as
 * emitted).  flux_q32, hist, stats [nchan][4] and power_q32 [nchan][4] are bzr_illuminate_spectral's, now including
 * the rays that reflected.
 *   reflected_flux_q32, reflected_hist  [nchan][bins_v][bins_u], each may be NULL, host or device memory per `flags`
 *     like flux_q32, accumulating: the part of flux_q32 / hist that comes from landed rays with at least one
 *     reflection -- the stray-light map.
 *   ledger_count, ledger_power_q32  [nchan][BZR_LEDGER_ROWS][BZR_LEDGER_FIELDS], host memory always, each may be
 *     NULL, overwritten like stats: where the power went.  Every traced ray (not culled: at least one segment) of
 *     channel c is counted once in row min(bounces, BZR_MAX_BOUNCES), bounces being bzr_trace_chain_tir's out_bounces
 *     (summed over the lenses): under LOST if it ended NONE, under EXITED if it ended OUTSIDE, and under LANDED as
 *     well if it meets the target.  The power entries add q(w) of the weight the ray ended with.  Culled rays are in
 *     no row.
 * By construction, per channel c (sums over the rows r):
 *   sum_r EXITED = stats[c][EXITED]     sum_r LANDED = stats[c][LANDED]     (and the power sums against power_q32[c])
 *   sum_r (LOST + EXITED) = stats[c][EMITTED] - stats[c][CULLED]: every traced ray is in exactly one of the two.
 *     The ledger's power is what the rays ended with, power_q32[c][EMITTED] what they started with, so the power form
 *     of this line holds where no surface takes power (BZR_SURFACE_LOSSLESS); with Fresnel surfaces the difference
 *     is what the refractions reflected away.
 *   sum_{r >= 1} LANDED power = the sum over the cells of what this call added to reflected_flux_q32[c]
 * With max_bounces = 0, flux_q32, hist, stats and power_q32 are bzr_illuminate_spectral's bit for bit, the reflected
 * maps get nothing added and only ledger row 0 is non-zero.  max_bounces above BZR_MAX_BOUNCES, and every argument
 * bzr_illuminate_spectral rejects, return BZR_ERR_INVALID_ARGUMENT before any output is touched. */
enum { BZR_LEDGER_LOST = 0, BZR_LEDGER_EXITED = 1, BZR_LEDGER_LANDED = 2, BZR_LEDGER_FIELDS = 3 };
#define BZR_LEDGER_ROWS (BZR_MAX_BOUNCES + 1)
bzr_status bzr_illuminate_tir(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table, uint32_t nlens,
                              uint32_t nchan, const bzr_emitter *em, uint64_t total_rays, const bzr_target *target,
                              const bzr_radiometry *rad, uint32_t max_bounces,
                              uint64_t *flux_q32, uint32_t *hist,
                              uint64_t *reflected_flux_q32, uint32_t *reflected_hist,
                              uint64_t *stats, uint64_t *power_q32,
                              uint64_t *ledger_count, uint64_t *ledger_power_q32, uint32_t flags);
/* bzr_illuminate_tir over the chain of bzr_trace_chain_absorb: the same outputs with the same meanings, emitter stream,
 * sphere cull (geometric, unchanged), batching rule and flags.  gap_table [nlens + 1][nchan], glass_absorb and
 * gap_absorb [nlens][nchan] are that call's (host memory, each may be NULL: vacuum, all zero) and are checked as there.
 * The emitter sits in the medium gap_table[0]: the leg from the emitter to the first lens is attenuated with
 * gap_absorb[0].  The leg from the last lens to the target is neither refracted again nor attenuated: row nlens of
 * gap_table is the medium the rays leave into and land in.  rad->surface == BZR_SURFACE_LOSSLESS takes the Fresnel
 * term out and leaves the absorption in.
 * The ledger's count identities all hold.  With absorption its power line changes: under BZR_SURFACE_LOSSLESS
 * sum_r (LOST + EXITED) power no longer equals power_q32[c][EMITTED] - power_q32[c][CULLED]; the difference is what
 * the media absorbed before the rays ended.
 * With gap_table of ones or NULL and both absorption tables zero or NULL every output is bzr_illuminate_tir's bit for
 * bit. */
bzr_status bzr_illuminate_media(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                const bzr_target *target, const bzr_radiometry *rad, uint32_t max_bounces,
                                uint64_t *flux_q32, uint32_t *hist,
                                uint64_t *reflected_flux_q32, uint32_t *reflected_hist,
                                uint64_t *stats, uint64_t *power_q32,
                                uint64_t *ledger_count, uint64_t *ledger_power_q32, uint32_t flags);
/* ---- far field: luminous intensity, power per steradian against direction ---- */
/* A direction frame and its map.  axis_u and axis_v are unit and orthogonal, as bzr_target's; the pole is
 * n = axis_u x axis_v, normalised on the host as the target's normal is.  Directions are mapped by the Lambert
 * azimuthal equal-area projection about the pole, rho = 2 sin(theta / 2): equal areas in (X, Y) are equal solid
 * angles.  The map is the square [-R, R)^2 with R = extent, 0 < R <= sqrt(2) as a float (bit pattern 0x3FB504F3 at
 * the most), in bins_u x bins_v cells (row-major, u fastest).  Its corners reach rho = 2 at the most, so every cell
 * is a whole cell of exactly (2R / bins_u)(2R / bins_v) steradians.  R = sqrt(2) holds the forward hemisphere in
 * the inscribed disc and backward directions in the corners.
 *
 * The cell rule, defined by its operations so that the device, bzr_farfield_cell and a numpy restatement agree bit
 * for bit: for a direction d (used as given, not normalised), in IEEE binary32 with one rounding per operation and
 * no contraction -- under BZR_MODE_FAST too -- and dot products in the order x0 y0 + (x1 y1 + x2 y2):
 *   mu = d . n    a = d . axis_u    b = d . axis_v
 *   g = 1 + mu;   h = 2 / g;   k = sqrt(h)                 (division and root correctly rounded)
 *   X = a k;   Y = b k;   u = X + R;   v = Y + R;   S = R + R
 *   binned  iff  g > 0 && u >= 0 && u < S && v >= 0 && v < S      (a NaN anywhere fails; so does mu = -1)
 *   cu = S / bins_u;   cv = S / bins_v                     (the bin counts converted to binary32)
 *   iu = min((uint32) (u / cu), bins_u - 1);   iv likewise;   cell = iv * bins_u + iu
 * A ray within rounding of a cell's or the map's edge may fall on either side of it. */
typedef struct bzr_farfield {
  float axis_u[3], axis_v[3];
  float extent;
  uint32_t bins_u, bins_v;
} bzr_farfield;
enum { BZR_FAR_SEEN = 0, BZR_FAR_BINNED = 1 };
/* Bins a traced batch by direction.  rays_soa [6][n] as bzr_trace_chain_* writes out_rays (rows 3..5 are read).
 * weight [n] (NULL: every ray 1.0f), status [n] (NULL: every ray is seen; otherwise only rays with status
 * BZR_RR_OUTSIDE are), channel [n] (NULL: channel 0; a ray with channel >= nchan is skipped) live in host or device
 * memory per `flags`, as the maps do.  far_flux_q32 and far_hist [nchan][bins_v][bins_u] accumulate (zero them
 * first); at least one is given.  A binned ray of channel c adds q(w), bzr_illuminate_power's fixed point, to its
 * cell of far_flux_q32[c] and one count to far_hist[c].  far_stats and far_power_q32 [nchan][2] (host memory
 * always, each may be NULL, overwritten): per channel the count and the sum of q(w) of the rays seen (BZR_FAR_SEEN)
 * and binned (BZR_FAR_BINNED).
 * Returns BZR_ERR_INVALID_ARGUMENT before any output is touched for: a NULL far, zero bins, nchan x cells >= 2^32,
 * an extent that is not finite or outside (0, sqrt(2)], nchan outside 1..BZR_MAX_CHANNELS, both maps NULL, unknown
 * flags and BZR_RAYS_AOS.  n = 0 returns BZR_OK and touches nothing.  Both pipeline flags and BZR_MODE_FAST are
 * accepted and change nothing.
 * Host pointers: synchronous, staged through the context's scratch like bzr_emit.  BZR_DEVICE_PTRS: asynchronous on
 * the context's stream, unless far_stats or far_power_q32 is given: the call then waits for them.
 * Lanes of a wave that hold the same (channel, cell) are summed before the atomic; integer sums are order-free, so
 * the maps' bits do not depend on it. */
bzr_status bzr_farfield_bin(bzr_ctx *ctx, const bzr_farfield *far, const float *rays_soa, const float *weight,
                            const uint32_t *status, const uint8_t *channel, uint32_t n, uint32_t nchan,
                            uint64_t *far_flux_q32, uint32_t *far_hist,
                            uint64_t *far_stats, uint64_t *far_power_q32, uint32_t flags);
/* bzr_illuminate_media with a far-field frame: every traced ray that ends OUTSIDE is binned as bzr_farfield_bin bins
 * it, with its final weight, into far_flux_q32 / far_hist [nchan][bins_v][bins_u] (at least one given; host or
 * device memory per `flags` like flux_q32; accumulating).  A ray with at least one reflection is also added to
 * far_reflected_flux_q32 (may be NULL): stray light and glare in angle.  far_stats and far_power_q32 [nchan][2]
 * (host memory, each may be NULL, overwritten): per channel, [BZR_FAR_SEEN] equals stats / power_q32
 * [c][BZR_ILLUM_EXITED].  target may be NULL: flux_q32, hist and the reflected maps must then be NULL, and the LANDED
 * entries of stats, power_q32 and the ledger are 0.  With a target every bzr_illuminate_media output is that call's
 * bit for bit.  The argument checks are bzr_illuminate_media's and bzr_farfield_bin's. */
bzr_status bzr_illuminate_farfield(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                   const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                   uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                   const bzr_target *target, const bzr_radiometry *rad, uint32_t max_bounces,
                                   uint64_t *flux_q32, uint32_t *hist,
                                   uint64_t *reflected_flux_q32, uint32_t *reflected_hist,
                                   uint64_t *stats, uint64_t *power_q32,
                                   uint64_t *ledger_count, uint64_t *ledger_power_q32, uint32_t flags,
                                   const bzr_farfield *far, uint64_t *far_flux_q32, uint32_t *far_hist,
                                   uint64_t *far_reflected_flux_q32, uint64_t *far_stats, uint64_t *far_power_q32);
/* bzr_illuminate_farfield over the chain of bzr_trace_chain_ghost: ghost_seed follows max_bounces, and ray j of the
 * emitter (its 64-bit ray number, whatever the batching) draws G(ghost_seed, j, e).  far may be NULL: the five far
 * outputs must then be NULL and the call is bzr_illuminate_media with the roulette; at least one of target and far is
 * given.  Ghost rays arrive where reflected rays do: in the reflected maps, far_reflected_flux_q32 and ledger rows >= 1.
 * With rad->surface == BZR_SURFACE_LOSSLESS (no draw is taken) or max_bounces = 0 every output is
 * bzr_illuminate_farfield's bit for bit.
 * The ledger's count identities hold.  Its power line: at a drawn exit nothing is lost -- the ray carries its whole
 * weight out or back in -- so under BZR_SURFACE_FRESNEL what leaves the account, beside absorption, is the 1 - T share
 * at every entry into a lens and at the exits of rays whose budget was spent; the expectation of every row-0 sum is
 * bzr_illuminate_farfield's. */
bzr_status bzr_illuminate_ghost(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                const bzr_target *target, const bzr_radiometry *rad, uint32_t max_bounces,
                                uint64_t ghost_seed, uint64_t *flux_q32, uint32_t *hist,
                                uint64_t *reflected_flux_q32, uint32_t *reflected_hist,
                                uint64_t *stats, uint64_t *power_q32,
                                uint64_t *ledger_count, uint64_t *ledger_power_q32, uint32_t flags,
                                const bzr_farfield *far, uint64_t *far_flux_q32, uint32_t *far_hist,
                                uint64_t *far_reflected_flux_q32, uint64_t *far_stats, uint64_t *far_power_q32);
/* bzr_illuminate_ghost over the chain of bzr_trace_chain_bidir: `axis` follows ghost_seed (checked as there), and two
 * host outputs follow the ledger: back_count and back_power_q32, each [nchan][BZR_LEDGER_ROWS], each may be NULL, both
 * overwritten.  A ray that ends BZR_RR_BACK is counted in row min(bounces, BZR_MAX_BOUNCES) of its channel, with q(w)
 * summed beside it; it is in no ledger field, does not land, is not binned in the far field and is not in
 * stats[EXITED].  OUTSIDE rays land and are binned as in bzr_illuminate_ghost.  Per channel
 *   sum over rows (LOST + EXITED) + sum over rows BACK = EMITTED - CULLED.
 * With rad->surface == BZR_SURFACE_LOSSLESS no draw is taken, and the call is bzr_illuminate_farfield bit for bit
 * wherever the side rule sends no ray backward (the back rows are then zero).  The chain is fused: an explicit
 * BZR_PIPELINE_STAGED returns BZR_ERR_INVALID_ARGUMENT. */
bzr_status bzr_illuminate_bidir(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                const bzr_target *target, const bzr_radiometry *rad, uint32_t max_bounces,
                                uint64_t ghost_seed, const float axis[3], uint64_t *flux_q32, uint32_t *hist,
                                uint64_t *reflected_flux_q32, uint32_t *reflected_hist,
                                uint64_t *stats, uint64_t *power_q32,
                                uint64_t *ledger_count, uint64_t *ledger_power_q32,
                                uint64_t *back_count, uint64_t *back_power_q32, uint32_t flags,
                                const bzr_farfield *far, uint64_t *far_flux_q32, uint32_t *far_hist,
                                uint64_t *far_reflected_flux_q32, uint64_t *far_stats, uint64_t *far_power_q32);
/* bzr_illuminate_bidir over the chain of bzr_trace_chain_coated: `coat` follows axis (checked as there); the same
 * outputs, ledger and BACK rows.  With rad->surface == BZR_SURFACE_LOSSLESS the coating is ignored (no draw, no T): the
 * call is bzr_illuminate_bidir's lossless call bit for bit.  With coat == NULL or mask == 0 it is bzr_illuminate_bidir
 * bit for bit. */
bzr_status bzr_illuminate_coated(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                 const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                 uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                 const bzr_target *target, const bzr_radiometry *rad, uint32_t max_bounces,
                                 uint64_t ghost_seed, const float axis[3], const bzr_coating *coat,
                                 uint64_t *flux_q32, uint32_t *hist,
                                 uint64_t *reflected_flux_q32, uint32_t *reflected_hist,
                                 uint64_t *stats, uint64_t *power_q32,
                                 uint64_t *ledger_count, uint64_t *ledger_power_q32,
                                 uint64_t *back_count, uint64_t *back_power_q32, uint32_t flags,
                                 const bzr_farfield *far, uint64_t *far_flux_q32, uint32_t *far_hist,
                                 uint64_t *far_reflected_flux_q32, uint64_t *far_stats, uint64_t *far_power_q32);
/* Host helpers (no device).  bzr_farfield_cell: the cell rule above on the host, the device's twin: *cell is the
 * cell of direction d, or -1 where d is not binned (maps of 2^31 cells or more are refused).
 * bzr_farfield_directions: each cell centre in binary64, cell-major: dir_xyz [cells][3] the unit direction,
 * polar_rad [cells] its angle from the pole, azimuth_rad [cells] = atan2(Y, X) (each may be NULL).  The inverse map:
 * rho^2 = X^2 + Y^2, mu = 1 - rho^2 / 2, (a, b) = (X, Y) sqrt(1 - rho^2 / 4), d = a axis_u + b axis_v + mu n.
 * bzr_farfield_intensity: out[m][cell] = scale x flux_q32[m][cell] / 2^32 / cell solid angle for nmaps maps: power
 * per steradian; pass scale = 1 / emitted power for a normalised pattern. */
bzr_status bzr_farfield_cell(const bzr_farfield *far, const float d[3], int32_t *cell);
bzr_status bzr_farfield_directions(const bzr_farfield *far, double *dir_xyz, double *polar_rad, double *azimuth_rad);
bzr_status bzr_farfield_intensity(const bzr_farfield *far, const uint64_t *flux_q32, uint32_t nmaps, double scale,
                                  double *out);
/* The bounding sphere bzr_illuminate culls with: center xyz, radius. */
bzr_status bzr_mesh_bounding_sphere(const bzr_mesh *mesh, float out[4]);

/* ---- multi-GPU frames: a rank's results into its gather buffer (bzr_amd/frame.py) ---- */
/* No reference counterpart: the reference is single-process (its refraction chain loop,
 * reference/test.cpp:376-401, keeps the results in host vectors); this is the step between
 * bzr_trace_chain and the per-frame gather of a sharded image. */
enum { BZR_PACK_IMAGE = 0, BZR_PACK_RAYS = 1, BZR_PACK_COMPACT = 2 };
/* One chain frame's outputs (bzr_trace_chain: rays_soa [6][n], status [n], segments [n]; device
 * pointers) into `packed` (device) on the context's stream, without a host sync.  npad >= n is the
 * padded per-rank column count of the gather buffer.
 *   BZR_PACK_IMAGE    packed[npad] words: word i = status | segments << 8 (rays_soa may be NULL)
 *   BZR_PACK_RAYS     packed[7][npad]: the 6 ray rows, then the word row
 *   BZR_PACK_COMPACT  npad / 4 words of bytes, byte i = (status & 3) | segments << 2; then the
 *                     survivor count (uint32); then 6 rows of cap + 1 floats holding the rays of the
 *                     survivors (segments >= 2 or status != 0) in ray order.  0 < cap <= npad, npad a
 *                     multiple of 4; survivors past cap are counted but not written (the reader checks
 *                     count <= cap).
 * Columns >= n (and the last column of each compact row) are not written.  With n = 0 the input
 * pointers may be NULL. */
bzr_status bzr_pack_frame(bzr_ctx *ctx, int32_t layout, const float *rays_soa, const uint32_t *status,
                          const uint32_t *segments, uint32_t n, uint32_t npad, uint32_t cap, void *packed);

/* ---- host preprocessing (reference Mesh / BezierMesh construction) ---- */
enum { BZR_ENVELOPE_ELLIPSOID = 0, BZR_ENVELOPE_TESTLENS = 1 };
bzr_status bzr_trimesh_create(bzr_trimesh **out);
bzr_status bzr_trimesh_destroy(bzr_trimesh *m);
bzr_status bzr_trimesh_copy(const bzr_trimesh *src, bzr_trimesh **out);
bzr_status bzr_trimesh_size(const bzr_trimesh *m, uint32_t *n);
bzr_status bzr_trimesh_get(const bzr_trimesh *m, float *xyz /* 9*n */);
bzr_status bzr_trimesh_set(bzr_trimesh *m, const float *xyz, uint32_t n);
bzr_status bzr_trimesh_make_solid_of_revolution(bzr_trimesh *m, int32_t sectors, int32_t belts, int32_t envelope,
                                                float sx, float sy, float sz);
bzr_status bzr_trimesh_make_ellipsoid(bzr_trimesh *m, int32_t sectors, int32_t belts, float sx, float sy, float sz);
bzr_status bzr_trimesh_read_stl(bzr_trimesh *m, const char *path);
bzr_status bzr_trimesh_write_stl(const bzr_trimesh *m, const char *path);
bzr_status bzr_trimesh_transform(bzr_trimesh *m, const float transform_colmajor[9], const float displacement[3]);
bzr_status bzr_trimesh_split(bzr_trimesh *m, int32_t divisor);
bzr_status bzr_trimesh_split_maxside(bzr_trimesh *m, float max_side);
bzr_status bzr_trimesh_standardize_vertices(bzr_trimesh *m);
bzr_status bzr_trimesh_standardize_normals(bzr_trimesh *m);
/* Face neighbours after standardize_normals: 3 fellow indices + 3 common-side starts per face. */
bzr_status bzr_trimesh_neighbours(const bzr_trimesh *m, uint32_t *fellow /* 3*n */, uint8_t *start /* 3*n */);
/* BezierMesh(Mesh): writes 3*n patches. */
bzr_status bzr_bezier_build(const bzr_trimesh *m, bzr_patch *out);
/* BezierMesh::splitThickBezierTriangles -> new (unstandardized) triangle mesh */
bzr_status bzr_bezier_split_thick(const bzr_trimesh *m, bzr_trimesh *out);
/* BezierMesh::interpolate(divisor) -> tessellated triangle mesh */
bzr_status bzr_bezier_interpolate(const bzr_trimesh *m, int32_t divisor, bzr_trimesh *out);

#ifdef __cplusplus
}
#endif
#endif
