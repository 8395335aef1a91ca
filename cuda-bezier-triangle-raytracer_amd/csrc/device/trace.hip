// trace.hip -- CDNA4 kernels of the hot path + the device half of the C ABI.
//
// Reference semantics (one ray per lane, IEEE binary32, reference operation order):
//   BezierMesh::intersect      reference/bezierMesh.cpp:206-227
//   BezierTriangle::intersect  reference/bezierTriangle.cpp:123-195
//   BezierLens::refract        reference/bezierLens.cpp:4-34
//   refraction chain driver    reference/test.cpp:376-401
//
// Two interchangeable scan strategies, identical output bits (tests/test_gpu_parity.py):
//   culled (default)  k_traverse walks the lens BVH (bvh.cpp) wave-uniformly: node and patch
//                     boxes are fetched with scalar loads, each lane slab-tests its own ray, the
//                     wave descends while any lane hits (ballot), and lanes whose ray passes a
//                     patch's exact planar gate append that patch to their candidate list.
//                     k_resolve_* then runs the Newton stage over each ray's candidates and keeps
//                     the (t, patch index) lexicographic minimum -- the same winner as the
//                     reference's in-order strict-< scan.  Lists that overflow, stacks that
//                     overflow and rays beyond the boxes' validity radius fall back to the full
//                     in-order scan inside k_resolve_*, so every ray gets the reference result.
//   brute force       (BZR_ACCEL_NONE) the reference's own scan: every patch's 64-byte planar
//                     record fetched once per wave with scalar loads, Newton for passing lanes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>
#include <string>
#include <vector>

#include "../host/bvh.hpp"
#include "../host/staging.hpp"
#include "bzr.h"
#include "ctx.hpp"
#include "patch_math.hpp"
#include "pass_order.hpp"
#include "emitter.hpp"

using namespace bzr_dev;

// ------------------------------------------------------------------ errors
namespace {
thread_local std::string t_error;
bzr_status set_error(bzr_status s, const std::string &msg) {
  t_error = msg;
  return s;
}
#define BZR_HIP(call)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (call);                                                                               \
    if (e_ != hipSuccess) return set_error(BZR_ERR_HIP, std::string(#call ": ") + hipGetErrorString(e_)); \
  } while (0)
}  // namespace

extern "C" const char *bzr_last_error(void) { return t_error.c_str(); }
extern "C" int32_t bzr_abi_version(void) { return BZR_ABI_VERSION; }
// the host half of the library reports its errors through here
extern "C" void bzr_internal_set_error(const char *msg) { t_error = msg ? msg : ""; }

// ------------------------------------------------------------ device mesh
struct bzr_mesh {
  int device;
  uint32_t n;
  float4 *planar;   // 4 float4 per patch: n.xyz c | hin hout M00 M01 | M02 M10 M11 M12 | M20 M21 M22 0
  float *full;      // 66 words per patch (bzr_patch)
  bzr_host::Bvh4Node *nodes;  // 4-wide BVH over the patches' gate-region boxes (bvh.cpp), far tier
  float4 *leaf;     // 4 float4 per BVH leaf slot: the planar record, patch index in the last word
  bzr_host::Bvh4Node *nodes_near;  // the near tier's tree and leaf slots (bvh.hpp kTierNear)
  float4 *leaf_near;
  bzr_host::Bvh4ObbNode *obb;       // both tiers' wide-patch subtrees (oriented boxes, bvh.hpp)
  bzr_host::Bvh4ObbNode *obb_near;
  float4 *kids;      // the far tree's children AoS (2 float4 per child: lo.xyz ref, hi.xyz 0): the bundle walk's
  float4 *kids_near; // per-lane child records (kids_of), and the near tree's
  float4 *wide;      // two levels per node for k_traverse's bundle walk (wide_of): node i's 16
  float4 *wide_near; // grandchild slots, 2 float4 each as in kids
  float4 *swide;      // the same records of the trees with split leaf boxes (bvh.hpp build_bvh split), which the
  float4 *swide_near; // fused refract and chain kernels' bundle walk takes (empty when the mesh is not split)
  uint32_t split;     // strips per narrow patch in those trees (1: not split)
  float4 *always;   // 8 float4 per always-tested patch (bvh.hpp Bvh::always): planar record with the patch index
                    // in its last word, then the wedge pre-test (always_wedge: w.xyz L H B C 0) and 8 pad words
  uint32_t n_always;
  uint32_t nnodes;
  float s_max;      // far tier: origins beyond take the full scan
  float s_near;     // near tier: waves whose rays all start within it walk the tighter tree
  float sphere[4];  // Ritter sphere over the gate-region boxes (bvh.cpp): the illumination pre-cull
};

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kMaxLenses = 8;
constexpr uint32_t kMaxCand = 40;  // candidate list length per ray and segment
constexpr uint32_t kOverflow = 0x8000u;  // count flag: resolve with the full scan (the low bits keep the listed count)
// Traversal stack entries per wave (LDS).  BZR_STACK (A/B and test knob): a tiny stack makes waves run out
// mid-walk, which sends the affected lanes to the in-order full scan (tests/test_gpu_variants.py).
#ifndef BZR_STACK
#define BZR_STACK 64
#endif
constexpr int kStack = BZR_STACK;
// Device work counters (bzr_ctx_counters) are kept in this many copies, summed by the report: a wave adds
// to copy (wave index mod kCounterReplicas), so a frame's ~10^5 waves do not queue on a few addresses.
constexpr uint32_t kCounterReplicas = 64;

// 64-byte wave-uniform records read through the constant address space: one s_load_dwordx16 each
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(4))) const u32x16 cu32x16;

// Blocks are dealt round-robin to the 8 XCDs (each with its own L2 and scalar caches).  This maps
// block b to a bijective index under which each XCD owns one contiguous range of the grid, so the
// blocks an XCD runs together work on neighbouring rays (same BVH nodes, same patches).
constexpr uint32_t kXcds = 8;
__device__ __forceinline__ uint32_t xcd_contiguous(uint32_t b, uint32_t nblocks) {
  const uint32_t q = nblocks / kXcds, r = nblocks % kXcds, x = b % kXcds;
  return x * q + (x < r ? x : r) + b / kXcds;
}
// Threads per k_traverse block (kTravBlock): one-wave blocks let a finished wave be replaced
// at once, as in k_trace; 256 (4 waves sharing a CU's scalar cache on neighbouring rays, rounds 1-3) measured
// 0.5-1 % slower on cfg5 and 0.1-0.2 % on cfg3 at bench level, 128 4 % slower on cfg3
// (profiles/r04_bench_ab_trav_block.jsonl).
// BZR_TRAV_ABLOCK: the always list's bundle pre-test once per 256-thread block instead of once per wave, for
// meshes whose always list takes more than one 64-patch round (kAblockMin < n_always <= kAblockMax; others keep
// the one-wave kernel).  Before the walk every wave's bundle is in LDS; the block's union bundle tests the
// always-listed patches, one per thread, and keeps a mask in LDS.  1 (default): each wave gate-tests the
// block-kept patches per lane; 0: off.  A dropped patch is one no ray of the block (so of the wave) can pass: the
// candidates are unchanged.  cfg5 (131 always-listed patches): k_traverse 4.01 -> 3.84 ms per frame
// (profiles/r05_ab_traverse_ablock.jsonl).
#ifndef BZR_TRAV_ABLOCK
#define BZR_TRAV_ABLOCK 1
#endif
static_assert(BZR_TRAV_ABLOCK == 0 || BZR_TRAV_ABLOCK == 1, "BZR_TRAV_ABLOCK: 0 or 1");
#ifndef BZR_ABLOCK_BLOCK
#define BZR_ABLOCK_BLOCK 256
#endif
constexpr uint32_t kAblockMin = 64, kAblockMax = 1024, kAblockBlock = BZR_ABLOCK_BLOCK;  // threads per pre-testing block
constexpr int kTravBlock = 64;
// Waves whose ray directions spread wider than this (bundle_setup_swap) take the per-lane walk instead of the
// bundle walk.
constexpr float kBundleSpread = 0.5f;
// Slots per node of the wide records (bzr_mesh wide / wide_near: each node's grandchildren): k_traverse's
// bundle walk takes two tree levels per batch over them, 4 nodes per batch instead of 16 nodes' children
// (profiles/r04_ab_wide_walk.jsonl).
constexpr uint32_t kWideSlots = 16u;
// BZR_TRACE_WIDE (default 1, with BZR_TRACE_BUNDLE): k_trace's bundle walk over the same two-level records.
#ifndef BZR_TRACE_WIDE
#define BZR_TRACE_WIDE 1
#endif
// Blocks of k_resolve at most (its overflow part is grid-stride over (overflow ray, patch slice) items).
constexpr uint32_t kOverflowBlocks = 2048u;
// BZR_DENSE_MIN (default 16): the staged pair layout.  A patch bucket's pairs fill whole 64-pair chunks of
// that one patch (dense chunks: patch-uniform Newton passes, every lane busy); its last, partial chunk is
// padded to a whole chunk when it holds at least this many pairs, else its pairs go to the sparse region
// behind the dense chunks, where k_newton_lane runs one pair per lane with the lane's own patch record.
// 64 = no padding.  (A sparse chunk costs ~4 dense ones -- 4 waves per SIMD, per-lane record loads -- so a
// remainder of r pairs is cheaper padded from r ~ 16 on; cfg5: DESIGN.md.)  Padding is below 64 slots per
// patch, which sizes the pair array at cap + 64 (nb + 1).
#ifndef BZR_DENSE_MIN
#define BZR_DENSE_MIN 16
#endif
constexpr uint32_t kDenseMin = BZR_DENSE_MIN;
static_assert(kDenseMin >= 1 && kDenseMin <= 64, "BZR_DENSE_MIN: 1..64");
// Staged winner keys (t order << 32 | patch << 6 | list slot j) and pair records (ray | j << 26,
// patch | follow side << 30): chunk rays below 2^26, list slots below 64, patch indices below 2^25 (keys
// take 26 bits; the pair array's 32-bit indices, 64 padding slots per patch).
constexpr uint32_t kStagedPatchLimit = 1u << 25, kRayMask = (1u << 26) - 1u, kNoPair = 0xFFFFFFFFu;
struct MeshView {
  const float4 *__restrict__ planar;
  const float *__restrict__ full;
  const bzr_host::Bvh4Node *__restrict__ nodes;
  const float4 *__restrict__ leaf;
  const bzr_host::Bvh4Node *__restrict__ nodes_near;
  const float4 *__restrict__ leaf_near;
  const bzr_host::Bvh4ObbNode *__restrict__ obb;
  const bzr_host::Bvh4ObbNode *__restrict__ obb_near;
  const float4 *__restrict__ always;  // patches without a proven gate region: gate-tested by every wave-segment
  const float4 *__restrict__ kids;       // AoS child records of nodes / nodes_near (bzr_mesh)
  const float4 *__restrict__ kids_near;
  const float4 *__restrict__ wide;       // 16 grandchild records per node (wide_of)
  const float4 *__restrict__ wide_near;
  uint32_t n_always;
  uint32_t n;
  float s_max;
  float s_near;
  float ri;
  uint32_t split;                        // > 1: swide's leaves name a slot several times (TraceLds seen)
  const float4 *__restrict__ swide;      // wide / wide_near of the split trees (the unsplit ones when split == 1)
  const float4 *__restrict__ swide_near;
};
struct LensSet {
  MeshView lens[kMaxLenses];
  uint32_t count;
};

__device__ __forceinline__ void store_hit(float *__restrict__ hits, uint32_t n, uint32_t i, const Hit &h,
                                          uint32_t patch) {
  hits[i] = h.t;
  hits[(size_t)1 * n + i] = h.point.x;
  hits[(size_t)2 * n + i] = h.point.y;
  hits[(size_t)3 * n + i] = h.point.z;
  hits[(size_t)4 * n + i] = h.cs;
  hits[(size_t)5 * n + i] = h.bary.x;
  hits[(size_t)6 * n + i] = h.bary.y;
  hits[(size_t)7 * n + i] = h.bary.z;
  hits[(size_t)8 * n + i] = h.normal.x;
  hits[(size_t)9 * n + i] = h.normal.y;
  hits[(size_t)10 * n + i] = h.normal.z;
  reinterpret_cast<uint32_t *>(hits)[(size_t)11 * n + i] = h.what;
  reinterpret_cast<uint32_t *>(hits)[(size_t)12 * n + i] = patch;
}

__device__ __forceinline__ Hit no_hit() {
  Hit h;
  h.t = FLT_MAX;
  h.what = kNone;
  h.point = h.bary = h.normal = mk(0.0f, 0.0f, 0.0f);
  h.cs = 0.0f;
  return h;
}

// Planar gate of BezierTriangle::intersect with cThis (reference/bezierTriangle.cpp:124-131),
// evaluated from the 64-byte scan record; same arithmetic as patch_intersect's first lines.
// `gt` gets the plane distance t (whatever the decision).
__device__ __forceinline__ bool planar_gate(float4 q0, float4 q1, float4 q2, float4 q3, f3 s, f3 d, float &gt) {
  // Branch-free: every term is evaluated and the conditions are combined with '&' (the same decision as
  // plane_ray's early outs -- a lane with |cos| < 1e-5 fails whatever its t), so the walk runs no
  // exec-mask bookkeeping (s_and_saveexec / s_or exec per condition) on the scalar unit.
  const f3 n = mk(q0.x, q0.y, q0.z);
  const float cs = dot(d, n);
  const float t = div_rn(q0.w - dot(n, s), cs);
  const f3 ip = add(s, scale(d, t));
  gt = t;
  const bool valid = (fabsf(cs) >= 0.00001f) & (t > 0.0f) & (fabsf(t) > -q1.x) & (fabsf(t) > q1.y);
  const float b0 = q1.z * ip.x + (q1.w * ip.y + q2.x * ip.z);
  const float b1 = q2.y * ip.x + (q2.z * ip.y + q2.w * ip.z);
  const float b2 = q3.x * ip.x + (q3.y * ip.y + q3.z * ip.z);
  return valid & (b0 >= 0.0f) & (b0 <= 1.0f) & (b1 >= 0.0f) & (b1 <= 1.0f) & (b2 >= 0.0f) & (b2 <= 1.0f);
}
__device__ __forceinline__ bool planar_gate(float4 q0, float4 q1, float4 q2, float4 q3, f3 s, f3 d) {
  float gt;
  return planar_gate(q0, q1, q2, q3, s, d, gt);
}

// One iteration of the reference loop body: patch b with cThis, and on a follow-side result its
// named neighbour with cNone (reference/bezierMesh.cpp:212-216).  `src` gets the patch that hit.
template <bool kFast = false>
__device__ __forceinline__ Hit evaluate_patch(const MeshView &m, uint32_t b, f3 s, f3 d, uint32_t &src) {
  uint32_t idx = b;
  bool limitNone = false;
  Hit h;
  for (int pass = 0; pass < 2; ++pass) {
    Patch p = load_patch(m.full + (size_t)rec::kWords * idx);
    h = patch_intersect<false, kFast>(p, s, d, limitNone);
    if (pass == 0 && h.what <= kFollow2) {
      idx = __float_as_uint(m.full[(size_t)rec::kWords * idx + rec::kNeigh + h.what]);
      limitNone = true;
      continue;
    }
    break;
  }
  src = idx;
  return h;
}

// BezierMesh::intersect by the reference's brute-force scan: index order, strict-< minimum.
__device__ __forceinline__ Hit mesh_intersect_scan(const MeshView &m, f3 s, f3 d, uint32_t &patch) {
  Hit best = no_hit();
  patch = 0xFFFFFFFFu;
  for (uint32_t b = 0; b < m.n; ++b) {
    const float4 *q = m.planar + 4u * b;  // wave-uniform address -> scalar loads
    if (!planar_gate(q[0], q[1], q[2], q[3], s, d)) continue;
    uint32_t src;
    Hit h = evaluate_patch(m, b, s, d, src);
    if (h.what == kIntersect && h.t < best.t) {
      best = h;
      patch = src;
    }
  }
  return best;
}

// The refraction of BezierLens::refract after the mesh intersection.  Returns the status;
// o_s/o_d = refracted ray when status != NONE.  kGain: `gain` = the refraction's Fresnel transmittance
// (patch_math_body.inc fresnel_t, from this step's own eta and s2) when the status is not NONE.
template <bool kGain>
__device__ __forceinline__ uint32_t refract_hit_t(const Hit &h, float ri, f3 s, f3 d, uint32_t expected, f3 &o_s,
                                                  f3 &o_d, float &gain) {
  o_s = s;
  o_d = d;
  uint32_t st = BZR_RR_NONE;
  if (h.what == kIntersect) {
    st = h.cs < 0.0f ? BZR_RR_INSIDE : BZR_RR_OUTSIDE;
    o_s = h.point;
    float eta = st == BZR_RR_INSIDE ? div_rn(1.0f, ri) : ri;
    float s2 = eta * eta * (1.0f - h.cs * h.cs);
    // (ahead of the branch: lanes with s2 >= 0.99 return NONE and their gain is not read)
    if constexpr (kGain) gain = fresnel_t(eta, h.cs, s2);
    if (s2 < 0.99f) {
      if (s2 > 1e-12f) {
        float sgn = st == BZR_RR_INSIDE ? 1.0f : -1.0f;
        f3 nn = scale(h.normal, sgn);
        float c1 = fabsf(h.cs);
        float c2 = sqrt_rn(1.0f - s2);
        o_d = normalized(add(scale(d, eta), scale(nn, eta * c1 - c2)));
      }
    } else {
      st = BZR_RR_NONE;
    }
  }
  return st == expected ? st : BZR_RR_NONE;
}
__device__ __forceinline__ uint32_t refract_hit(const Hit &h, float ri, f3 s, f3 d, uint32_t expected, f3 &o_s,
                                                f3 &o_d) {
  float gain;
  return refract_hit_t<false>(h, ri, s, d, expected, o_s, o_d, gain);
}

// Snell's step with total internal reflection (kModeTir).  A ray that leaves glass (expected OUTSIDE, cs >= 0) with
// s2 = ri^2 (1 - cs^2) >= 1 cannot refract: when `may_reflect` (the ray's channel is in the table and its bounce
// budget in this lens is not spent) it is mirrored at the hit -- k = 2 cs, r = d - n k per component, o_d =
// normalized(r), o_s = the hit's point -- and the step returns kReflected, a status only the chain drivers see:
// the ray stays inside and meets the same lens again.  Everything else is refract_hit_t: s2 < 0.99 refracts,
// 0.99 <= s2 < 1 (the reference's grazing limit), a NaN s2 and a refused reflection return NONE.
constexpr uint32_t kReflected = 3u;
template <bool kGain>
__device__ __forceinline__ uint32_t tir_hit_t(const Hit &h, float ri, f3 s, f3 d, uint32_t expected, bool may_reflect,
                                              f3 &o_s, f3 &o_d, float &gain) {
  const float s2 = ri * ri * (1.0f - h.cs * h.cs);
  if (expected == BZR_RR_OUTSIDE && may_reflect && h.what == kIntersect && h.cs >= 0.0f && s2 >= 1.0f) {
    const float k = 2.0f * h.cs;
    o_d = normalized(sub(d, scale(h.normal, k)));
    o_s = h.point;
    return kReflected;
  }
  return refract_hit_t<kGain>(h, ri, s, d, expected, o_s, o_d, gain);
}

// Snell's step between two media (kModeMedia): refract_hit_t with the step's eta handed in -- n0 / n1 for a segment
// expected INSIDE, n1 / n2 for one expected OUTSIDE (media_eta) -- in place of 1 / ri and ri.  A hit on the other side
// returns NONE whatever eta it was given.  s2, the refraction limit, the direction and the Fresnel term all come from
// this eta, in refract_hit_t's order; with eta = 1 / ri and ri they are its bits.  (A sibling, not refract_hit_t
// re-expressed: the instantiations of the older modes compile to the code they had.)
template <bool kGain>
__device__ __forceinline__ uint32_t refract_eta_t(const Hit &h, float eta, f3 s, f3 d, uint32_t expected, f3 &o_s,
                                                  f3 &o_d, float &gain) {
  o_s = s;
  o_d = d;
  uint32_t st = BZR_RR_NONE;
  if (h.what == kIntersect) {
    st = h.cs < 0.0f ? BZR_RR_INSIDE : BZR_RR_OUTSIDE;
    o_s = h.point;
    float s2 = eta * eta * (1.0f - h.cs * h.cs);
    if constexpr (kGain) gain = fresnel_t(eta, h.cs, s2);
    if (s2 < 0.99f) {
      if (s2 > 1e-12f) {
        float sgn = st == BZR_RR_INSIDE ? 1.0f : -1.0f;
        f3 nn = scale(h.normal, sgn);
        float c1 = fabsf(h.cs);
        float c2 = sqrt_rn(1.0f - s2);
        o_d = normalized(add(scale(d, eta), scale(nn, eta * c1 - c2)));
      }
    } else {
      st = BZR_RR_NONE;
    }
  }
  return st == expected ? st : BZR_RR_NONE;
}
// tir_hit_t's form of it: the reflection test reads the same eta (s2 = eta^2 (1 - cs^2) >= 1 on a segment expected
// OUTSIDE), so a lens in a medium as dense as its glass reflects nothing.
template <bool kGain>
__device__ __forceinline__ uint32_t tir_eta_t(const Hit &h, float eta, f3 s, f3 d, uint32_t expected, bool may_reflect,
                                              f3 &o_s, f3 &o_d, float &gain) {
  const float s2 = eta * eta * (1.0f - h.cs * h.cs);
  if (expected == BZR_RR_OUTSIDE && may_reflect && h.what == kIntersect && h.cs >= 0.0f && s2 >= 1.0f) {
    const float k = 2.0f * h.cs;
    o_d = normalized(sub(d, scale(h.normal, k)));
    o_s = h.point;
    return kReflected;
  }
  return refract_eta_t<kGain>(h, eta, s, d, expected, o_s, o_d, gain);
}
// The Fresnel roulette's uniform (kModeGhost; include/bzr.h bzr_trace_chain_ghost): a 24-bit uniform in [0, 1) for
// ray number j = first_ray + i and draw e = 16 lens + reflections so far in that lens, off the emitter's uniform2
// stream by the xor.  The host folds everything of the first hash's argument that the call fixes into one word,
// base = (seed ^ 0x5851F42D4C957F2D) + golden (first_ray + 1) (ghost_base), so that mod 2^64 the argument
// (seed ^ ...) + golden (j + 1) is base + golden i: one 64-bit kernel argument, one 64 x 32 product per lane.
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
inline uint64_t ghost_base(uint64_t seed, uint64_t first_ray) {
  return (seed ^ 0x5851F42D4C957F2Dull) + kGolden * (first_ray + 1ull);
}
__device__ __forceinline__ float ghost_uniform(uint64_t base, uint32_t i, uint32_t e) {
  const uint64_t r = mix64(base + kGolden * (uint64_t)i);
  const uint64_t h = mix64(r + kGolden * ((uint64_t)e + 1ull));
  return (float)(uint32_t)(h >> 40) * 0x1p-24f;
}
// tir_eta_t with the roulette (kModeGhost).  A hit that tir_eta_t would test for total reflection -- expected OUTSIDE,
// `may_reflect`, an intersection with cs >= 0 -- and that Snell's step would refract (s2 < 0.99) draws when `may_draw`
// (u: the lane's uniform for this segment, made by the caller):
// u >= T mirrors the ray exactly as a total reflection does (kReflected); u < T refracts it with gain 1, the roulette
// having taken the 1 - T share.  Everything else is tir_eta_t.  (A sibling: the older instantiations keep their code.)
template <bool kGain>
__device__ __forceinline__ uint32_t ghost_eta_t(const Hit &h, float eta, f3 s, f3 d, uint32_t expected, bool may_reflect,
                                                bool may_draw, float u, f3 &o_s, f3 &o_d, float &gain) {
  const float s2 = eta * eta * (1.0f - h.cs * h.cs);
  const bool leaving = expected == BZR_RR_OUTSIDE && may_reflect && h.what == kIntersect && h.cs >= 0.0f;
  const bool drawn = leaving && may_draw && s2 < 0.99f;
  bool mirror = leaving && s2 >= 1.0f;
  if (drawn) mirror = u >= fresnel_t(eta, h.cs, s2);
  if (mirror) {
    const float k = 2.0f * h.cs;
    o_d = normalized(sub(d, scale(h.normal, k)));
    o_s = h.point;
    return kReflected;
  }
  const uint32_t st = refract_eta_t<kGain>(h, eta, s, d, expected, o_s, o_d, gain);
  if (drawn) gain = 1.0f;
  return st;
}
// The bidirectional walk's step (kModeBidir; include/bzr.h bzr_trace_chain_bidir): ghost_eta_t on either side of the
// glass.  `expected` names the side the segment must meet -- INSIDE (cs < 0) for an open segment, OUTSIDE (cs >= 0)
// for a glass segment -- and on that side, with `may_reflect` (the channel is in the table, the ray's budget is not
// spent), s2 >= 1 mirrors the ray and s2 < 0.99 draws when `may_draw`: u >= T mirrors, u < T refracts with gain 1.
// The mirror step is tir_eta_t's for both signs of cs.  Everything else is refract_eta_t.  (A sibling again.)
template <bool kGain>
__device__ __forceinline__ uint32_t bidir_eta_t(const Hit &h, float eta, f3 s, f3 d, uint32_t expected, bool may_reflect,
                                                bool may_draw, float u, f3 &o_s, f3 &o_d, float &gain) {
  const float s2 = eta * eta * (1.0f - h.cs * h.cs);
  const bool side = expected == BZR_RR_INSIDE ? h.cs < 0.0f : h.cs >= 0.0f;
  const bool facing = may_reflect && h.what == kIntersect && side;
  const bool drawn = facing && may_draw && s2 < 0.99f;
  bool mirror = facing && s2 >= 1.0f;
  if (drawn) mirror = u >= fresnel_t(eta, h.cs, s2);
  if (mirror) {
    const float k = 2.0f * h.cs;
    o_d = normalized(sub(d, scale(h.normal, k)));
    o_s = h.point;
    return kReflected;
  }
  const uint32_t st = refract_eta_t<kGain>(h, eta, s, d, expected, o_s, o_d, gain);
  if (drawn) gain = 1.0f;
  return st;
}
// bidir_eta_t on coated surfaces (kModeCoat; include/bzr.h bzr_coating): T is chosen per lane between fresnel_t and
// coat_t(row, mu), `coated` saying which and `row` being the lane's row of the table (always inside the table's part of
// the context's buffer, whatever the hit is).  T matters to the lanes that `pays`: `live` (the caller's: the lane is in
// this round and its channel in the table), a hit on the expected side, s2 < 0.99 -- they draw against it or multiply
// it in.  Both forms are skipped by a wave vote, not per lane: fresnel_t's two divisions and square root when no
// paying lane meets bare glass, the table's gather when none meets a coating.  A lane that does not look its T up
// reads entry 0 and 1 of its row and drops them.  (A sibling again: bidir_eta_t's instantiations keep their code.)
__device__ __forceinline__ uint32_t coat_eta_t(const Hit &h, float eta, f3 s, f3 d, uint32_t expected, bool live,
                                               bool may_reflect, bool may_draw, float u, bool coated,
                                               const float *__restrict__ row, f3 &o_s, f3 &o_d, float &gain) {
  const float s2 = eta * eta * (1.0f - h.cs * h.cs);
  const bool open = expected == BZR_RR_INSIDE;
  const bool side = open ? h.cs < 0.0f : h.cs >= 0.0f;
  const bool met = h.what == kIntersect && side;
  const bool facing = may_reflect && met;
  const bool drawn = facing && may_draw && s2 < 0.99f;
  const bool pays = live && met && s2 < 0.99f;
  const bool looks = pays && coated;
  float t = 1.0f;
  if (__any(pays && !coated)) t = fresnel_t(eta, h.cs, s2);
  if (__any(looks)) {
    float f;
    int i = coat_cell(open ? fabsf(h.cs) : sqrt_rn(1.0f - s2), f);
    i = looks ? i : 0;
    const float tc = coat_mix(row[i], row[i + 1], f);
    if (looks) t = tc;
  }
  bool mirror = facing && s2 >= 1.0f;
  if (drawn) mirror = u >= t;
  if (mirror) {
    const float k = 2.0f * h.cs;
    o_d = normalized(sub(d, scale(h.normal, k)));
    o_s = h.point;
    return kReflected;
  }
  float unused;
  const uint32_t st = refract_eta_t<false>(h, eta, s, d, expected, o_s, o_d, unused);
  gain = drawn ? 1.0f : t;
  return st;
}
// The walk's side rule: does the surface a glass segment met face forward along the chain's axis `a`?  One dot product
// in binary32, the last two products summed first (no contraction: the build's -ffp-contract=off).
__device__ __forceinline__ bool bidir_back(f3 n, f3 a) { return n.x * a.x + (n.y * a.y + n.z * a.z) >= 0.0f; }
// The walk's per-lane word (k_trace<kModeBidir>'s LDS row `state`, k_chain_scan<8>'s register): bits 0-3 the key
// 2 lens + phase (phase 1: inside that lens's glass; 0: in the open, heading for it), bit 4 fwd, bit 5 travelling,
// bits 8-10 the final status once it no longer travels.
constexpr uint32_t kBidirFwd = 1u << 4, kBidirTravels = 1u << 5;
__device__ __forceinline__ uint32_t bidir_ended(uint32_t status) { return status << 8; }
// The word of a ray that has just come into gap g heading `fwd`: it ends OUTSIDE behind the last lens, BACK in front of
// the first, and otherwise heads for lens g (fwd) or g - 1.
__device__ __forceinline__ uint32_t bidir_open(uint32_t g, bool fwd, uint32_t nlens) {
  if (fwd && g == nlens) return bidir_ended(BZR_RR_OUTSIDE);
  if (!fwd && g == 0u) return bidir_ended(BZR_RR_BACK);
  return 2u * (fwd ? g : g - 1u) | (fwd ? kBidirFwd : 0u) | kBidirTravels;
}
// One event's step from the word `w0` (key 2 l + gl): `r` the step's result (NONE, kReflected, or the side refracted
// to), gi the gap the segment's leg lies in (open) or leads to (glass), `back` the side rule's answer.
__device__ __forceinline__ uint32_t bidir_next(uint32_t w0, uint32_t r, bool gl, uint32_t l, uint32_t gi, bool back,
                                               uint32_t nlens) {
  if (r == BZR_RR_NONE) return bidir_ended(BZR_RR_NONE);
  if (r == kReflected) return gl ? w0 : bidir_open(gi, (w0 & kBidirFwd) == 0u, nlens);  // in glass: the same lens again
  if (!gl) return (2u * l + 1u) | kBidirTravels;                                        // refracted in
  return bidir_open(gi, back, nlens);                                                   // refracted out into gap gi
}
// The segment's eta: one correctly rounded division, n0 / n1 going in, n1 / n2 coming out (bounce segments included).
__device__ __forceinline__ float media_eta(float n0, float n1, float n2, bool outside) {
  return div_rn(outside ? n1 : n0, outside ? n2 : n1);
}

// The optical path's per-leg step (kModeOpl), for a segment from origin s that ended in a refraction or a reflection
// at the winning hit's point p: len = |p - s|, the polyline through the points the chain continues from (not the
// hit's t, BezierIntersection's value from before the last Newton step).  A leg in air (the segment expected INSIDE)
// adds len to opl; a leg in glass (expected OUTSIDE, bounce segments included) adds len to glass and ri len to opl.
// Exact binary32 in both modes, like the Fresnel term: it belongs to the chain step.
__device__ __forceinline__ void opl_leg(f3 s, f3 p, float ri, bool in_glass, float &opl, float &glass) {
  const f3 e = sub(p, s);
  const float len = sqrt_rn(dot(e, e));
  if (in_glass) {
    glass = glass + len;
    const float m = ri * len;
    opl = opl + m;
  } else {
    opl = opl + len;
  }
}
// kModeMedia's form: the leg in front of the lens (expected INSIDE) lies in a medium of index n0 and adds m = n0 len
// to opl; the leg in glass is opl_leg's.  `nm`: n1 in glass, n0 in front.  glass stays the length in lens glass.
__device__ __forceinline__ void opl_leg_media(f3 s, f3 p, float nm, bool in_glass, float &opl, float &glass) {
  const f3 e = sub(p, s);
  const float len = sqrt_rn(dot(e, e));
  if (in_glass) glass = glass + len;
  const float m = nm * len;
  opl = opl + m;
}
// kModeAbsorb's form: opl_leg_media that also hands back the leg's length, for the Beer-Lambert term.  (A sibling: the
// older instantiations keep the function they had.)
__device__ __forceinline__ float opl_leg_absorb(f3 s, f3 p, float nm, bool in_glass, float &opl, float &glass) {
  const f3 e = sub(p, s);
  const float len = sqrt_rn(dot(e, e));
  if (in_glass) glass = glass + len;
  const float m = nm * len;
  opl = opl + m;
  return len;
}
// The leg's attenuation: att(a len), and exactly 1 where the coefficient is 0 (the select keeps 0 x inf out of the
// weight, so zero tables give kModeMedia's bits whatever the leg).
__device__ __forceinline__ float leg_attenuation(float a, float len) {
  const float x = a * len;
  return a > 0.0f ? att(x) : 1.0f;
}

__device__ __forceinline__ void load_ray(const float *__restrict__ r, uint32_t n, uint32_t i, f3 &s, f3 &d) {
  s = mk(r[i], r[(size_t)n + i], r[(size_t)2 * n + i]);
  d = mk(r[(size_t)3 * n + i], r[(size_t)4 * n + i], r[(size_t)5 * n + i]);
}
__device__ __forceinline__ void store_ray(float *__restrict__ r, uint32_t n, uint32_t i, f3 s, f3 d) {
  r[i] = s.x;
  r[(size_t)n + i] = s.y;
  r[(size_t)2 * n + i] = s.z;
  r[(size_t)3 * n + i] = d.x;
  r[(size_t)4 * n + i] = d.y;
  r[(size_t)5 * n + i] = d.z;
}

// ------------------------------------------------------------ culled path
__device__ __forceinline__ float safe_inv(float x) {
  // slab test only (no parity requirement): keep 1/d finite so (b - o) * inv never makes 0 * inf
  return 1.0f / (fabsf(x) < 1e-20f ? copysignf(1e-20f, x) : x);
}

// Slab test of the ray (origin s, per-axis reciprocal direction inv, sinv = s * inv) against a box.
// Conservative only (the gate-region boxes are padded for its rounding, bvh.cpp): with FMA each
// plane distance is one fma(lo, inv, -s*inv), error <= (|s| + |t|) * 2^-23 < the pad.
__device__ __forceinline__ bool slab(float4 lo, float4 hi, f3 s, f3 sinv, f3 inv) {
  (void)s;
  float ax = __builtin_fmaf(lo.x, inv.x, -sinv.x), bx = __builtin_fmaf(hi.x, inv.x, -sinv.x);
  float ay = __builtin_fmaf(lo.y, inv.y, -sinv.y), by = __builtin_fmaf(hi.y, inv.y, -sinv.y);
  float az = __builtin_fmaf(lo.z, inv.z, -sinv.z), bz = __builtin_fmaf(hi.z, inv.z, -sinv.z);
  float tnear = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  float tfar = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
  return tnear <= tfar && tfar >= 0.0f;
}

// Ray vs oriented box (bvh.hpp Bvh4ObbNode): the slab test in the box's frame.  Culling only (no parity
// requirement): FMA and v_rcp_f32 are fine, their error is inside the box's doubled padding (bvh.cpp).
__device__ __forceinline__ float clamped_rcp(float x) {
  return __builtin_amdgcn_rcpf(fabsf(x) < 1e-20f ? copysignf(1e-20f, x) : x);
}
// q: one child's 64-byte record (bvh.hpp Bvh4ObbChild)
__device__ __forceinline__ bool obb_hit(const u32x16 &q, f3 s, f3 d) {
  const float rx = s.x - __uint_as_float(q[0]), ry = s.y - __uint_as_float(q[1]), rz = s.z - __uint_as_float(q[2]);
  float tnear = -FLT_MAX, tfar = FLT_MAX;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ux = __uint_as_float(q[3 + 3 * a]), uy = __uint_as_float(q[4 + 3 * a]), uz = __uint_as_float(q[5 + 3 * a]);
    const float o = __builtin_fmaf(rx, ux, __builtin_fmaf(ry, uy, rz * uz));
    const float dd = __builtin_fmaf(d.x, ux, __builtin_fmaf(d.y, uy, d.z * uz));
    const float h = __uint_as_float(q[12 + a]), inv = clamped_rcp(dd);
    const float t1 = (-h - o) * inv, t2 = (h - o) * inv;
    tnear = fmaxf(tnear, fminf(t1, t2));
    tfar = fminf(tfar, fmaxf(t1, t2));
  }
  return tnear <= tfar && tfar >= 0.0f;
}

// The children of BVH node `ref` (an AABB node, or an oriented-box node when ref has kObbFlag): their
// refs and which lanes' rays hit their boxes (wave-uniform fetch: two or four 64-byte scalar loads).
__device__ __forceinline__ void node_children(const bzr_host::Bvh4Node *nodes, const bzr_host::Bvh4ObbNode *obb,
                                              uint32_t ref, bool act, f3 s, f3 d, f3 sinv, f3 inv, bool (&hit)[4],
                                              uint32_t (&ch)[4]) {
  if (ref & bzr_host::kObbFlag) {  // one 64-byte scalar load per child (16 SGPRs live at a time)
    const cu32x16 *np = (const cu32x16 *)(uintptr_t)(obb + (ref & ~bzr_host::kObbFlag));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const u32x16 q = np[c];
      ch[c] = q[15];
      hit[c] = act & (ch[c] != bzr_host::kEmptyChild) & obb_hit(q, s, d);
    }
    return;
  }
  // the whole 128-byte node in two 64-byte scalar loads and one wait (all words used unconditionally)
  const cu32x16 *np = (const cu32x16 *)(uintptr_t)(nodes + ref);
  const u32x16 na = np[0], nb = np[1];
  // words: lo.x[0..3] lo.y lo.z hi.x | hi.y hi.z child[0..3] pad
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float4 lo = make_float4(__uint_as_float(na[c]), __uint_as_float(na[4 + c]), __uint_as_float(na[8 + c]), 0.0f);
    const float4 hi = make_float4(__uint_as_float(na[12 + c]), __uint_as_float(nb[c]), __uint_as_float(nb[4 + c]), 0.0f);
    ch[c] = nb[8 + c];
    hit[c] = act & (ch[c] != bzr_host::kEmptyChild) & slab(lo, hi, s, sinv, inv);
  }
}

// Per-segment pipeline of the culled path (one BezierMesh::intersect per ray of a chunk of n rays;
// external arrays -- rays, alive, outputs -- are indexed off + i with row stride ld):
//   k_traverse  BVH walk, exact planar gate -> up to kMaxCand candidates per ray, a per-patch
//               histogram (rank of each (ray, patch) pair within its patch bucket) and the list
//               of rays that need the full scan (list/stack overflow, origin beyond s_max)
//   scan        exclusive sum over the buckets of (dense chunks << 32 | sparse pairs) (bucket_split;
//               hipCUB or k_scan_small) -> each bucket's dense chunk and sparse offsets, the totals
//   k_place     (ray, patch) pair records into their bucket's dense chunks or the sparse region (8-byte
//               records: the Newton stage reads the ray itself from the ray array -- neighbouring rays,
//               mostly cached -- instead of a 32-byte copy travelling with the pair); marks the padded
//               lanes of each bucket's last dense chunk; clears the histogram for the next segment
//   k_newton    the Newton stage over the dense chunks: one patch per chunk, its record in scalar
//               registers (uniform loads); hits go to the ray's list slot and a per-ray 64-bit atomicMin
//               on (t order, patch, slot)
//   k_newton_lane  the sparse region: one pair per lane, the lane's own patch record
//   k_resolve   follow-side results: the named neighbour with cNone, per lane; then the reference's
//               in-order scan for the overflow list, sliced over patches -> key
//   k_finish    winner -> BezierIntersection / refraction (overflow rays: their winner re-evaluated)
// For one ray (t order, patch, slot) orders like (t, scanned patch index): the atomicMin winner is the
// reference's strict-< in-order winner (record()).
struct Work {
  uint32_t *ctr;     // [0] follow count, [1] overflow count, [2] rays traced, [3] pairs listed
  uint32_t *hist;    // [nb + 1] pair counts per patch (hist[nb] = 0); 256 bytes after ctr
  unsigned long long *offs;  // [nb + 1] exclusive prefix of bucket_split(hist); offs[nb] = the totals
  uint32_t *cand;    // [kMaxCand][n]
  uint32_t *rank;    // [kMaxCand][n]
  uint32_t *count;   // [n] list length, | kOverflow: the full scan
  unsigned long long *key;  // [n]
  float *slot;       // [kMaxCand][n] x kSlotWords: the hit of ray i's list slot j at j * n + i (AoS, 48 bytes)
  uint2 *pairs;      // [cap + 64 (nb + 1)] pair records (ray | j << 26, patch): dense chunks, then the sparse
                     // region; a follow request adds its side << 30 to the patch word
  uint32_t *fol;     // [cap] follow requests: pair indices
  uint32_t *ovf;     // [n]
  void *cub;
  size_t cub_bytes;
  uint32_t cap;      // kMaxCand * chunk
};
constexpr uint32_t kSlotWords = 12;  // t, point, cos, bary, normal, source patch

// kModePower: kModeStage plus the ray's power -- one weight per ray, multiplied by the Fresnel transmittance
// (patch_math_body.inc fresnel_t) of each successful refraction.  A mode of its own, not a run-time branch of
// kModeStage: the instantiations of the other three modes compile to the code they had.
// kModeSpectral: kModePower with the refractive index read per lane -- ray i carries channel[i], lens l refracts it
// with ri_table[l][channel[i]].  A channel at or above nchan ends the ray at its first surface like a miss (NONE,
// one segment, ray and weight as they came).  Again a mode of its own: the other four compile to the code they had.
// kModeTir: kModeSpectral with total internal reflection (tir_hit_t) -- a ray that cannot leave a lens is mirrored
// and traced against the same lens again, up to max_bounces times per lens.  A mode of its own once more.
// kModeOpl: kModeTir with the ray's optical path length and its length inside glass (opl_leg), two more words per ray.
// A mode of its own again: the other six compile to the code they had.
// kModeMedia: kModeOpl with a medium in front of, between and behind the lenses -- gap_table[l][channel[i]] is the
// index in front of lens l, row `count` the one behind the last lens.  Snell's step, the reflection test, the Fresnel
// term (refract_eta_t, tir_eta_t) and the leg in front of a lens (opl_leg_media) read them.  A mode of its own once
// more: the other seven compile to the code they had.
// The context's table buffer (upload_ri_table): the index table, kModeMedia's gap table kGapPart floats long, then
// kModeAbsorb's two parts of kAbsorbPart floats each, the glass's and the front media's.  A kModeAbsorb job reaches
// both through its gap_table pointer: with a pointer of their own in TraceJob the two non-counting k_trace<kModeAbsorb>
// came out with 36 B of scratch reserved (never accessed), in every order of the tail that was tried (DESIGN (a)).
constexpr uint32_t kGapPart = (kMaxLenses + 1u) * BZR_MAX_CHANNELS, kAbsorbPart = kMaxLenses * BZR_MAX_CHANNELS;
// kModeCoat's table lies behind those, kCoatPart floats from the gap table: rows of BZR_COAT_SAMPLES floats, row
// (2 l + side) nchan + c for surface (l, side) and channel c; kCoatFloats is the worst case, 16 x 64 x 129 (528 KB).
constexpr uint32_t kCoatPart = kGapPart + 2u * kAbsorbPart;
constexpr uint32_t kCoatFloats = 2u * kMaxLenses * BZR_MAX_CHANNELS * BZR_COAT_SAMPLES;
// kModeAbsorb: kModeMedia with Beer-Lambert absorption -- every leg that ends in a refraction or a reflection
// multiplies the weight by att(a len) (leg_attenuation), a = gap_absorb[l][channel[i]] in front of lens l and
// glass_absorb[l][channel[i]] inside it, ahead of the Fresnel gain; a reflection now touches the weight.  A mode of its
// own again: the other eight compile to the code they had.
// kModeGhost: kModeAbsorb with the Fresnel roulette at glass exits (ghost_eta_t) -- a ray that would refract out of a
// lens with bounce budget left reflects with probability 1 - T and otherwise leaves without the T factor; the ray's
// 64-bit number is first_ray + its index in the call.  A mode of its own again: the other nine compile to the code they
// had.  Its one job word, ghost_base, shares kModeHits' `hits` slot of TraceJob: with a field of its own behind gap_table
// the non-counting k_trace<kModeGhost> came out with 36 and 68 B of scratch reserved (never accessed), kModeAbsorb's
// artefact again, and every k_trace of the parent with another kernarg size (DESIGN (a)).
// kModeBidir: the bidirectional walk (include/bzr.h bzr_trace_chain_bidir) -- kModeGhost's words per ray, but the roulette
// runs at every surface (bidir_eta_t) and a ray goes to whichever neighbour lens the surface it left faces, so the lens is
// per lane: the wave picks one (lens, phase) key per round (k_trace below).  Fused and scan only; no staged form.  Its
// three job words, the chain's axis, share kModeRefract's `expected` and `expected_all` slots of TraceJob, as ghost_base
// shares `hits`: TraceJob keeps its size and the older kernels their code.  A mode of its own: the other ten compile to
// the code they had.
// kModeCoat: kModeBidir with tabulated reflectances (include/bzr.h bzr_coating) -- the walk, the schedule and the words
// are kModeBidir's; the step is coat_eta_t, which takes T per lane from fresnel_t or from the surface's row in the
// context's buffer (kCoatPart).  Its one job word, the mask of coated surfaces, rides in the high half of max_bounces
// (the budget is at most BZR_MAX_BOUNCES): TraceJob keeps its size and k_chain_scan its arguments.  A mode of its own:
// the other eleven compile to the code they had.
enum OutMode {
  kModeHits = 0, kModeRefract = 1, kModeStage = 2, kModePower = 3, kModeSpectral = 4, kModeTir = 5, kModeOpl = 6,
  kModeMedia = 7, kModeAbsorb = 8, kModeGhost = 9, kModeBidir = 10,
  kModeCoat = 11
};
constexpr bool has_ghost(int mode) { return mode == kModeGhost; }
constexpr bool has_coat(int mode) { return mode == kModeCoat; }
constexpr bool has_bidir(int mode) { return mode == kModeBidir || has_coat(mode); }
constexpr bool has_absorb(int mode) { return mode == kModeAbsorb || has_ghost(mode) || has_bidir(mode); }
constexpr bool has_media(int mode) { return mode == kModeMedia || has_absorb(mode); }
constexpr bool has_opl(int mode) { return mode == kModeOpl || has_media(mode); }
constexpr bool is_stage(int mode) {
  return mode == kModeStage || mode == kModePower || mode == kModeSpectral || mode == kModeTir || has_opl(mode);
}
constexpr bool has_power(int mode) {
  return mode == kModePower || mode == kModeSpectral || mode == kModeTir || has_opl(mode);
}
constexpr bool has_channels(int mode) { return mode == kModeSpectral || mode == kModeTir || has_opl(mode); }
constexpr bool has_tir(int mode) { return mode == kModeTir || has_opl(mode); }
struct Out {
  float *hits;               // kModeHits: SoA [13][ld]
  float *rays;               // kModeRefract: output rays; kModeStage: rays in flight (in place)
  const uint32_t *expected;  // per ray, or null -> expected_all
  uint32_t expected_all;
  uint32_t *status;
  uint32_t *segments;        // kModeStage, optional
  float ri;
  uint32_t first;            // kModeStage: the chain's first stage -- every ray is alive, its input comes
                             // from the caller's rays and its ray / status / segments are all written here
  float *weight;             // kModePower: the weights in flight [ld] (as rays: in place)
  const float *weight_in;    // kModePower, first stage: the caller's weights, or null -> 1
  const uint8_t *channel;    // kModeSpectral: the rays' channels [ld] (indexed like status and weight)
  const float *ri_row;       // kModeSpectral: this lens's row of the index table [nchan] (device memory)
  uint32_t nchan;
  uint32_t lossless;         // kModeSpectral: the weights stay as they are (the gain counts as 1)
  // kModeTir (channel may be null: every ray is channel 0).  An OUTSIDE stage marks the rays it reflected in `pend`
  // (their status stays INSIDE); a lens's first OUTSIDE stage traces the rays whose status is not NONE, each later
  // one (`bounce_stage`) only the rays whose pend word is set.  The chain's first stage clears both rows.
  uint32_t *pend;            // [ld] 1: reflected by the last OUTSIDE stage, to be traced against this lens again
  uint32_t *bounces;         // [ld] optional: the ray's reflections so far
  uint32_t bounce_stage;     // this stage traces the pending rays only
  uint32_t may_reflect;      // the rays this stage traces have bounce budget left in this lens
  // kModeOpl: the optical path and the glass path in flight [ld], in place like weight.  The chain's first stage
  // writes every ray's two words (opl_in or 0; 0), later stages add the leg of the rays they refracted or reflected.
  float *opl;
  const float *opl_in;       // first stage: the caller's path so far, or null -> 0
  float *glass;              // optional
  // kModeMedia: the rows of the gap table [nchan] in front of this lens and behind it (device memory, like ri_row)
  const float *gap_row, *gap_next;
  // kModeAbsorb: this lens's rows of the two absorption tables [nchan] (device memory): its glass, the medium in front
  const float *glass_absorb, *gap_absorb;
  // kModeGhost: the roulette's base word for index 0 of these rows (ghost_base: ray gi draws with base + golden gi) and
  // this stage's draw number e = 16 lens + reflections so far in it (an OUTSIDE stage that may reflect)
  uint64_t ghost_base;
  uint32_t ghost_e;
};

template <int kMode>
__device__ __forceinline__ void emit(const Out &o, uint32_t ld, uint32_t gi, f3 s, f3 d, const Hit &h, uint32_t patch) {
  if (kMode == kModeHits) {
    store_hit(o.hits, ld, gi, h, patch);
  } else {
    f3 os, od;
    float gain = 1.0f;
    float ri = o.ri;
    bool in_table = true;
    uint32_t col = 0u;  // the ray's column of the tables
    if constexpr (has_channels(kMode)) {
      const uint32_t ch = (has_tir(kMode) && !o.channel) ? 0u : o.channel[gi];
      in_table = ch < o.nchan;
      col = in_table ? ch : 0u;
      ri = o.ri_row[col];
    }
    uint32_t st;
    float nm = ri;  // kModeMedia: the index of the medium this segment's leg lies in
    if constexpr (has_media(kMode)) {
      const bool outside = o.expected_all == BZR_RR_OUTSIDE;
      const float n0 = o.gap_row[col];
      if (!outside) nm = n0;
      if constexpr (has_ghost(kMode)) {
        const bool draws = outside && o.may_reflect && !o.lossless;  // (stage-uniform)
        const float u = draws ? ghost_uniform(o.ghost_base, gi, o.ghost_e) : 0.0f;
        st = ghost_eta_t<true>(h, media_eta(n0, ri, o.gap_next[col], outside), s, d, o.expected_all,
                               in_table && o.may_reflect, draws, u, os, od, gain);
      } else
      st = tir_eta_t<true>(h, media_eta(n0, ri, o.gap_next[col], outside), s, d, o.expected_all, in_table && o.may_reflect,
                           os, od, gain);
    } else if constexpr (has_tir(kMode))
      st = tir_hit_t<true>(h, ri, s, d, o.expected_all, in_table && o.may_reflect, os, od, gain);
    else
      st = refract_hit_t<has_power(kMode)>(h, ri, s, d, o.expected ? o.expected[gi] : o.expected_all, os, od, gain);
    if constexpr (has_channels(kMode)) {
      if (!in_table) st = BZR_RR_NONE;
      if (o.lossless) gain = 1.0f;
    }
    float leg_att = 1.0f;  // kModeAbsorb: the leg's attenuation
    if constexpr (has_opl(kMode)) {  // (st: the expected status, kReflected or NONE; os: the hit's point)
      if (o.first || st != BZR_RR_NONE) {
        float opl = o.first ? (o.opl_in ? o.opl_in[gi] : 0.0f) : o.opl[gi];
        float glass = (o.first || !o.glass) ? 0.0f : o.glass[gi];
        if (st != BZR_RR_NONE) {
          if constexpr (has_absorb(kMode)) {
            const bool outside = o.expected_all == BZR_RR_OUTSIDE;
            const float len = opl_leg_absorb(s, os, nm, outside, opl, glass);
            leg_att = leg_attenuation((outside ? o.glass_absorb : o.gap_absorb)[col], len);
          } else if constexpr (has_media(kMode)) opl_leg_media(s, os, nm, o.expected_all == BZR_RR_OUTSIDE, opl, glass);
          else opl_leg(s, os, ri, o.expected_all == BZR_RR_OUTSIDE, opl, glass);
        }
        o.opl[gi] = opl;
        if (o.glass) o.glass[gi] = glass;
      }
    }
    bool reflected = false;
    if constexpr (has_tir(kMode)) {  // in memory a reflected ray is inside and pending; its weight is not touched
      reflected = st == kReflected;
      if (o.first || o.expected_all == BZR_RR_OUTSIDE) o.pend[gi] = reflected ? 1u : 0u;
      if (o.bounces && (o.first || reflected)) o.bounces[gi] = o.first ? 0u : o.bounces[gi] + 1u;
      if (reflected) st = BZR_RR_INSIDE;
    }
    if (kMode == kModeRefract || st != BZR_RR_NONE || (is_stage(kMode) && o.first)) {
      if (st == BZR_RR_NONE) {
        os = s;
        od = d;
      }
      store_ray(o.rays, ld, gi, os, od);
    }
    o.status[gi] = st;
    if (is_stage(kMode) && o.segments) o.segments[gi] = o.first ? 1u : o.segments[gi] + 1u;
    if constexpr (has_absorb(kMode)) {  // the leg attenuates a reflected ray too; the gain belongs to a refraction only
      if (o.first || st != BZR_RR_NONE) {
        float w = o.first ? (o.weight_in ? o.weight_in[gi] : 1.0f) : o.weight[gi];
        if (st != BZR_RR_NONE) {
          w = w * leg_att;
          if (!reflected) w = w * gain;
        }
        o.weight[gi] = w;
      }
    } else if constexpr (has_power(kMode)) {  // the first stage writes every ray's weight, later ones the refracted rays'
      if (o.first || (st != BZR_RR_NONE && !reflected)) {
        float w = o.first ? (o.weight_in ? o.weight_in[gi] : 1.0f) : o.weight[gi];
        if (st != BZR_RR_NONE) w = w * gain;
        o.weight[gi] = w;
      }
    }
  }
}

// Monotone map of t to uint32 (IEEE total order; -0 canonicalised to +0 so they tie like `<`).
__device__ __forceinline__ uint32_t t_order(float t) {
  uint32_t u = __float_as_uint(t == 0.0f ? 0.0f : t);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint32_t popc64(unsigned long long m) { return (uint32_t)__popcll(m); }
__device__ __forceinline__ bool lane_bit(unsigned long long m, uint32_t lane) { return ((m >> lane) & 1ull) != 0ull; }
// Number of lanes below this one in `mask`.
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// One intersecting pair result: its slot, then the ray's running (t, pair) minimum.  t that cannot
// beat the reference's initial FLT_MAX (NaN, FLT_MAX, +inf) is dropped; -0 ties with +0.
// A staged hit of ray `ray`'s list slot j (candidate patch b; the hit itself may be b's neighbour src after a
// follow): its 48-byte record goes to slot j * n + ray, and the ray's key takes the lexicographic minimum of
// (t order, b, j).  A ray's candidates are distinct patches, so for one ray that orders like the reference's
// (t, scanned patch index) with strict < -- the follow side's hit ranks at its candidate's position, as in
// reference/bezierMesh.cpp:206-227 (oracle orc_mesh_intersect).
// BZR_RECORD_RET (default 1; 0 = the round-4 record): take the key's old value back and write the slot only when
// this pair is the ray's best so far -- the final key's pair always wrote its slot (the minimum is unique), later
// losers skip their 48 bytes; the wave then waits for the atomic before its stores.  cfg5 per 8 M-ray chunk:
// k_newton writes 542 -> 450 MB, k_resolve 41 -> 33 MB (profiles/r05_cfg5_staged_recret.txt); time within noise
// (lone cfg5 +0.4 %, cfg3 -0.1 %; frames in flight cfg5 +0.3 %, cfg3 +1.1 %; profiles/r05_ab_record_ret.jsonl).
#ifndef BZR_RECORD_RET
#define BZR_RECORD_RET 1
#endif
__device__ __forceinline__ void write_slot(float *__restrict__ slot, uint32_t n, uint32_t ray, uint32_t j, const Hit &h,
                                           uint32_t src) {
  float4 *r = reinterpret_cast<float4 *>(slot) + (size_t)3 * ((size_t)j * n + ray);  // AoS: 48 bytes per slot
  r[0] = make_float4(h.t, h.point.x, h.point.y, h.point.z);
  r[1] = make_float4(h.cs, h.bary.x, h.bary.y, h.bary.z);
  r[2] = make_float4(h.normal.x, h.normal.y, h.normal.z, __uint_as_float(src));
}
__device__ __forceinline__ void record(float *__restrict__ slot, uint32_t n, uint32_t ray, uint32_t j, uint32_t b,
                                       const Hit &h, uint32_t src, unsigned long long *key) {
  if (!(h.t < FLT_MAX)) return;
  const unsigned long long k = ((unsigned long long)t_order(h.t) << 32) | (b << 6) | j;
#if BZR_RECORD_RET
  if (!(k < atomicMin(key, k))) return;
#endif
  write_slot(slot, n, ray, j, h, src);
#if !BZR_RECORD_RET
  atomicMin(key, k);
#endif
}

// Word group g of a 64-byte leaf record (planar record, patch index in the last word): q0..q3 of the gate.
__device__ __forceinline__ float4 leaf_q(const u32x16 &r, int g) {
  return make_float4(__uint_as_float(r[4 * g]), __uint_as_float(r[4 * g + 1]), __uint_as_float(r[4 * g + 2]),
                     g == 3 ? 0.0f : __uint_as_float(r[4 * g + 3]));
}

// The always list (bvh.hpp Bvh::always): patches without a proven gate region, gate-tested by every
// wave-segment.  Record k = kAlwaysQuads float4: the 64-byte leaf record, then the wedge pre-test words.
constexpr uint32_t kAlwaysQuads = 8;
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(4))) const u32x8 cu32x8;

// The planar gate of always-listed patch k for the active lanes, behind two exact pre-tests that only
// reject lanes whose gate surely fails (the rejections are strict comparisons, so NaN rejects nothing):
//   1. t = num / cs must be > 0 with |cs| >= 1e-5: decided from the signs of num and cs (no division);
//   2. the float plane point must lie in the patch's wedge (bvh.cpp always_wedge): w.p~ within
//      [L - B|p~| - C(|s|+|p~|), H + ...] at p~ = s + d (num x rcp(cs)) -- ~3 % of cfg5's pairs pass.
// Only then the exact gate (the division and fl(M p)), so the always list costs ~25 VALU per pair
// instead of ~50.  Same candidates as the gate alone.
// `gt` gets the gate's plane distance t for the lanes that pass.
__device__ __forceinline__ bool always_gate_rec(const u32x16 &r, const u32x8 &wq, bool act, f3 s, f3 d, uint32_t &patch,
                                                float &gt) {
  patch = r[15];
  gt = 0.0f;
  const float4 q0 = leaf_q(r, 0);
  const f3 n = mk(q0.x, q0.y, q0.z);
  const float cs = dot(d, n), num = q0.w - dot(n, s);
  bool keep = act & (fabsf(cs) >= 0.00001f) & (((num > 0.0f) & (cs > 0.0f)) | ((num < 0.0f) & (cs < 0.0f)));
  // NaN num / cs: keep (the gate itself decides)
  keep |= act & ((num != num) | (cs != cs));
  if (!__any(keep)) return false;
  const float tt = num * __builtin_amdgcn_rcpf(cs);
  const f3 p = mk(__builtin_fmaf(d.x, tt, s.x), __builtin_fmaf(d.y, tt, s.y), __builtin_fmaf(d.z, tt, s.z));
  const float pm = fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)), sm = fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fabsf(s.z));
  const float w = __builtin_fmaf(__uint_as_float(wq[0]), p.x, __builtin_fmaf(__uint_as_float(wq[1]), p.y, __uint_as_float(wq[2]) * p.z));
  const float slack = __builtin_fmaf(__uint_as_float(wq[5]), pm, __uint_as_float(wq[6]) * (sm + pm));
  keep &= !(w > __uint_as_float(wq[4]) + slack) & !(w < __uint_as_float(wq[3]) - slack);
  if (!__any(keep)) return false;
  return keep & planar_gate(q0, leaf_q(r, 1), leaf_q(r, 2), leaf_q(r, 3), s, d, gt);
}
__device__ __forceinline__ bool always_gate_rec(const u32x16 &r, const u32x8 &wq, bool act, f3 s, f3 d, uint32_t &patch) {
  float gt;
  return always_gate_rec(r, wq, act, s, d, patch, gt);
}
__device__ __forceinline__ bool always_gate(const float4 *always, uint32_t k, bool act, f3 s, f3 d, uint32_t &patch,
                                            float &gt) {
  const u32x16 r = *((const cu32x16 *)(uintptr_t)(always + (size_t)kAlwaysQuads * k));
  const u32x8 wq = *((const cu32x8 *)(uintptr_t)(always + (size_t)kAlwaysQuads * k + 4));
  return always_gate_rec(r, wq, act, s, d, patch, gt);
}
__device__ __forceinline__ bool always_gate(const float4 *always, uint32_t k, bool act, f3 s, f3 d, uint32_t &patch) {
  float gt;
  return always_gate(always, k, act, s, d, patch, gt);
}

// Wave-level pre-test of the always list.  The active rays of a wave form a bundle: origins in the box
// [slo, shi], directions in [dlo, dhi] (wave min / max, once per segment).  Lane j tests always-listed
// patch 64 b + j against the whole bundle in interval arithmetic: the ranges of cs = n.d and num = c - n.s
// over the bundle (widened for the lanes' own float dot products), the plane distance t = num / cs over
// the corners (t > 0 and |cs| >= 1e-5 needed), the plane points P = S + D T, and the wedge of
// always_gate: w.P against [L - B|P| - ..., H + ...].  A patch whose interval misses is gate-failed by every
// ray of the wave; only the survivors (a ballot mask, one bit per patch) take the per-lane tests -- 64
// patches per VALU instruction instead of one.  Every margin rounds outward (u = 2^-24): the lanes' dot
// products 8u, the corner quotients 6u, the points 8u, the wedge product and the bound 64u of (|S| + |P|).
// Non-finite bundles (or t ranges beyond 1e30) keep everything.
// The bundle lives in LDS (13 words per wave: slo, shi, dlo, dhi, finite flag) and is read at its points of
// use (volatile: not hoisted): in registers it stayed live across the fused kernel's walk and cost two
// waves per SIMD of occupancy (69 -> 98 VGPRs).
// Wave min / max by ds_swizzle (xor within 32 lanes; the pattern is an immediate, so no lane-index
// registers -- __shfl_xor's bpermute addresses were hoisted and kept 5 VGPRs live across the whole kernel)
// and the two halves combined through readlane: the result is uniform.
template <int kXor>
__device__ __forceinline__ float swz(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1F | (kXor << 10)));
}
__device__ __forceinline__ float halves(float v, bool mx) {
  const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  return mx ? fmaxf(a, b) : fminf(a, b);
}
__device__ __forceinline__ float wave_minf(float v) {
  v = fminf(v, swz<1>(v));
  v = fminf(v, swz<2>(v));
  v = fminf(v, swz<4>(v));
  v = fminf(v, swz<8>(v));
  v = fminf(v, swz<16>(v));
  return halves(v, false);
}
__device__ __forceinline__ float wave_maxf(float v) {
  v = fmaxf(v, swz<1>(v));
  v = fmaxf(v, swz<2>(v));
  v = fmaxf(v, swz<4>(v));
  v = fmaxf(v, swz<8>(v));
  v = fmaxf(v, swz<16>(v));
  return halves(v, true);
}
// The 12 reductions one after another (a loop that is not unrolled), each stored to the wave's LDS words as
// soon as it is done, so only one is in registers at a time; word 12 = 1 when every box bound is finite
// (false also for an empty bundle, whose boxes are +-inf).  Words 13..21: bundle_setup_swap.
constexpr uint32_t kBundleWords = 22;
__device__ __forceinline__ void bundle_to_lds(bool act, f3 s, f3 d, float *out, uint32_t lane) {
  const float inf = __builtin_inff();
  float m = 0.0f;
#pragma unroll 1
  for (uint32_t k = 0; k < 12u; ++k) {
    const uint32_t a = k % 3u;
    const f3 v = k < 6u ? s : d;
    const float x = a == 0u ? v.x : (a == 1u ? v.y : v.z);
    const bool lo = (k / 3u) % 2u == 0u;
    const float r = lo ? wave_minf(act ? x : inf) : wave_maxf(act ? x : -inf);
    m = fmaxf(m, fabsf(r));
    if (lane == 0u) out[k] = r;
  }
  if (lane == 0u) out[12] = m <= 1e30f ? 1.0f : 0.0f;
  __builtin_amdgcn_wave_barrier();  // the words are read back by every lane of this wave
}
// Floats reduced as order-preserving integers (sign-magnitude flipped to two's complement): a float fminf / fmaxf
// step costs a DPP move, two canonicalising v_max and the min (IEEE mode), an integer step is one v_min_i32 with
// the DPP operand folded in.  NaN lanes contribute the identity (as fminf / fmaxf ignore them); -0 orders below +0
// (either is a valid bound).  The map is its own inverse.
__device__ __forceinline__ int float_order(float x) {
  const int b = __float_as_int(x);
  return b ^ ((b >> 31) & 0x7FFFFFFF);
}
// The whole bundle, the 12 reductions as one reduce-scatter on gfx950's half-wave swaps (no LDS round trips):
// words 0..12 as bundle_to_lds, and for the bundle walk 13..21 -- per axis rl = 1 / Dl', rh = 1 / Dh' and mixed = 1
// when Dl' < 0 < Dh', where Dl' <= Dl and Dh' >= Dh are the direction bounds moved away from zero (|D'| >= 1e-20: a
// wider direction box, so a superset of the rays).  The words are, bit for bit, those of twelve separate min / max
// reductions followed by one lane's scalar code (tests/test_gpu_bundle_setup.py holds both statements); the host
// mirrors (bvh.cpp bundle_box_h, bundle_spread_h) predict the walk from them.
// One ordered integer per component: max x = -min(-x) and float_order(-x) = ~float_order(x), so all twelve
// reductions are v_min_i32 -- the maxima as minima of ~order -- and values of either kind share a register.  An
// inactive lane contributes order(+inf) = ~order(-inf) = 0x7F800000 to both, a NaN lane INT_MAX (= ~INT_MIN) to both.
// v_permlane32_swap on (min s_k, min d_k) and on (max s_k, max d_k), then min: the low half of a register reduces
// the origin's bound, the high half the direction's (12 -> 6 registers).  v_permlane16_swap on the (min, max) pairs,
// then min: register k's rows 0..3 reduce Sl_k, Sh_k, Dl_k, Dh_k -- words k, 3 + k, 6 + k, 9 + k (6 -> 3).  Four
// row_ror steps leave every lane of a row with the row's result; the rows of maxima (1 and 3) flip the sign back.
// The row leaders store words 0..11; word 12 is an exponent test on every lane voted into a scalar (fmaxf skips a
// NaN bound, so only magnitudes in (1e30, inf] clear it); lanes 0..5 then read one direction bound each and write
// its clamped, correctly rounded reciprocal, lanes 0..2 the mixed flags (lo < 0 iff !(Dl > 1e-20), hi > 0 iff
// !(Dh < -1e-20): the clamps' own tests).
__device__ __forceinline__ float bundle_setup_swap(bool act, f3 s, f3 d, float *out, uint32_t lane) {
  asm volatile("" : "+v"(lane));  // (laundered, as in bundle_batch: no lane-derived constant outlives the setup)
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const float c[6] = {s.x, s.y, s.z, d.x, d.y, d.z};
  const int idle = act ? INT_MAX : 0x7F800000;
  int mn[6], mx[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const bool in = act && c[i] == c[i];
    const int o = float_order(c[i]);
    mn[i] = in ? o : idle;
    mx[i] = in ? ~o : idle;
  }
  // (the steps of the registers side by side: a swap or a DPP read then lies behind the write it reads, and the
  // hazard recogniser pads nothing)
  u32x2 p[6];
  int h[6], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p[k] = __builtin_amdgcn_permlane32_swap((unsigned)mn[k], (unsigned)mn[3 + k], false, false);
    p[3 + k] = __builtin_amdgcn_permlane32_swap((unsigned)mx[k], (unsigned)mx[3 + k], false, false);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) h[k] = min((int)p[k][0], (int)p[k][1]);
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = __builtin_amdgcn_permlane16_swap((unsigned)h[k], (unsigned)h[3 + k], false, false);
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = min((int)p[k][0], (int)p[k][1]);
#define BZR_ROR_STEP(ctrl)                      \
  _Pragma("unroll") for (int k = 0; k < 3; ++k) \
      w[k] = min(w[k], __builtin_amdgcn_update_dpp(INT_MAX, w[k], ctrl, 0xF, 0xF, false));
  BZR_ROR_STEP(0x128)  // row_ror:8 (every lane has a source: the identity is never read)
  BZR_ROR_STEP(0x124)  // row_ror:4
  BZR_ROR_STEP(0x122)  // row_ror:2
  BZR_ROR_STEP(0x121)  // row_ror:1
#undef BZR_ROR_STEP
  const int sign = (int)((lane & 16u) << 27);
  int b[3];
  bool huge = false;  // a bound with 1e30 < |x| <= inf (1e30f = 0x7149F2CA)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    b[k] = (w[k] ^ ((w[k] >> 31) & 0x7FFFFFFF)) ^ sign;
    huge |= ((uint32_t)(b[k] & 0x7FFFFFFF) - 0x7149F2CBu) <= 0x7F800000u - 0x7149F2CBu;
  }
  const bool finite = __ballot(huge) == 0ull;
  if ((lane & 15u) == 0u) {
    float *o = out + 3u * (lane >> 4);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = __int_as_float(b[k]);
    if (lane == 0u) out[12] = finite ? 1.0f : 0.0f;
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < 6u) {  // lane a: Dl_a -> rl_a, lane 3 + a: Dh_a -> rh_a
    const float x = out[6u + lane];
    const float lo = x > 1e-20f ? x : fminf(x, -1e-20f), hi = x < -1e-20f ? x : fmaxf(x, 1e-20f);
    out[13u + lane] = 1.0f / (lane < 3u ? lo : hi);
    if (lane < 3u) out[19u + lane] = (!(x > 1e-20f) && !(out[9u + lane] < -1e-20f)) ? 1.0f : 0.0f;
  }
  __builtin_amdgcn_wave_barrier();
  // the walk choice's width measure: the widest direction interval (bvh.cpp bundle_spread_h), read back from the
  // words (into a scalar: the walk's control flow hangs on it and must stay uniform)
  const float spread = fmaxf(fmaxf(out[9] - out[6], out[10] - out[7]), out[11] - out[8]);
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(spread)));
}
// Wave-bundle box test (the bundle walk): false only when no ray s + t d, t >= 0, with s in [Sl, Sh] and d in
// [Dl', Dh'] (per axis, so a superset of the wave's active rays) meets the box.  On axis a the reachable
// coordinates at time t are [Sl + t Dl', Sh + t Dh'], which meet [lo, hi] iff Sl + t Dl' <= hi and
// Sh + t Dh' >= lo: with A = (hi - Sl) / Dl' and B = (lo - Sh) / Dh', t in [B, A] when 0 < Dl' (and B <= A
// whenever A >= 0, so [min, max] decides alike), t in [A, B] when Dh' < 0 (same), and t >= max(A, B) when
// the axis is mixed.  A and B carry at most ~3u relative rounding (one subtraction, the rounded reciprocal,
// one product); the bounds are widened by 8u relative + 2^-126 before tnear <= tfar and tfar >= 0, and a
// NaN keeps the box.  The per-lane walk's boxes are padded for the lanes' own float slab test; this test
// is conservative against the exact rays, so it keeps every box an exact ray of the wave meets (host
// mirror: bvh.cpp bundle_box_h, checked by tests/test_culling_conservative.py).
__device__ __forceinline__ bool bundle_box(const float *B, float4 lo, float4 hi) {
  float tn = -__builtin_inff(), tf = __builtin_inff();
  const float l3[3] = {lo.x, lo.y, lo.z}, h3[3] = {hi.x, hi.y, hi.z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float A = (h3[a] - B[a]) * B[13 + a], Bq = (l3[a] - B[3 + a]) * B[16 + a];
    const float mn = fminf(A, Bq), mx = fmaxf(A, Bq);
    const bool mix = B[19 + a] > 0.0f;
    tn = fmaxf(tn, mix ? mx : mn);
    tf = fminf(tf, mix ? __builtin_inff() : mx);
  }
  tn -= fabsf(tn) * 0x1p-21f + 0x1p-126f;
  tf += fabsf(tf) * 0x1p-21f + 0x1p-126f;
  return !(B[12] > 0.0f) | (!(tn > tf) & !(tf < 0.0f));
}
// One batch of the bundle walk (k_trace and k_traverse): the k <= 16 axis-aligned nodes on top of the wave's
// LDS stack `stk` (the top one is axis-aligned; an oriented-box node below it ends the batch), lane 4 q + c
// taking node q's child c from the AoS child records `kids`.  Hit inner children are pushed, hit leaf slots
// written to `pend` (returns how many).  Returns with `full` set when the stack could not take every hit
// child (those subtrees are dropped: the caller sends its active lanes to the full scan).
// kSlots = 16: the same over the two-level records `wide` (4 nodes per batch, lane 16 q + s taking slot s of
// node q), so a batch descends two levels of the tree.
// seen (uniform; null for a tree without split leaf boxes): the wave-segment's bit set over leaf slots.  A split
// tree names a slot once per cell box, and a bundle that straddles cells reaches it more than once: a hit leaf is
// queued only if its bit was clear (LDS atomic or with return, so of two lanes of one batch naming the same slot
// exactly one keeps it).  Slots are below kSplitSlotCap (build_bvh splits no larger mesh).
template <int kCap, uint32_t kSlots = 4>
__device__ __forceinline__ uint32_t bundle_batch(const float4 *kids, uint32_t *stk, int &sp, uint32_t *pend,
                                                 const float *B, uint32_t lane, bool &full, uint32_t &knodes,
                                                 uint32_t base = 0u, uint32_t *seen = nullptr) {
  // (the lane index laundered: lane-derived addresses hoisted out of the walk stayed live across the Newton
  // passes of k_trace and cost it a wave of occupancy)
  asm volatile("" : "+v"(lane));
  constexpr uint32_t kShift = kSlots == 16u ? 4u : 2u;
  constexpr int kNodes = 64 / (int)kSlots;
  const uint32_t q = lane >> kShift, c = lane & (kSlots - 1u);
  // at most (kCap - sp) / (kSlots - 1) nodes (at least one), so their <= kSlots children each fit: the stack
  // overflows only from a nearly full stack (a wide bundle; the walk choice sends those to the per-lane walk)
  const int room = (kCap - sp) / (int)(kSlots - 1u), avail = sp < kNodes ? sp : kNodes;
  const uint32_t kmax = (uint32_t)(avail < room ? avail : (room > 1 ? room : 1));
  const uint32_t nd = q < kmax ? stk[sp - 1 - (int)q] : 0u;
  const unsigned long long ob = __ballot(c == 0u && q < kmax && (nd & bzr_host::kObbFlag));
  const uint32_t k = ob ? (uint32_t)__builtin_ctzll(ob) >> kShift : kmax;
  const bool slot = q < k;
  const float4 *kp = kids + ((size_t)(slot ? nd : 0u) * kSlots + c) * 2u;
  const float4 lo = kp[0], hi = kp[1];
  const uint32_t ref = __float_as_uint(lo.w);
  const bool hit = slot && ref != bzr_host::kEmptyChild && bundle_box(B, lo, hi);
  const bool isleaf = (ref & bzr_host::kLeafFlag) != 0u;
  bool fresh = hit && isleaf;
  if (seen) {
    const uint32_t sl = ref & ~bzr_host::kLeafFlag, bit = 1u << (sl & 31u);
    if (fresh && sl < bzr_host::kSplitSlotCap) fresh = (atomicOr(&seen[sl >> 5], bit) & bit) == 0u;
  }
  const unsigned long long lm = __ballot(fresh), im = __ballot(hit && !isleaf);
  knodes = k;
  sp -= (int)k;
  const int below = (int)lanes_below(im);
  if (hit && !isleaf && sp + below < kCap) stk[sp + below] = ref;
  const int ni = (int)popc64(im);
  full = sp + ni > kCap;
  sp = full ? kCap : sp + ni;
  if (fresh) pend[base + lanes_below(lm)] = ref & ~bzr_host::kLeafFlag;
  return popc64(lm);
}
// Interval of n.x over x in [lo, hi] (n fixed).
__device__ __forceinline__ void ivdot(f3 n, f3 lo, f3 hi, float &a, float &b) {
  a = (n.x >= 0.0f ? n.x * lo.x : n.x * hi.x) + (n.y >= 0.0f ? n.y * lo.y : n.y * hi.y) + (n.z >= 0.0f ? n.z * lo.z : n.z * hi.z);
  b = (n.x >= 0.0f ? n.x * hi.x : n.x * lo.x) + (n.y >= 0.0f ? n.y * hi.y : n.y * lo.y) + (n.z >= 0.0f ? n.z * hi.z : n.z * lo.z);
}
__device__ __forceinline__ float absmax(float lo, float hi) { return fmaxf(fabsf(lo), fabsf(hi)); }
// false: no ray of the bundle (LDS words bl) can pass always-listed patch k's gate.
__device__ __forceinline__ bool always_bundle_keep_rec(float4 q0, float4 w0, float4 w1, const float *bl) {
  const float *B = bl;
  if (!(B[12] > 0.0f)) return true;
  constexpr float u = 0x1p-24f;
  const f3 n = mk(q0.x, q0.y, q0.z);
  float csl, csh, nsl, nsh;
  ivdot(n, mk(B[6], B[7], B[8]), mk(B[9], B[10], B[11]), csl, csh);
  ivdot(n, mk(B[0], B[1], B[2]), mk(B[3], B[4], B[5]), nsl, nsh);
  const float mc = 8.0f * u * (fabsf(n.x) * absmax(B[6], B[9]) + fabsf(n.y) * absmax(B[7], B[10]) + fabsf(n.z) * absmax(B[8], B[11]));
  const float ms = 8.0f * u * (fabsf(n.x) * absmax(B[0], B[3]) + fabsf(n.y) * absmax(B[1], B[4]) + fabsf(n.z) * absmax(B[2], B[5]) + fabsf(q0.w));
  csl -= mc;
  csh += mc;
  const float numl = (q0.w - nsh) - ms, numh = (q0.w - nsl) + ms;
  if (csl > -0.00001f && csh < 0.00001f) return false;  // |cs| < 1e-5 for every ray
  if (!(csl > 0.0f || csh < 0.0f)) return true;          // cs of either sign: t unbounded
  const float r1 = __builtin_amdgcn_rcpf(csl), r2 = __builtin_amdgcn_rcpf(csh);
  const float a1 = numl * r1, a2 = numl * r2, a3 = numh * r1, a4 = numh * r2;
  float tlo = fminf(fminf(a1, a2), fminf(a3, a4)), thi = fmaxf(fmaxf(a1, a2), fmaxf(a3, a4));
  tlo -= 6.0f * u * fabsf(tlo);
  thi += 6.0f * u * fabsf(thi);
  if (!(thi <= 1e30f)) return true;  // huge or NaN: no bound
  if (thi <= 0.0f) return false;     // t > 0 for no ray
  tlo = fmaxf(tlo, 0.0f);
  // plane points P = S + D T and the wedge w.P, one axis at a time
  float wlo = 0.0f, whi = 0.0f, pm0 = 0.0f, smax = 0.0f, wabs = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float dl = B[6 + a], dh = B[9 + a], sl = B[a], sh = B[3 + a];
    const float x1 = dl * tlo, x2 = dl * thi, x3 = dh * tlo, x4 = dh * thi;
    const float pl = sl + fminf(fminf(x1, x2), fminf(x3, x4)), ph = sh + fmaxf(fmaxf(x1, x2), fmaxf(x3, x4));
    const float wa = a == 0 ? w0.x : (a == 1 ? w0.y : w0.z);
    wlo += wa >= 0.0f ? wa * pl : wa * ph;
    whi += wa >= 0.0f ? wa * ph : wa * pl;
    wabs += fabsf(wa);
    pm0 = fmaxf(pm0, absmax(pl, ph));
    smax = fmaxf(smax, absmax(sl, sh));
  }
  // the points' own rounding e on every axis moves w.P by at most |w|_1 e; the wedge product's and the
  // bound's rounding are inside 64 u (|S| + |P|)
  const float e = 8.0f * u * (smax + pm0);
  const float pmax = pm0 + e;
  wlo -= wabs * e;
  whi += wabs * e;
  const float slack = w1.y * pmax + (w1.z + 64.0f * u) * (smax + pmax);
  return !(wlo > w1.x + slack) & !(whi < w0.w - slack);
}
__device__ __forceinline__ bool always_bundle_keep(const float4 *always, uint32_t k, uint32_t n_always, const float *bl) {
  if (k >= n_always) return false;
  const float4 *a = always + (size_t)kAlwaysQuads * k;
  return always_bundle_keep_rec(a[0], a[4], a[5], bl);
}

// Wave-level pre-test of a tree leaf's planar gate (the bundle walk's queued leaves, one per lane): false
// only when no ray of the bundle (LDS words bl: origins [Sl, Sh], directions [Dl, Dh]) can pass the gate of
// planar record q0..q3 (planar_gate).  The interval steps and margins of always_bundle_keep (cs and num with
// the lanes' dot-product rounding, the corner quotients of t widened 6u -- v_rcp_f32 --, the plane points P =
// S + D T widened by e = 8u (|S| + |P|)), then the gate's own tests over the intervals: t > max(0, -hin,
// hout) for some ray, and each barycentric row b_k = M_k P (M_k . [Pl, Ph]) within [0, 1] widened by
// |M_k|_1 (e + 8u |P|) (the lanes' fl(M p) rounding is <= 3u |M_k|_1 |p|, the interval sums' own <= 3u).
// Host mirror: bvh.cpp bundle_gate_keep_h (tests/test_culling_conservative.py).
__device__ __forceinline__ bool bundle_gate_keep(const float *B, float4 q0, float4 q1, float4 q2, float4 q3) {
  if (!(B[12] > 0.0f)) return true;
  constexpr float u = 0x1p-24f;
  const f3 n = mk(q0.x, q0.y, q0.z);
  float csl, csh, nsl, nsh;
  ivdot(n, mk(B[6], B[7], B[8]), mk(B[9], B[10], B[11]), csl, csh);
  ivdot(n, mk(B[0], B[1], B[2]), mk(B[3], B[4], B[5]), nsl, nsh);
  const float mc = 8.0f * u * (fabsf(n.x) * absmax(B[6], B[9]) + fabsf(n.y) * absmax(B[7], B[10]) + fabsf(n.z) * absmax(B[8], B[11]));
  const float ms = 8.0f * u * (fabsf(n.x) * absmax(B[0], B[3]) + fabsf(n.y) * absmax(B[1], B[4]) + fabsf(n.z) * absmax(B[2], B[5]) + fabsf(q0.w));
  csl -= mc;
  csh += mc;
  const float numl = (q0.w - nsh) - ms, numh = (q0.w - nsl) + ms;
  if (csl > -0.00001f && csh < 0.00001f) return false;  // |cs| < 1e-5 for every ray
  if (!(csl > 0.0f || csh < 0.0f)) return true;          // cs of either sign: t unbounded
  const float r1 = __builtin_amdgcn_rcpf(csl), r2 = __builtin_amdgcn_rcpf(csh);
  const float a1 = numl * r1, a2 = numl * r2, a3 = numh * r1, a4 = numh * r2;
  float tlo = fminf(fminf(a1, a2), fminf(a3, a4)), thi = fmaxf(fmaxf(a1, a2), fmaxf(a3, a4));
  tlo -= 6.0f * u * fabsf(tlo);
  thi += 6.0f * u * fabsf(thi);
  if (!(thi <= 1e30f)) return true;                                   // huge or NaN: no bound
  if (thi <= fmaxf(fmaxf(-q1.x, q1.y), 0.0f)) return false;          // t > max(0, -hin, hout) for no ray
  tlo = fmaxf(tlo, 0.0f);
  float pl[3], ph[3], pm0 = 0.0f, smax = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float dl = B[6 + a], dh = B[9 + a], sl = B[a], sh = B[3 + a];
    const float x1 = dl * tlo, x2 = dl * thi, x3 = dh * tlo, x4 = dh * thi;
    pl[a] = sl + fminf(fminf(x1, x2), fminf(x3, x4));
    ph[a] = sh + fmaxf(fmaxf(x1, x2), fmaxf(x3, x4));
    pm0 = fmaxf(pm0, absmax(pl[a], ph[a]));
    smax = fmaxf(smax, absmax(sl, sh));
  }
  const float e = 8.0f * u * (smax + pm0), ep = e + 8.0f * u * pm0;
  const f3 P0 = mk(pl[0], pl[1], pl[2]), P1 = mk(ph[0], ph[1], ph[2]);
  const f3 row[3] = {mk(q1.z, q1.w, q2.x), mk(q2.y, q2.z, q2.w), mk(q3.x, q3.y, q3.z)};
  bool keep = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float lo, hi;
    ivdot(row[k], P0, P1, lo, hi);
    const float eb = (fabsf(row[k].x) + fabsf(row[k].y) + fabsf(row[k].z)) * ep + 1e-30f;
    keep &= !(hi + eb < 0.0f) & !(lo - eb > 1.0f);
  }
  return keep;
}

// BZR_TRAV_PHASES (diagnostic build, default 0): k_traverse stamps s_memtime at its phase boundaries and, with
// device counters on, adds each wave's cycles per phase to counter slots (their own counts are small beside
// them): node_visits <- setup (ray loads, bundle reductions), leaf_fetches <- the queued leaves' per-lane
// gates, gate_tests <- the walk's batches and leaf pre-tests, overflow_rays <- the per-lane walk, follows <-
// the always list, segments <- the ranking (variant travph: scripts/ab.py prints them as its counters; the
// stamps cost ~4 %).
#ifndef BZR_TRAV_PHASES
#define BZR_TRAV_PHASES 0
#endif
#if BZR_TRAV_PHASES
#define BZR_PHASE(k)                                          \
  {                                                           \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    ph_acc[ph_cur] += now_ - ph_t;                            \
    ph_t = now_;                                              \
    ph_cur = (k);                                             \
  }
#else
#define BZR_PHASE(k)
#endif
// The lanes whose gate of patch b passed list it as their next candidate (while the list has room; a lane
// past kMaxCand overflows to the full scan).  (Counting the listing lanes into b's histogram word right here --
// b is wave-uniform, so one atomic without return per wave -- and ranking the pairs in k_place instead of
// after the walk: k_traverse -1.6 % on cfg5 and -9 % on cfg3, but k_place's grouped ranking atomics cost more
// than that, cfg3 frames +7.6 %; profiles/r04_ab_rank_late.jsonl.)
__device__ __forceinline__ void list_candidate(bool pass, uint32_t b, const Work &w, uint32_t n, uint32_t i,
                                               uint32_t &cnt) {
  const bool lst = pass && cnt < kMaxCand;
  if (lst) w.cand[(size_t)cnt * n + i] = b;
  if (pass) cnt = cnt < kMaxCand ? cnt + 1 : (cnt | kOverflow);
}
// Candidate search.  `alive` (optional): a ray is traced iff alive[off + i] != BZR_RR_NONE.
// One wave's 64 rays i (lane l of the wave holds ray i); `stk` is the wave's LDS stack.
template <int kBlk, int kAblock, bool kFast>
__device__ __forceinline__ void traverse_rays(const MeshView &m, const float *__restrict__ rays, uint32_t ld,
                                              uint32_t off, const uint32_t *__restrict__ alive, uint32_t n,
                                              const Work &w, unsigned long long *counters, uint32_t i, uint32_t *stk,
                                              float *bl, uint32_t *pend, uint32_t *raw, float *ubl = nullptr,
                                              unsigned long long *akeep = nullptr) {
#if BZR_TRAV_PHASES
  unsigned long long ph_acc[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, ph_t = __builtin_amdgcn_s_memtime();
  uint32_t ph_cur = 0;
#endif
  uint32_t c_nodes = 0, c_leaves = 0, c_gates = 0;  // work counters (with counters on; wave-uniform)
  bool active = i < n && (alive == nullptr || alive[off + i] != BZR_RR_NONE);
  f3 s = mk(0.0f, 0.0f, 0.0f), d = s;
  if (i < n) load_ray(rays, ld, off + i, s, d);
  uint32_t cnt = 0;
  // gate-region boxes hold for ray origins within s_max (bvh.cpp); farther rays take the full scan
  if (active && !(fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fabsf(s.z)) <= m.s_max)) {
    cnt |= kOverflow;
    active = false;
  }
  // tree tier, wave-uniform: the near tree's tighter boxes hold when every active ray starts within s_near
  const bool far_ray = active && !(fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fabsf(s.z)) <= m.s_near);
  const bool near_tier = !__any(far_ray);
  const bzr_host::Bvh4Node *nodes = near_tier ? m.nodes_near : m.nodes;
  const bzr_host::Bvh4ObbNode *obb = near_tier ? m.obb_near : m.obb;
  const float4 *leaf = near_tier ? m.leaf_near : m.leaf;
  // (the per-lane walk's reciprocals: that walk never runs after the bundle walk, which ends with an empty
  // stack, but dropping them here put k_traverse<256, 1> at 3 VGPR spills (scratch) instead of 0 -- the
  // register allocator is sensitive to it; kept)
  const f3 inv = mk(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
  const f3 sinv = mk(s.x * inv.x, s.y * inv.y, s.z * inv.z);
  int sp = 0;  // the node to visit next stays in a scalar register; the other hit children go to stk
  uint32_t next = (m.n > 0 && __any(active)) ? 0u : 0xFFFFFFFFu;
  unsigned long long next_hm = 0ull;
  // the bundle walk (trace_segment's): batches of up to 16 nodes against the wave's ray bundle, hit leaves
  // queued in pend and gate-tested by every active lane
  const bool walk = next != 0xFFFFFFFFu;  // (the bundle words are then in bl, for the always list too)
  bool bwalk = false;                    // the walk choice (trace_segment's)
  bool narrow = false;                   // else every node is tested per lane (as oriented-box nodes are)
  if (walk) {
    narrow = bundle_setup_swap(active, s, d, bl, threadIdx.x & 63u) <= kBundleSpread;
    if ((threadIdx.x & 63u) == 0u) stk[0] = 0u;
    sp = 1;
    next = 0xFFFFFFFFu;
    bwalk = true;
  }
  const float4 *wide = near_tier ? m.wide_near : m.wide;
  uint32_t npend = 0, pi = 0;  // leaves queued in pend, next to gate-test (uniform)
  uint32_t nraw = 0;  // leaves queued in raw, not yet pre-tested
  // the always list's block pre-test (every thread of the block gets here: no early exit above)
  if constexpr (kAblock != 0) {
    if (!walk) bundle_setup_swap(active, s, d, bl, threadIdx.x & 63u);  // (an empty wave's bundle is the identity)
    __syncthreads();
    if (threadIdx.x < 13u) {  // the union over the block's waves with rays (bl - wave * kBundleWords: wave 0's)
      const float *b0 = bl - (threadIdx.x >> 6) * kBundleWords;
      const uint32_t k = threadIdx.x;
      float v = k < 12u ? ((k % 6u) < 3u ? __builtin_inff() : -__builtin_inff()) : 1.0f;
      bool any = false;
      for (uint32_t q = 0; q < (uint32_t)kBlk / 64u; ++q) {
        const float *bq = b0 + q * kBundleWords;
        if (!(bq[0] <= bq[3])) continue;  // no active ray in wave q
        any = true;
        const float x = bq[k];
        v = k == 12u ? fminf(v, x) : ((k % 6u) < 3u ? fminf(v, x) : fmaxf(v, x));
      }
      ubl[k] = (k == 12u && !any) ? 0.0f : v;
    }
    __syncthreads();
    for (uint32_t base = 0; base < m.n_always; base += kBlk) {
      const unsigned long long km = __ballot(always_bundle_keep(m.always, base + threadIdx.x, m.n_always, ubl));
      if ((threadIdx.x & 63u) == 0u) akeep[(base + threadIdx.x) >> 6] = km;
    }
    __syncthreads();
  }
  while (bwalk) {
    if (pi < npend) {
      BZR_PHASE(1)
      // two queued leaves per step: both 64-byte records in flight together (one wait for two round trips)
      const bool two = pi + 1u < npend;
      const uint32_t slot0 = __builtin_amdgcn_readfirstlane(pend[pi]);
      const uint32_t slot1 = __builtin_amdgcn_readfirstlane(pend[two ? pi + 1u : pi]);
      pi += two ? 2u : 1u;
      u32x16 r0, r1;
      asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                   : "=&s"(r0), "=&s"(r1)
                   : "s"(leaf + 4u * slot0), "s"(leaf + 4u * slot1));
      if (counters) {
        c_leaves += two ? 2u : 1u;
        c_gates += (two ? 2u : 1u) * (uint32_t)__popcll(__ballot(active));
      }
      list_candidate(active & planar_gate(leaf_q(r0, 0), leaf_q(r0, 1), leaf_q(r0, 2), leaf_q(r0, 3), s, d),
                     r0[15], w, n, i, cnt);
      if (two)
        list_candidate(active & planar_gate(leaf_q(r1, 0), leaf_q(r1, 1), leaf_q(r1, 2), leaf_q(r1, 3), s, d),
                       r1[15], w, n, i, cnt);
      continue;
    }
    BZR_PHASE(2)
    if (sp == 0 || nraw > 64u) {  // the queued leaves' wave-level gate pre-test: the survivors go to pend
      if (nraw == 0u) break;
      pi = npend = 0;
      for (uint32_t j0 = 0; j0 < nraw; j0 += 64u) {
        const uint32_t j = j0 + (threadIdx.x & 63u);
        uint32_t slot = 0u;
        bool keep = false;
        if (j < nraw) {
          slot = raw[j];
          const float4 *lq = leaf + 4u * slot;
          keep = bundle_gate_keep(bl, lq[0], lq[1], lq[2], lq[3]);
        }
        const unsigned long long km = __ballot(keep);
        if (keep) pend[npend + lanes_below(km)] = slot;
        npend += (uint32_t)__popcll(km);
      }
      nraw = 0u;
      continue;
    }
    uint32_t *qbuf = raw;  // where this step queues its leaves
    uint32_t &qn = nraw;
    const uint32_t top = __builtin_amdgcn_readfirstlane(stk[sp - 1]);
    if (!narrow || (top & bzr_host::kObbFlag)) {  // one node, its children tested by each lane's own ray
      --sp;
      if (counters) ++c_nodes;
      bool hit[4];
      uint32_t ch[4];
      // (the reciprocals computed here, not kept from the segment's start: wide waves are rare, and 6
        // registers live across the Newton passes would cost occupancy)
        const f3 linv = mk(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
        node_children(nodes, obb, top, active, s, d, mk(s.x * linv.x, s.y * linv.y, s.z * linv.z), linv, hit, ch);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned long long hm = __ballot(hit[c]);
        if (hm == 0ull) continue;
        if (ch[c] & bzr_host::kLeafFlag) {
          if ((threadIdx.x & 63u) == 0u) qbuf[qn] = ch[c] & ~bzr_host::kLeafFlag;
          ++qn;
        } else if (sp < kStack) {
          if ((threadIdx.x & 63u) == 0u) stk[sp] = ch[c];
          ++sp;
        } else if ((hm >> (threadIdx.x & 63u)) & 1ull) {
          cnt |= kOverflow;  // stack exhausted: full scan
        }
      }
      continue;
    }
    bool full;
    uint32_t k;
    qn += bundle_batch<kStack, kWideSlots>(wide, stk, sp, qbuf, bl, threadIdx.x & 63u, full, k, qn);
    if (full && active) cnt |= kOverflow;  // stack exhausted: every active lane takes the full scan
    if (counters) c_nodes += k;
  }
  BZR_PHASE(3)
  while (next != 0xFFFFFFFFu || sp > 0) {  // the per-lane walk
    const uint32_t node = next != 0xFFFFFFFFu ? next : __builtin_amdgcn_readfirstlane(stk[--sp]);
    next = 0xFFFFFFFFu;
    if (counters) ++c_nodes;
    bool hit[4];
    uint32_t ch[4];
    node_children(nodes, obb, node, active, s, d, sinv, inv, hit, ch);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned long long hm = __ballot(hit[c]);
      if (hm == 0ull) continue;
      if (ch[c] & bzr_host::kLeafFlag) {
        const u32x16 r = *((const cu32x16 *)(uintptr_t)leaf + (ch[c] & ~bzr_host::kLeafFlag));
        const float4 q0 = make_float4(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3]));
        const float4 q1 = make_float4(__uint_as_float(r[4]), __uint_as_float(r[5]), __uint_as_float(r[6]), __uint_as_float(r[7]));
        const float4 q2 = make_float4(__uint_as_float(r[8]), __uint_as_float(r[9]), __uint_as_float(r[10]), __uint_as_float(r[11]));
        const float4 q3 = make_float4(__uint_as_float(r[12]), __uint_as_float(r[13]), __uint_as_float(r[14]), 0.0f);
        if (counters) {
          ++c_leaves;
          c_gates += (uint32_t)__popcll(hm);
        }
        list_candidate(hit[c] & planar_gate(q0, q1, q2, q3, s, d), r[15], w, n, i, cnt);
      } else {
        if (next != 0xFFFFFFFFu) {
          if (sp < kStack) stk[sp++] = next;
          else if ((next_hm >> (threadIdx.x & 63u)) & 1ull) cnt |= kOverflow;  // stack exhausted: full scan
        }
        next = ch[c];
        next_hm = hm;
      }
    }
  }
  // the always list (patches without a proven gate region, bvh.cpp): gate-tested for every active ray
  BZR_PHASE(4)
  if (m.n_always && __any(active)) {
    if (!walk)  // (the bundle walk built it already)
      bundle_to_lds(active, s, d, bl, threadIdx.x & 63u);
    if constexpr (kAblock != 0) {
      const uint32_t words = (m.n_always + 63u) / 64u;
      for (uint32_t q = 0; q < words; ++q) {
        for (unsigned long long am = akeep[q]; am; am &= am - 1ull) {
          uint32_t b;
          if (counters) {
            ++c_leaves;
            c_gates += (uint32_t)__popcll(__ballot(active));
          }
          const bool pass = always_gate(m.always, q * 64u + __builtin_ctzll(am), active, s, d, b);
          list_candidate(pass, b, w, n, i, cnt);
        }
      }
    } else
    for (uint32_t ab = 0; ab * 64u < m.n_always; ++ab) {
      unsigned long long am = __ballot(always_bundle_keep(m.always, ab * 64u + (threadIdx.x & 63u), m.n_always, bl));
      for (; am; am &= am - 1ull) {
        uint32_t b;
        if (counters) {
          ++c_leaves;
          c_gates += (uint32_t)__popcll(__ballot(active));
        }
        const bool pass = always_gate(m.always, ab * 64u + __builtin_ctzll(am), active, s, d, b);
        list_candidate(pass, b, w, n, i, cnt);
      }
    }

  }
  if (counters) {  // rays traced (one atomic per wave: on one address, so only with counters on)
    const unsigned long long traced = __ballot(i < n && (alive == nullptr || alive[off + i] != BZR_RR_NONE));
    if ((threadIdx.x & 63u) == 0 && traced) atomicAdd(&w.ctr[2], (uint32_t)__popcll(traced));
    // walk work (bzr_ctx_counters node_visits / leaf_fetches / gate_tests), spread over the replicas
    const uint32_t lane = threadIdx.x & 63u, rep = (i >> 6) % kCounterReplicas;
    const uint32_t v = lane == 0u ? c_nodes : (lane == 1u ? c_leaves : c_gates);
    const uint32_t which = lane == 0u ? BZR_COUNTER_NODE_VISITS : (lane == 1u ? BZR_COUNTER_LEAF_FETCHES : BZR_COUNTER_GATE_TESTS);
    if (!BZR_TRAV_PHASES && lane < 3u && v) atomicAdd(&counters[(size_t)rep * BZR_COUNTER_COUNT + which], (unsigned long long)v);
  }
  if (i >= n) return;
  w.count[i] = cnt;
  w.key[i] = ~0ull;
  if (cnt > kMaxCand) w.ovf[atomicAdd(&w.ctr[1], 1u)] = i;
  // Rank of each (ray, patch) pair within its patch bucket.  Neighbouring rays mostly share
  // patches: the lanes naming the same patch form a group (found with ballots, no memory traffic),
  // each group's first lane adds the group size -- all groups in one atomic instruction -- and the
  // lanes take their rank from the returned base.
  const uint32_t lane = threadIdx.x & 63u;
  BZR_PHASE(5)
  const uint32_t listed = cnt <= kMaxCand ? cnt : 0u;
  // Four list slots per round: their candidate loads first, then the grouping, then all four rounds'
  // returning atomics in flight together (one wait instead of four: vmcnt retires in issue order).
  constexpr int kRankBatch = 4;
  for (uint32_t j0 = 0; __any(j0 < listed); j0 += kRankBatch) {
    uint32_t b[kRankBatch], leader[kRankBatch], below[kRankBatch], base[kRankBatch];
#pragma unroll
    for (int k = 0; k < kRankBatch; ++k)
      b[k] = j0 + k < listed ? w.cand[(size_t)(j0 + k) * n + i] : 0u;
#pragma unroll
    for (int k = 0; k < kRankBatch; ++k) {
      const bool pend = j0 + k < listed;
      unsigned long long group = 0ull;
      bool todo = pend;
      for (;;) {
        const unsigned long long mask = __ballot(todo);
        if (mask == 0ull) break;
        const uint32_t b0 = __builtin_amdgcn_readlane(b[k], __builtin_ctzll(mask));
        const bool same = todo && b[k] == b0;
        const unsigned long long g = __ballot(same);
        if (same) {
          group = g;
          todo = false;
        }
      }
      leader[k] = pend ? (uint32_t)__builtin_ctzll(group) : lane;
      below[k] = lanes_below(group);
      base[k] = 0u;
      if (pend && lane == leader[k]) base[k] = atomicAdd(&w.hist[b[k]], (uint32_t)__popcll(group));
    }
#pragma unroll
    for (int k = 0; k < kRankBatch; ++k) {
      const uint32_t bs = __shfl(base[k], (int)leader[k], 64);
      if (j0 + k < listed) w.rank[(size_t)(j0 + k) * n + i] = bs + below[k];
    }
  }
#if BZR_TRAV_PHASES
  BZR_PHASE(0)
  if (counters && lane < 6u) {
    const uint32_t id[6] = {BZR_COUNTER_NODE_VISITS, BZR_COUNTER_LEAF_FETCHES, BZR_COUNTER_GATE_TESTS,
                            BZR_COUNTER_OVERFLOW_RAYS, BZR_COUNTER_FOLLOWS, BZR_COUNTER_SEGMENTS};
    unsigned long long v = 0ull;
    uint32_t which = 0;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k)
      if (lane == k) {
        v = ph_acc[k];
        which = id[k];
      }
    atomicAdd(&counters[(size_t)((i >> 6) % kCounterReplicas) * BZR_COUNTER_COUNT + which], v);
  }
#endif
}

// Candidate search, one 64-ray wave per 64 consecutive rays, the blocks in XCD-contiguous ray ranges.
// BZR_TRAV_WPE (default 8; 0 = the compiler's choice, 7 waves): amdgpu_waves_per_eu lower bound for k_traverse.
// At 8 waves per SIMD it keeps 64 VGPRs (35 SGPRs spill into VGPR lanes, no scratch): its walk waits on memory
// 45 % of its cycles, and the eighth wave hides more of it -- k_traverse -8 % on cfg5 (4.91 -> 4.52 ms per
// frame) and -10 % on cfg3 (0.221 -> 0.200 ms), frames -4.2 / -4.8 %, same bits (two box runs agree;
// profiles/r04_ab_traverse_wpe8.jsonl).
#ifndef BZR_TRAV_WPE
#define BZR_TRAV_WPE 8
#endif
#if BZR_TRAV_WPE
#define BZR_TRAV_ATTR __attribute__((amdgpu_waves_per_eu(BZR_TRAV_WPE)))
#else
#define BZR_TRAV_ATTR
#endif
template <int kBlk, int kAblock, bool kFast>
__global__ __launch_bounds__(kBlk) BZR_TRAV_ATTR void k_traverse(MeshView m, const float *__restrict__ rays, uint32_t ld,
                                                         uint32_t off, const uint32_t *__restrict__ alive, uint32_t n,
                                                         Work w, unsigned long long *counters) {
  __shared__ uint32_t stack[kBlk / 64][kStack];
  __shared__ float bundle[kBlk / 64][kBundleWords];  // the wave's ray bundle (bundle walk, always list)
  __shared__ uint32_t pend[kBlk / 64][128];  // the bundle walk's queued leaf slots
  uint32_t *wpend = pend[threadIdx.x >> 6];
  __shared__ uint32_t raw[kBlk / 64][128];  // leaves before the pre-test (up to two batches' worth)
  uint32_t *wraw = raw[threadIdx.x >> 6];
  const uint32_t b = xcd_contiguous(blockIdx.x, gridDim.x);
  if constexpr (kAblock != 0) {
    __shared__ float ubl[16];                                  // the block's union bundle (words 0..12)
    __shared__ unsigned long long akeep[kAblockMax / 64u];     // block-kept always-listed patches
    traverse_rays<kBlk, kAblock, kFast>(m, rays, ld, off, alive, n, w, counters, b * kBlk + threadIdx.x,
                                        stack[threadIdx.x >> 6], bundle[threadIdx.x >> 6], wpend, wraw, ubl, akeep);
  } else {
    traverse_rays<kBlk, 0, kFast>(m, rays, ld, off, alive, n, w, counters, b * kBlk + threadIdx.x, stack[threadIdx.x >> 6],
                                  bundle[threadIdx.x >> 6], wpend, wraw);
  }
}

// A bucket of c pairs in the staged layout (BZR_DENSE_MIN): (dense chunks << 32) | pairs in the sparse region.
struct BucketSplit {
  __host__ __device__ __forceinline__ unsigned long long operator()(uint32_t c) const {
    const uint32_t rem = c & 63u;
    const bool pad = rem >= kDenseMin;
    return ((unsigned long long)((c >> 6) + (pad ? 1u : 0u)) << 32) | (pad ? 0u : rem);
  }
};

// Threads t < nb: bucket t's padded lanes (the last dense chunk's lanes past its pairs) get the kNoPair
// record, its histogram word is cleared for the next segment, and (pair_count: with device counters on) the
// wave adds its buckets' pair counts to ctr[3].  Threads t < n: ray t's listed pairs go to their places -- rank r of bucket b is dense pair
// 64 dense_base(b) + r while r < 64 dense_chunks(b), else sparse pair r - 64 dense_chunks(b) of the bucket.
__global__ __launch_bounds__(kBlock) void k_place(uint32_t n, uint32_t nb, Work w, uint32_t *__restrict__ pair_count) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  uint32_t c = 0;
  if (t < nb) {
    c = w.hist[t];
    if (c) {
      w.hist[t] = 0u;
      if ((c & 63u) >= kDenseMin) {
        const uint32_t p0 = static_cast<uint32_t>(w.offs[t] >> 32) * 64u + c, p1 = (p0 + 63u) & ~63u;
        for (uint32_t p = p0; p < p1; ++p) w.pairs[p] = make_uint2(kNoPair, t);
      }
    }
  }
  // the wave's buckets' pairs (bzr_ctx_counters "pairs": the pairs the Newton stage runs): one atomic per
  // bucket wave -- per ray wave, the atomics on one address cost k_place 30 %
  if (pair_count && blockIdx.x * kBlock < nb) {
    uint32_t sum = c;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) sum += __shfl_xor(sum, k, 64);
    if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(pair_count, sum);
  }
  if (t >= n) return;
  const uint32_t c0 = w.count[t];
  if (c0 > kMaxCand) return;  // (an overflow ray's list is not ranked: the full scan takes it)
  const uint32_t cnt = c0;
  if (cnt == 0) return;
  const unsigned long long tot = w.offs[nb];
  const uint32_t sparse0 = static_cast<uint32_t>(tot >> 32) * 64u;  // the sparse region's first pair
  // four list slots per round: their loads first, then the offsets, then the stores
  for (uint32_t j0 = 0; j0 < cnt; j0 += 4u) {
    uint32_t b[4], r[4];
    unsigned long long o0[4], o1[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t j = j0 + k < cnt ? j0 + k : j0;
      b[k] = w.cand[(size_t)j * n + t];
      r[k] = w.rank[(size_t)j * n + t];
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      o0[k] = w.offs[b[k]];
      o1[k] = w.offs[b[k] + 1u];
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      if (j0 + k >= cnt) break;
      const uint32_t dbase = static_cast<uint32_t>(o0[k] >> 32), dlen = 64u * (static_cast<uint32_t>(o1[k] >> 32) - dbase);
      const uint32_t p = r[k] < dlen ? dbase * 64u + r[k] : sparse0 + static_cast<uint32_t>(o0[k]) + (r[k] - dlen);
      w.pairs[p] = make_uint2(t | ((j0 + k) << 26), b[k]);
    }
  }
}

constexpr uint32_t kFolBuf = 256;  // per-wave LDS staging of follow requests

// Copies a wave's staged follow requests to the global list (one atomicAdd for all of them).
__device__ __forceinline__ void flush_follow(uint32_t *buf, uint32_t &nf, uint32_t *__restrict__ fol,
                                             uint32_t *__restrict__ nfol, uint32_t lane) {
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(nfol, nf);
  base = __builtin_amdgcn_readfirstlane(base);
  for (uint32_t k = lane; k < nf; k += 64u) fol[base + k] = buf[k];
  nf = 0;
}

// Persistent waves over the dense chunks: wave g takes chunks g, g + W, ... and fetches the next chunk's
// pair records while it computes the current one.  A dense chunk holds one patch (its lane 0 always a real
// pair), processed with the record in scalar registers, `full` being a __restrict__ constant-address-space
// read; the padded lanes of a bucket's last chunk (kNoPair) idle.
// kNewtonWpe: amdgpu_waves_per_eu lower bound for k_newton.  At 8 waves per SIMD the
// compiler spills ~33 SGPRs to VGPR lanes and keeps 64 VGPRs; measured 2.4 % faster per frame than
// the unconstrained 7 waves (66 VGPRs, 106 SGPRs), same output bits.
constexpr int kNewtonWpe = 8;
#define BZR_NEWTON_ATTR __attribute__((amdgpu_waves_per_eu(kNewtonWpe)))
template <bool kFast>
__global__ __launch_bounds__(kBlock) BZR_NEWTON_ATTR void k_newton(const float *__restrict__ full,
                                                   const unsigned long long *__restrict__ total,
                                                   uint2 *__restrict__ pairs, const float *__restrict__ rays,
                                                   uint32_t ld, uint32_t off, uint32_t n, float *__restrict__ slot,
                                                   unsigned long long *__restrict__ key,
                                                   uint32_t *__restrict__ fol, uint32_t *__restrict__ nfol) {
  __shared__ uint32_t fbuf[kWaves][kFolBuf];
  const uint32_t wv = threadIdx.x >> 6;
  uint32_t nf = 0;  // staged follow requests of this wave (uniform)
  const uint32_t D = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(*total >> 32));  // dense chunks
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t W = gridDim.x * kWaves;
  // (chunks in dispatch order: XCD-contiguous order measured 6 % slower)
  uint32_t q = blockIdx.x * kWaves + (threadIdx.x >> 6);
  q = __builtin_amdgcn_readfirstlane(q);
  uint2 pr = make_uint2(kNoPair, 0u);
  if (q < D) pr = pairs[q * 64u + lane];
  for (; q < D; q += W) {
    const uint32_t p = q * 64u + lane;
    const bool todo = pr.x != kNoPair;
    const uint32_t ray = pr.x & kRayMask, j = pr.x >> 26;
    const uint32_t b = __builtin_amdgcn_readfirstlane(pr.y);  // the chunk's patch (lane 0 is a real pair)
    f3 s = mk(0.0f, 0.0f, 0.0f), d = s;
    if (todo) load_ray(rays, ld, off + ray, s, d);  // pairs of one patch: mostly neighbouring rays
    const uint32_t qn = q + W;
    if (qn < D) pr = pairs[qn * 64u + lane];  // prefetch the next chunk's pair records
    bool is_fol = false;
    const auto pa = uniform_patch(full, b);
    if (todo) {
      const Hit h = patch_intersect<true, kFast>(pa, s, d, false);
      if (h.what == kIntersect) record(slot, n, ray, j, b, h, b, &key[ray]);
      is_fol = h.what <= kFollow2;
      if (is_fol) reinterpret_cast<uint32_t *>(pairs)[2u * p + 1u] = b | (h.what << 30);  // the side, for k_resolve
    }
    // follow requests: staged in this wave's LDS buffer, published with one atomic per flush
    const unsigned long long fm = __ballot(is_fol);
    if (fm) {
      if (is_fol) fbuf[wv][nf + lanes_below(fm)] = p;
      nf += (uint32_t)__popcll(fm);
      if (nf > kFolBuf - 64u) flush_follow(fbuf[wv], nf, fol, nfol, lane);
    }
  }
  if (nf) flush_follow(fbuf[wv], nf, fol, nfol, lane);
}

// The sparse region (buckets' remainders below BZR_DENSE_MIN pairs): every lane runs its own pair with its
// own patch record, so a chunk of many small buckets costs one pass instead of one per patch.
template <bool kFast>
__global__ __launch_bounds__(kBlock) void k_newton_lane(const float *__restrict__ full,
                                                        const unsigned long long *__restrict__ total,
                                                        uint2 *__restrict__ pairs, const float *__restrict__ rays,
                                                        uint32_t ld, uint32_t off, uint32_t n, float *__restrict__ slot,
                                                        unsigned long long *__restrict__ key,
                                                        uint32_t *__restrict__ fol, uint32_t *__restrict__ nfol) {
  const unsigned long long tot = *total;
  const uint32_t base = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(tot >> 32)) * 64u;
  const uint32_t S = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(tot));
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t c = blockIdx.x * kWaves + (threadIdx.x >> 6); c * 64u < S; c += gridDim.x * kWaves) {
    const uint32_t p = base + c * 64u + lane;
    bool is_fol = false;
    const uint2 pr = c * 64u + lane < S ? pairs[p] : make_uint2(kNoPair, 0u);
    if (pr.x != kNoPair) {
      const uint32_t ray = pr.x & kRayMask, j = pr.x >> 26, b = pr.y;
      f3 s, d;
      load_ray(rays, ld, off + ray, s, d);
      const Patch pa = load_patch(full + (size_t)rec::kWords * b);
      const Hit h = patch_intersect<true, kFast>(pa, s, d, false);
      if (h.what == kIntersect) record(slot, n, ray, j, b, h, b, &key[ray]);
      is_fol = h.what <= kFollow2;
      if (is_fol) reinterpret_cast<uint32_t *>(pairs)[2u * p + 1u] = b | (h.what << 30);
    }
    const unsigned long long fm = __ballot(is_fol);
    if (fm) {
      uint32_t fb = 0;
      if (lane == 0u) fb = atomicAdd(nfol, (uint32_t)__popcll(fm));
      fb = __builtin_amdgcn_readfirstlane(fb);
      if (is_fol) fol[fb + lanes_below(fm)] = p;
    }
  }
}

template <int kMode, bool kFast>
// (k_finish at 6 or 8 waves per SIMD through amdgpu_waves_per_eu measured no faster than the compiler's choice
// -- it is HBM-bound at ~6 TB/s either way, profiles/r04_ab_finish_split.jsonl)
// BZR_FINISH_NORAY (default 1; 0 = the round-4 k_finish): the intersect segments' k_finish reads no ray -- a
// BezierIntersection needs none -- and the overflow rays (whose winner k_finish would evaluate again, with the ray)
// are emitted by k_finish_ovf just before it; 24 B per ray less, one small launch more per chunk.  First measured
// with the count tested before the key was loaded (the key and slot loads then waited on it): cfg5 +0.6 %, cfg3
// -0.6 to -1 % with frames in flight, lone frames slower (profiles/r05_ab_finish_noray.jsonl).  With count and
// key loaded together: lone frames cfg5 -0.5 %, cfg3 -1.2 %; frames in flight cfg5 +-0.3 %, cfg3 +1.9 %
// (profiles/r05_ab_finish_noray_v2.jsonl), same bits; the intersect k_finish drops from 112 to 12 VGPRs (the
// overflow rays' re-evaluation moved out).  Its HBM reads did not move (385.7 MB per 8 M-ray cfg5 chunk either
// way, profiles/r05_cfg5_staged_noray.txt): the compiler had already sunk the old kernel's ray loads into its
// overflow branch (its ISA loads count and key, then the slot).  Kept for the VGPRs and the lone frames.
#ifndef BZR_FINISH_NORAY
#define BZR_FINISH_NORAY 1
#endif
__global__ __launch_bounds__(kBlock) void k_finish(MeshView m, const float *rays, uint32_t ld, uint32_t off, uint32_t n,
                                                   Work w, Out o) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 4) w.ctr[threadIdx.x] = 0u;  // last reader of the counters this segment
  if (i >= n) return;
  const uint32_t gi = off + i;
  if constexpr (kMode == kModeHits && BZR_FINISH_NORAY) {
    // count and key together (testing the count first would make the key and slot loads wait on it)
    const uint32_t c = w.count[i];
    const unsigned long long k = w.key[i];
    if (c > kMaxCand) return;  // an overflow ray: k_finish_ovf emitted it
    Hit h = no_hit();
    uint32_t patch = 0xFFFFFFFFu;
    if (k != ~0ull) {
      const size_t sl = (size_t)(static_cast<uint32_t>(k) & 63u) * n + i;
      const float4 *r = reinterpret_cast<const float4 *>(w.slot) + 3 * sl;
      const float4 r0 = r[0], r1 = r[1], r2 = r[2];
      h.t = r0.x;
      h.point = mk(r0.y, r0.z, r0.w);
      h.cs = r1.x;
      h.bary = mk(r1.y, r1.z, r1.w);
      h.normal = mk(r2.x, r2.y, r2.z);
      h.what = kIntersect;
      patch = __float_as_uint(r2.w);
    }
    store_hit(o.hits, ld, gi, h, patch);
    return;
  }
  if (is_stage(kMode) && !o.first && o.status[gi] == BZR_RR_NONE) return;
  if constexpr (has_tir(kMode))  // a bounce stage: the rays that left this lens keep every word
    if (o.bounce_stage && o.pend[gi] == 0u) return;
  // the ray is loaded unconditionally: making the load depend on w.count (an intersect chunk's hits need it
  // only for an overflow ray) serialises the two reads and measured slower (cfg3 k_finish 0.059 -> 0.069 ms,
  // profiles/r04_ab_traverse_wpe8.jsonl, variant "finish")
  f3 s, d;
  load_ray(rays, ld, gi, s, d);
  Hit h = no_hit();
  uint32_t patch = 0xFFFFFFFFu;
  const unsigned long long k = w.key[i];
  if (w.count[i] > kMaxCand) {  // overflow ray: k_resolve left (t order, scanned patch) -- evaluate it again
    // (in a separate launch over the overflow list instead, k_finish would drop from 112 VGPRs to far fewer:
    // measured no faster -- an HBM-bound kernel -- and +30 % on cfg2's short frames; r04_ab_finish_split.jsonl)
    if (k != ~0ull) h = evaluate_patch<kFast>(m, static_cast<uint32_t>(k), s, d, patch);
  } else if (k != ~0ull) {
    const size_t sl = (size_t)(static_cast<uint32_t>(k) & 63u) * n + i;  // the winner's list slot (record())
    const float4 *r = reinterpret_cast<const float4 *>(w.slot) + 3 * sl;  // AoS: 48 bytes per slot
    const float4 r0 = r[0], r1 = r[1], r2 = r[2];
    h.t = r0.x;
    h.point = mk(r0.y, r0.z, r0.w);
    h.cs = r1.x;
    h.bary = mk(r1.y, r1.z, r1.w);
    h.normal = mk(r2.x, r2.y, r2.z);
    h.what = kIntersect;
    patch = __float_as_uint(r2.w);
  }
  emit<kMode>(o, ld, gi, s, d, h, patch);
}

// BZR_FINISH_NORAY: the overflow rays of an intersect segment (the w.ovf list), emitted before k_finish (which
// clears the counters and skips these rays): their winner -- k_resolve's full-scan key -- evaluated again.
template <bool kFast>
__global__ __launch_bounds__(kBlock) void k_finish_ovf(MeshView m, const float *rays, uint32_t ld, uint32_t off, Work w,
                                                       Out o) {
  const uint32_t V = __builtin_amdgcn_readfirstlane(w.ctr[1]);
  for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < V; q += gridDim.x * kBlock) {
    const uint32_t i = w.ovf[q], gi = off + i;
    f3 s, d;
    load_ray(rays, ld, gi, s, d);
    Hit h = no_hit();
    uint32_t patch = 0xFFFFFFFFu;
    const unsigned long long k = w.key[i];
    if (k != ~0ull) h = evaluate_patch<kFast>(m, static_cast<uint32_t>(k), s, d, patch);
    store_hit(o.hits, ld, gi, h, patch);
  }
}

// The rays k_traverse could not take: the reference's full in-order scan, split into
// (overflow ray, patch slice) items so a few rays over a large mesh still fill the chip.  Each thread
// scans patches t, t+256, ... of its slice (strict <: per thread the lowest index wins ties), and each
// wave folds its (t order, patch index) lexicographic minimum into the ray's key with one atomicMin:
// the winner of the reference's single in-order scan.  k_finish evaluates the winning patch again
// (same arithmetic, same bits) and emits it.  (Waves walking a slice with scalar-loaded records for
// 64 rays at once, as k_intersect_scan does, measured 4x slower: the serial walk waits on each load.)
constexpr uint32_t kOvfSlice = kBlock * 8;  // patches per item
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) {
    unsigned long long o = __shfl_xor(v, k, 64);
    v = o < v ? o : v;
  }
  return v;
}

// Follow-side retries and the overflow rays' full scans in one launch (both feed the per-ray keys
// k_finish reads; they are independent of each other): threads first take follow requests, then
// blocks take (overflow ray, patch slice) items.  With no overflow rays the second loop is empty --
// one launch per segment saved over separate kernels.
template <bool kFast>
__global__ __launch_bounds__(kBlock) void k_resolve(MeshView m, const float *__restrict__ rays, uint32_t ld,
                                                    uint32_t off, uint32_t n, Work w) {
  const uint32_t F = __builtin_amdgcn_readfirstlane(w.ctr[0]);
  for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < F; q += gridDim.x * kBlock) {
    const uint2 pr = w.pairs[w.fol[q]];
    const uint32_t ray = pr.x & kRayMask, j = pr.x >> 26, b = pr.y & ~(3u << 30), what = pr.y >> 30;
    f3 s, d;
    load_ray(rays, ld, off + ray, s, d);
    const uint32_t nbr = __float_as_uint(m.full[(size_t)rec::kWords * b + rec::kNeigh + what]);
    Patch pa = load_patch(m.full + (size_t)rec::kWords * nbr);
    Hit h = patch_intersect<false, kFast>(pa, s, d, true);
    if (h.what == kIntersect) record(w.slot, n, ray, j, b, h, nbr, &w.key[ray]);  // ranks at its candidate
  }
  const uint32_t V = __builtin_amdgcn_readfirstlane(w.ctr[1]);
  const uint32_t S = (m.n + kOvfSlice - 1) / kOvfSlice;
  const uint64_t items = (uint64_t)V * S;  // 64-bit: 2^20-ray chunks x slices of meshes above ~8M patches
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t q = (uint32_t)(item / S), lo = (uint32_t)(item - (uint64_t)q * S) * kOvfSlice, hi = min(m.n, lo + kOvfSlice);
    const uint32_t i = w.ovf[q];
    f3 s, d;
    load_ray(rays, ld, off + i, s, d);
    float best_t = FLT_MAX;
    uint32_t best_b = 0xFFFFFFFFu;
    // (not unrolled: newton_tail's wave vote in div_heights is a convergent operation)
    for (uint32_t b = lo + threadIdx.x; b < hi; b += kBlock) {
      const float4 *qq = m.planar + 4u * b;
      if (!planar_gate(qq[0], qq[1], qq[2], qq[3], s, d)) continue;
      uint32_t src;
      Hit h = evaluate_patch<kFast>(m, b, s, d, src);
      if (h.what == kIntersect && h.t < best_t) {
        best_t = h.t;
        best_b = b;
      }
    }
    const unsigned long long win =
        wave_min_u64(best_b != 0xFFFFFFFFu ? ((unsigned long long)t_order(best_t) << 32) | best_b : ~0ull);
    if ((threadIdx.x & 63u) == 0 && win != ~0ull) atomicMin(&w.key[i], win);
  }
}

__global__ void k_count(Work w, uint32_t nb, unsigned long long *__restrict__ counters) {
  if (threadIdx.x != 0) return;
  counters[BZR_COUNTER_SEGMENTS] += w.ctr[2];
  counters[BZR_COUNTER_PAIRS] += w.ctr[3];
  counters[BZR_COUNTER_FOLLOWS] += w.ctr[0];
  counters[BZR_COUNTER_OVERFLOW_RAYS] += w.ctr[1];
  // k_newton_lane's chunks; Newton passes = dense chunks + those
  const unsigned long long tot = w.offs[nb];
  const uint32_t sparse_chunks = (static_cast<uint32_t>(tot) + 63u) / 64u;
  counters[BZR_COUNTER_LANE_CHUNKS] += sparse_chunks;
  counters[BZR_COUNTER_NEWTON_ROUNDS] += static_cast<uint32_t>(tot >> 32) + sparse_chunks;
}

// Exclusive prefix sum of bucket_split(hist) in one block (meshes of up to kScanSmall - 1 patches; larger
// ones use hipCUB over the same values): offs[i] = sum of BucketSplit(hist[j]) over j < i.  (k_place clears
// the histogram.)
constexpr uint32_t kScanThreads = 1024, kScanPer = 8, kScanSmall = kScanThreads * kScanPer;
__global__ __launch_bounds__(kScanThreads) void k_scan_small(const uint32_t *__restrict__ hist,
                                                             unsigned long long *__restrict__ offs, uint32_t count) {
  __shared__ unsigned long long wave_total[kScanThreads / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, base = t * kScanPer;
  unsigned long long v[kScanPer], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; ++k) {
    v[k] = base + k < count ? BucketSplit()(hist[base + k]) : 0ull;
    sum += v[k];
  }
  unsigned long long x = sum;  // inclusive scan over the wave
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wave_total[wv] = x;
  __syncthreads();
  unsigned long long before = 0;
  for (uint32_t k = 0; k < wv; ++k) before += wave_total[k];
  unsigned long long run = before + x - sum;
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; ++k) {
    if (base + k < count) offs[base + k] = run;
    run += v[k];
  }
}

// ------------------------------------------------------------ fused path (default)
// One kernel per call: each wave takes 64 rays and runs every segment of them (one BezierMesh::intersect,
// or the whole refraction chain) without leaving the wave.  Per segment (trace_segment):
//  - the wave walks the lens BVH as k_traverse does and collects, in LDS, each leaf whose exact planar
//    gate passes for some lanes (wave-uniform patch index + lane mask, up to kEntries per batch);
//  - the collected leaves run through ONE Newton site, in order: the lanes that passed run
//    BezierTriangle::intersect with the patch record in SGPRs (uniform constant-address loads); lanes
//    whose result is follow-side K retry the named neighbour with cNone (reference/bezierMesh.cpp:212-216;
//    the neighbour of side K is uniform too).  A retry whose neighbour is a collected leaf still to come
//    joins that leaf's pass; one whose neighbour already ran takes the result that pass parked for it
//    (below); only the rest take a pass of their own;
//  - parking: a leaf's pass also runs, in its otherwise idle lanes, the cNone evaluation
//    for the lanes of later leaves that neighbour it -- the retry those lanes would ask for -- and parks
//    the result in LDS (one per lane and segment; not for kModeHits, whose 12-word winner leaves no room).
// Each lane keeps the lexicographic minimum of (t order key, scanned patch index) -- the reference's
// strict-< in-order winner, as in the staged path -- with the winning hit in LDS.  The schedule decides
// which pass evaluates a (lane, patch, limit), never the evaluation or its key.  Nothing per pair leaves
// the CU: HBM sees the rays in and the results out.  A patch sits in one leaf, so a wave runs a patch's
// pass at most once per segment (plus retries that could neither join nor use a parked result); lanes
// that need neither idle through it (lane utilisation).  Rays whose origin lies beyond the
// tree's validity radius, or whose stack overflows, take the reference's in-order scan in the same wave
// (same Newton site, patches in index order).
struct TraceCtr {  // wave-uniform work counters (kCount)
  uint32_t nodes = 0, leaves = 0, gate_tests = 0, rounds = 0, pairs = 0, follows = 0, segments = 0, ovf = 0;
  uint32_t shorts = 0;  // passes that skipped the last Newton normal (BZR_TRACE_SHORT)
  uint32_t rounds_odd = 0, runs_odd = 0;  // odd chain segments (a lens's back surface): passes, pairs + follows
};
// k_trace's BVH walk phase runs at wave priority 3 (s_setprio), back to 0 for the Newton passes.  The walk is a
// chain of dependent scalar loads with little VALU work; issuing
// it ahead of the VALU-bound passes of the CU's other waves keeps its loads in flight (cfg4 -3 %).
// The intersect kernel (kModeHits) parks cNone results as the refraction kernels do: cfg5
// fused -7.8 % Newton passes, +3.2 % Mrays/s; cfg3 +1 % (profiles/r03_ab_cfg{5,3}_fused_parkhits.jsonl).
// BZR_TRACE_BUNDLE (default 1): k_trace walks the tree with the wave-bundle test in batches (trace_segment)
// instead of one node at a time with each lane's slab test (0; rim waves whose bundle is wide take that walk
// anyway).  Round 3 measured the 4-wide bundle walk slower on the chains (cfg4 +5 to +6 %, cfg2 +3 %; cfg5
// fused -7 %, profiles/r03s2_ab_trace_bundle.jsonl): the bundle setup and the per-level batches cost what
// the fewer slab tests saved.  Round 4's integer DPP reductions and two-level batches (BZR_TRACE_WIDE) turn
// it around: bench.py with frames in flight, same bits, cfg4 11 074 -> 11 525 Mrays/s (+4.1 %), cfg2 +1.1 %,
// cfg5 fused +14 %, cfg3 fused +0.7 % (profiles/r04_bench_ab_trace_wide.jsonl; one serialized frame is
// within 1 %: the walk's VALU is what overlapping frames compete for).
#ifndef BZR_TRACE_BUNDLE
#define BZR_TRACE_BUNDLE 1
#endif
// BZR_TRACE_SHORT (default 1; 0 = off): a Newton pass none of whose lanes can win skips the last iteration's
// surface normal (newton_tail's hook).  The last iteration enters with the t it returns, so each lane knows its
// key (t order, scanned patch) before that iteration: when no lane of the pass has a key below its running best
// -- and none is a parking lane, whose result must be whole -- consider() would drop every result, and the
// normal and cosine only it reads are not evaluated.  On entering a lens most rays pass the gates of a front
// and a back patch, and the back patch's pass loses once the front one has run.  The vote is wave-uniform
// (__any over the lanes in the call) and takes the same decision consider() takes: no output bit depends on it.
// A losing pass is only short when its lanes' winners ran before it, so with 1 a batch of collected leaves runs
// in the order of their gates' plane distance (each entry's first passing lane's), near side first, ties as
// collected.  The order is kept up while the batch is collected (batch_append: each arriving leaf takes its place
// in one word of nibbles, pass_order.hpp) and the pass loop reads the entries through it; nothing is sorted or
// moved afterwards.  The winner is the minimum of (t order, scanned patch) over a set, so the order of the passes
// cannot reach it.  2: the vote without the reorder.
// cfg4: 26 % of the passes short (17.6 % with 2), each 242 of 2 130 VALU shorter; bench.py 11 503 -> 11 699 Mrays/s,
// lone frames 4.344 -> 4.271 ms (2: 4.299); cfg2 in flight +2.9 %, lone frames 0.400 -> 0.414 ms
// (profiles/r07_bench_ab.jsonl, r07_ab_short_cfg{4,2}.jsonl).
#ifndef BZR_TRACE_SHORT
#define BZR_TRACE_SHORT 1
#endif
static_assert(BZR_TRACE_SHORT >= 0 && BZR_TRACE_SHORT <= 2, "BZR_TRACE_SHORT: 0, 1 or 2");
constexpr uint32_t kEntries = 16;  // collected leaves per batch: power of two, <= 64
static_assert(kEntries >= 4 && kEntries <= 64 && (kEntries & (kEntries - 1)) == 0, "kEntries");
// Words kept per lane: the winner (all of BezierIntersection for kModeHits; what refraction reads
// otherwise: point, cos, normal) and a parked retry result (t, point, cos, normal).
template <int kMode>
struct TraceWords {
  static constexpr int kHit = kMode == kModeHits ? 12 : 7;
  // kModeHits parks the barycentrics too (11 words): 6.4 KB of LDS per wave, which its 6 waves per SIMD
  // (80 VGPRs) leave room for (24 waves x 6.4 KB <= 160 KB)
  static constexpr int kPark = kMode != kModeHits ? 8 : 11;
  // traversal stack entries: the bundle walk's batches push up to 64 children at once, so the refraction
  // kernels (4.6 KB of LDS per wave at 7 waves per SIMD) take twice BZR_STACK; the intersect kernel's LDS
  // (6.5 KB per wave at 6 waves per SIMD) has no room left
  static constexpr int kStackCap = (BZR_TRACE_BUNDLE && kMode != kModeHits) ? 2 * kStack : kStack;
};
// kModeTir keeps the lane's counters (segments | reflections << 16) and its weight here between segments: two
// registers less across the walks.  (An empty base in every other mode: their layout is what it was.)
template <int kMode>
struct TraceKeep {};
template <>
struct TraceKeep<kModeTir> {
  uint32_t count[64];
  float weight[64];
};
// kModeOpl: and the lane's optical path and glass path (512 B more per wave: 5 976 B, 24 waves per CU still fit).
template <>
struct TraceKeep<kModeOpl> {
  uint32_t count[64];
  float weight[64];
  float opl[64];
  float glass[64];
};
template <>
struct TraceKeep<kModeMedia> : TraceKeep<kModeOpl> {};  // kModeMedia keeps what kModeOpl keeps: no new word per lane
template <>
struct TraceKeep<kModeAbsorb> : TraceKeep<kModeMedia> {};  // and so does kModeAbsorb
template <>
struct TraceKeep<kModeGhost> : TraceKeep<kModeAbsorb> {};  // and kModeGhost: the draw is recomputed, nothing waits
// kModeBidir: and the lane's place in the walk (bidir_open's word: key, fwd, travelling, final status), 256 B more per
// wave: 6 232 B, 24 waves per CU still fit in 160 KiB (149 568 B).  The draw is recomputed here too.
template <>
struct TraceKeep<kModeBidir> : TraceKeep<kModeAbsorb> {
  uint32_t state[64];
};
template <>
struct TraceKeep<kModeCoat> : TraceKeep<kModeBidir> {};  // kModeCoat keeps what kModeBidir keeps: the table is read
// The bundle walk's set of leaf slots already queued in this wave-segment (bundle_batch `seen`), one bit per
// slot: the refract and chain kernels walk the trees with split leaf boxes (MeshView swide).  The intersect
// kernel's 6.7 KB per wave leave no room for it (24 waves x 7.7 KB > 160 KB), and the power, spectral and TIR
// kernels sit at their 80-VGPR budget, where the set's few instructions in the walk cost them 12 to 44 bytes of
// scratch per lane: those four walk the unsplit tree.
template <int kMode>
constexpr bool kSplitWalk = BZR_TRACE_BUNDLE && BZR_TRACE_WIDE && (kMode == kModeRefract || kMode == kModeStage);
template <bool kOn>
struct TraceSeen {};
template <>
struct TraceSeen<true> {
  alignas(16) uint32_t seen[bzr_host::kSplitSlotCap / 32];
};
template <int kMode>
struct TraceLds : TraceKeep<kMode>, TraceSeen<kSplitWalk<kMode>> {  // per wave
  uint32_t stack[TraceWords<kMode>::kStackCap];
  float hit[TraceWords<kMode>::kHit][64];    // the lane's current winner (written only when it improves)
  unsigned long long emask[kEntries];        // collected leaves: gate ballot
  float bundle[kBundleWords];                // the always list's ray bundle (always_bundle_keep)
  uint32_t eid[kEntries];                    // and patch index
#if BZR_TRACE_SHORT == 1
  uint32_t ekey[kEntries];                   // and order key (entry_key): the passes run near side first
#endif
#if BZR_TRACE_BUNDLE
  uint32_t pend[64];                         // the bundle walk's queued leaf slots
#endif
  float park[TraceWords<kMode>::kPark ? TraceWords<kMode>::kPark : 1][64];
};

__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)), lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  return ((unsigned long long)hi << 32) | lo;  // (readfirstlane returns int: widen the unsigned halves)
}

// The lane's candidate `h` from scanned patch `scan` (the hit itself from patch `src`).
template <int kMode>
__device__ __forceinline__ void consider(const Hit &h, uint32_t scan, uint32_t src, unsigned long long &best,
                                         TraceLds<kMode> &L, uint32_t lane) {
  if (h.what == kIntersect && h.t < FLT_MAX) {
    const unsigned long long k = ((unsigned long long)t_order(h.t) << 32) | scan;
    if (k < best) {
      best = k;
      if constexpr (kMode == kModeHits) {
        L.hit[0][lane] = h.t;
        L.hit[1][lane] = h.point.x;
        L.hit[2][lane] = h.point.y;
        L.hit[3][lane] = h.point.z;
        L.hit[4][lane] = h.cs;
        L.hit[5][lane] = h.bary.x;
        L.hit[6][lane] = h.bary.y;
        L.hit[7][lane] = h.bary.z;
        L.hit[8][lane] = h.normal.x;
        L.hit[9][lane] = h.normal.y;
        L.hit[10][lane] = h.normal.z;
        L.hit[11][lane] = __uint_as_float(src);
      } else {
        L.hit[0][lane] = h.point.x;
        L.hit[1][lane] = h.point.y;
        L.hit[2][lane] = h.point.z;
        L.hit[3][lane] = h.cs;
        L.hit[4][lane] = h.normal.x;
        L.hit[5][lane] = h.normal.y;
        L.hit[6][lane] = h.normal.z;
      }
    }
  }
}

// newton_tail's hook for a pass of trace_segment: the last normal is needed when some lane of the call may
// still win -- a parking lane (`spec`: its result is kept whole), or a lane whose key, from the t that enters
// the last iteration and the scanned patch consider() will get, is below its best.  A NaN t cannot win, as in
// consider(); best == ~0 loses to every finite key.  `skipped` records a "no" for the counters.
struct PassVote {
  unsigned long long best;
  uint32_t scan;
  bool spec;
  bool *skipped;
  __device__ __forceinline__ bool operator()(float t) const {
#if BZR_TRACE_SHORT
    const bool may = spec || (t < FLT_MAX && (((unsigned long long)t_order(t) << 32) | scan) < best);
    const bool any = __any(may);
    *skipped = !any;
    return any;
#else
    (void)t;
    return true;
#endif
  }
};

// Order key of a collected entry: the gate's plane distance of its first passing lane (pm: the gate ballot), as
// raw bits -- a passing lane's t is > 0 (planar_gate), and among positive floats (+inf included) the bits order
// and tie as t_order does.
__device__ __forceinline__ uint32_t entry_key(float gt, unsigned long long pm) {
  return (uint32_t)__builtin_amdgcn_readlane(__float_as_int(gt), (int)__builtin_ctzll(pm));
}
static_assert(kEntries <= kOrderEntries, "a batch's order is one word of nibbles (pass_order.hpp)");
// Entry `ne` of the batch being collected (patch index, gate ballot and order key; all arguments but `lane` are
// wave-uniform) goes to the list as collected, and the batch's order word takes it in: near side first (kOrder:
// the stable ascending order of the keys, pass_order.hpp) or as collected.  The keys of the earlier entries are
// read back one per lane; the order itself lives in two scalar registers, and no entry is moved.
template <bool kOrder, typename Lds>
__device__ __forceinline__ void batch_append(Lds &L, uint32_t ne, unsigned long long &order, uint32_t id,
                                             unsigned long long pm, uint32_t key, uint32_t lane) {
  uint32_t front = ne;
  if constexpr (kOrder) {
    front = 0u;
    if (ne) {
      __builtin_amdgcn_wave_barrier();
      front = popc64(__ballot(L.ekey[lane & (kEntries - 1u)] <= key) & ((1ull << ne) - 1ull));
    }
  }
  order = order_insert(order, ne, front);
  if (lane == 0u) {
    L.eid[ne] = id;
    L.emask[ne] = pm;
    if constexpr (kOrder) L.ekey[ne] = key;
  }
}

// The lane's winner back from LDS (best != ~0).
template <int kMode>
__device__ __forceinline__ Hit winner(TraceLds<kMode> &L, uint32_t lane, uint32_t &patch) {
  Hit h = no_hit();
  h.what = kIntersect;
  if constexpr (kMode == kModeHits) {
    h.t = L.hit[0][lane];
    h.point = mk(L.hit[1][lane], L.hit[2][lane], L.hit[3][lane]);
    h.cs = L.hit[4][lane];
    h.bary = mk(L.hit[5][lane], L.hit[6][lane], L.hit[7][lane]);
    h.normal = mk(L.hit[8][lane], L.hit[9][lane], L.hit[10][lane]);
    patch = __float_as_uint(L.hit[11][lane]);
  } else {  // refract_hit reads point, cos and normal
    h.point = mk(L.hit[0][lane], L.hit[1][lane], L.hit[2][lane]);
    h.cs = L.hit[3][lane];
    h.normal = mk(L.hit[4][lane], L.hit[5][lane], L.hit[6][lane]);
    patch = 0xFFFFFFFFu;
  }
  return h;
}

// A parked cNone result: t (NaN when it is not an intersection, which consider() drops like a miss),
// point, cos, normal -- what consider() and the refraction read.
template <int kMode>
__device__ __forceinline__ void park(const Hit &h, TraceLds<kMode> &L, uint32_t lane) {
  if constexpr (TraceWords<kMode>::kPark > 0) {
    L.park[0][lane] = h.what == kIntersect ? h.t : __uint_as_float(0x7FC00000u);
    L.park[1][lane] = h.point.x;
    L.park[2][lane] = h.point.y;
    L.park[3][lane] = h.point.z;
    L.park[4][lane] = h.cs;
    L.park[5][lane] = h.normal.x;
    L.park[6][lane] = h.normal.y;
    L.park[7][lane] = h.normal.z;
    if constexpr (TraceWords<kMode>::kPark >= 11) {  // kModeHits: the whole BezierIntersection
      L.park[8][lane] = h.bary.x;
      L.park[9][lane] = h.bary.y;
      L.park[10][lane] = h.bary.z;
    }
  }
}
template <int kMode>
__device__ __forceinline__ Hit parked(TraceLds<kMode> &L, uint32_t lane) {
  Hit h = no_hit();
  if constexpr (TraceWords<kMode>::kPark > 0) {
    h.t = L.park[0][lane];
    h.point = mk(L.park[1][lane], L.park[2][lane], L.park[3][lane]);
    h.cs = L.park[4][lane];
    h.normal = mk(L.park[5][lane], L.park[6][lane], L.park[7][lane]);
    if constexpr (TraceWords<kMode>::kPark >= 11) h.bary = mk(L.park[8][lane], L.park[9][lane], L.park[10][lane]);
    h.what = kIntersect;
  }
  return h;
}

// One BezierMesh::intersect for the wave's active lanes; the winner is left in `best` / L.hit.
template <int kMode, bool kFast, bool kCount>
__device__ __forceinline__ void trace_segment(const MeshView &m, f3 s, f3 d, bool act, unsigned long long &best,
                                              TraceLds<kMode> &L, uint32_t lane, TraceCtr &ctr) {
  constexpr bool kPark = TraceWords<kMode>::kPark > 0;
  constexpr uint32_t kNo = 0xFFFFFFFFu;
  constexpr int kCap = TraceWords<kMode>::kStackCap;
  constexpr bool kOrder = BZR_TRACE_SHORT == 1;  // the batch's passes near side first
  best = ~0ull;
  const float amax = fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fabsf(s.z));
  bool ovf = false;  // this lane takes the in-order full scan
  if (act && !(amax <= m.s_max)) {
    ovf = true;
    act = false;
  }
  const bool near_tier = !__any(act && !(amax <= m.s_near));
  const bzr_host::Bvh4Node *nodes = near_tier ? m.nodes_near : m.nodes;
  const bzr_host::Bvh4ObbNode *obb = near_tier ? m.obb_near : m.obb;
  const float4 *leaf = near_tier ? m.leaf_near : m.leaf;
  const f3 inv = mk(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
  const f3 sinv = mk(s.x * inv.x, s.y * inv.y, s.z * inv.z);
  // The node to visit next is held in a scalar register (`next`); only the other hit children go to the
  // LDS stack, so a descent costs no LDS round trip (same visit order as pushing them all).
  int sp = 0;
  uint32_t next = (m.n > 0 && __any(act)) ? 0u : kNo;
  unsigned long long next_hm = 0ull;  // the lanes whose rays hit `next`'s box
  uint32_t scan = kNo;                // next patch of the full scan (kNo: not scanning)
  uint32_t join = kNo, join_src = 0;  // a retry waiting for a later leaf's pass: that leaf, scanned patch
  uint32_t parked_nb = kNo;           // the patch whose cNone result is parked for this lane
  // the always list: batches of 64 patches bundle-tested against the wave (uniform state; the bundle is
  // built once per segment into LDS, so no register holds it across the walk and the Newton passes)
  uint32_t ab = (m.n_always && __any(act)) ? 0u : (m.n_always + 63u) / 64u;  // next batch
  unsigned long long am = 0ull;  // the current batch's patches left to gate-test
  bool bwalk = false;  // this wave-segment takes the bundle walk
#if BZR_TRACE_BUNDLE
  // The bundle walk: the wave's active rays as one bundle (bundle_box), the tree taken in batches of up to
  // 16 nodes -- one child per lane -- from the top of the LDS stack; hit inner children are pushed, hit
  // leaves queued (L.pend) and gate-tested one by one with every active lane's own exact planar gate.
  uint32_t npend = 0, pi = 0;  // queued leaves, next to gate-test (uniform)
  const float4 *kids = near_tier ? m.kids_near : m.kids;
  // the walk choice, per wave-segment: a bundle whose directions spread wider than kBundleSpread (rim
  // waves of refracted rays, incoherent batches) walks per lane instead -- its hull would reach far more
  // boxes than its rays do
  bool narrow = false;  // else every node is tested per lane (the oriented-box nodes always are)
  if (next != kNo) {
    narrow = bundle_setup_swap(act, s, d, L.bundle, lane) <= kBundleSpread;
    if constexpr (kSplitWalk<kMode>) {  // a narrow wave walks the split tree: no slot queued yet
      static_assert(sizeof(L.seen) == 64 * sizeof(uint4), "one uint4 per lane clears the slot set");
      if (narrow && m.split > 1u) reinterpret_cast<uint4 *>(L.seen)[lane] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (lane == 0u) L.stack[0] = 0u;
    sp = 1;
    next = kNo;
    bwalk = true;
  }
#endif
  for (;;) {
    uint32_t ne = 0;  // collected leaves (uniform)
    unsigned long long order = 0ull;  // nibble p: the entry whose pass runs p-th (uniform; pass_order.hpp)
    __builtin_amdgcn_s_setprio(3);  // the walk is latency-bound: issue it ahead of Newton passes
#if BZR_TRACE_BUNDLE
    while (bwalk && ne < kEntries) {
      if (pi < npend) {  // a queued leaf: every active lane's planar gate
        const uint32_t slot = __builtin_amdgcn_readfirstlane(L.pend[pi]);
        ++pi;
        const u32x16 r = *((const cu32x16 *)(uintptr_t)leaf + slot);
        float gt;
        const bool pass = act & planar_gate(leaf_q(r, 0), leaf_q(r, 1), leaf_q(r, 2), leaf_q(r, 3), s, d, gt);
        if (kCount) {
          ++ctr.leaves;
          ctr.gate_tests += popc64(__ballot(act));
        }
        const unsigned long long pm = __ballot(pass);
        if (pm) {
          batch_append<kOrder>(L, ne, order, r[15], pm, kOrder ? entry_key(gt, pm) : 0u, lane);
          ++ne;
        }
        continue;
      }
      if (sp == 0) break;
      pi = npend = 0;
      const uint32_t top = __builtin_amdgcn_readfirstlane(L.stack[sp - 1]);
      if (!narrow || (top & bzr_host::kObbFlag)) {  // one node, its children tested by each lane's own ray
        --sp;
        if (kCount) ++ctr.nodes;
        bool hit[4];
        uint32_t ch[4];
        // (the reciprocals computed here, not kept from the segment's start: wide waves are rare, and 6
        // registers live across the Newton passes would cost occupancy)
        const f3 linv = mk(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
        node_children(nodes, obb, top, act, s, d, mk(s.x * linv.x, s.y * linv.y, s.z * linv.z), linv, hit, ch);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const unsigned long long hm = __ballot(hit[c]);
          if (hm == 0ull) continue;
          if (ch[c] & bzr_host::kLeafFlag) {
            if (lane == 0u) L.pend[npend] = ch[c] & ~bzr_host::kLeafFlag;
            ++npend;
          } else if (sp < kCap) {
            if (lane == 0u) L.stack[sp] = ch[c];
            ++sp;
          } else if (lane_bit(hm, lane)) {
            ovf = true;  // traversal stack exhausted: these lanes take the full scan
          }
        }
        continue;
      }
      bool full;
      uint32_t k;
#if BZR_TRACE_WIDE
      // (a wave walks one tree for the whole segment: the split one in batches when it is narrow, else -- no
      // oriented-box node exists in a split build -- the unsplit one per lane above; both start at node 0)
      if constexpr (kSplitWalk<kMode>)
        npend = bundle_batch<kCap, 16>(near_tier ? m.swide_near : m.swide, L.stack, sp, L.pend, L.bundle, lane, full, k,
                                       0u, m.split > 1u ? L.seen : nullptr);
      else
        npend = bundle_batch<kCap, 16>(near_tier ? m.wide_near : m.wide, L.stack, sp, L.pend, L.bundle, lane, full, k);
#else
      npend = bundle_batch<kCap>(kids, L.stack, sp, L.pend, L.bundle, lane, full, k);
#endif
      if (full) ovf |= act;  // traversal stack exhausted: every active lane takes the full scan
      if (kCount) ctr.nodes += k;
    }
#else
    while ((next != kNo || sp > 0) && ne + 4u <= kEntries) {
      const uint32_t node = next != kNo ? next : __builtin_amdgcn_readfirstlane(L.stack[--sp]);
      next = kNo;
      if (kCount) ++ctr.nodes;
      bool hit[4];
      uint32_t ch[4];
      node_children(nodes, obb, node, act, s, d, sinv, inv, hit, ch);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned long long hm = __ballot(hit[c]);
        if (hm == 0ull) continue;
        if (ch[c] & bzr_host::kLeafFlag) {
          const u32x16 r = *((const cu32x16 *)(uintptr_t)leaf + (ch[c] & ~bzr_host::kLeafFlag));
          const float4 g0 = make_float4(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3]));
          const float4 g1 = make_float4(__uint_as_float(r[4]), __uint_as_float(r[5]), __uint_as_float(r[6]), __uint_as_float(r[7]));
          const float4 g2 = make_float4(__uint_as_float(r[8]), __uint_as_float(r[9]), __uint_as_float(r[10]), __uint_as_float(r[11]));
          const float4 g3 = make_float4(__uint_as_float(r[12]), __uint_as_float(r[13]), __uint_as_float(r[14]), 0.0f);
          float gt;
          const bool pass = hit[c] & planar_gate(g0, g1, g2, g3, s, d, gt);
          if (kCount) {
            ++ctr.leaves;
            ctr.gate_tests += popc64(hm);
          }
          const unsigned long long pm = __ballot(pass);
          if (pm) {
            batch_append<kOrder>(L, ne, order, r[15], pm, kOrder ? entry_key(gt, pm) : 0u, lane);
            ++ne;
          }
        } else {
          if (next != kNo) {
            if (sp < kCap) L.stack[sp++] = next;
            else if (lane_bit(next_hm, lane)) ovf = true;  // traversal stack exhausted: these lanes take the full scan
          }
          next = ch[c];
          next_hm = hm;
        }
      }
    }
#endif
    // tree done: the always list (patches without a proven gate region, bvh.cpp), gate-tested by every
    // wave-segment -- the candidates no box may cull
    while (next == kNo && sp == 0 && ne < kEntries) {  // (bundle walk: its leaf queue is empty here too)
      if (am == 0ull) {
        if (ab * 64u >= m.n_always) break;
        if (ab == 0u && !BZR_TRACE_BUNDLE) bundle_to_lds(act, s, d, L.bundle, lane);
        am = __ballot(always_bundle_keep(m.always, ab * 64u + lane, m.n_always, L.bundle));
        ++ab;
        continue;
      }
      const uint32_t k = (ab - 1u) * 64u + __builtin_ctzll(am);
      am &= am - 1ull;
      uint32_t b;
      float gt;
      const bool pass = always_gate(m.always, k, act, s, d, b, gt);
      if (kCount) {
        ++ctr.leaves;
        ctr.gate_tests += popc64(__ballot(act));
      }
      const unsigned long long pm = __ballot(pass);
      if (pm) {
        batch_append<kOrder>(L, ne, order, b, pm, kOrder ? entry_key(gt, pm) : 0u, lane);
        ++ne;
      }
    }
    if (ne == 0u) {  // tree done: the reference's in-order scan for the lanes that could not use it
#define BZR_SEG_END break;
      if (scan == kNo) {
        if (!__any(ovf)) BZR_SEG_END
        scan = 0;
        if (kCount) ctr.ovf += popc64(__ballot(ovf));
      }
      bool pass = false;
      for (; scan < m.n; ++scan) {
        const float4 *g = m.planar + 4u * scan;  // wave-uniform address -> scalar loads
        pass = ovf && planar_gate(g[0], g[1], g[2], g[3], s, d);
        if (__any(pass)) break;
      }
      if (scan >= m.n) BZR_SEG_END
#undef BZR_SEG_END
      const unsigned long long pm = __ballot(pass);
      if (lane == 0u) {
        L.eid[0] = scan;
        L.emask[0] = pm;
      }
      ne = 1;
      ++scan;
    }
    // the collected leaves' passes, in the batch's order: the next entry is the order word's lowest nibble, and
    // `todo` (uniform, one bit per entry; ne <= 16) holds the entries whose passes are still to come -- what the
    // join and park logic below looks among.  (The full scan's single entry: order 0, entry 0.)
    __builtin_amdgcn_s_setprio(0);
    for (uint32_t todo = (1u << ne) - 1u; todo; order >>= 4) {
      const uint32_t ei = order_at(order, 0u);
      todo ^= 1u << ei;
      const bool more = todo != 0u;
      const uint32_t b = __builtin_amdgcn_readfirstlane(L.eid[ei]);
      const auto hp = uniform_patch(m.full, b);
      const bool run0 = lane_bit(uniform_u64(L.emask[ei]), lane);
      const bool joined = join == b;  // an earlier leaf's retry on this one
      const uint32_t sidx = joined ? join_src : b;
      if (joined) join = kNo;
      bool spec = false;  // park this leaf's cNone result for lanes of later leaves that neighbour it
      if (kPark && more) {
        unsigned long long sm = 0ull;
#pragma unroll
        for (uint32_t side = 0; side < 3u; ++side) {
          const uint32_t nb = __float_as_uint(hp.r[rec::kNeigh + side]);
          const unsigned long long later = __ballot(L.eid[lane & (kEntries - 1u)] == nb) & todo;
          if (later) sm |= uniform_u64(L.emask[__builtin_ctzll(later)]);
        }
        spec = lane_bit(sm, lane) && !run0 && !joined && parked_nb == kNo;
      }
      if (kCount) {
        ++ctr.rounds;
        // (kGatePlane's promise, checked here: a run0 lane that the record's own gate turns away is no pair)
        ctr.pairs += popc64(__ballot(run0 && patch_gate(hp, s, d)));
        ctr.follows += popc64(__ballot(joined));
      }
      uint32_t what = kNone;
      bool skipped = false;
      if (run0 || joined || spec) {
        const Hit h = patch_intersect<kGatePlane, kFast>(hp, s, d, joined || spec, PassVote{best, sidx, spec, &skipped});
        if (spec) {
          park(h, L, lane);
          parked_nb = b;
        } else {
          consider(h, sidx, b, best, L, lane);
          if (!joined) what = h.what;
        }
      }
      if (kCount && __any(skipped)) ++ctr.shorts;
      for (uint32_t side = 0; side < 3u; ++side) {
        bool fl = run0 && what == side;
        if (!__any(fl)) continue;
        const uint32_t nb = __float_as_uint(hp.r[rec::kNeigh + side]);
        if (kPark) {  // computed by an earlier pass
          const bool use = fl && parked_nb == nb;
          if (use) {
            consider(parked(L, lane), b, nb, best, L, lane);
            fl = false;
          }
          if (kCount) ctr.follows += popc64(__ballot(use));
          if (!__any(fl)) continue;
        }
        // the neighbour among the leaves still to come: the retry joins its pass
        const unsigned long long later = __ballot(L.eid[lane & (kEntries - 1u)] == nb) & todo;
        if (later) {
          const unsigned long long fm = uniform_u64(L.emask[__builtin_ctzll(later)]);
          if (fl && join == kNo && !lane_bit(fm, lane)) {
            join = nb;
            join_src = b;
            fl = false;
          }
        }
        if (!__any(fl)) continue;
        if (kCount) {
          ++ctr.rounds;
          ctr.follows += popc64(__ballot(fl));
        }
        const auto pa = uniform_patch(m.full, nb);
        skipped = false;
        if (fl) {
          const Hit h = patch_intersect<false, kFast>(pa, s, d, true, PassVote{best, b, false, &skipped});
          consider(h, b, nb, best, L, lane);
        }
        if (kCount && __any(skipped)) ++ctr.shorts;
      }
    }
  }
}

// Trace job of one launch.  Modes: kModeHits (one BezierMesh::intersect per ray -> hits), kModeRefract
// (one BezierLens::refract -> ray', status), kModeStage (the chain over lenses [0, count): refract(INSIDE)
// then refract(OUTSIDE) per lens, a NONE ends the ray -- reference/test.cpp:376-401), kModePower (kModeStage with
// the rays' power: wherever kModeStage is named below, kModePower's fields are the same), kModeSpectral (kModePower
// with each lens's index taken per ray from ri_table by the ray's channel).
struct TraceJob {
  const float *rays;         // input [6][n]
  union {                    // (one word, two modes that never meet: TraceJob keeps its size, see kModeGhost above)
    float *hits;             // kModeHits [13][n]
    uint64_t ghost_base;     // kModeGhost: the roulette's base word for ray 0 of the job (ghost_base())
  };
  float *out_rays;           // kModeRefract / kModeStage [6][n] (may alias rays in kModeStage)
  uint32_t *status;          // kModeRefract / kModeStage [n]
  uint32_t *segments;        // kModeStage, optional [n]
  union {                    // (one word, two modes that never meet, as above)
    const uint32_t *expected;  // kModeRefract: per ray, or null -> expected_all
    float axis_xy[2];          // kModeBidir: the chain's forward axis, x and y
  };
  const uint32_t *alive_in;  // kModeStage: rays with alive_in[i] == NONE are skipped and left untouched
  union {
    uint32_t expected_all;
    float axis_z;              // kModeBidir: and z
  };
  uint32_t n;
  uint32_t ld;               // row stride of rays / out_rays / hits (>= n)
  unsigned long long *wave_clock;  // optional test hook: [2 * waves] start, duration (s_memtime ticks)
  uint32_t wave_real;              // wave_clock holds [4 * waves]: + s_memrealtime start, duration (100 MHz)
  const uint32_t *order;           // optional: block b traces tile order[b] (cost-ordered dispatch, run_fused)
  uint32_t *cost;                  // optional: per tile, its cost bin (sched_bin of the block's duration)
  float *weight;                   // kModePower [n]: the traced rays' power (may alias weight_in)
  const float *weight_in;          // kModePower [n]: the power the rays start with, or null -> 1
  const uint8_t *channel;          // kModeSpectral [n]: the rays' channels
  const float *ri_table;           // kModeSpectral [count][nchan]: lens l's index for channel c (device memory)
  uint32_t nchan;
  uint32_t lossless;               // kModeSpectral: the weights stay as they are (the gain counts as 1)
  uint32_t *bounces;               // kModeTir, optional [n]: the rays' reflections (channel may be null: channel 0)
  uint32_t max_bounces;            // kModeTir: reflections allowed per ray and lens (<= BZR_MAX_BOUNCES)
                                   // kModeCoat: and, in bits 16-31, the mask of coated surfaces (bit 2 l + side)
  float *opl;                      // kModeOpl [n]: the traced rays' optical path length (may alias opl_in)
  const float *opl_in;             // kModeOpl [n]: the path the rays start with, or null -> 0
  float *glass;                    // kModeOpl, optional [n]: the rays' geometric length inside glass
  const float *gap_table;          // kModeMedia [count + 1][nchan]: the index in front of lens l, row count behind the last
                                   // kModeAbsorb: and, kGapPart floats behind it, glass_absorb [count][nchan], and
                                   // kAbsorbPart floats behind that gap_absorb [count][nchan] (the context's buffer)
                                   // kModeCoat: and, kCoatPart floats behind it, the coating table's rows
};

// kTraceWpe: amdgpu_waves_per_eu lower bound for k_trace.  The chain kernel needs 72 VGPRs
// (7 waves per SIMD) by itself; the intersect kernel (kModeHits: a 12-word winner) would take 82 (5 waves)
// since the always list's bundle code, and the bound holds it at 80 (6 waves, as before) without scratch.
constexpr int kTraceWpe = 6;
// BZR_BIDIR_PICK: which (lens, phase) key a k_trace<kModeBidir> wave runs next -- 0: the lowest key held by a travelling
// lane, 1 (default): the key most travelling lanes hold (cfg4 4096^2 at budget 2: 17.86 against 18.05 ms).  The results
// do not depend on it (DESIGN (a), Appendix A).
#ifndef BZR_BIDIR_PICK
#define BZR_BIDIR_PICK 1
#endif
#define BZR_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(kTraceWpe)))
// Threads per k_trace block: its waves share nothing but the CU, so one-wave blocks let
// a finished wave be replaced at once (waves run 1-4 segments; 64 vs 256: cfg4 -3 %, cfg5 -7 %).
// Block b takes 64-ray tile b, the dispatch order itself (XCD x gets every 8th tile), unless the cost order
// below names another: a lens covers the middle of the image, so XCD-contiguous ranges give the middle XCDs
// ~2x the work of the outer ones, and a lens's records fit every XCD's L2 anyway (cfg4: 6.26 ms contiguous,
// 5.67 in dispatch order; cfg5 fused within 1 %).
constexpr int kTraceBlock = 64, kTraceWaves = kTraceBlock / 64;
// Cost-ordered dispatch (BZR_TRACE_SCHED, default on).  A frame's waves differ up to ~6x
// in duration (rim waves meet many patches), and the hardware dispatches blocks in index order as slots free
// up -- greedy list scheduling.  One frame alone therefore ends on whichever long waves were dispatched late.
// Each k_trace block records its duration's cost bin; k_sched_* order the tiles longest-first (a counting
// sort over kSchedBins classes, 4 per octave of cycles), and the context's next fused call of the same size
// dispatches in that order: longest-processing-time-first list scheduling.  Every tile is traced exactly
// once either way and waves share nothing, so the output bits do not depend on the order.
#ifndef BZR_TRACE_SCHED
#define BZR_TRACE_SCHED 1
#endif
// BZR_TRACE_SCHED_REFRESH (default 16): the order is rebuilt from the latest costs on the first call of a size
// and then every this many calls (the three order kernels cost a short frame with others in flight ~8 % when
// run on every call; the costs of a frame loop's tiles barely change from frame to frame).
#ifndef BZR_TRACE_SCHED_REFRESH
#define BZR_TRACE_SCHED_REFRESH 16
#endif
// BZR_TRACE_SCHED_OCT (default 4): cost classes per octave of cycles (1, 2 or 4).  Within a class the tiles keep
// roughly their input order (each k_sched_place block reserves its tiles' places in dispatch order), so coarser
// classes keep more of the input order's locality.
#ifndef BZR_TRACE_SCHED_OCT
#define BZR_TRACE_SCHED_OCT 4
#endif
constexpr uint32_t kSchedBins = 128, kSchedMinTiles = 2048, kSchedThreads = 256;
__device__ __forceinline__ uint32_t sched_bin(unsigned long long cycles) {
  const uint32_t c = static_cast<uint32_t>(cycles > 0xFFFFFFFFull ? 0xFFFFFFFFull : cycles) | 4u;
  const uint32_t lg = 31u - __clz(c);                           // >= 2
  constexpr uint32_t kSub = BZR_TRACE_SCHED_OCT == 4 ? 2u : (BZR_TRACE_SCHED_OCT == 2 ? 1u : 0u);
  const uint32_t key = 4u * lg + (((c >> (lg - 2u)) & 3u) >> (2u - kSub) << (2u - kSub));  // <= 127
  return kSchedBins - 1u - key;                                  // bin 0 = the longest
}
// tiles per bin (hist zeroed by the previous k_sched_scan, or at allocation)
__global__ __launch_bounds__(kSchedThreads) void k_sched_count(const uint32_t *__restrict__ bin, uint32_t tiles,
                                                               uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[kSchedBins];
  for (uint32_t k = threadIdx.x; k < kSchedBins; k += kSchedThreads) h[k] = 0u;
  __syncthreads();
  const uint32_t t = blockIdx.x * kSchedThreads + threadIdx.x;
  if (t < tiles) atomicAdd(&h[bin[t] & (kSchedBins - 1u)], 1u);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kSchedBins; k += kSchedThreads)
    if (h[k]) atomicAdd(&hist[k], h[k]);
}
// offs = exclusive scan of hist; hist back to zero for the next count
__global__ __launch_bounds__(kSchedBins) void k_sched_scan(uint32_t *__restrict__ hist, uint32_t *__restrict__ offs) {
  __shared__ uint32_t v[kSchedBins];
  const uint32_t k = threadIdx.x;
  const uint32_t mine = hist[k];
  v[k] = mine;
  __syncthreads();
  for (uint32_t s = 1; s < kSchedBins; s <<= 1) {
    const uint32_t a = k >= s ? v[k - s] : 0u;
    __syncthreads();
    v[k] += a;
    __syncthreads();
  }
  offs[k] = v[k] - mine;
  hist[k] = 0u;
}
// order[offs[bin] + rank within the bin] = tile (block-aggregated reservations)
__global__ __launch_bounds__(kSchedThreads) void k_sched_place(const uint32_t *__restrict__ bin, uint32_t tiles,
                                                               uint32_t *__restrict__ offs, uint32_t *__restrict__ order) {
  __shared__ uint32_t h[kSchedBins], base[kSchedBins];
  for (uint32_t k = threadIdx.x; k < kSchedBins; k += kSchedThreads) h[k] = 0u;
  __syncthreads();
  const uint32_t t = blockIdx.x * kSchedThreads + threadIdx.x;
  const uint32_t b = t < tiles ? (bin[t] & (kSchedBins - 1u)) : 0u;
  const uint32_t r = t < tiles ? atomicAdd(&h[b], 1u) : 0u;
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kSchedBins; k += kSchedThreads)
    base[k] = h[k] ? atomicAdd(&offs[k], h[k]) : 0u;
  __syncthreads();
  if (t < tiles) order[base[b] + r] = t;
}
template <int kMode, bool kFast, bool kCount>
__global__ __launch_bounds__(kTraceBlock) BZR_TRACE_ATTR void k_trace(LensSet lenses, TraceJob job,
                                                                      unsigned long long *__restrict__ counters) {
  __shared__ TraceLds<kMode> lds[kTraceWaves];
  const uint32_t lane = threadIdx.x & 63u;
  TraceLds<kMode> &L = lds[threadIdx.x >> 6];
  const uint32_t tile = job.order ? job.order[blockIdx.x] : uint32_t(blockIdx.x);
  const uint32_t i = tile * kTraceBlock + threadIdx.x;
  const unsigned long long t_start = (job.wave_clock || job.cost) ? __builtin_amdgcn_s_memtime() : 0ull;
  const unsigned long long r_start = (job.wave_clock && job.wave_real) ? __builtin_amdgcn_s_memrealtime() : 0ull;
  const uint32_t n = job.n;
  TraceCtr ctr;
  bool alive = i < n;
  if (is_stage(kMode) && job.alive_in && alive) alive = job.alive_in[i] != BZR_RR_NONE;
  const bool traced = alive;
  f3 s = mk(0.0f, 0.0f, 0.0f), d = s;
  if (i < n) load_ray(job.rays, job.ld, i, s, d);
  float wgt = 1.0f;  // kModePower: the lane's power (loaded behind the first segment's walk, below)
  const uint32_t nseg = is_stage(kMode) ? 2u * lenses.count : 1u;
  uint32_t st = BZR_RR_NONE, seg = 0;
  if constexpr (has_bidir(kMode)) {
    // The walk is per lane, the segment per wave.  Each lane's place (bidir_open's word) waits in LDS beside the
    // counters, the weight and the two paths.  Each round the wave votes for one key 2 lens + phase among the lanes
    // still travelling (BZR_BIDIR_PICK), runs that lens's trace_segment over the lanes holding it and steps them; it
    // ends when no lane travels.  A ray's step reads nothing but its own words and (ghost_base, its index), so the
    // order of the rounds changes the time alone.  Every round steps at least one lane and a lane makes at most
    // (max_bounces + 1)(2 count + 1) segments: the loop ends.
    static_assert(sizeof(TraceLds<kMode>) * 24u <= 160u * 1024u, "24 waves of k_trace<kModeBidir> per CU");
    L.count[lane] = 0u;
    L.weight[lane] = 1.0f;
    L.opl[lane] = 0.0f;
    L.glass[lane] = 0.0f;
    L.state[lane] = alive ? bidir_open(0u, true, lenses.count) : bidir_ended(BZR_RR_NONE);
    for (uint32_t round = 0;; ++round) {
      const uint32_t w0 = L.state[lane];
      const bool travels = (w0 & kBidirTravels) != 0u;
      uint32_t key = 16u;
#if BZR_BIDIR_PICK == 0
      for (uint32_t k = 0; k < 2u * lenses.count; ++k)  // the lowest key first
        if (__ballot(travels && (w0 & 15u) == k)) {
          key = k;
          break;
        }
#else
      uint32_t most = 0u;  // the key most lanes hold first (ties: the lowest)
      for (uint32_t k = 0; k < 2u * lenses.count; ++k) {
        const uint32_t held = popc64(__ballot(travels && (w0 & 15u) == k));
        if (held > most) {
          most = held;
          key = k;
        }
      }
#endif
      if (key == 16u) break;
      key = (uint32_t)__builtin_amdgcn_readfirstlane(key);
      const uint32_t l = key >> 1;
      const bool gl = (key & 1u) != 0u;  // a glass segment (expected OUTSIDE), or an open one (expected INSIDE)
      const bool act = travels && (w0 & 15u) == key;
      const MeshView &m = lenses.lens[l];
      unsigned long long best;
      const uint32_t r0 = ctr.rounds, p0 = ctr.pairs + ctr.follows;
      trace_segment<kMode, kFast, kCount>(m, s, d, act, best, L, lane, ctr);
      if (kCount) {
        ctr.segments += popc64(__ballot(act));
        if (gl) {
          ctr.rounds_odd += ctr.rounds - r0;
          ctr.runs_odd += ctr.pairs + ctr.follows - p0;
        }
      }
      // (the caller's weight and path behind the first walk, as below; every traced lane is in the first round)
      if (round == 0u && i < n && job.weight_in) L.weight[lane] = job.weight_in[i];
      if (round == 0u && i < n && job.opl_in) L.opl[lane] = job.opl_in[i];
      // everything of the step is read or made here, behind the segment's passes: the lane's word and counters from
      // LDS, its channel and table entries from memory, the draw from the job's base word and the rebuilt ray index
      const uint32_t cnt = L.count[lane];  // segments so far (low half), reflections so far (high half)
      float u = 0.0f;
      if (!job.lossless)
        u = ghost_uniform(job.ghost_base, (uint32_t)__builtin_amdgcn_readfirstlane(tile * kTraceBlock) + threadIdx.x,
                          256u + (cnt & 0xFFFFu));
      Hit h = no_hit();
      uint32_t patch = 0xFFFFFFFFu;
      if (best != ~0ull) h = winner(L, lane, patch);
      const uint32_t ch = (i < n && job.channel) ? job.channel[i] : 0u;
      const bool in_table = ch < job.nchan;
      const uint32_t c = in_table ? ch : 0u;
      const float ri = job.ri_table[l * job.nchan + c];
      const bool back = bidir_back(h.normal, mk(job.axis_xy[0], job.axis_xy[1], job.axis_z));
      // the gap the leg lies in (open: the ray's own) or leads to (glass: behind the surface it met)
      const uint32_t gi = gl ? (back ? l + 1u : l) : ((L.state[lane] & kBidirFwd) ? l : l + 1u);
      const float ng = job.gap_table[gi * job.nchan + c];
      const float eta = div_rn(gl ? ri : ng, gl ? ng : ri);
      f3 os, od;
      float gain = 1.0f;
      uint32_t r;
      if constexpr (has_coat(kMode)) {
        // (the surface's number 2 l + side, its mask bit and the lane's row: l < count, c < nchan, so the row lies in
        // the table's part of the buffer for every lane, hit or not)
        const uint32_t sf = 2u * l + (back ? 1u : 0u);
        r = coat_eta_t(h, eta, s, d, gl ? uint32_t(BZR_RR_OUTSIDE) : uint32_t(BZR_RR_INSIDE), act && in_table,
                       in_table && (cnt >> 16) < (job.max_bounces & 0xFFFFu), !job.lossless, u,
                       ((job.max_bounces >> (16u + sf)) & 1u) != 0u,
                       job.gap_table + kCoatPart + (sf * job.nchan + c) * uint32_t(BZR_COAT_SAMPLES), os, od, gain);
      } else {
        r = bidir_eta_t<true>(h, eta, s, d, gl ? uint32_t(BZR_RR_OUTSIDE) : uint32_t(BZR_RR_INSIDE),
                              in_table && (cnt >> 16) < job.max_bounces, !job.lossless, u, os, od, gain);
      }
      if (!in_table) r = BZR_RR_NONE;
      if (job.lossless) gain = 1.0f;
      if (act) {
        if (r != BZR_RR_NONE) {
          const float len = opl_leg_absorb(s, os, gl ? ri : ng, gl, L.opl[lane], L.glass[lane]);
          const float a = job.gap_table[kGapPart + (gl ? l * job.nchan + c : kAbsorbPart + gi * job.nchan + c)];
          const float leg_att = leg_attenuation(a, len);
          s = os;
          d = od;
          L.weight[lane] = r == kReflected ? L.weight[lane] * leg_att : (L.weight[lane] * leg_att) * gain;
        }
        L.count[lane] = cnt + (r == kReflected ? 0x10001u : 1u);
        L.state[lane] = bidir_next(w0, r, gl, l, gi, back, lenses.count);
      }
    }
    st = (L.state[lane] >> 8) & 7u;
    seg = L.count[lane];
    wgt = L.weight[lane];
    if (traced && job.bounces) job.bounces[i] = seg >> 16;
    seg &= 0xFFFFu;
    if (traced) {
      job.opl[i] = L.opl[lane];
      if (job.glass) job.glass[i] = L.glass[lane];
    }
  } else if constexpr (has_tir(kMode)) {
    // The lens stays wave-uniform: per lens one INSIDE segment (b == 0), then up to 1 + max_bounces OUTSIDE segments
    // over the lanes still inside it (`pend`); lanes that left the lens wait, and a wave vote ends the lens's
    // segments when none is pending.  The last OUTSIDE segment may not reflect, so no lane leaves the loop pending.
    // The lane's counters (segments in the low half, reflections in the high half) and its weight wait in LDS.
    L.count[lane] = 0u;
    L.weight[lane] = 1.0f;
    if constexpr (has_opl(kMode)) {  // the lane's optical path and glass path wait there too
      L.opl[lane] = 0.0f;
      L.glass[lane] = 0.0f;
    }
    for (uint32_t l = 0; l < lenses.count; ++l) {
      if (!__any(alive)) break;
      const MeshView &m = lenses.lens[l];
      bool pend = false;
      for (uint32_t b = 0; b < job.max_bounces + 2u; ++b) {
        const bool act = b == 0u ? alive : pend;
        if (!__any(act)) break;
        unsigned long long best;
        const uint32_t r0 = ctr.rounds, w0 = ctr.pairs + ctr.follows;
        trace_segment<kMode, kFast, kCount>(m, s, d, act, best, L, lane, ctr);
        if (kCount) {
          ctr.segments += popc64(__ballot(act));
          if (b != 0u) {  // back surfaces (odd), bounce segments included
            ctr.rounds_odd += ctr.rounds - r0;
            ctr.runs_odd += ctr.pairs + ctr.follows - w0;
          }
        }
        // (the caller's weight behind the first walk, as below: fetched ahead of the loop, all four kernels came out
        // with 36 B of scratch reserved)
        if (l == 0u && b == 0u && i < n && job.weight_in) L.weight[lane] = job.weight_in[i];
        if constexpr (has_opl(kMode))
          if (l == 0u && b == 0u && i < n && job.opl_in) L.opl[lane] = job.opl_in[i];
        // kModeGhost: the lane's uniform for this segment, both hashes made here from the job's base word, behind the
        // segment's passes and ahead of the winner's words (e is wave-uniform; nothing of the roulette lives across a walk)
        bool draws = false;
        float u = 0.0f;
        if constexpr (has_ghost(kMode)) {
          draws = b != 0u && b <= job.max_bounces && !job.lossless;
          // (the ray's index is put together again from the wave's tile: its product with the golden ratio, two
          // registers, would otherwise be hoisted out of both loops and live across every walk)
          if (draws)
            u = ghost_uniform(job.ghost_base, (uint32_t)__builtin_amdgcn_readfirstlane(tile * kTraceBlock) + threadIdx.x,
                              16u * l + b - 1u);
        }
        Hit h = no_hit();
        uint32_t patch = 0xFFFFFFFFu;
        if (best != ~0ull) h = winner(L, lane, patch);
        const uint32_t ch = (i < n && job.channel) ? job.channel[i] : 0u;  // (reloaded, as kModeSpectral below)
        const bool in_table = ch < job.nchan;
        const float ri = job.ri_table[l * job.nchan + (in_table ? ch : 0u)];
        f3 os, od;
        float gain = 1.0f;
        uint32_t r;
        float nm = ri;  // kModeMedia: the index of the medium this segment's leg lies in
        if constexpr (has_media(kMode)) {
          // the lane's n0 and n2 are read here like ri, behind the segment's passes: nothing new lives across a walk
          const uint32_t c = l * job.nchan + (in_table ? ch : 0u);
          const float n0 = job.gap_table[c];
          if (b == 0u) nm = n0;
          if constexpr (has_ghost(kMode))
            r = ghost_eta_t<true>(h, media_eta(n0, ri, job.gap_table[c + job.nchan], b != 0u), s, d,
                                  b == 0u ? uint32_t(BZR_RR_INSIDE) : uint32_t(BZR_RR_OUTSIDE),
                                  in_table && b <= job.max_bounces, draws, u, os, od, gain);
          else
          r = tir_eta_t<true>(h, media_eta(n0, ri, job.gap_table[c + job.nchan], b != 0u), s, d,
                              b == 0u ? uint32_t(BZR_RR_INSIDE) : uint32_t(BZR_RR_OUTSIDE),
                              in_table && b <= job.max_bounces, os, od, gain);
        } else {
          r = tir_hit_t<true>(h, ri, s, d, b == 0u ? uint32_t(BZR_RR_INSIDE) : uint32_t(BZR_RR_OUTSIDE),
                              in_table && b <= job.max_bounces, os, od, gain);
        }
        if (!in_table) r = BZR_RR_NONE;
        if (job.lossless) gain = 1.0f;
        if (act) {
          float leg_att = 1.0f;  // kModeAbsorb: the leg's attenuation
          if constexpr (has_absorb(kMode)) {
            // the lane's coefficient is read where n0 and n2 were, behind the segment's passes
            if (r != BZR_RR_NONE) {
              const float len = opl_leg_absorb(s, os, nm, b != 0u, L.opl[lane], L.glass[lane]);
              const uint32_t c = l * job.nchan + (in_table ? ch : 0u);
              leg_att = leg_attenuation(job.gap_table[kGapPart + (b != 0u ? 0u : kAbsorbPart) + c], len);
            }
          } else if constexpr (has_media(kMode)) {
            if (r != BZR_RR_NONE) opl_leg_media(s, os, nm, b != 0u, L.opl[lane], L.glass[lane]);
          } else if constexpr (kMode == kModeOpl) {  // the leg from s to the hit (os), before s moves there
            if (r != BZR_RR_NONE) opl_leg(s, os, ri, b != 0u, L.opl[lane], L.glass[lane]);
          }
          L.count[lane] += r == kReflected ? 0x10001u : 1u;
          if (r == kReflected) {  // stays pending; the weight is not touched (kModeAbsorb: but for the leg)
            s = os;
            d = od;
            if constexpr (has_absorb(kMode)) L.weight[lane] = L.weight[lane] * leg_att;
          } else {
            pend = b == 0u && r != BZR_RR_NONE;
            if (r == BZR_RR_NONE) alive = false;
            else {
              s = os;
              d = od;
              if constexpr (has_absorb(kMode)) L.weight[lane] = (L.weight[lane] * leg_att) * gain;
              else L.weight[lane] = L.weight[lane] * gain;
            }
          }
        }
      }
    }
    // (no status register: a lane still alive has left every lens, any other ended NONE)
    st = alive ? uint32_t(BZR_RR_OUTSIDE) : uint32_t(BZR_RR_NONE);
    seg = L.count[lane];
    wgt = L.weight[lane];
    if (traced && job.bounces) job.bounces[i] = seg >> 16;
    seg &= 0xFFFFu;
    if constexpr (has_opl(kMode)) {
      if (traced) {
        job.opl[i] = L.opl[lane];
        if (job.glass) job.glass[i] = L.glass[lane];
      }
    }
  } else
  for (uint32_t k = 0; k < nseg; ++k) {
    if (!__any(alive)) break;
    const MeshView &m = lenses.lens[k >> 1];
    unsigned long long best;
    const uint32_t r0 = ctr.rounds, w0 = ctr.pairs + ctr.follows;
    trace_segment<kMode, kFast, kCount>(m, s, d, alive, best, L, lane, ctr);
    if (kCount) {
      ctr.segments += popc64(__ballot(alive));
      if (k & 1u) {  // per-segment lane utilisation: front (even) vs back (odd) surfaces
        ctr.rounds_odd += ctr.rounds - r0;
        ctr.runs_odd += ctr.pairs + ctr.follows - w0;
      }
    }
    // The caller's weight is first needed by the first refraction.  Loaded here, its register is not live across
    // the first (longest) walk; loaded with the ray, the non-counting kernels came out with 36 B of scratch
    // reserved (never accessed), here with none.
    if constexpr (has_power(kMode))
      if (k == 0u && i < n && job.weight_in) wgt = job.weight_in[i];
    Hit h = no_hit();
    uint32_t patch = 0xFFFFFFFFu;
    if (best != ~0ull) h = winner(L, lane, patch);
    if (kMode == kModeHits) {
      if (alive) store_hit(job.hits, job.ld, i, h, patch);
    } else {
      const uint32_t expected = kMode == kModeRefract ? (job.expected ? (alive ? job.expected[i] : 0u) : job.expected_all)
                                                      : ((k & 1u) ? uint32_t(BZR_RR_OUTSIDE) : uint32_t(BZR_RR_INSIDE));
      f3 os, od;
      float gain = 1.0f;
      float ri = m.ri;
      bool in_table = true;
      // kModeSpectral: the lane's channel is read again from the row behind each segment's passes (a byte, cached
      // since the first segment), so no register holds it across the walks (DESIGN (a), "Spectral channels")
      if constexpr (kMode == kModeSpectral) {
        const uint32_t ch = i < n ? job.channel[i] : 0u;
        in_table = ch < job.nchan;
        ri = job.ri_table[(k >> 1) * job.nchan + (in_table ? ch : 0u)];
      }
      uint32_t r = refract_hit_t<has_power(kMode)>(h, ri, s, d, expected, os, od, gain);
      if constexpr (kMode == kModeSpectral) {
        if (!in_table) r = BZR_RR_NONE;
        if (job.lossless) gain = 1.0f;
      }
      if (alive) {
        ++seg;
        st = r;
        if (r == BZR_RR_NONE) alive = false;
        else {
          s = os;
          d = od;
          if constexpr (has_power(kMode)) wgt = wgt * gain;
        }
      }
    }
  }
  if (kMode != kModeHits && traced) {
    store_ray(job.out_rays, job.ld, i, s, d);
    job.status[i] = st;
    if (is_stage(kMode) && job.segments) job.segments[i] = seg;
    if constexpr (has_power(kMode)) job.weight[i] = wgt;
  }
  if (job.cost && threadIdx.x == 0u) job.cost[tile] = sched_bin(__builtin_amdgcn_s_memtime() - t_start);
  if (job.wave_clock && lane == 0u) {  // the wave's tile (ray index / 64): start tick and duration
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    if (job.wave_real) {  // diagnostic: the wave's shader clock = d(s_memtime) / d(s_memrealtime) x 100 MHz
      const unsigned long long r_end = __builtin_amdgcn_s_memrealtime();
      job.wave_clock[4 * (i >> 6)] = t_start;
      job.wave_clock[4 * (i >> 6) + 1] = t_end - t_start;
      job.wave_clock[4 * (i >> 6) + 2] = r_start;
      job.wave_clock[4 * (i >> 6) + 3] = r_end - r_start;
    } else {
      job.wave_clock[2 * (i >> 6)] = t_start;
      job.wave_clock[2 * (i >> 6) + 1] = t_end - t_start;
    }
  }
  if (kCount && lane < 11u) {  // one atomic per counter per wave, spread over kCounterReplicas copies
    const uint32_t v[11] = {ctr.segments, ctr.pairs, ctr.follows, ctr.ovf, ctr.nodes, ctr.leaves, ctr.gate_tests,
                            ctr.rounds, ctr.rounds_odd, ctr.runs_odd, ctr.shorts};
    const uint32_t id[11] = {BZR_COUNTER_SEGMENTS, BZR_COUNTER_PAIRS, BZR_COUNTER_FOLLOWS, BZR_COUNTER_OVERFLOW_RAYS,
                             BZR_COUNTER_NODE_VISITS, BZR_COUNTER_LEAF_FETCHES, BZR_COUNTER_GATE_TESTS,
                             BZR_COUNTER_NEWTON_ROUNDS, BZR_COUNTER_ROUNDS_ODD, BZR_COUNTER_RUNS_ODD,
                             BZR_COUNTER_SHORT_PASSES};
    uint32_t mine = 0, which = 0;
#pragma unroll
    for (uint32_t k = 0; k < 11u; ++k)
      if (lane == k) {
        mine = v[k];
        which = id[k];
      }
    const uint32_t rep = (blockIdx.x * kTraceWaves + (threadIdx.x >> 6)) % kCounterReplicas;
    if (mine) atomicAdd(&counters[(size_t)rep * BZR_COUNTER_COUNT + which], (unsigned long long)mine);
  }
}

// ------------------------------------------------------------ brute-force path
__global__ __launch_bounds__(kBlock) void k_intersect_scan(MeshView m, const float *__restrict__ rays, uint32_t n,
                                                           float *__restrict__ hits) {
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  f3 s, d;
  load_ray(rays, n, i, s, d);
  uint32_t patch;
  Hit h = mesh_intersect_scan(m, s, d, patch);
  store_hit(hits, n, i, h, patch);
}

__global__ __launch_bounds__(kBlock) void k_refract_scan(MeshView m, const float *__restrict__ rays,
                                                         const uint32_t *__restrict__ expected, uint32_t expected_all,
                                                         uint32_t n, float *__restrict__ out_rays,
                                                         uint32_t *__restrict__ out_status) {
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  f3 s, d, os, od;
  load_ray(rays, n, i, s, d);
  uint32_t patch;
  Hit h = mesh_intersect_scan(m, s, d, patch);
  uint32_t st = refract_hit(h, m.ri, s, d, expected ? expected[i] : expected_all, os, od);
  if (st == BZR_RR_NONE) {
    os = s;
    od = d;
  }
  store_ray(out_rays, n, i, os, od);
  out_status[i] = st;
}

// The chain by the reference's brute-force scan.  kScan 1: with the rays' power (kModePower's brute-force form, the
// A/B reference of the two culled paths); weight_in may be null (1) and may alias out_weight.  kScan 2: kModeSpectral's
// form, the index from ri_table[l][channel[i]].  kScan 3: kModeTir's form -- per lane, a lens's OUTSIDE segment is
// repeated while the ray reflects, up to max_bounces times per lens; channel may be null (channel 0), out_bounces
// is optional.  kScan 4: kModeOpl's form -- kScan 3 with the optical path and the glass path (opl_leg); opl_in may be
// null (0) and may alias out_opl, out_glass is optional.  kScan 5: kModeMedia's form -- kScan 4 with gap_table [count +
// 1][nchan] (tir_eta_t, opl_leg_media).  kScan 6: kModeAbsorb's form -- kScan 5 with the two absorption tables
// [count][nchan] (leg_attenuation).  kScan 7: kModeGhost's form -- kScan 6 with the roulette (ghost_eta_t) for ray number
// first_ray + i (ghost_at: ghost_base for ray 0).  (An int, not an enum: instantiations 0 to 3 keep their names.)
template <int kScan>
__global__ __launch_bounds__(kBlock) void k_chain_scan(LensSet lenses, const float *__restrict__ rays, uint32_t n,
                                                       float *__restrict__ out_rays, uint32_t *__restrict__ out_status,
                                                       uint32_t *__restrict__ out_segments, const float *weight_in,
                                                       float *out_weight, const uint8_t *__restrict__ channel,
                                                       const float *__restrict__ ri_table, uint32_t nchan,
                                                       uint32_t *__restrict__ out_bounces, uint32_t max_bounces,
                                                       const float *opl_in, float *out_opl, float *out_glass,
                                                       const float *__restrict__ gap_table,
                                                       const float *__restrict__ glass_absorb,
                                                       const float *__restrict__ gap_absorb, uint64_t ghost_at,
                                                       float axis_x, float axis_y, float axis_z) {
  constexpr bool kPower = kScan != 0, kSpectral = kScan >= 2, kTir = kScan >= 3, kOpl = kScan >= 4, kMedia = kScan >= 5;
  constexpr bool kAbsorb = kScan >= 6, kGhost = kScan == 7, kBidir = kScan == 8 || kScan == 9, kCoat = kScan == 9;
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  f3 s, d;
  load_ray(rays, n, i, s, d);
  float wgt = 1.0f;
  if constexpr (kPower) wgt = weight_in ? weight_in[i] : 1.0f;
  uint32_t ch = 0u;
  bool in_table = true;
  if constexpr (kSpectral) {
    ch = (kTir && !channel) ? 0u : channel[i];
    in_table = ch < nchan;
    if (!in_table) ch = 0u;
  }
  uint32_t st = BZR_RR_NONE, seg = 0, bounces = 0;
  float opl = 0.0f, glass = 0.0f;
  if constexpr (kOpl) opl = opl_in ? opl_in[i] : 0.0f;
  bool alive = true;
  if constexpr (kBidir) {
    // the walk per lane, event by event (bidir_open's word in a register); max_bounces is the budget of the whole path
    uint32_t w = bidir_open(0u, true, lenses.count);
    while (w & kBidirTravels) {
      const uint32_t l = (w & 15u) >> 1;
      const bool gl = (w & 1u) != 0u;
      uint32_t patch;
      Hit h = mesh_intersect_scan(lenses.lens[l], s, d, patch);
      const float ri = ri_table[l * nchan + ch];
      const bool back = bidir_back(h.normal, mk(axis_x, axis_y, axis_z));
      const uint32_t gi = gl ? (back ? l + 1u : l) : ((w & kBidirFwd) ? l : l + 1u);
      const float ng = gap_table[gi * nchan + ch];
      f3 os, od;
      float gain = 1.0f;
      uint32_t r;
      if constexpr (kCoat) {
        // (the mask rides in max_bounces' high half and the table lies behind gap_absorb's part, as in k_trace)
        const uint32_t sf = 2u * l + (back ? 1u : 0u);
        r = coat_eta_t(h, div_rn(gl ? ri : ng, gl ? ng : ri), s, d, gl ? BZR_RR_OUTSIDE : BZR_RR_INSIDE, in_table,
                       in_table && bounces < (max_bounces & 0xFFFFu), true, ghost_uniform(ghost_at, i, 256u + seg),
                       ((max_bounces >> (16u + sf)) & 1u) != 0u,
                       gap_absorb + kAbsorbPart + (sf * nchan + ch) * uint32_t(BZR_COAT_SAMPLES), os, od, gain);
      } else {
        r = bidir_eta_t<true>(h, div_rn(gl ? ri : ng, gl ? ng : ri), s, d, gl ? BZR_RR_OUTSIDE : BZR_RR_INSIDE,
                              in_table && bounces < max_bounces, true, ghost_uniform(ghost_at, i, 256u + seg), os,
                              od, gain);
      }
      if (!in_table) r = BZR_RR_NONE;
      ++seg;
      if (r != BZR_RR_NONE) {
        const float len = opl_leg_absorb(s, os, gl ? ri : ng, gl, opl, glass);
        const float att_leg = leg_attenuation(gl ? glass_absorb[l * nchan + ch] : gap_absorb[gi * nchan + ch], len);
        s = os;
        d = od;
        wgt = r == kReflected ? wgt * att_leg : (wgt * att_leg) * gain;
        if (r == kReflected) ++bounces;
      }
      w = bidir_next(w, r, gl, l, gi, back, lenses.count);
    }
    st = (w >> 8) & 7u;
    alive = false;
  }
  for (uint32_t l = 0; l < lenses.count && alive; ++l) {
    // kTir: j counts the lens's segments -- INSIDE, then OUTSIDE while the ray reflects (the last may not)
    for (uint32_t j = 0; j < (kTir ? max_bounces + 2u : 2u) && alive; ++j) {
      f3 os, od;
      uint32_t patch;
      ++seg;
      Hit h = mesh_intersect_scan(lenses.lens[l], s, d, patch);
      float gain = 1.0f;
      float ri = lenses.lens[l].ri;
      if constexpr (kSpectral) ri = ri_table[l * nchan + ch];
      float nm = ri;
      if constexpr (kMedia) {
        const float n0 = gap_table[l * nchan + ch];
        if (j == 0u) nm = n0;
        if constexpr (kGhost)
          st = ghost_eta_t<true>(h, media_eta(n0, ri, gap_table[(l + 1u) * nchan + ch], j != 0u), s, d,
                                 j == 0 ? BZR_RR_INSIDE : BZR_RR_OUTSIDE, in_table && j <= max_bounces, j != 0u,
                                 j != 0u ? ghost_uniform(ghost_at, i, 16u * l + j - 1u) : 0.0f, os, od, gain);
        else
        st = tir_eta_t<true>(h, media_eta(n0, ri, gap_table[(l + 1u) * nchan + ch], j != 0u), s, d,
                             j == 0 ? BZR_RR_INSIDE : BZR_RR_OUTSIDE, in_table && j <= max_bounces, os, od, gain);
      } else if constexpr (kTir)
        st = tir_hit_t<true>(h, ri, s, d, j == 0 ? BZR_RR_INSIDE : BZR_RR_OUTSIDE, in_table && j <= max_bounces, os, od, gain);
      else
        st = refract_hit_t<kPower>(h, ri, s, d, j == 0 ? BZR_RR_INSIDE : BZR_RR_OUTSIDE, os, od, gain);
      if constexpr (kSpectral)
        if (!in_table) st = BZR_RR_NONE;
      if constexpr (kAbsorb) {
        if (st != BZR_RR_NONE) {
          const float len = opl_leg_absorb(s, os, nm, j != 0u, opl, glass);
          wgt = wgt * leg_attenuation((j != 0u ? glass_absorb : gap_absorb)[l * nchan + ch], len);
        }
      } else if constexpr (kMedia) {
        if (st != BZR_RR_NONE) opl_leg_media(s, os, nm, j != 0u, opl, glass);
      } else if constexpr (kOpl)
        if (st != BZR_RR_NONE) opl_leg(s, os, ri, j != 0u, opl, glass);
      if constexpr (kTir) {
        if (st == kReflected) {  // inside still: the same lens again, the weight as it is
          s = os;
          d = od;
          ++bounces;
          st = BZR_RR_INSIDE;
          continue;
        }
        if (j != 0u) j = max_bounces + 2u;  // refracted out, or lost: this lens is done
      }
      if (st == BZR_RR_NONE) {
        alive = false;
      } else {
        s = os;
        d = od;
        if constexpr (kPower) wgt = wgt * gain;
      }
    }
  }
  store_ray(out_rays, n, i, s, d);
  out_status[i] = st;
  if (out_segments) out_segments[i] = seg;
  if constexpr (kPower) out_weight[i] = wgt;
  if constexpr (kTir)
    if (out_bounces) out_bounces[i] = bounces;
  if constexpr (kOpl) {
    out_opl[i] = opl;
    if (out_glass) out_glass[i] = glass;
  }
}

template <bool kFast>
__global__ __launch_bounds__(kBlock) void k_patch(MeshView m, const uint32_t *__restrict__ idx,
                                                  const uint32_t *__restrict__ limit, const float *__restrict__ rays,
                                                  uint32_t n, float *__restrict__ hits) {
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  f3 s, d;
  load_ray(rays, n, i, s, d);
  uint32_t pi = idx[i];
  Hit h;
  if (pi < m.n) {
    Patch p = load_patch(m.full + (size_t)rec::kWords * pi);
    h = patch_intersect<false, kFast>(p, s, d, limit[i] != 0u);
  } else {
    h = no_hit();
    h.t = 0.0f;
  }
  store_hit(hits, n, i, h, pi);
}

// ------------------------------------------------------------ host helpers
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

MeshView view_of(const bzr_mesh *m, float ri = 1.0f) {
  return MeshView{m->planar, m->full, m->nodes, m->leaf, m->nodes_near, m->leaf_near, m->obb, m->obb_near,
                  m->always, m->kids, m->kids_near, m->wide, m->wide_near, m->n_always, m->n, m->s_max, m->s_near, ri, m->split,
                  m->split > 1u ? m->swide : m->wide, m->split > 1u ? m->swide_near : m->wide_near};
}
unsigned grid_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

bzr_status ensure_buffer(void *&buf, size_t &have, size_t bytes) {
  if (have >= bytes) return BZR_OK;
  if (buf) BZR_HIP(hipFree(buf));
  buf = nullptr;
  have = 0;
  BZR_HIP(hipMalloc(&buf, bytes));
  have = bytes;
  return BZR_OK;
}

// A context-owned allocation (`buf`, `have` bytes) grown to what `layout` takes, then carved by it
// (host/staging.hpp: the layout runs twice, so it is the one statement of what the call stages).
using bzr_staging::Staging;
template <typename Layout>
bzr_status carve_buffer(void *&buf, size_t &have, Layout &&layout) {
  const bzr_status s =
      bzr_staging::carve(buf, [&](size_t bytes) { return ensure_buffer(buf, have, bytes); }, layout, bzr_status(-1));
  return s == -1 ? set_error(BZR_ERR_INVALID_ARGUMENT, "staging layout took different sizes in its two passes") : s;
}

// The caller's rays into the kernels' rows `r` ([6][n] on the device): copied from host memory and/or
// transposed from [n][6] records (BZR_RAYS_AOS; a host source lands in `tmp` first).
bzr_status rays_in(bzr_ctx *ctx, const float *rays, float *r, uint32_t n, bool host, bool aos, float *tmp) {
  if (host) BZR_HIP(hipMemcpyAsync(aos ? tmp : r, rays, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  if (aos) BZR_HIP(bzr_rays_relayout(ctx->stream, host ? tmp : rays, r, n, true));
  return BZR_OK;
}
// The kernels' output rows `d_out` to the caller's out_rays: transposed to [n][6] records (BZR_RAYS_AOS; for a
// host destination into `tmp` first) and/or copied to host memory (queued, not waited for).
bzr_status rays_out(bzr_ctx *ctx, const float *d_out, float *out_rays, uint32_t n, bool host, bool aos, float *tmp) {
  if (aos) BZR_HIP(bzr_rays_relayout(ctx->stream, d_out, host ? tmp : out_rays, n, false));
  if (host) BZR_HIP(hipMemcpyAsync(out_rays, aos ? tmp : d_out, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->stream));
  return BZR_OK;
}

bzr_status check_ctx_mesh(bzr_ctx *ctx, const bzr_mesh *mesh) {
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (!mesh) return set_error(BZR_ERR_INVALID_ARGUMENT, "null mesh");
  if (mesh->device != ctx->device) return set_error(BZR_ERR_INVALID_ARGUMENT, "mesh lives on another device");
  return BZR_OK;
}

bool use_scan(uint32_t flags) { return (flags & BZR_ACCEL_NONE) != 0; }
bool use_fast(uint32_t flags) { return (flags & BZR_MODE_FAST) != 0; }
// Culled-path pipeline for a call of n rays over meshes of at most nb patches (include/bzr.h): forced by
// BZR_PIPELINE_STAGED / BZR_PIPELINE_FUSED, otherwise fused for dense batches (rays per patch >= 256;
// rays per patch stands in for how many patches a wave's 64 rays meet).  Chosen for callers that keep
// frames in flight (bench.py): cfg4 at 4096^2 (5461 rays per patch) and cfg2 at 1024^2
// (341) run fused -- cfg2 5593 vs 5205 Mrays/s at three / two frames in flight, though a lone cfg2 frame
// is faster staged; cfg3 (145) and cfg5 (223) run staged.  Meshes of kStagedPatchLimit patches or more
// (the staged key and pair encoding's limit) always run fused, which takes any mesh.
constexpr uint64_t kFusedRaysPerPatch = 256;
bool use_staged(uint32_t flags, uint64_t n, uint64_t nb) {
  if (flags & BZR_PIPELINE_STAGED) return true;
  if (flags & BZR_PIPELINE_FUSED) return false;
  return nb < kStagedPatchLimit && n < kFusedRaysPerPatch * nb;
}
// BZR_MODE_FAST runs on the culled pipeline's kernels only; the brute-force scan is the parity reference.
constexpr uint32_t kKnownFlags = BZR_DEVICE_PTRS | BZR_MODE_FAST | BZR_ACCEL_NONE | BZR_PIPELINE_STAGED | BZR_PIPELINE_FUSED;
// aos_ok: the call takes BZR_RAYS_AOS (the ray-batch entries: intersect, refract, trace_chain)
bzr_status check_flags(uint32_t flags, bool aos_ok = false) {
  if ((flags & BZR_RAYS_AOS) && !aos_ok) return set_error(BZR_ERR_INVALID_ARGUMENT, "BZR_RAYS_AOS is not accepted by this call");
  if (aos_ok) flags &= ~uint32_t(BZR_RAYS_AOS);
  if (flags & ~kKnownFlags) return set_error(BZR_ERR_INVALID_ARGUMENT, "unknown flag bits " + std::to_string(flags & ~kKnownFlags));
  if ((flags & BZR_PIPELINE_STAGED) && (flags & BZR_PIPELINE_FUSED))
    return set_error(BZR_ERR_INVALID_ARGUMENT, "BZR_PIPELINE_STAGED and BZR_PIPELINE_FUSED are exclusive");
  if (use_fast(flags) && use_scan(flags))
    return set_error(BZR_ERR_INVALID_ARGUMENT, "BZR_MODE_FAST needs the culled path (drop BZR_ACCEL_NONE)");
  return BZR_OK;
}

hipEvent_t take_event(bzr_ctx *ctx) {
  if (!ctx->spare.empty()) {
    hipEvent_t e = ctx->spare.back();
    ctx->spare.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

// Launch on `stream`; with timing enabled, bracket the launch with events on that stream.
template <typename... Args>
void launch_on(bzr_ctx *ctx, hipStream_t stream, dim3 block, int kernel_id, void (*kernel)(Args...), dim3 grid,
               typename std::decay<Args>::type... args) {
  const bool timed = ctx->timing && kernel_id >= 0;
  hipEvent_t a = nullptr, b = nullptr;
  if (timed) {
    a = take_event(ctx);
    b = take_event(ctx);
    (void)hipEventRecord(a, stream);
  }
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
  if (timed) {
    (void)hipEventRecord(b, stream);
    ctx->marks.push_back({kernel_id, a, b});
  }
}
// Launch on the context's stream.
template <typename... Args>
void launch(bzr_ctx *ctx, int kernel_id, void (*kernel)(Args...), dim3 grid, typename std::decay<Args>::type... args) {
  launch_on(ctx, ctx->stream, dim3(kBlock), kernel_id, kernel, grid, args...);
}

// Event bracket around a group of launches (timing enabled only).
struct Span {
  bzr_ctx *ctx;
  int id;
  hipEvent_t a = nullptr;
  Span(bzr_ctx *c, int kernel_id) : ctx(c), id(kernel_id) {
    if (ctx->timing) {
      a = take_event(ctx);
      (void)hipEventRecord(a, ctx->stream);
    }
  }
  ~Span() {
    if (!a) return;
    hipEvent_t b = take_event(ctx);
    (void)hipEventRecord(b, ctx->stream);
    ctx->marks.push_back({id, a, b});
  }
};

// Blocks of `kernel` (kBlock threads) the device holds at once: the persistent-grid size.
template <typename K>
uint32_t resident_blocks(bzr_ctx *ctx, K kernel) {
  static thread_local std::vector<std::pair<const void *, uint32_t>> cache;  // (kernel, blocks) per device below
  const void *key = reinterpret_cast<const void *>(kernel);
  for (auto const &c : cache)
    if (c.first == key) return c.second;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 1) cus = 256;
  uint32_t blocks = static_cast<uint32_t>(per_cu) * static_cast<uint32_t>(cus);
  cache.emplace_back(key, blocks);
  return blocks;
}

// Grid of the persistent staged kernel k_newton in units of the device's resident capacity.  A grid
// of exactly the resident capacity holds every wave slot until the kernel ends, so another frame's kernels (frames
// in flight, their own streams) cannot start beside it; k x capacity ends in k generations of blocks, between
// which the dispatcher also takes the other streams' blocks.
// 2 x the resident capacity on meshes of at least 2^17 patches, else 1 x.
// Measured (profiles/r06_ab_gridx_cfg5.jsonl, same bits): cfg5 (301 056 patches, 8 M-ray chunks) k_newton 4.33 ->
// 4.15 ms per lone frame and +0.8 to +1.5 % at bench level on three boxes, 4 x / 8 x / 16 x lose (every wave's
// follow-list flush is an atomic on one counter); cfg3 (28 800 patches) k_newton 0.174 -> 0.205 ms lone, -1 to -2 %
// at bench level.
constexpr uint32_t kNewtonGrid2Patches = 1u << 17;
uint32_t newton_gridx(uint32_t nb) { return nb >= kNewtonGrid2Patches ? 2u : 1u; }
constexpr uint32_t kResolveBlocks = 1024u;  // k_resolve's block cap for the follow retries

// Workspace of the culled path for chunks of up to `chunk` rays over meshes of up to `nb` patches.
using SplitIt = hipcub::TransformInputIterator<unsigned long long, BucketSplit, const uint32_t *>;
// The layout: `hist` directly behind `ctr` (run_culled clears both with one memset), the scan's `cub_bytes` last.
constexpr void work_layout(Staging &st, Work &w, uint32_t chunk, uint32_t nb, size_t cub_bytes) {
  const uint32_t hn = nb;  // histogram slots, one per patch
  const size_t cap = (size_t)kMaxCand * chunk;
  w.ctr = st.take<uint32_t>(8);
  w.hist = st.take<uint32_t>(hn + 1);
  w.offs = st.take<unsigned long long>(hn + 1);
  w.cand = st.take<uint32_t>(cap);
  w.rank = st.take<uint32_t>(cap);
  w.count = st.take<uint32_t>(chunk);
  w.key = st.take<unsigned long long>(chunk);
  w.slot = st.take<float>(kSlotWords * cap);
  w.pairs = st.take<uint2>(cap + 64 * ((size_t)nb + 1));  // dense chunks (< 64 padding slots per patch) + sparse
  w.fol = st.take<uint32_t>(cap);
  w.ovf = st.take<uint32_t>(chunk);
  w.cub = st.take<char>(cub_bytes ? cub_bytes : 1);
  w.cub_bytes = cub_bytes;
  w.cap = static_cast<uint32_t>(cap);
}
bzr_status ensure_work(bzr_ctx *ctx, uint32_t chunk, uint32_t nb, Work &w) {
  size_t cub_bytes = 0;
  BZR_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, SplitIt(static_cast<const uint32_t *>(nullptr), BucketSplit()),
                                           static_cast<unsigned long long *>(nullptr), nb + 1, ctx->stream));
  const size_t had = ctx->work_bytes;
  if (bzr_status s = carve_buffer(ctx->work, ctx->work_bytes, [&](Staging &st) { work_layout(st, w, chunk, nb, cub_bytes); }))
    return s;
  if (ctx->work_bytes != had) ctx->zero_ctr = nullptr;  // reallocated (possibly at the same address)
  return BZR_OK;
}

// Rays per chunk of the staged path, whose workspace is ~2.7 KB per ray + 0.5 KB per patch: at most
// kChunk (2^23 = 8M rays, ~23 GB) and at most what a quarter of the device's free memory holds (at the
// context's first staged call), with the
// batch split into equal chunks (rounded to whole waves).  Measured on cfg5 (67M rays): 1M-ray chunks
// 28.3 ms per frame, 4M 21.4, 8M 20.0, 16M 20.0 -- small chunks leave the kernels short of waves.
constexpr uint32_t kChunkLog2 = 23, kChunk = 1u << kChunkLog2;
// what work_layout takes per ray (per list slot cand, rank, slot, pair and fol; per ray count, key and ovf): the
// growth of the layout over one wave of rays, with the mesh and the scan's bytes held fixed
constexpr size_t work_bytes(uint32_t chunk) {
  Work w{};
  return bzr_staging::measure([&](Staging &st) { work_layout(st, w, chunk, 0, 0); });
}
constexpr size_t kWorkBytesPerRay = (work_bytes(128) - work_bytes(64)) / 64;
static_assert(kChunkLog2 <= 26, "pair records hold a chunk's ray index in 26 bits");
static_assert((uint64_t)kMaxCand * kChunk + 64ull * (kStagedPatchLimit + 1) < (1ull << 32),
              "32-bit pair indices");
static_assert(kMaxCand <= 64, "winner keys hold a list slot in 6 bits");
// The chunking rule, host arithmetic only (bzr_debug_chunk_plan exports it).  Cap: whole waves, at least one, at most
// kChunk; free_b == 0 (free memory unknown) gives kChunk.
uint32_t chunk_cap_of(uint64_t free_b) {
  uint64_t cap = kChunk;
  if (free_b) cap = std::min<uint64_t>(cap, std::max<uint64_t>(free_b / 4 / kWorkBytesPerRay / 64 * 64, 64));
  return static_cast<uint32_t>(cap);
}
// Chunk length for n rays under `cap`: n itself when it fits, else equal pieces rounded up to whole waves.
uint32_t chunk_len(uint64_t n, uint64_t cap) {
  const uint64_t pieces = (n + cap - 1) / cap;
  if (pieces <= 1) return static_cast<uint32_t>(std::max<uint64_t>(n, 1));
  return static_cast<uint32_t>(std::min<uint64_t>(cap, ((n + pieces - 1) / pieces + 63) / 64 * 64));
}
// The cap in force: the automatic one (sized once), lowered by the test hook bzr_debug_chunk_cap if set.
uint32_t chunk_cap(bzr_ctx *ctx) {
  if (!ctx->chunk_cap) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    ctx->chunk_cap = chunk_cap_of(free_b);
  }
  return ctx->chunk_limit ? std::min(ctx->chunk_cap, ctx->chunk_limit) : ctx->chunk_cap;
}
uint32_t chunk_for(bzr_ctx *ctx, uint64_t n) { return chunk_len(n, chunk_cap(ctx)); }

// One BezierMesh::intersect per ray of rays [off, off + n) (+ refraction, per kMode).
template <int kMode, bool kFast>
bzr_status run_culled(bzr_ctx *ctx, const MeshView &mv, const float *rays, uint32_t ld, uint32_t off, uint32_t n,
                      const uint32_t *alive, const Out &o, Work &w) {
  const uint32_t nb = mv.n;
  const uint32_t hn = nb;
  const bool small_scan = hn + 1 <= kScanSmall;
  if (nb >= kStagedPatchLimit)  // (the automatic choice sends such meshes to the fused path, which takes any mesh)
    return set_error(BZR_ERR_INVALID_ARGUMENT, "staged path: mesh of " + std::to_string(nb) +
                                                   " patches, at or above 2^25; use BZR_PIPELINE_FUSED");
  if (!(ctx->zero_ctr == w.ctr && ctx->zero_hn >= hn))  // counters + histogram [0, hn] to zero
    BZR_HIP(hipMemsetAsync(w.ctr, 0, reinterpret_cast<char *>(w.hist + hn + 1) - reinterpret_cast<char *>(w.ctr),
                           ctx->stream));
  ctx->zero_ctr = nullptr;  // valid again only once this segment is fully enqueued
  unsigned long long *const ctr = (ctx->counting && ctx->counters) ? ctx->counters : nullptr;
  if (BZR_TRAV_ABLOCK && mv.n_always > kAblockMin && mv.n_always <= kAblockMax)  // block-level always-list pre-test
    launch_on(ctx, ctx->stream, dim3(kAblockBlock), BZR_KERNEL_TRAVERSE, k_traverse<kAblockBlock, BZR_TRAV_ABLOCK, kFast>,
              dim3((n + kAblockBlock - 1) / kAblockBlock), mv, rays, ld, off, alive, n, w, ctr);
  else
    launch_on(ctx, ctx->stream, dim3(kTravBlock), BZR_KERNEL_TRAVERSE, k_traverse<kTravBlock, 0, kFast>,
              dim3((n + kTravBlock - 1) / kTravBlock), mv, rays, ld, off, alive, n, w, ctr);
  {
    Span sp(ctx, BZR_KERNEL_BUCKET);
    if (small_scan)
      hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(kScanThreads), 0, ctx->stream, w.hist, w.offs, hn + 1);
    else
      BZR_HIP(hipcub::DeviceScan::ExclusiveSum(w.cub, w.cub_bytes, SplitIt(w.hist, BucketSplit()), w.offs, hn + 1,
                                               ctx->stream));
    launch(ctx, -1, k_place, dim3(grid_for(std::max(n, nb))), n, nb, w,
           (ctx->counting && ctx->counters) ? w.ctr + 3 : nullptr);
  }
  // persistent grid: the resident capacity of the device, never more than the worst-case chunk count
  const uint32_t gn = std::min<uint32_t>(std::max<uint32_t>((kMaxCand * n + kBlock - 1) / kBlock, 1u),
                                         resident_blocks(ctx, k_newton<kFast>) * newton_gridx(nb));
  launch(ctx, BZR_KERNEL_NEWTON, k_newton<kFast>, dim3(gn), mv.full, w.offs + hn, w.pairs, rays, ld, off, n, w.slot, w.key,
         w.fol, w.ctr);
  launch(ctx, BZR_KERNEL_NEWTON_LANE, k_newton_lane<kFast>, dim3(std::min<uint32_t>(std::max<uint32_t>(n / 1024u, 1u), 1024u)),
         mv.full, w.offs + hn, w.pairs, rays, ld, off, n, w.slot, w.key, w.fol, w.ctr);
  {  // follow retries + overflow rays (whose keys the Newton stage left untouched: their lists are empty)
    const uint64_t items = (uint64_t)n * ((nb + kOvfSlice - 1) / kOvfSlice);
    const uint32_t grid = std::max(std::min<uint32_t>(grid_for(n / 8 + 1), kResolveBlocks),
                                   (uint32_t)std::min<uint64_t>(items, kOverflowBlocks));
    launch(ctx, BZR_KERNEL_FOLLOW, k_resolve<kFast>, dim3(std::max<uint32_t>(grid, 1u)), mv, rays, ld, off, n, w);
  }
  if (ctx->counting && ctx->counters)  // before k_finish, which clears the counters
    hipLaunchKernelGGL(k_count, dim3(1), dim3(64), 0, ctx->stream, w, nb, ctx->counters);
  if (kMode == kModeHits && BZR_FINISH_NORAY)  // the overflow rays first (k_finish clears their count)
    // (grid-stride over the overflow list, whose length only the device knows.  64 blocks: a batch whose rays all
    // lie beyond s_max re-evaluates them 16 K at a time, while k_resolve's full scan of the same rays costs a gate per
    // ray and patch; 512 blocks cost cfg3 frames ~1 % in launch for nothing on the bench configs)
    launch(ctx, BZR_KERNEL_FINISH, k_finish_ovf<kFast>, dim3(std::min<uint32_t>(grid_for(n), 64u)), mv, rays, ld, off,
           w, o);
  launch(ctx, BZR_KERNEL_FINISH, k_finish<kMode, kFast>, dim3(grid_for(n)), mv, rays, ld, off, n, w, o);
  BZR_HIP(hipGetLastError());
  ctx->zero_ctr = w.ctr;  // k_place cleared the histogram, k_finish the counters
  ctx->zero_hn = hn;
  return BZR_OK;
}

// The fused path: one k_trace launch for the whole job (no workspace, no chunking).
template <int kMode>
bzr_status run_fused(bzr_ctx *ctx, const LensSet &set, const TraceJob &job, uint32_t flags) {
  if (job.n == 0) return BZR_OK;
  const bool fast = use_fast(flags), count = ctx->counting && ctx->counters;
  const dim3 grid((job.n + kTraceBlock - 1) / kTraceBlock), block(kTraceBlock);
  TraceJob j = job;
  j.wave_clock = (ctx->wave_clock && ctx->wave_clock_cap >= (job.n + 63) / 64) ? ctx->wave_clock : nullptr;
  j.wave_real = ctx->wave_clock_real ? 1u : 0u;
  j.order = nullptr;
  j.cost = nullptr;
  const uint32_t tiles = grid.x;
  const bool sched = BZR_TRACE_SCHED && tiles >= kSchedMinTiles;
  if (sched) {  // this call's tile costs; the order of the last call of the same size, if any
    if (ctx->sched_cap < tiles) {
      if (ctx->sched) BZR_HIP(hipFree(ctx->sched));
      ctx->sched = nullptr;
      ctx->sched_cap = ctx->sched_waves = 0;
      BZR_HIP(hipMalloc(&ctx->sched, ((size_t)2 * tiles + 2 * kSchedBins) * sizeof(uint32_t)));
      BZR_HIP(hipMemsetAsync(ctx->sched + (size_t)2 * tiles, 0, kSchedBins * sizeof(uint32_t), ctx->stream));
      ctx->sched_cap = tiles;
    }
    j.cost = ctx->sched;
    // the saved order belongs to a call of this size over the same lenses in the same mode (any other
    // call rebuilds it -- its bits would not change either way, the order is a permutation of whole tiles)
    uint64_t key = 0xcbf29ce484222325ull ^ (uint64_t)kMode;
    for (uint32_t l = 0; l < set.count; ++l)
      key = (key ^ reinterpret_cast<uintptr_t>(set.lens[l].full)) * 0x100000001b3ull;
    if (ctx->sched_key != key) {
      ctx->sched_key = key;
      ctx->sched_waves = 0;
    }
    if (ctx->sched_waves == tiles) {
      j.order = ctx->sched + ctx->sched_cap;
      ++ctx->sched_calls;
    } else {
      ctx->sched_calls = 0;
    }
  }
  const bool rebuild = sched && ctx->sched_calls % BZR_TRACE_SCHED_REFRESH == 0;
  auto go = [&](auto kernel) { launch_on(ctx, ctx->stream, block, BZR_KERNEL_TRACE, kernel, grid, set, j, ctx->counters); };
  if (fast) {
    if (count) go(k_trace<kMode, true, true>);
    else go(k_trace<kMode, true, false>);
  } else {
    if (count) go(k_trace<kMode, false, true>);
    else go(k_trace<kMode, false, false>);
  }
  BZR_HIP(hipGetLastError());
  if (rebuild) {  // the next calls' order: tiles longest-first (counting sort of the cost bins)
    uint32_t *order = ctx->sched + ctx->sched_cap, *hist = ctx->sched + (size_t)2 * ctx->sched_cap, *offs = hist + kSchedBins;
    const dim3 sg((tiles + kSchedThreads - 1) / kSchedThreads);
    hipLaunchKernelGGL(k_sched_count, sg, dim3(kSchedThreads), 0, ctx->stream, ctx->sched, tiles, hist);
    hipLaunchKernelGGL(k_sched_scan, dim3(1), dim3(kSchedBins), 0, ctx->stream, hist, offs);
    hipLaunchKernelGGL(k_sched_place, sg, dim3(kSchedThreads), 0, ctx->stream, ctx->sched, tiles, offs, order);
    BZR_HIP(hipGetLastError());
    ctx->sched_waves = tiles;
  }
  return BZR_OK;
}

// kModeSpectral's index table into the context's device copy.  The copy is rewritten only when the table differs
// from what it holds, and then only after everything queued on the stream has finished (kernels of an earlier
// device-pointer call may still read the old one); the copy itself is synchronous, so the caller's table is not
// read after the call returns.  A frame loop with one table therefore uploads it once.
constexpr uint32_t kMaxChannels = BZR_MAX_CHANNELS;
// (one allocation: kModeMedia's gap table [nlens + 1][nchan] lies behind the index table's kMaxLenses rows)
constexpr size_t kRiTableFloats = (size_t)kMaxLenses * kMaxChannels, kGapTableFloats = kGapPart;
// (and kModeAbsorb's two tables [nlens][nchan] behind those: the glass part, then the gap part)
constexpr size_t kAbsorbTableFloats = kAbsorbPart;
constexpr size_t kGlassAbsorbAt = kRiTableFloats + kGapTableFloats, kGapAbsorbAt = kGlassAbsorbAt + kAbsorbTableFloats;
// (and kModeCoat's rows behind those)
constexpr size_t kCoatAt = kGapAbsorbAt + kAbsorbTableFloats;
static_assert(kCoatAt == kRiTableFloats + kCoatPart, "the kernels reach the coating's rows through gap_table");
bzr_status upload_ri_table(bzr_ctx *ctx, const float *table, uint32_t nlens, uint32_t nchan) {
  const size_t count = (size_t)nlens * nchan;
  if (!ctx->ri_table) BZR_HIP(hipMalloc(&ctx->ri_table, (kCoatAt + kCoatFloats) * sizeof(float)));
  if (ctx->ri_table_host.size() == count && std::memcmp(ctx->ri_table_host.data(), table, count * sizeof(float)) == 0)
    return BZR_OK;
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  ctx->ri_table_host.clear();
  BZR_HIP(hipMemcpy(ctx->ri_table, table, count * sizeof(float), hipMemcpyHostToDevice));
  ctx->ri_table_host.assign(table, table + count);
  return BZR_OK;
}
// kModeMedia's gap table beside it, under the same rule and with a host copy of its own: a call that changes only one
// of the two tables rewrites that one, and the entry points that take no gap table never touch this half.  A null
// table is vacuum, every entry 1.  (upload_ri_table, called first, has allocated the buffer.)
bzr_status upload_gap_table(bzr_ctx *ctx, const float *table, uint32_t nlens, uint32_t nchan) {
  const size_t count = (size_t)(nlens + 1) * nchan;
  const std::vector<float> ones(table ? 0 : count, 1.0f);
  if (!table) table = ones.data();
  if (ctx->gap_table_host.size() == count && std::memcmp(ctx->gap_table_host.data(), table, count * sizeof(float)) == 0)
    return BZR_OK;
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  ctx->gap_table_host.clear();
  BZR_HIP(hipMemcpy(ctx->ri_table + kRiTableFloats, table, count * sizeof(float), hipMemcpyHostToDevice));
  ctx->gap_table_host.assign(table, table + count);
  return BZR_OK;
}
// kModeAbsorb's two parts behind it, each under the same rule with a host copy of its own (`host`, of the part at
// float offset `at`): compared and rewritten on its own, and never touched by the entry points that take no
// absorption.  A null table is all zero.
bzr_status upload_absorb_table(bzr_ctx *ctx, const float *table, uint32_t nlens, uint32_t nchan, size_t at,
                               std::vector<float> &host) {
  const size_t count = (size_t)nlens * nchan;
  const std::vector<float> zeros(table ? 0 : count, 0.0f);
  if (!table) table = zeros.data();
  if (host.size() == count && std::memcmp(host.data(), table, count * sizeof(float)) == 0) return BZR_OK;
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  host.clear();
  BZR_HIP(hipMemcpy(ctx->ri_table + at, table, count * sizeof(float), hipMemcpyHostToDevice));
  host.assign(table, table + count);
  return BZR_OK;
}
// A coating's checks (include/bzr.h bzr_coating): the mask's bits below 2 nlens, a table where the mask is not zero,
// every entry of a masked row finite and in [0, 1].  Rows of unmasked surfaces are not read.
bzr_status check_coating(const bzr_coating *coat, uint32_t nlens, uint32_t nchan) {
  if (!coat || coat->mask == 0u) return BZR_OK;
  if (nlens < 16u && (coat->mask >> (2u * nlens)) != 0u)
    return set_error(BZR_ERR_INVALID_ARGUMENT, "coating mask names a surface at or above 2 nlens");
  if (!coat->table) return set_error(BZR_ERR_INVALID_ARGUMENT, "coating mask without a table");
  const size_t per = (size_t)nchan * BZR_COAT_SAMPLES;
  for (uint32_t sf = 0; sf < 2u * nlens; ++sf) {
    if (!((coat->mask >> sf) & 1u)) continue;
    for (size_t k = 0; k < per; ++k) {
      const float v = coat->table[sf * per + k];
      if (!(v >= 0.0f) || !(v <= 1.0f))
        return set_error(BZR_ERR_INVALID_ARGUMENT, "coating table entries must be finite and in [0, 1]");
    }
  }
  return BZR_OK;
}
// kModeCoat's rows behind the absorption parts, under upload_absorb_table's rule: the context keeps the mask, the shape
// and the masked rows of what the device holds (coat_key, coat_host: the rows packed in surface order), and the device
// copy is rewritten only when one of them differs.  A masked row is then always one the device has received -- a row of
// zeros too, which an image with zeros for the unmasked rows could not tell from a row never sent.  Only the masked
// rows are copied.  A call without coated surfaces touches nothing.
bzr_status upload_coat_table(bzr_ctx *ctx, const bzr_coating *coat, uint32_t nlens, uint32_t nchan) {
  if (!coat || coat->mask == 0u) return BZR_OK;
  const size_t per = (size_t)nchan * BZR_COAT_SAMPLES;
  const uint64_t key = ((uint64_t)coat->mask << 32) | ((uint64_t)nlens << 16) | nchan;
  std::vector<float> rows;
  for (uint32_t sf = 0; sf < 2u * nlens; ++sf)
    if ((coat->mask >> sf) & 1u) rows.insert(rows.end(), coat->table + sf * per, coat->table + (sf + 1u) * per);
  if (ctx->coat_key == key && ctx->coat_host.size() == rows.size() &&
      std::memcmp(ctx->coat_host.data(), rows.data(), rows.size() * sizeof(float)) == 0)
    return BZR_OK;
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  ctx->coat_key = 0;
  ctx->coat_host.clear();
  size_t at = 0;
  for (uint32_t sf = 0; sf < 2u * nlens; ++sf)
    if ((coat->mask >> sf) & 1u) {
      BZR_HIP(hipMemcpy(ctx->ri_table + kCoatAt + sf * per, rows.data() + at, per * sizeof(float), hipMemcpyHostToDevice));
      at += per;
    }
  ctx->coat_host = std::move(rows);
  ctx->coat_key = key;
  return BZR_OK;
}
// Every used entry of an absorption table finite and not below zero (a null table is all zero).
bzr_status check_absorb_table(const float *table, uint32_t nlens, uint32_t nchan, const char *what) {
  if (!table) return BZR_OK;
  for (size_t k = 0; k < (size_t)nlens * nchan; ++k)
    if (!(table[k] >= 0.0f) || !std::isfinite(table[k])) return set_error(BZR_ERR_INVALID_ARGUMENT, what);
  return BZR_OK;
}
// Every used entry of a gap table finite and above zero (a null table is vacuum).
bzr_status check_gap_table(const float *gap_table, uint32_t nlens, uint32_t nchan) {
  if (!gap_table) return BZR_OK;
  for (size_t k = 0; k < (size_t)(nlens + 1) * nchan; ++k)
    if (!(gap_table[k] > 0.0f) || !std::isfinite(gap_table[k]))
      return set_error(BZR_ERR_INVALID_ARGUMENT, "gap_table entries must be finite and > 0");
  return BZR_OK;
}
bzr_status check_channels(const float *ri_table, uint32_t nchan) {
  if (nchan == 0 || nchan > kMaxChannels) return set_error(BZR_ERR_INVALID_ARGUMENT, "nchan must be 1..64");
  if (!ri_table) return set_error(BZR_ERR_INVALID_ARGUMENT, "null ri_table");
  return BZR_OK;
}

uint32_t max_patches(const LensSet &set) {
  uint32_t nb = 0;
  for (uint32_t l = 0; l < set.count; ++l) nb = std::max(nb, set.lens[l].n);
  return nb;
}

LensSet single_lens(const MeshView &mv) {
  LensSet set{};
  set.count = 1;
  set.lens[0] = mv;
  return set;
}

template <int kMode>
bzr_status run_segment(bool fast, bzr_ctx *ctx, const MeshView &mv, const float *rays, uint32_t ld, uint32_t off,
                       uint32_t n, const uint32_t *alive, const Out &o, Work &w) {
  return fast ? run_culled<kMode, true>(ctx, mv, rays, ld, off, n, alive, o, w)
              : run_culled<kMode, false>(ctx, mv, rays, ld, off, n, alive, o, w);
}

// The chain of `job` over `set`: one fused launch, or (`staged`) stage by stage in chunks of `ch` rays with the
// workspace `w` (ensure_work for `ch` and the set's largest mesh): out_rays holds the rays in flight, status != NONE
// marks them alive, `pend` is kModeTir's pending row [job.ld].  A job without alive_in starts with the chain's first
// stage, which reads job.rays and writes every ray's ray / status / segments (no copy or fill launches).
template <int kMode>
bzr_status run_chain(bzr_ctx *ctx, const LensSet &set, const TraceJob &job, uint32_t flags, bool staged, uint32_t *pend,
                     uint32_t ch, Work &w) {
  constexpr bool kTir = has_tir(kMode);
  // kModeAbsorb reads its two absorption parts through gap_table (kGapPart): the pointer must be the context's
  if (has_absorb(kMode) && job.gap_table != ctx->ri_table + kRiTableFloats)
    return set_error(BZR_ERR_INVALID_ARGUMENT, "kModeAbsorb: gap_table must be the context's table buffer");
  if (!staged) return run_fused<kMode>(ctx, set, job, flags);
  for (uint32_t off = 0; off < job.n; off += ch) {
    const uint32_t m = std::min(ch, job.n - off);
    for (uint32_t l = 0; l < set.count; ++l) {
      // kModeTir: per lens the INSIDE stage, then 1 + max_bounces OUTSIDE stages -- the first over the rays whose
      // status is not NONE, each later one over the rays the stage before it reflected (the pending row); the last
      // may not reflect.  The stages are queued whether or not a ray is pending (no read-back decides it).
      for (uint32_t j = 0; j < (kTir ? 2 + job.max_bounces : 2); ++j) {
        Out o{};
        o.rays = job.out_rays;
        o.expected_all = j == 0 ? uint32_t(BZR_RR_INSIDE) : uint32_t(BZR_RR_OUTSIDE);
        o.pend = pend;
        o.bounces = job.bounces;
        o.bounce_stage = (kTir && j >= 2) ? 1u : 0u;
        o.may_reflect = (kTir && j >= 1 && j <= job.max_bounces) ? 1u : 0u;
        o.status = job.status;
        o.segments = job.segments;
        o.ri = set.lens[l].ri;
        o.first = (l == 0 && j == 0 && !job.alive_in) ? 1u : 0u;
        o.weight = job.weight;
        o.weight_in = job.weight_in;
        o.channel = job.channel;
        o.ri_row = has_channels(kMode) ? job.ri_table + (size_t)l * job.nchan : nullptr;
        o.nchan = job.nchan;
        o.lossless = job.lossless;
        o.opl = job.opl;
        o.opl_in = job.opl_in;
        o.glass = job.glass;
        if constexpr (has_media(kMode)) {
          o.gap_row = job.gap_table + (size_t)l * job.nchan;
          o.gap_next = o.gap_row + job.nchan;
        }
        if constexpr (has_absorb(kMode)) {
          o.glass_absorb = job.gap_table + kGapPart + (size_t)l * job.nchan;
          o.gap_absorb = o.glass_absorb + kAbsorbPart;
        }
        if constexpr (has_ghost(kMode)) {
          o.ghost_base = job.ghost_base;
          o.ghost_e = 16u * l + j - 1u;  // (read by an OUTSIDE stage that may reflect: j >= 1)
        }
        if (bzr_status s = run_segment<kMode>(use_fast(flags), ctx, set.lens[l], o.first ? job.rays : job.out_rays, job.ld,
                                              off, m, o.first ? nullptr : (o.bounce_stage ? pend : job.status), o, w))
          return s;
      }
    }
  }
  BZR_HIP(hipGetLastError());
  return BZR_OK;
}

}  // namespace

// ------------------------------------------------------------------- C ABI
extern "C" bzr_status bzr_device_count(int32_t *count) {
  if (!count) return set_error(BZR_ERR_INVALID_ARGUMENT, "null count");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  *count = c;
  return BZR_OK;
}

extern "C" bzr_status bzr_ctx_create(int32_t device, bzr_ctx **out) {
  if (!out) return set_error(BZR_ERR_INVALID_ARGUMENT, "null out");
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return set_error(BZR_ERR_NO_DEVICE, "no HIP device visible: libbzr has no CPU path");
  if (device < 0 || device >= count) return set_error(BZR_ERR_INVALID_ARGUMENT, "device index out of range");
  DeviceGuard g(device);
  bzr_ctx *c = new (std::nothrow) bzr_ctx();
  if (!c) return set_error(BZR_ERR_OUT_OF_MEMORY, "context allocation");
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
  if (e != hipSuccess) {
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
    return set_error(BZR_ERR_HIP, std::string("context streams: ") + hipGetErrorString(e));
  }
  c->stream = c->own;
  *out = c;
  return BZR_OK;
}

extern "C" bzr_status bzr_ctx_timing(bzr_ctx *ctx, int32_t enable) {
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  ctx->timing = enable != 0;
  return BZR_OK;
}

extern "C" bzr_status bzr_ctx_timing_report(bzr_ctx *ctx, float ms[BZR_KERNEL_COUNT], uint32_t calls[BZR_KERNEL_COUNT]) {
  if (!ctx || !ms || !calls) return set_error(BZR_ERR_INVALID_ARGUMENT, "null argument");
  DeviceGuard g(ctx->device);
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  for (auto const &mk : ctx->marks) {
    float t = 0.0f;
    BZR_HIP(hipEventElapsedTime(&t, mk.start, mk.stop));
    ctx->ms[mk.kernel] += t;
    ctx->calls[mk.kernel] += 1;
    ctx->spare.push_back(mk.start);
    ctx->spare.push_back(mk.stop);
  }
  ctx->marks.clear();
  for (int k = 0; k < BZR_KERNEL_COUNT; ++k) {
    ms[k] = static_cast<float>(ctx->ms[k]);
    calls[k] = ctx->calls[k];
    ctx->ms[k] = 0.0;
    ctx->calls[k] = 0;
  }
  return BZR_OK;
}

extern "C" bzr_status bzr_ctx_counters(bzr_ctx *ctx, int32_t enable) {
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  DeviceGuard g(ctx->device);
  if (enable && !ctx->counters) {
    BZR_HIP(hipMalloc(&ctx->counters, kCounterReplicas * BZR_COUNTER_COUNT * sizeof(unsigned long long)));
    BZR_HIP(hipMemsetAsync(ctx->counters, 0, kCounterReplicas * BZR_COUNTER_COUNT * sizeof(unsigned long long),
                           ctx->stream));
  }
  ctx->counting = enable != 0;
  return BZR_OK;
}

extern "C" bzr_status bzr_ctx_counters_report(bzr_ctx *ctx, uint64_t counts[BZR_COUNTER_COUNT]) {
  if (!ctx || !counts) return set_error(BZR_ERR_INVALID_ARGUMENT, "null argument");
  for (int k = 0; k < BZR_COUNTER_COUNT; ++k) counts[k] = 0;
  if (!ctx->counters) return BZR_OK;
  DeviceGuard g(ctx->device);
  std::vector<unsigned long long> host((size_t)kCounterReplicas * BZR_COUNTER_COUNT);
  const size_t bytes = host.size() * sizeof(unsigned long long);
  BZR_HIP(hipMemcpyAsync(host.data(), ctx->counters, bytes, hipMemcpyDeviceToHost, ctx->stream));
  BZR_HIP(hipMemsetAsync(ctx->counters, 0, bytes, ctx->stream));
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  for (uint32_t r = 0; r < kCounterReplicas; ++r)
    for (int k = 0; k < BZR_COUNTER_COUNT; ++k) counts[k] += host[(size_t)r * BZR_COUNTER_COUNT + k];
  return BZR_OK;
}

extern "C" bzr_status bzr_ctx_destroy(bzr_ctx *ctx) {
  if (!ctx) return BZR_OK;
  DeviceGuard g(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipStreamSynchronize(ctx->own);
  for (auto const &mk : ctx->marks) {
    (void)hipEventDestroy(mk.start);
    (void)hipEventDestroy(mk.stop);
  }
  for (auto e : ctx->spare) (void)hipEventDestroy(e);
  if (ctx->handoff) (void)hipEventDestroy(ctx->handoff);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->work) (void)hipFree(ctx->work);
  if (ctx->counters) (void)hipFree(ctx->counters);
  if (ctx->pack) (void)hipFree(ctx->pack);
  if (ctx->sched) (void)hipFree(ctx->sched);
  if (ctx->ri_table) (void)hipFree(ctx->ri_table);
  (void)hipStreamDestroy(ctx->own);
  delete ctx;
  return BZR_OK;
}

namespace {
// Switch the context's stream; work already queued on the old stream (which shares the context's
// workspace) is ordered before anything launched on the new one.
bzr_status switch_stream(bzr_ctx *ctx, hipStream_t next) {
  if (next == ctx->stream) return BZR_OK;
  DeviceGuard g(ctx->device);
  if (!ctx->handoff) BZR_HIP(hipEventCreateWithFlags(&ctx->handoff, hipEventDisableTiming));
  BZR_HIP(hipEventRecord(ctx->handoff, ctx->stream));
  BZR_HIP(hipStreamWaitEvent(next, ctx->handoff, 0));
  ctx->stream = next;
  return BZR_OK;
}
}  // namespace

extern "C" bzr_status bzr_ctx_set_stream(bzr_ctx *ctx, void *stream) {
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  return switch_stream(ctx, reinterpret_cast<hipStream_t>(stream));
}

extern "C" bzr_status bzr_ctx_use_own_stream(bzr_ctx *ctx) {
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  return switch_stream(ctx, ctx->own);
}

extern "C" bzr_status bzr_ctx_get_stream(bzr_ctx *ctx, void **stream) {
  if (!ctx || !stream) return set_error(BZR_ERR_INVALID_ARGUMENT, "null argument");
  *stream = reinterpret_cast<void *>(ctx->stream);
  return BZR_OK;
}

extern "C" bzr_status bzr_sync(bzr_ctx *ctx) {
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  DeviceGuard g(ctx->device);
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  return BZR_OK;
}

extern "C" bzr_status bzr_mesh_create(bzr_ctx *ctx, const void *patches, uint32_t n, uint32_t stride, bzr_mesh **out) {
  if (!ctx || !out || (!patches && n)) return set_error(BZR_ERR_INVALID_ARGUMENT, "null argument");
  if (stride < sizeof(bzr_patch)) return set_error(BZR_ERR_INVALID_ARGUMENT, "stride smaller than bzr_patch");
  *out = nullptr;
  DeviceGuard g(ctx->device);
  std::vector<float> full((size_t)n * rec::kWords);  // index order
  std::vector<float4> planar((size_t)n * 4);
  const char *src = static_cast<const char *>(patches);
  for (uint32_t i = 0; i < n; ++i) {
    float *r = &full[(size_t)i * rec::kWords];
    std::memcpy(r, src + (size_t)i * stride, sizeof(bzr_patch));
    const float *m = r + rec::kMinv;  // col-major: M(i,j) = m[j*3+i]
    planar[4 * i + 0] = make_float4(r[0], r[1], r[2], r[3]);
    planar[4 * i + 1] = make_float4(r[rec::kHin], r[rec::kHout], m[0], m[3]);
    planar[4 * i + 2] = make_float4(m[6], m[1], m[4], m[7]);
    planar[4 * i + 3] = make_float4(m[2], m[5], m[8], 0.0f);
  }
  bzr_host::Bvh bvh, bvh_near;
  try {
    bvh = bzr_host::build_bvh(full.data(), n, rec::kWords, bzr_host::kTierFar);
    bvh_near = bzr_host::build_bvh(full.data(), n, rec::kWords, bzr_host::kTierNear);
  } catch (std::exception const &e) {
    return set_error(BZR_ERR_OUT_OF_MEMORY, std::string("BVH build: ") + e.what());
  }
  auto leaves = [&](bzr_host::Bvh const &t) {  // BVH slot order, patch index in the last word
    std::vector<float4> leaf((size_t)n * 4);
    for (uint32_t k = 0; k < n; ++k) {
      uint32_t b = t.order[k];
      for (int j = 0; j < 4; ++j) leaf[4 * k + j] = planar[4 * b + j];
      std::memcpy(&leaf[4 * k + 3].w, &b, 4);
    }
    return leaf;
  };
  const std::vector<float4> leaf = leaves(bvh), leaf_near = leaves(bvh_near);
  auto kids_of = [](bzr_host::Bvh const &t) {  // node i, child c -> float4 pair 2 (4 i + c): lo.xyz ref, hi.xyz 0
    std::vector<float4> k(t.nodes4.size() * 8);
    for (size_t i = 0; i < t.nodes4.size(); ++i)
      for (int c = 0; c < 4; ++c) {
        auto const &nd = t.nodes4[i];
        float ref;
        std::memcpy(&ref, &nd.child[c], 4);
        k[8 * i + 2 * c] = make_float4(nd.lo[0][c], nd.lo[1][c], nd.lo[2][c], ref);
        k[8 * i + 2 * c + 1] = make_float4(nd.hi[0][c], nd.hi[1][c], nd.hi[2][c], 0.0f);
      }
    return k;
  };
  const std::vector<float4> kids = kids_of(bvh), kids_near = kids_of(bvh_near);
  // two levels per node (k_traverse's bundle walk): slot 4 c + g of node i is
  // grandchild g of its child c when that child is an axis-aligned inner node, else (a leaf, an oriented-box
  // node) slot 4 c is the child itself and 4 c + 1..3 are empty.  A walk over these slots skips the children's own boxes,
  // so it reaches a superset of the leaves the 4-wide walk reaches (every leaf still takes its exact gate).
  auto wide_of = [](bzr_host::Bvh const &t) {
    constexpr uint32_t S = kWideSlots;
    float empty;
    const uint32_t e = bzr_host::kEmptyChild;
    std::memcpy(&empty, &e, 4);
    std::vector<float4> k(t.nodes4.size() * 2 * S, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (size_t s = 0; s < k.size(); s += 2) k[s].w = empty;
    auto put = [&](size_t slot, const bzr_host::Bvh4Node &nd, int c) {  // child c of nd into a slot
      float ref;
      std::memcpy(&ref, &nd.child[c], 4);
      k[2 * slot] = make_float4(nd.lo[0][c], nd.lo[1][c], nd.lo[2][c], ref);
      k[2 * slot + 1] = make_float4(nd.hi[0][c], nd.hi[1][c], nd.hi[2][c], 0.0f);
    };
    for (size_t i = 0; i < t.nodes4.size(); ++i)
      for (int c = 0; c < 4; ++c) {
        const bzr_host::Bvh4Node &nd = t.nodes4[i];
        const uint32_t ch = nd.child[c];
        const bool inner = ch != bzr_host::kEmptyChild && !(ch & (bzr_host::kLeafFlag | bzr_host::kObbFlag));
        if (!inner) {
          put(S * i + 4 * c, nd, c);
          continue;
        }
        for (int g = 0; g < 4; ++g) put(S * i + 4 * c + g, t.nodes4[ch], g);
      }
    return k;
  };
  const std::vector<float4> wide = wide_of(bvh), wide_near = wide_of(bvh_near);
  // the same two tiers with split leaf boxes, for the fused refract and chain kernels' bundle walk: same slots (order,
  // leaf records, always list), more leaf references
  std::vector<float4> swide, swide_near;
  uint32_t split = 1;
  if (bzr_host::kSplitDefault > 1 && n - bvh.always.size() <= bzr_host::kSplitSlotCap) {
    try {
      const bzr_host::Bvh sb = bzr_host::build_bvh(full.data(), n, rec::kWords, bzr_host::kTierFar, bzr_host::kSplitDefault);
      const bzr_host::Bvh sn = bzr_host::build_bvh(full.data(), n, rec::kWords, bzr_host::kTierNear, bzr_host::kSplitDefault);
      if (sb.order != bvh.order || sn.order != bvh_near.order || sb.split != sn.split)
        return set_error(BZR_ERR_INVALID_ARGUMENT, "split BVH disagrees with the unsplit one on the leaf slots");
      if (sb.split > 1) {
        swide = wide_of(sb);
        swide_near = wide_of(sn);
        split = sb.split;
      }
    } catch (std::exception const &e) {
      return set_error(BZR_ERR_OUT_OF_MEMORY, std::string("BVH build: ") + e.what());
    }
  }
  // the always list: the same patches in both tiers (whether a gate region is proven does not depend on
  // the tier's origin radius)
  if (bvh.always != bvh_near.always) return set_error(BZR_ERR_INVALID_ARGUMENT, "BVH tiers disagree on the always list");
  std::vector<float4> always(bvh.always.size() * kAlwaysQuads);
  for (size_t k = 0; k < bvh.always.size(); ++k) {
    const uint32_t b = bvh.always[k];
    for (int j = 0; j < 4; ++j) always[kAlwaysQuads * k + j] = planar[4 * b + j];
    std::memcpy(&always[kAlwaysQuads * k + 3].w, &b, 4);
    std::memcpy(&always[kAlwaysQuads * k + 4], &bvh.always_wedge[8 * k], 8 * sizeof(float));
  }
  bzr_mesh *mesh = new (std::nothrow) bzr_mesh();
  if (!mesh) return set_error(BZR_ERR_OUT_OF_MEMORY, "mesh allocation");
  mesh->device = ctx->device;
  mesh->n = n;
  mesh->nnodes = static_cast<uint32_t>(bvh.nodes4.size());
  mesh->n_always = static_cast<uint32_t>(bvh.always.size());
  mesh->split = split;
  mesh->swide = mesh->swide_near = nullptr;
  mesh->s_max = bvh.s_max;
  mesh->s_near = std::min(bvh_near.s_max, bvh.s_max);
  for (int k = 0; k < 4; ++k) mesh->sphere[k] = bvh.sphere[k];
  struct Up {
    void **dst;
    const void *src;
    size_t bytes;
  } ups[] = {
      {reinterpret_cast<void **>(&mesh->planar), planar.data(), planar.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->full), full.data(), full.size() * sizeof(float)},
      {reinterpret_cast<void **>(&mesh->nodes), bvh.nodes4.data(), bvh.nodes4.size() * sizeof(bzr_host::Bvh4Node)},
      {reinterpret_cast<void **>(&mesh->leaf), leaf.data(), leaf.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->nodes_near), bvh_near.nodes4.data(),
       bvh_near.nodes4.size() * sizeof(bzr_host::Bvh4Node)},
      {reinterpret_cast<void **>(&mesh->leaf_near), leaf_near.data(), leaf_near.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->obb), bvh.obb.data(), bvh.obb.size() * sizeof(bzr_host::Bvh4ObbNode)},
      {reinterpret_cast<void **>(&mesh->obb_near), bvh_near.obb.data(),
       bvh_near.obb.size() * sizeof(bzr_host::Bvh4ObbNode)},
      {reinterpret_cast<void **>(&mesh->always), always.data(), always.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->kids), kids.data(), kids.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->kids_near), kids_near.data(), kids_near.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->wide), wide.data(), wide.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->wide_near), wide_near.data(), wide_near.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->swide), swide.data(), swide.size() * sizeof(float4)},
      {reinterpret_cast<void **>(&mesh->swide_near), swide_near.data(), swide_near.size() * sizeof(float4)},
  };
  hipError_t e = hipSuccess;
  for (auto &u : ups) {
    if (e == hipSuccess) e = hipMalloc(u.dst, u.bytes ? u.bytes : 16);
    if (e == hipSuccess && u.bytes) e = hipMemcpyAsync(*u.dst, u.src, u.bytes, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    for (auto &u : ups) (void)hipFree(*u.dst);
    delete mesh;
    return set_error(BZR_ERR_HIP, std::string("mesh upload: ") + hipGetErrorString(e));
  }
  *out = mesh;
  return BZR_OK;
}

extern "C" bzr_status bzr_mesh_destroy(bzr_mesh *mesh) {
  if (!mesh) return BZR_OK;
  DeviceGuard g(mesh->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(mesh->planar);
  (void)hipFree(mesh->full);
  (void)hipFree(mesh->nodes);
  (void)hipFree(mesh->leaf);
  (void)hipFree(mesh->nodes_near);
  (void)hipFree(mesh->leaf_near);
  (void)hipFree(mesh->obb);
  (void)hipFree(mesh->obb_near);
  (void)hipFree(mesh->always);
  (void)hipFree(mesh->kids);
  (void)hipFree(mesh->kids_near);
  (void)hipFree(mesh->wide);
  (void)hipFree(mesh->wide_near);
  (void)hipFree(mesh->swide);
  (void)hipFree(mesh->swide_near);
  delete mesh;
  return BZR_OK;
}

extern "C" bzr_status bzr_mesh_size(const bzr_mesh *mesh, uint32_t *n) {
  if (!mesh || !n) return set_error(BZR_ERR_INVALID_ARGUMENT, "null argument");
  *n = mesh->n;
  return BZR_OK;
}

// BezierMesh::intersect of n rays given as device rows into device hit rows [13][n]: the body of bzr_intersect
// and bzr_intersect_records, on the context's stream.
static bzr_status intersect_rows(bzr_ctx *ctx, const bzr_mesh *mesh, const float *d_rays, uint32_t n, float *d_hits,
                                 uint32_t flags) {
  MeshView mv = view_of(mesh);
  if (use_scan(flags)) {
    launch(ctx, BZR_KERNEL_INTERSECT_SCAN, k_intersect_scan, dim3(grid_for(n)), mv, d_rays, n, d_hits);
  } else if (!use_staged(flags, n, mesh->n)) {
    TraceJob job{};
    job.rays = d_rays;
    job.hits = d_hits;
    job.n = job.ld = n;
    if (bzr_status s = run_fused<kModeHits>(ctx, single_lens(mv), job, flags)) return s;
  } else {
    Work w;
    const uint32_t ch = chunk_for(ctx, n);
    if (bzr_status s = ensure_work(ctx, ch, mesh->n, w)) return s;
    Out o{};
    o.hits = d_hits;
    for (uint32_t off = 0; off < n; off += ch)
      if (bzr_status s = run_segment<kModeHits>(use_fast(flags), ctx, mv, d_rays, n, off, std::min(ch, n - off), nullptr, o, w))
        return s;
  }
  BZR_HIP(hipGetLastError());
  return BZR_OK;
}

extern "C" bzr_status bzr_intersect(bzr_ctx *ctx, const bzr_mesh *mesh, const float *rays, uint32_t n, float *hits,
                                    uint32_t flags) {
  if (bzr_status s = check_flags(flags, true)) return s;
  if (bzr_status s = check_ctx_mesh(ctx, mesh)) return s;
  if (n == 0) return BZR_OK;
  if (!rays || !hits) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  const float *d_rays = rays;
  float *d_hits = hits;
  const bool host = !(flags & BZR_DEVICE_PTRS), aos = (flags & BZR_RAYS_AOS) != 0;
  if (host || aos) {
    float *r = nullptr, *tmp = nullptr;
    if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
          st.take(r, (size_t)n * 6);
          if (host) st.take(d_hits, (size_t)n * 13);
          if (host && aos) st.take(tmp, (size_t)n * 6);
        }))
      return s;
    if (bzr_status s = rays_in(ctx, rays, r, n, host, aos, tmp)) return s;
    d_rays = r;
  }
  if (bzr_status s = intersect_rows(ctx, mesh, d_rays, n, d_hits, flags)) return s;
  if (host) {
    BZR_HIP(hipMemcpyAsync(hits, d_hits, (size_t)n * 13 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BZR_OK;
}

extern "C" bzr_status bzr_intersect_records(bzr_ctx *ctx, const bzr_mesh *mesh, const float *rays, uint32_t n,
                                            bzr_hit_record *records, uint32_t *patch_index, uint32_t flags) {
  if (bzr_status s = check_flags(flags, true)) return s;
  if (bzr_status s = check_ctx_mesh(ctx, mesh)) return s;
  if (n == 0) return BZR_OK;
  if (!rays || !records) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  const bool host = !(flags & BZR_DEVICE_PTRS), aos = (flags & BZR_RAYS_AOS) != 0;
  // staging: the rays' rows (unless the caller's device rows are used as they are), the hit rows, and for host
  // callers the records and patch words before their copies
  const size_t hb = (size_t)n * 52, pb = (size_t)n * 4;
  const bool stage_rays = host || aos;
  const float *d_rays = rays;
  float *r = nullptr, *tmp = nullptr, *d_hits = nullptr;
  void *d_rec = records;
  uint32_t *d_patch = patch_index;
  if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
        if (stage_rays) st.take(r, (size_t)n * 6);
        if (host && aos) st.take(tmp, (size_t)n * 6);
        st.take(d_hits, (size_t)n * 13);
        if (host) d_rec = st.take<uint32_t>((size_t)n * 13);
        if (host && patch_index) st.take(d_patch, n);
      }))
    return s;
  if (stage_rays) {
    if (bzr_status s = rays_in(ctx, rays, r, n, host, aos, tmp)) return s;
    d_rays = r;
  }
  if (bzr_status s = intersect_rows(ctx, mesh, d_rays, n, d_hits, flags)) return s;
  BZR_HIP(bzr_hits_to_records(ctx->stream, d_hits, n, d_rec, d_patch));
  if (host) {
    BZR_HIP(hipMemcpyAsync(records, d_rec, hb, hipMemcpyDeviceToHost, ctx->stream));
    if (patch_index) BZR_HIP(hipMemcpyAsync(patch_index, d_patch, pb, hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BZR_OK;
}

extern "C" bzr_status bzr_patch_intersect(bzr_ctx *ctx, const bzr_mesh *mesh, const uint32_t *idx, const uint32_t *limit,
                                          const float *rays, uint32_t n, float *hits, uint32_t flags) {
  if (bzr_status s = check_flags(flags)) return s;
  if (bzr_status s = check_ctx_mesh(ctx, mesh)) return s;
  if (n == 0) return BZR_OK;
  if (!idx || !limit || !rays || !hits) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  const uint32_t *d_idx = idx, *d_lim = limit;
  const float *d_rays = rays;
  float *d_hits = hits;
  bool host = !(flags & BZR_DEVICE_PTRS);
  if (host) {
    const size_t ib = (size_t)n * 4, rb = (size_t)n * 24;
    uint32_t *a = nullptr, *b = nullptr;
    float *r = nullptr;
    if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
          st.take(a, n), st.take(b, n), st.take(r, (size_t)n * 6), st.take(d_hits, (size_t)n * 13);
        }))
      return s;
    BZR_HIP(hipMemcpyAsync(a, idx, ib, hipMemcpyHostToDevice, ctx->stream));
    BZR_HIP(hipMemcpyAsync(b, limit, ib, hipMemcpyHostToDevice, ctx->stream));
    BZR_HIP(hipMemcpyAsync(r, rays, rb, hipMemcpyHostToDevice, ctx->stream));
    d_idx = a;
    d_lim = b;
    d_rays = r;
  }
  auto *kp = use_fast(flags) ? &k_patch<true> : &k_patch<false>;
  launch(ctx, BZR_KERNEL_PATCH, kp, dim3(grid_for(n)), view_of(mesh), d_idx, d_lim, d_rays, n,
                     d_hits);
  BZR_HIP(hipGetLastError());
  if (host) {
    BZR_HIP(hipMemcpyAsync(hits, d_hits, (size_t)n * 52, hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BZR_OK;
}

extern "C" bzr_status bzr_refract(bzr_ctx *ctx, const bzr_mesh *mesh, float ri, const float *rays, const uint32_t *expected,
                                  uint32_t expected_all, uint32_t n, float *out_rays, uint32_t *out_status,
                                  uint32_t flags) {
  if (bzr_status s = check_flags(flags, true)) return s;
  if (bzr_status s = check_ctx_mesh(ctx, mesh)) return s;
  if (n == 0) return BZR_OK;
  if (!rays || !out_rays || !out_status) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  const float *d_rays = rays;
  const uint32_t *d_exp = expected;
  float *d_out = out_rays;
  uint32_t *d_st = out_status;
  const bool host = !(flags & BZR_DEVICE_PTRS), aos = (flags & BZR_RAYS_AOS) != 0;
  float *tmp = nullptr;  // host + AoS: the records on the device, in and out
  if (host || aos) {
    float *r = nullptr;
    uint32_t *e = nullptr;
    if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
          st.take(r, (size_t)n * 6), st.take(d_out, (size_t)n * 6);
          if (host) st.take(e, n), st.take(d_st, n);
          if (host && aos) st.take(tmp, (size_t)n * 6);
        }))
      return s;
    if (host && expected) {
      BZR_HIP(hipMemcpyAsync(e, expected, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
      d_exp = e;
    }
    if (bzr_status s = rays_in(ctx, rays, r, n, host, aos, tmp)) return s;
    d_rays = r;
  }
  MeshView mv = view_of(mesh, ri);
  if (use_scan(flags)) {
    launch(ctx, BZR_KERNEL_REFRACT_SCAN, k_refract_scan, dim3(grid_for(n)), mv, d_rays, d_exp, expected_all,
                       n, d_out, d_st);
  } else if (!use_staged(flags, n, mesh->n)) {
    TraceJob job{};
    job.rays = d_rays;
    job.out_rays = d_out;
    job.status = d_st;
    job.expected = d_exp;
    job.expected_all = expected_all;
    job.n = job.ld = n;
    if (bzr_status s = run_fused<kModeRefract>(ctx, single_lens(mv), job, flags)) return s;
  } else {
    Work w;
    const uint32_t ch = chunk_for(ctx, n);
    if (bzr_status s = ensure_work(ctx, ch, mesh->n, w)) return s;
    Out o{};
    o.rays = d_out;
    o.expected = d_exp;
    o.expected_all = expected_all;
    o.status = d_st;
    o.ri = ri;
    for (uint32_t off = 0; off < n; off += ch)
      if (bzr_status s = run_segment<kModeRefract>(use_fast(flags), ctx, mv, d_rays, n, off, std::min(ch, n - off), nullptr, o, w))
        return s;
  }
  BZR_HIP(hipGetLastError());
  if (bzr_status s = rays_out(ctx, d_out, out_rays, n, host, aos, tmp)) return s;
  if (host) {
    BZR_HIP(hipMemcpyAsync(out_status, d_st, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BZR_OK;
}

// bzr_trace_chain (kModeStage) and bzr_trace_chain_power (kModePower: + weight_in, may be null, and out_weight,
// plain [n] rows in either ray layout); bzr_trace_chain_spectral (kModeSpectral: kModePower with `ri` the index
// table [nlens][nchan] and `channel` one byte per ray, a plain [n] row, host or device memory as the rays);
// bzr_trace_chain_tir (kModeTir: kModeSpectral with a null `channel` allowed, + max_bounces and out_bounces, an
// optional plain [n] row).  The staged kModeTir chain keeps one more word per ray, the pending row, in the scratch.
// bzr_trace_chain_opl (kModeOpl: kModeTir + opl_in, may be null, out_opl and the optional out_glass, plain [n] rows).
// bzr_trace_chain_media (kModeMedia: kModeOpl + `gap`, the media table [nlens + 1][nchan] in host memory, null: vacuum).
// bzr_trace_chain_absorb (kModeAbsorb: kModeMedia + `glass_abs` and `gap_abs`, the absorption tables [nlens][nchan] in
// host memory, null: all zero).
// bzr_trace_chain_ghost (kModeGhost: kModeAbsorb + `ghost_seed` and `first_ray`, the roulette's seed and ray 0's number).
template <int kMode>
static bzr_status trace_chain(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri, uint32_t nlens,
                              const float *rays, const float *weight_in, uint32_t n, float *out_rays, float *out_weight,
                              uint32_t *out_status, uint32_t *out_segments, uint32_t flags,
                              const uint8_t *channel = nullptr, uint32_t nchan = 0, uint32_t max_bounces = 0,
                              uint32_t *out_bounces = nullptr, const float *opl_in = nullptr, float *out_opl = nullptr,
                              float *out_glass = nullptr, const float *gap = nullptr, const float *glass_abs = nullptr,
                              const float *gap_abs = nullptr, uint64_t ghost_seed = 0, uint64_t first_ray = 0,
                              const float *axis = nullptr, const bzr_coating *coat = nullptr) {
  constexpr bool kPower = has_power(kMode), kSpectral = has_channels(kMode), kTir = has_tir(kMode);
  constexpr bool kOpl = has_opl(kMode), kMedia = has_media(kMode), kAbsorb = has_absorb(kMode);
  if (bzr_status s = check_flags(flags, true)) return s;
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (nlens == 0 || nlens > kMaxLenses) return set_error(BZR_ERR_INVALID_ARGUMENT, "nlens must be 1..8");
  if (kSpectral) {
    if (bzr_status s = check_channels(ri, nchan)) return s;
    if (!kTir && !channel) return set_error(BZR_ERR_INVALID_ARGUMENT, "null channel row");
    if (!out_weight) return set_error(BZR_ERR_INVALID_ARGUMENT, "null out_weight");
    if (max_bounces > BZR_MAX_BOUNCES) return set_error(BZR_ERR_INVALID_ARGUMENT, "max_bounces must be 0..8");
    if (kMedia)
      if (bzr_status s = check_gap_table(gap, nlens, nchan)) return s;
    // (kAbsorb: bzr_trace_chain_absorb has checked its two tables already, ahead of the context check)
  }
  if (!lenses || !ri) return set_error(BZR_ERR_INVALID_ARGUMENT, "null lens list");
  LensSet set{};
  set.count = nlens;
  for (uint32_t l = 0; l < nlens; ++l) {
    if (bzr_status s = check_ctx_mesh(ctx, lenses[l])) return s;
    set.lens[l] = view_of(lenses[l], kSpectral ? 1.0f : ri[l]);
  }
  if (n == 0) return BZR_OK;
  if (!rays || !out_rays || !out_status || (kPower && !out_weight)) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  if (rays == out_rays) return set_error(BZR_ERR_INVALID_ARGUMENT, "rays and out_rays must not alias");
  DeviceGuard g(ctx->device);
  const float *d_rays = rays;
  float *d_out = out_rays;
  uint32_t *d_st = out_status, *d_seg = out_segments, *d_bnc = out_bounces, *d_pend = nullptr;
  const float *d_win = weight_in, *d_oin = opl_in;
  float *d_w = out_weight, *d_opl = out_opl, *d_glass = out_glass;
  const uint8_t *d_ch = channel;
  const bool host = !(flags & BZR_DEVICE_PTRS), aos = (flags & BZR_RAYS_AOS) != 0;
  if (kSpectral)
    if (bzr_status s = upload_ri_table(ctx, ri, nlens, nchan)) return s;
  if (kMedia)
    if (bzr_status s = upload_gap_table(ctx, gap, nlens, nchan)) return s;
  if (kAbsorb) {
    if (bzr_status s = upload_absorb_table(ctx, glass_abs, nlens, nchan, kGlassAbsorbAt, ctx->glass_absorb_host)) return s;
    if (bzr_status s = upload_absorb_table(ctx, gap_abs, nlens, nchan, kGapAbsorbAt, ctx->gap_absorb_host)) return s;
  }
  if (has_coat(kMode)) {  // the rows, and the mask into the high half of the kernels' max_bounces word
    if (bzr_status s = upload_coat_table(ctx, coat, nlens, nchan)) return s;
    max_bounces |= (coat ? coat->mask : 0u) << 16;
  }
  // (kModeBidir has no staged form: its entry point has refused the explicit flag, the automatic choice is fused)
  const bool staged = !has_bidir(kMode) && !use_scan(flags) && use_staged(flags, n, max_patches(set));
  float *r = nullptr, *tmp = nullptr;  // tmp, host + AoS: the records on the device, in and out
  uint8_t *c = nullptr;
  // kModeTir: the staged chain's pending row (one word per ray) and a host caller's bounce row, behind the rest
  if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
        if (host || aos) st.take(r, (size_t)n * 6), st.take(d_out, (size_t)n * 6);
        if (host) st.take(d_st, n), st.take(d_seg, n);
        if (host && kPower) st.take(d_w, n);
        if (host && kSpectral && channel) st.take(c, n);
        if (host && aos) st.take(tmp, (size_t)n * 6);
        if (kTir && staged) st.take(d_pend, n);
        if (kTir && host && out_bounces) st.take(d_bnc, n);
        if (kOpl && host) st.take(d_opl, n);
        if (kOpl && host && out_glass) st.take(d_glass, n);
      }))
    return s;
  if (host && kPower && weight_in) {
    BZR_HIP(hipMemcpyAsync(d_w, weight_in, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    d_win = d_w;
  }
  if (host && kOpl && opl_in) {
    BZR_HIP(hipMemcpyAsync(d_opl, opl_in, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    d_oin = d_opl;
  }
  if (c) {
    BZR_HIP(hipMemcpyAsync(c, channel, n, hipMemcpyHostToDevice, ctx->stream));
    d_ch = c;
  }
  if (host || aos) {
    if (bzr_status s = rays_in(ctx, rays, r, n, host, aos, tmp)) return s;
    d_rays = r;
  }
  if (use_scan(flags)) {
    launch(ctx, BZR_KERNEL_CHAIN_SCAN,
           k_chain_scan<has_coat(kMode) ? 9 : has_bidir(kMode) ? 8 : has_ghost(kMode) ? 7 : kAbsorb ? 6 : kMedia ? 5 : kOpl ? 4 : (kTir ? 3 : (kSpectral ? 2 : (kPower ? 1 : 0)))>,
           dim3(grid_for(n)), set, d_rays, n, d_out, d_st, d_seg, d_win, d_w, d_ch, (const float *)ctx->ri_table, nchan, d_bnc,
           max_bounces, d_oin, d_opl, d_glass, kMedia ? (const float *)ctx->ri_table + kRiTableFloats : nullptr,
           kAbsorb ? (const float *)ctx->ri_table + kGlassAbsorbAt : nullptr,
           kAbsorb ? (const float *)ctx->ri_table + kGapAbsorbAt : nullptr, ghost_base(ghost_seed, first_ray),
           axis ? axis[0] : 0.0f, axis ? axis[1] : 0.0f, axis ? axis[2] : 0.0f);
    BZR_HIP(hipGetLastError());
  } else {
    TraceJob job{};
    job.rays = d_rays;
    job.out_rays = d_out;
    job.status = d_st;
    job.segments = d_seg;
    job.n = job.ld = n;
    job.weight = d_w;
    job.weight_in = d_win;
    job.channel = d_ch;
    job.ri_table = ctx->ri_table;
    job.nchan = nchan;
    job.bounces = d_bnc;
    job.max_bounces = max_bounces;
    job.opl = d_opl;
    job.opl_in = d_oin;
    job.glass = d_glass;
    job.gap_table = kMedia ? ctx->ri_table + kRiTableFloats : nullptr;
    job.ghost_base = ghost_base(ghost_seed, first_ray);
    if constexpr (has_bidir(kMode)) {
      job.axis_xy[0] = axis[0];
      job.axis_xy[1] = axis[1];
      job.axis_z = axis[2];
      if (bzr_status s = run_fused<kMode>(ctx, set, job, flags)) return s;
    } else {
    Work w;
    const uint32_t ch = staged ? chunk_for(ctx, n) : 0u;
    if (staged)
      if (bzr_status s = ensure_work(ctx, ch, max_patches(set), w)) return s;
    if (bzr_status s = run_chain<kMode>(ctx, set, job, flags, staged, d_pend, ch, w)) return s;
    }
  }
  if (bzr_status s = rays_out(ctx, d_out, out_rays, n, host, aos, tmp)) return s;
  if (host) {
    BZR_HIP(hipMemcpyAsync(out_status, d_st, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_segments)
      BZR_HIP(hipMemcpyAsync(out_segments, d_seg, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (kPower) BZR_HIP(hipMemcpyAsync(out_weight, d_w, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (kTir && out_bounces)
      BZR_HIP(hipMemcpyAsync(out_bounces, d_bnc, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (kOpl) BZR_HIP(hipMemcpyAsync(out_opl, d_opl, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (kOpl && out_glass)
      BZR_HIP(hipMemcpyAsync(out_glass, d_glass, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BZR_OK;
}

extern "C" bzr_status bzr_trace_chain(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri, uint32_t nlens,
                                      const float *rays, uint32_t n, float *out_rays, uint32_t *out_status,
                                      uint32_t *out_segments, uint32_t flags) {
  return trace_chain<kModeStage>(ctx, lenses, ri, nlens, rays, nullptr, n, out_rays, nullptr, out_status, out_segments, flags);
}

extern "C" bzr_status bzr_trace_chain_power(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri, uint32_t nlens,
                                            const float *rays, const float *weight_in, uint32_t n, float *out_rays,
                                            float *out_weight, uint32_t *out_status, uint32_t *out_segments,
                                            uint32_t flags) {
  return trace_chain<kModePower>(ctx, lenses, ri, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                                 out_segments, flags);
}

extern "C" bzr_status bzr_trace_chain_spectral(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                               uint32_t nlens, uint32_t nchan, const float *rays, const uint8_t *channel,
                                               const float *weight_in, uint32_t n, float *out_rays, float *out_weight,
                                               uint32_t *out_status, uint32_t *out_segments, uint32_t flags) {
  return trace_chain<kModeSpectral>(ctx, lenses, ri_table, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                                    out_segments, flags, channel, nchan);
}

extern "C" bzr_status bzr_trace_chain_tir(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                          uint32_t nlens, uint32_t nchan, const float *rays, const uint8_t *channel,
                                          const float *weight_in, uint32_t n, uint32_t max_bounces, float *out_rays,
                                          float *out_weight, uint32_t *out_status, uint32_t *out_segments,
                                          uint32_t *out_bounces, uint32_t flags) {
  return trace_chain<kModeTir>(ctx, lenses, ri_table, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                               out_segments, flags, channel, nchan, max_bounces, out_bounces);
}

extern "C" bzr_status bzr_trace_chain_opl(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                          uint32_t nlens, uint32_t nchan, const float *rays, const uint8_t *channel,
                                          const float *weight_in, const float *opl_in, uint32_t n, uint32_t max_bounces,
                                          float *out_rays, float *out_weight, uint32_t *out_status,
                                          uint32_t *out_segments, uint32_t *out_bounces, float *out_opl, float *out_glass,
                                          uint32_t flags) {
  // (both ahead of the context check: they need no device to be refused)
  if (!out_opl) return set_error(BZR_ERR_INVALID_ARGUMENT, "null out_opl");
  if (max_bounces > BZR_MAX_BOUNCES) return set_error(BZR_ERR_INVALID_ARGUMENT, "max_bounces must be 0..8");
  return trace_chain<kModeOpl>(ctx, lenses, ri_table, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                               out_segments, flags, channel, nchan, max_bounces, out_bounces, opl_in, out_opl, out_glass);
}

extern "C" bzr_status bzr_trace_chain_media(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                            const float *gap_table, uint32_t nlens, uint32_t nchan, const float *rays,
                                            const uint8_t *channel, const float *weight_in, const float *opl_in,
                                            uint32_t n, uint32_t max_bounces, float *out_rays, float *out_weight,
                                            uint32_t *out_status, uint32_t *out_segments, uint32_t *out_bounces,
                                            float *out_opl, float *out_glass, uint32_t flags) {
  if (!out_opl) return set_error(BZR_ERR_INVALID_ARGUMENT, "null out_opl");
  if (max_bounces > BZR_MAX_BOUNCES) return set_error(BZR_ERR_INVALID_ARGUMENT, "max_bounces must be 0..8");
  return trace_chain<kModeMedia>(ctx, lenses, ri_table, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                                 out_segments, flags, channel, nchan, max_bounces, out_bounces, opl_in, out_opl, out_glass,
                                 gap_table);
}

extern "C" bzr_status bzr_trace_chain_absorb(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                             const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                             uint32_t nlens, uint32_t nchan, const float *rays, const uint8_t *channel,
                                             const float *weight_in, const float *opl_in, uint32_t n,
                                             uint32_t max_bounces, float *out_rays, float *out_weight,
                                             uint32_t *out_status, uint32_t *out_segments, uint32_t *out_bounces,
                                             float *out_opl, float *out_glass, uint32_t flags) {
  if (!out_opl) return set_error(BZR_ERR_INVALID_ARGUMENT, "null out_opl");
  if (max_bounces > BZR_MAX_BOUNCES) return set_error(BZR_ERR_INVALID_ARGUMENT, "max_bounces must be 0..8");
  // (the tables too are refused ahead of the context check, where their extent is valid; trace_chain checks the rest)
  if (nlens >= 1 && nlens <= kMaxLenses && nchan >= 1 && nchan <= kMaxChannels) {
    if (bzr_status s = check_absorb_table(glass_absorb, nlens, nchan, "glass_absorb entries must be finite and >= 0")) return s;
    if (bzr_status s = check_absorb_table(gap_absorb, nlens, nchan, "gap_absorb entries must be finite and >= 0")) return s;
  }
  return trace_chain<kModeAbsorb>(ctx, lenses, ri_table, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                                  out_segments, flags, channel, nchan, max_bounces, out_bounces, opl_in, out_opl, out_glass,
                                  gap_table, glass_absorb, gap_absorb);
}

extern "C" bzr_status bzr_trace_chain_ghost(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                            const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                            uint32_t nlens, uint32_t nchan, const float *rays, const uint8_t *channel,
                                            const float *weight_in, const float *opl_in, uint32_t n,
                                            uint32_t max_bounces, uint64_t ghost_seed, uint64_t first_ray,
                                            float *out_rays, float *out_weight, uint32_t *out_status,
                                            uint32_t *out_segments, uint32_t *out_bounces, float *out_opl,
                                            float *out_glass, uint32_t flags) {
  // (bzr_trace_chain_absorb's checks, in its order)
  if (!out_opl) return set_error(BZR_ERR_INVALID_ARGUMENT, "null out_opl");
  if (max_bounces > BZR_MAX_BOUNCES) return set_error(BZR_ERR_INVALID_ARGUMENT, "max_bounces must be 0..8");
  if (nlens >= 1 && nlens <= kMaxLenses && nchan >= 1 && nchan <= kMaxChannels) {
    if (bzr_status s = check_absorb_table(glass_absorb, nlens, nchan, "glass_absorb entries must be finite and >= 0")) return s;
    if (bzr_status s = check_absorb_table(gap_absorb, nlens, nchan, "gap_absorb entries must be finite and >= 0")) return s;
  }
  return trace_chain<kModeGhost>(ctx, lenses, ri_table, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                                 out_segments, flags, channel, nchan, max_bounces, out_bounces, opl_in, out_opl, out_glass,
                                 gap_table, glass_absorb, gap_absorb, ghost_seed, first_ray);
}

// The chain's forward axis: finite and not zero (only the sign of one dot product with it is used).
static bzr_status check_axis(const float *axis) {
  if (!axis) return set_error(BZR_ERR_INVALID_ARGUMENT, "null axis");
  if (!std::isfinite(axis[0]) || !std::isfinite(axis[1]) || !std::isfinite(axis[2]) ||
      (axis[0] == 0.0f && axis[1] == 0.0f && axis[2] == 0.0f))
    return set_error(BZR_ERR_INVALID_ARGUMENT, "axis must be finite and not zero");
  return BZR_OK;
}
static bzr_status check_bidir_flags(uint32_t flags) {
  if (flags & BZR_PIPELINE_STAGED)
    return set_error(BZR_ERR_INVALID_ARGUMENT, "the bidirectional chain has no staged pipeline: fused, or BZR_ACCEL_NONE");
  return BZR_OK;
}

extern "C" bzr_status bzr_trace_chain_bidir(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                            const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                            uint32_t nlens, uint32_t nchan, const float *rays, const uint8_t *channel,
                                            const float *weight_in, const float *opl_in, uint32_t n,
                                            uint32_t max_bounces, uint64_t ghost_seed, uint64_t first_ray,
                                            const float axis[3], float *out_rays, float *out_weight,
                                            uint32_t *out_status, uint32_t *out_segments, uint32_t *out_bounces,
                                            float *out_opl, float *out_glass, uint32_t flags) {
  // (bzr_trace_chain_ghost's checks, in its order, then the walk's own)
  if (!out_opl) return set_error(BZR_ERR_INVALID_ARGUMENT, "null out_opl");
  if (max_bounces > BZR_MAX_BOUNCES) return set_error(BZR_ERR_INVALID_ARGUMENT, "max_bounces must be 0..8");
  if (nlens >= 1 && nlens <= kMaxLenses && nchan >= 1 && nchan <= kMaxChannels) {
    if (bzr_status s = check_absorb_table(glass_absorb, nlens, nchan, "glass_absorb entries must be finite and >= 0")) return s;
    if (bzr_status s = check_absorb_table(gap_absorb, nlens, nchan, "gap_absorb entries must be finite and >= 0")) return s;
  }
  if (bzr_status s = check_axis(axis)) return s;
  if (bzr_status s = check_bidir_flags(flags)) return s;
  return trace_chain<kModeBidir>(ctx, lenses, ri_table, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                                 out_segments, flags, channel, nchan, max_bounces, out_bounces, opl_in, out_opl, out_glass,
                                 gap_table, glass_absorb, gap_absorb, ghost_seed, first_ray, axis);
}

extern "C" bzr_status bzr_trace_chain_coated(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                             const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                             uint32_t nlens, uint32_t nchan, const float *rays, const uint8_t *channel,
                                             const float *weight_in, const float *opl_in, uint32_t n,
                                             uint32_t max_bounces, uint64_t ghost_seed, uint64_t first_ray,
                                             const float axis[3], const bzr_coating *coat, float *out_rays,
                                             float *out_weight, uint32_t *out_status, uint32_t *out_segments,
                                             uint32_t *out_bounces, float *out_opl, float *out_glass, uint32_t flags) {
  // (bzr_trace_chain_bidir's checks, in its order, then the coating's)
  if (!out_opl) return set_error(BZR_ERR_INVALID_ARGUMENT, "null out_opl");
  if (max_bounces > BZR_MAX_BOUNCES) return set_error(BZR_ERR_INVALID_ARGUMENT, "max_bounces must be 0..8");
  if (nlens >= 1 && nlens <= kMaxLenses && nchan >= 1 && nchan <= kMaxChannels) {
    if (bzr_status s = check_absorb_table(glass_absorb, nlens, nchan, "glass_absorb entries must be finite and >= 0")) return s;
    if (bzr_status s = check_absorb_table(gap_absorb, nlens, nchan, "gap_absorb entries must be finite and >= 0")) return s;
  }
  if (bzr_status s = check_axis(axis)) return s;
  if (bzr_status s = check_bidir_flags(flags)) return s;
  if (nlens >= 1 && nlens <= kMaxLenses && nchan >= 1 && nchan <= kMaxChannels)
    if (bzr_status s = check_coating(coat, nlens, nchan)) return s;
  return trace_chain<kModeCoat>(ctx, lenses, ri_table, nlens, rays, weight_in, n, out_rays, out_weight, out_status,
                                out_segments, flags, channel, nchan, max_bounces, out_bounces, opl_in, out_opl, out_glass,
                                gap_table, glass_absorb, gap_absorb, ghost_seed, first_ray, axis, coat);
}

// ------------------------------------------------------------ test hook: normalized()
namespace {
// The chain's Beer-Lambert term (patch_math_body.inc att), one value per lane.
__global__ __launch_bounds__(kBlock) void k_debug_attenuation(const float *__restrict__ x, uint32_t n,
                                                              float *__restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = att(x[i]);
}
// Row k of out (k < 3): the product's exact normalized() (patch_math.hpp unit_or_self, shared-reciprocal chain
// where its guard allows); rows 3..5: sqrt_rn / div_rn per component (the compiler's own lowering).
__global__ __launch_bounds__(kBlock) void k_debug_unit(const float *__restrict__ a, uint32_t n,
                                                       float *__restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const f3 v = mk(a[i], a[(size_t)n + i], a[(size_t)2 * n + i]);
  const f3 u = normalized(v);
  const float z = dot(v, v);
  f3 w = v;
  if (z > 0.0f) {
    const float s = sqrt_rn(z);
    w = mk(div_rn(v.x, s), div_rn(v.y, s), div_rn(v.z, s));
  }
  const float r[6] = {u.x, u.y, u.z, w.x, w.y, w.z};
#pragma unroll
  for (int k = 0; k < 6; ++k) out[(size_t)k * n + i] = r[k];
}
// newton_tail's bracket quotients (div_heights) beside one correctly rounded division each.
__global__ __launch_bounds__(kBlock) void k_debug_div_heights(const float *__restrict__ a, uint32_t n,
                                                              float *__restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float hin = a[i], hout = a[(size_t)n + i], ic = a[(size_t)2 * n + i];
  float din, dout;
  div_heights(hin, hout, ic, din, dout);
  out[i] = din;
  out[(size_t)n + i] = dout;
  out[(size_t)2 * n + i] = div_rn(hin, ic);
  out[(size_t)3 * n + i] = div_rn(hout, ic);
}
// The walk's bundle setup (bundle_setup_swap) on waves of 64 consecutive rays, one wave per block: row w of out =
// the wave's 22 bundle words and the returned spread.
__global__ __launch_bounds__(64) void k_debug_bundle_setup(const float *__restrict__ rays,
                                                           const uint8_t *__restrict__ active, uint32_t n,
                                                           float *__restrict__ out) {
  __shared__ float bl[kBundleWords];
  const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;  // (i < n: n is a multiple of 64)
  const f3 s = mk(rays[i], rays[(size_t)n + i], rays[(size_t)2 * n + i]);
  const f3 d = mk(rays[(size_t)3 * n + i], rays[(size_t)4 * n + i], rays[(size_t)5 * n + i]);
  const float spread = bundle_setup_swap(active[i] != 0, s, d, bl, lane);
  float *o = out + (size_t)blockIdx.x * (kBundleWords + 1u);
  if (lane < kBundleWords) o[lane] = bl[lane];
  if (lane == kBundleWords) o[lane] = spread;
}
// The fused pass loop's near-first order (batch_append), one wave and one key sequence per block: entry e of
// sequence w has key keys[16 w + e], patch index e and the ballot kDebugBallot * (e + 1); row w of out = the batch in
// the order its passes would run, 3 words per place (index, ballot low, ballot high; 0xFFFFFFFF past the length).
constexpr unsigned long long kDebugBallot = 0x9E3779B97F4A7C15ull;
struct DebugBatchLds {
  unsigned long long emask[kEntries];
  uint32_t eid[kEntries];
  uint32_t ekey[kEntries];
};
__global__ __launch_bounds__(64) void k_debug_pass_order(const uint32_t *__restrict__ keys,
                                                         const uint32_t *__restrict__ len, uint32_t *__restrict__ out) {
  __shared__ DebugBatchLds L;
  const uint32_t lane = threadIdx.x, w = blockIdx.x;
  const uint32_t n = min(__builtin_amdgcn_readfirstlane(len[w]), kEntries);
  unsigned long long order = 0ull;
  for (uint32_t e = 0; e < n; ++e)
    batch_append<true>(L, e, order, e, kDebugBallot * (e + 1u), __builtin_amdgcn_readfirstlane(keys[kEntries * w + e]),
                       lane);
  __builtin_amdgcn_wave_barrier();
  if (lane < kEntries) {
    const uint32_t ei = order_at(order, lane);
    uint32_t *o = out + (size_t)3 * (kEntries * w + lane);
    o[0] = lane < n ? L.eid[ei] : 0xFFFFFFFFu;
    o[1] = lane < n ? (uint32_t)L.emask[ei] : 0xFFFFFFFFu;
    o[2] = lane < n ? (uint32_t)(L.emask[ei] >> 32) : 0xFFFFFFFFu;
  }
}
// BZR_MODE_FAST's primitives (patch_math.hpp namespace fast): row 0 div_rn(a0, a1), row 1 sqrt_rn(|a0|), rows 2..4
// normalized(a).
__global__ __launch_bounds__(kBlock) void k_debug_fast_unit(const float *__restrict__ a, uint32_t n,
                                                            float *__restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const f3 v = mk(a[i], a[(size_t)n + i], a[(size_t)2 * n + i]);
  const f3 u = fast::normalized(v);
  const float r[5] = {fast::div_rn(v.x, v.y), fast::sqrt_rn(fabsf(v.x)), u.x, u.y, u.z};
#pragma unroll
  for (int k = 0; k < 5; ++k) out[(size_t)k * n + i] = r[k];
}
}  // namespace

extern "C" void bzr_internal_attenuation_host(const float *x, uint32_t n, float *out);  // host (capi_host.cpp)
// Host pointers in and out either way; with a context the values go through the staging buffer and one kernel.
extern "C" bzr_status bzr_debug_attenuation(void *ctxp, const float *x, uint32_t n, float *out) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (n == 0) return BZR_OK;
  if (!x || !out) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  if (!ctx) {
    bzr_internal_attenuation_host(x, n, out);
    return BZR_OK;
  }
  DeviceGuard g(ctx->device);
  float *d_x = nullptr, *d_out = nullptr;
  if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) { st.take(d_x, n), st.take(d_out, n); }))
    return s;
  BZR_HIP(hipMemcpyAsync(d_x, x, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_debug_attenuation, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, d_x, n, d_out);
  BZR_HIP(hipGetLastError());
  BZR_HIP(hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_fast_unit(void *ctxp, const float *a, uint32_t n, float *out) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (n == 0) return BZR_OK;
  if (!a || !out) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  hipLaunchKernelGGL(k_debug_fast_unit, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, a, n, out);
  BZR_HIP(hipGetLastError());
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_div_heights(void *ctxp, const float *a, uint32_t n, float *out) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (n == 0) return BZR_OK;
  if (!a || !out) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  hipLaunchKernelGGL(k_debug_div_heights, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, a, n, out);
  BZR_HIP(hipGetLastError());
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_bundle_setup(void *ctxp, const float *rays, const uint8_t *active, uint32_t n,
                                             float *out) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (n == 0) return BZR_OK;
  if (!rays || !active || !out) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  if (n % 64u) return set_error(BZR_ERR_INVALID_ARGUMENT, "n must be whole waves of 64 rays");
  DeviceGuard g(ctx->device);
  hipLaunchKernelGGL(k_debug_bundle_setup, dim3(n / 64u), dim3(64), 0, ctx->stream, rays, active, n, out);
  BZR_HIP(hipGetLastError());
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_pass_order(void *ctxp, const uint32_t *keys, const uint32_t *len, uint32_t n,
                                           uint32_t *out) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (n == 0) return BZR_OK;
  if (!keys || !len || !out) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  hipLaunchKernelGGL(k_debug_pass_order, dim3(n), dim3(64), 0, ctx->stream, keys, len, out);
  BZR_HIP(hipGetLastError());
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_chunk_plan(uint64_t free_bytes, uint64_t n, uint32_t *cap, uint32_t *chunk) {
  if (!cap || !chunk) return set_error(BZR_ERR_INVALID_ARGUMENT, "null argument");
  *cap = chunk_cap_of(free_bytes);
  *chunk = chunk_len(n, *cap);
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_chunk_cap(void *ctxp, uint32_t rays, uint32_t *effective) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  DeviceGuard g(ctx->device);
  ctx->chunk_limit = rays ? std::max(rays / 64u * 64u, 64u) : 0u;
  if (effective) *effective = chunk_cap(ctx);
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_wave_clock(void *ctxp, unsigned long long *clock, uint32_t waves) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  ctx->wave_clock = clock;
  ctx->wave_clock_cap = clock ? waves : 0u;
  ctx->wave_clock_real = false;
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_wave_clock_rate(void *ctxp, unsigned long long *clock, uint32_t waves) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  ctx->wave_clock = clock;
  ctx->wave_clock_cap = clock ? waves : 0u;
  ctx->wave_clock_real = clock != nullptr;
  return BZR_OK;
}

extern "C" bzr_status bzr_debug_unit(void *ctxp, const float *a, uint32_t n, float *out) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (n == 0) return BZR_OK;
  if (!a || !out) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  hipLaunchKernelGGL(k_debug_unit, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, a, n, out);
  BZR_HIP(hipGetLastError());
  return BZR_OK;
}

// ------------------------------------------------------------ tessellation
extern "C" uint32_t bzr_internal_unit_subtriangles(int32_t divisor, float *out);  // host (patch_build.cpp)

namespace {
// BezierMesh::interpolate (reference/bezierMesh.cpp:55-66): output triangle t = k * nb + b is
// sub-triangle k of patch b; its three vertices are BezierTriangle::interpolate at the sub-triangle's
// barycentric corners (reference/bezierTriangle.cpp:105-121, patch_math.hpp `interpolate`).
__global__ __launch_bounds__(kBlock) void k_tessellate(const float *__restrict__ full, uint32_t nb,
                                                       const float *__restrict__ bary, uint64_t total,
                                                       float *__restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= total) return;
  const uint32_t k = static_cast<uint32_t>(t / nb), b = static_cast<uint32_t>(t % nb);
  const PatchView<const float *> p{full + (size_t)rec::kWords * b};
  const float *bk = bary + (size_t)9 * k;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const f3 q = interpolate(p, mk(bk[3 * v], bk[3 * v + 1], bk[3 * v + 2]));
    out[(size_t)9 * t + 3 * v] = q.x;
    out[(size_t)9 * t + 3 * v + 1] = q.y;
    out[(size_t)9 * t + 3 * v + 2] = q.z;
  }
}
}  // namespace

extern "C" bzr_status bzr_mesh_interpolate(bzr_ctx *ctx, const bzr_mesh *mesh, int32_t divisor, float *out_xyz,
                                           uint32_t flags) {
  if (bzr_status s = check_flags(flags)) return s;
  if (bzr_status s = check_ctx_mesh(ctx, mesh)) return s;
  if (divisor < 1 || divisor > 4096) return set_error(BZR_ERR_INVALID_ARGUMENT, "divisor must be 1..4096");
  const uint32_t K = static_cast<uint32_t>(divisor) * static_cast<uint32_t>(divisor);
  const uint64_t total = (uint64_t)K * mesh->n;
  if (total == 0) return BZR_OK;
  if (!out_xyz) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  std::vector<float> bary((size_t)K * 9);
  if (bzr_internal_unit_subtriangles(divisor, bary.data()) != K)
    return set_error(BZR_ERR_INVALID_ARGUMENT, "sub-triangle count mismatch");
  const bool host = !(flags & BZR_DEVICE_PTRS);
  const size_t ob = (size_t)total * 9 * 4;
  float *d_bary = nullptr, *d_out = out_xyz;
  if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
        st.take(d_bary, bary.size());
        if (host) st.take(d_out, (size_t)total * 9);
      }))
    return s;
  BZR_HIP(hipMemcpyAsync(d_bary, bary.data(), bary.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_tessellate, dim3(static_cast<uint32_t>((total + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     ctx->stream, mesh->full, mesh->n, d_bary, total, d_out);
  BZR_HIP(hipGetLastError());
  if (host) BZR_HIP(hipMemcpyAsync(out_xyz, d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
  // the staged sub-triangle table must outlive the kernel: this call is synchronous
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  return BZR_OK;
}

// ------------------------------------------------------------ illumination
namespace {
// Ray power as unsigned 64-bit fixed point with 32 fraction bits: q(w) = trunc(w x 2^32) for w in [0, 1] (the
// product is exact in binary32, the conversion truncates).  Integer sums do not depend on the order of arrival.
__device__ __forceinline__ unsigned long long power_q32(float w) {
  return w > 0.0f ? (unsigned long long)(w * 4294967296.0f) : 0ull;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
  return v;
}

// Keyed form of the illumination kernels' wave reductions.  The lanes of a wave hold mixed keys, so the wave loops
// over the distinct keys among its `valid` lanes (the lowest such lane names the next one); per key, the lanes of
// that key reduce kN counts (`in[k]`: ballots) and the kN sums of q over them, and lane 0 adds them to the key's
// row: ctr[kStride key + k], sum[kStride key + k].  At most one atomic per wave, key and counter; the loop's trip
// count is wave-uniform.
template <int kN, uint32_t kStride>
__device__ __forceinline__ void keyed_rows(bool valid, uint32_t key, const bool (&in)[kN], unsigned long long q,
                                           unsigned long long *__restrict__ ctr, unsigned long long *__restrict__ sum) {
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const uint32_t c = __shfl(key, (int)__ffsll((long long)todo) - 1, 64);
    const bool mine = valid && key == c;
    unsigned long long cnt[kN], tot[kN];
#pragma unroll
    for (int k = 0; k < kN; ++k) cnt[k] = __ballot(mine && in[k]);
#pragma unroll
    for (int k = 0; k < kN; ++k)  // (a counter no lane of the key feeds has nothing to sum: the ballot is uniform)
      tot[k] = cnt[k] ? wave_sum_u64(mine && in[k] ? q : 0ull) : 0ull;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
      for (int k = 0; k < kN; ++k)
        if (cnt[k]) atomicAdd(&ctr[kStride * c + (uint32_t)k], (unsigned long long)__popcll(cnt[k]));
#pragma unroll
      for (int k = 0; k < kN; ++k)
        if (tot[k]) atomicAdd(&sum[kStride * c + (uint32_t)k], tot[k]);
    }
    todo &= ~__ballot(mine);
  }
}
// The per-channel form, keyed_rows<2, 4> by hand: the key is the lane's channel, the two counts (`a`, `b`: ballots)
// and the two sums of q go to the channel's row of four: ctr[4 c], ctr[4 c + 1], sum[4 c], sum[4 c + 1].  (Kept as
// its own text: expressed through keyed_rows, k_emit<2> and k_land<2> came out with other registers.)
__device__ __forceinline__ void channel_rows(bool valid, uint32_t ch, bool a, bool b, unsigned long long q,
                                             unsigned long long *__restrict__ ctr, unsigned long long *__restrict__ sum) {
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const uint32_t c = __shfl(ch, (int)__ffsll((long long)todo) - 1, 64);
    const bool mine = valid && ch == c;
    const unsigned long long na = __ballot(mine && a), nb = __ballot(mine && b);
    const unsigned long long qa = wave_sum_u64(mine && a ? q : 0ull), qb = wave_sum_u64(mine && b ? q : 0ull);
    if ((threadIdx.x & 63u) == 0u) {
      if (na) atomicAdd(&ctr[4u * c], (unsigned long long)__popcll(na));
      if (nb) atomicAdd(&ctr[4u * c + 1u], (unsigned long long)__popcll(nb));
      if (qa) atomicAdd(&sum[4u * c], qa);
      if (qb) atomicAdd(&sum[4u * c + 1u], qb);
    }
    todo &= ~__ballot(mine);
  }
}

// Rays first .. first+n-1 of the emitter into rays [6][ld].  With `status`: rays that cannot meet the
// first lens's bounding sphere (over its proven gate regions) and pass none of its always-listed patches'
// planar gates start as NONE (culled, never traced), the others INSIDE (the chain's first refraction
// expects to enter the lens); stats[EMITTED], stats[CULLED] count them.
// kPower (bzr_illuminate_power: status, segments and stats are given, patch is not read): plus each ray's initial
// power w0 (1, or with `lambert` the direction's x component: cos to the emitter's +x normal) and power[EMITTED],
// power[CULLED] = the sums of q(w0), reduced over the wave first.
// kIllum 2 (bzr_illuminate_spectral): kIllum 1 with ray first + i in channel (first + i) mod nchan, written to
// `channel`; stats and power are [nchan][4], each lane's share goes to its channel's row (channel_rows below).
// (kIllum is an int, not an enum: instantiations 0 and 1 keep the names they had as <false> and <true>.)
template <int kIllum>
__global__ __launch_bounds__(kBlock) void k_emit(bzr_emitter em, BeltTable bt, uint64_t first, uint32_t n, uint32_t ld,
                                                 float *__restrict__ rays, uint32_t *__restrict__ patch,
                                                 uint32_t *__restrict__ status, uint32_t *__restrict__ segments,
                                                 float4 sphere, const float4 *__restrict__ always, uint32_t n_always,
                                                 unsigned long long *__restrict__ stats, float *__restrict__ weight,
                                                 uint32_t lambert, unsigned long long *__restrict__ power,
                                                 uint8_t *__restrict__ channel, uint32_t nchan) {
  constexpr bool kPower = kIllum != 0, kSpectral = kIllum == 2;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool culled = false;
  f3 o = mk(0.0f, 0.0f, 0.0f), d = o;
  if (i < n) {
    uint32_t p;
    emit_ray(em, bt, first + i, o, d, p);
    store_ray(rays, ld, i, o, d);
    if (!kPower && patch) patch[i] = p;
    if (kPower || status) {
      const float sp[4] = {sphere.x, sphere.y, sphere.z, sphere.w};
      culled = !may_hit_sphere(o, d, sp);
    }
  }
  float w0 = 1.0f;
  if (kPower || status) {
    // the always list has no box inside the sphere: a ray outside it is kept if any of those gates passes
    for (uint32_t k = 0; k < n_always && __any(culled); ++k) {
      uint32_t b;
      if (always_gate(always, k, culled, o, d, b)) culled = false;
    }
    if constexpr (kPower) w0 = lambert ? d.x : 1.0f;
    if (i < n) {
      status[i] = culled ? BZR_RR_NONE : BZR_RR_INSIDE;
      if (kPower || segments) segments[i] = 0u;
      if constexpr (kPower) weight[i] = w0;
    }
  }
  if constexpr (kSpectral) {
    const uint32_t ch = i < n ? (uint32_t)((first + i) % nchan) : 0u;
    if (i < n) channel[i] = (uint8_t)ch;
    const unsigned long long q = i < n ? power_q32(w0) : 0ull;
    channel_rows(i < n, ch, i < n, culled, q, stats + BZR_ILLUM_EMITTED, power + BZR_ILLUM_EMITTED);
  } else if (kPower || stats) {
    const unsigned long long made = __ballot(i < n), cut = __ballot(culled);
    unsigned long long qe = 0ull, qc = 0ull;
    if constexpr (kPower) {
      const unsigned long long q = i < n ? power_q32(w0) : 0ull;
      qe = wave_sum_u64(q);
      qc = wave_sum_u64(culled ? q : 0ull);
    }
    if ((threadIdx.x & 63u) == 0u) {
      if (made) atomicAdd(&stats[BZR_ILLUM_EMITTED], (unsigned long long)__popcll(made));
      if (cut) atomicAdd(&stats[BZR_ILLUM_CULLED], (unsigned long long)__popcll(cut));
      if constexpr (kPower) {
        if (qe) atomicAdd(&power[BZR_ILLUM_EMITTED], qe);
        if (qc) atomicAdd(&power[BZR_ILLUM_CULLED], qc);
      }
    }
  }
}

// Rays that left the last lens (status OUTSIDE) meet the target plane: one count per landed ray.
// kPower (bzr_illuminate_power): each landed ray also adds q(its weight) to its cell of flux (64-bit atomic), the
// count only with `hist`; power[EXITED], power[LANDED] = the sums of q(w), one atomic per wave and counter.
// kIllum 2 (bzr_illuminate_spectral): flux and hist are [nchan][cells], a ray of channel c lands in cell
// c * cells + cell; stats and power are [nchan][4], reduced per channel (channel_rows).
template <int kIllum>
__global__ __launch_bounds__(kBlock) void k_land(bzr_target tg, float4 plane, float cell_u, float cell_v,
                                                 const float *__restrict__ rays, uint32_t ld, uint32_t n,
                                                 const uint32_t *__restrict__ status, uint32_t *__restrict__ hist,
                                                 unsigned long long *__restrict__ stats, const float *__restrict__ weight,
                                                 unsigned long long *__restrict__ flux,
                                                 unsigned long long *__restrict__ power,
                                                 const uint8_t *__restrict__ channel, uint32_t cells) {
  constexpr bool kPower = kIllum != 0, kSpectral = kIllum == 2;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool exited = false, landed = false;
  unsigned long long q = 0ull;
  uint32_t ch = 0u;
  if (i < n && status[i] == BZR_RR_OUTSIDE) {
    exited = true;
    if constexpr (kPower) q = power_q32(weight[i]);
    if constexpr (kSpectral) ch = channel[i];
    f3 s, d;
    load_ray(rays, ld, i, s, d);
    const int32_t cell = target_cell(tg, mk(plane.x, plane.y, plane.z), plane.w, cell_u, cell_v, s, d);
    if (cell >= 0) {
      landed = true;
      const size_t at = kSpectral ? (size_t)ch * cells + (uint32_t)cell : (size_t)cell;
      if constexpr (kPower) atomicAdd(&flux[at], q);
      if (!kPower || hist) atomicAdd(&hist[at], 1u);
    }
  }
  if constexpr (kSpectral) {
    channel_rows(exited, ch, exited, landed, q, stats + BZR_ILLUM_EXITED, power + BZR_ILLUM_EXITED);
    return;
  }
  const unsigned long long ex = __ballot(exited), la = __ballot(landed);
  unsigned long long qx = 0ull, ql = 0ull;
  if constexpr (kPower) {
    qx = wave_sum_u64(q);
    ql = wave_sum_u64(landed ? q : 0ull);
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (ex) atomicAdd(&stats[BZR_ILLUM_EXITED], (unsigned long long)__popcll(ex));
    if (la) atomicAdd(&stats[BZR_ILLUM_LANDED], (unsigned long long)__popcll(la));
    if constexpr (kPower) {
      if (qx) atomicAdd(&power[BZR_ILLUM_EXITED], qx);
      if (ql) atomicAdd(&power[BZR_ILLUM_LANDED], ql);
    }
  }
}

// bzr_illuminate_tir's landing kernel: k_land<2> over a chain that reflects, plus the stray-light maps and the bounce
// ledger.  A ray is traced when its segment count is not 0 (k_emit wrote 0, the chain counts every segment of a ray
// it traces); only a traced ray's status, bounce word and weight are read as data.  A landed ray that reflected at
// least once is binned into rflux / rhist (each may be null) as well.  Every traced ray of channel c is added to
// ledger row c * BZR_LEDGER_ROWS + min(bounces, BZR_MAX_BOUNCES): its count and q(w) under LOST (it ended NONE) or
// EXITED (OUTSIDE), and under LANDED too if it met the target -- reduced over the wave per (channel, row), like the
// stats and power rows per channel (keyed_rows).
struct LandTir {
  const uint32_t *segments, *bounces;  // [n] of the batch
  uint32_t *rhist;                     // [nchan][cells] or null
  unsigned long long *rflux;           // [nchan][cells] or null
  unsigned long long *count, *power;   // the ledger [nchan][BZR_LEDGER_ROWS][BZR_LEDGER_FIELDS]
};
__global__ __launch_bounds__(kBlock) void k_land_tir(bzr_target tg, float4 plane, float cell_u, float cell_v,
                                                     const float *__restrict__ rays, uint32_t ld, uint32_t n,
                                                     const uint32_t *__restrict__ status, uint32_t *__restrict__ hist,
                                                     unsigned long long *__restrict__ stats,
                                                     const float *__restrict__ weight,
                                                     unsigned long long *__restrict__ flux,
                                                     unsigned long long *__restrict__ power,
                                                     const uint8_t *__restrict__ channel, uint32_t cells, LandTir t) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool traced = false, lost = false, exited = false, landed = false;
  unsigned long long q = 0ull;
  uint32_t ch = 0u, row = 0u;
  if (i < n && t.segments[i] != 0u) {
    traced = true;
    const uint32_t st = status[i], bounces = t.bounces[i];
    lost = st == BZR_RR_NONE;
    exited = st == BZR_RR_OUTSIDE;
    q = power_q32(weight[i]);
    ch = channel[i];
    row = bounces < BZR_MAX_BOUNCES ? bounces : uint32_t(BZR_MAX_BOUNCES);
    if (exited) {
      f3 s, d;
      load_ray(rays, ld, i, s, d);
      const int32_t cell = target_cell(tg, mk(plane.x, plane.y, plane.z), plane.w, cell_u, cell_v, s, d);
      if (cell >= 0) {
        landed = true;
        const size_t at = (size_t)ch * cells + (uint32_t)cell;
        atomicAdd(&flux[at], q);
        if (hist) atomicAdd(&hist[at], 1u);
        if (bounces != 0u) {
          if (t.rflux) atomicAdd(&t.rflux[at], q);
          if (t.rhist) atomicAdd(&t.rhist[at], 1u);
        }
      }
    }
  }
  channel_rows(exited, ch, exited, landed, q, stats + BZR_ILLUM_EXITED, power + BZR_ILLUM_EXITED);
  const bool in[BZR_LEDGER_FIELDS] = {lost, exited, landed};
  static_assert(BZR_LEDGER_LOST == 0 && BZR_LEDGER_EXITED == 1 && BZR_LEDGER_LANDED == 2, "the ledger's field order");
  keyed_rows<BZR_LEDGER_FIELDS, BZR_LEDGER_FIELDS>(traced, ch * BZR_LEDGER_ROWS + row, in, q, t.count, t.power);
}

// bzr_illuminate_bidir's BACK rays: every traced ray of channel c whose status is BZR_RR_BACK adds one count and q(w) to
// row c * BZR_LEDGER_ROWS + min(bounces, BZR_MAX_BOUNCES) of the two back rows (keyed_rows, one counter per key).
// k_land_tir and k_land_far see such a ray as neither lost nor exited: it is in no ledger field, lands and bins nowhere.
__global__ __launch_bounds__(kBlock) void k_back_rows(uint32_t n, const uint32_t *__restrict__ status,
                                                      const uint32_t *__restrict__ segments,
                                                      const uint32_t *__restrict__ bounces,
                                                      const float *__restrict__ weight,
                                                      const uint8_t *__restrict__ channel,
                                                      unsigned long long *__restrict__ count,
                                                      unsigned long long *__restrict__ power) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool back = false;
  unsigned long long q = 0ull;
  uint32_t key = 0u;
  if (i < n && segments[i] != 0u && status[i] == BZR_RR_BACK) {
    back = true;
    q = power_q32(weight[i]);
    const uint32_t b = bounces[i];
    key = channel[i] * BZR_LEDGER_ROWS + (b < BZR_MAX_BOUNCES ? b : uint32_t(BZR_MAX_BOUNCES));
  }
  const bool in[1] = {true};
  keyed_rows<1, 1>(back, key, in, q, count, power);
}

// The far-field landing kernel (bzr_farfield_bin, bzr_illuminate_farfield): one thread per ray, binned by direction
// (emitter.hpp farfield_cell).  A ray is seen when `status` is null or its status is OUTSIDE, and its channel (0
// without `channel`) is below nchan; a seen ray that is binned adds q(w) (w = 1 without `weight`) to flux[key] and one
// count to hist[key], key = channel * cells + cell (each map may be null), and to rflux[key] too when `bounces` says
// it reflected (both null in bzr_farfield_bin).  stats and power are [nchan][2] (SEEN, BINNED; null: not kept),
// reduced per channel like channel_rows' rows.
// Far fields are peaked: a collimator sends most of a wave's lanes to a few keys, and 64-bit atomics on one address
// serialise.  So up to `rounds` times the lowest pending lane names a key, the lanes that hold it are summed
// (wave_sum_u64; a key held by one lane skips the sum) and that lane alone adds the totals; the lanes still pending
// after that issue their own atomics, so a diffuse wave does not pay 64 rounds.  Integer sums: the same bits for
// every `rounds` (0: plain per-lane atomics).
__global__ __launch_bounds__(kBlock) void k_land_far(FarFrame f, uint32_t cells, const float *__restrict__ rays,
                                                     uint32_t ld, uint32_t n, const uint32_t *__restrict__ status,
                                                     const float *__restrict__ weight,
                                                     const uint8_t *__restrict__ channel, uint32_t nchan,
                                                     const uint32_t *__restrict__ bounces,
                                                     unsigned long long *__restrict__ flux, uint32_t *__restrict__ hist,
                                                     unsigned long long *__restrict__ rflux,
                                                     unsigned long long *__restrict__ stats,
                                                     unsigned long long *__restrict__ power, uint32_t rounds) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool seen = false, binned = false, refl = false;
  unsigned long long q = 0ull;
  uint32_t ch = 0u, key = 0u;
  if (i < n && (!status || status[i] == BZR_RR_OUTSIDE)) {
    if (channel) ch = channel[i];
    if (ch < nchan) {
      seen = true;
      q = power_q32(weight ? weight[i] : 1.0f);
      const f3 d = mk(rays[(size_t)3 * ld + i], rays[(size_t)4 * ld + i], rays[(size_t)5 * ld + i]);
      uint32_t cell;
      if (farfield_cell(f, d, cell)) {
        binned = true;
        key = ch * cells + cell;
        refl = rflux && bounces[i] != 0u;
      }
    }
  }
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long todo = __ballot(binned);
  for (uint32_t r = 0; r < rounds && todo; ++r) {
    const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
    const uint32_t k = __shfl(key, (int)lead, 64);
    const bool mine = binned && key == k;
    const unsigned long long held = __ballot(mine), bounced = __ballot(mine && refl);
    unsigned long long tq = q, tr = q;
    if (held & (held - 1ull)) {  // more than one lane holds the key (wave-uniform)
      tq = wave_sum_u64(mine ? q : 0ull);
      tr = bounced ? wave_sum_u64(mine && refl ? q : 0ull) : 0ull;
    }
    if (lane == lead) {
      if (flux && tq) atomicAdd(&flux[k], tq);
      if (hist) atomicAdd(&hist[k], (uint32_t)__popcll(held));
      if (bounced && tr) atomicAdd(&rflux[k], tr);
    }
    todo &= ~held;
  }
  if (binned && ((todo >> lane) & 1ull)) {
    if (flux && q) atomicAdd(&flux[key], q);
    if (hist) atomicAdd(&hist[key], 1u);
    if (refl && q) atomicAdd(&rflux[key], q);
  }
  if (stats) {
    const bool in[2] = {seen, binned};
    static_assert(BZR_FAR_SEEN == 0 && BZR_FAR_BINNED == 1, "the far-field rows' field order");
    keyed_rows<2, 2u>(seen, ch, in, q, stats, power);
  }
}

// UniformHemisphere(belts)'s patch table (reference/hostUtil.cpp:3-14, same float expressions) and the
// belt boundaries cos(i * width) the device compares cos(incidence) against.
bzr_status belt_tables(uint32_t belts, std::vector<float> &cos_lo, std::vector<uint32_t> &count,
                       std::vector<uint32_t> &first) {
  if (belts == 0 || belts > 4096) return set_error(BZR_ERR_INVALID_ARGUMENT, "belts must be 1..4096");
  constexpr float kPi = 3.14159265358979323846f;  // cgPi, reference/3dGeomUtil.h:19
  const float width = kPi / 2.0f / (float)belts;
  cos_lo.assign(belts, 1.0f);
  count.resize(belts);
  first.resize(belts);
  uint32_t so_far = 0;
  for (uint32_t i = 0; i < belts; ++i) {
    count[i] = (uint32_t)std::ceil(static_cast<double>(4.0f * (float)belts) *
                                   std::sin(static_cast<double>((2.0f * (float)i + 1.0f) / (4.0f * (float)belts) * kPi)));
    first[i] = so_far;
    so_far += count[i];
    if (i) cos_lo[i] = std::cos((float)i * width);
  }
  return BZR_OK;
}

bzr_status check_emitter(const bzr_emitter *em) {
  if (!em) return set_error(BZR_ERR_INVALID_ARGUMENT, "null emitter");
  if (!em->parts_u || !em->parts_v || !em->points_per_part || !em->rays_per_point)
    return set_error(BZR_ERR_INVALID_ARGUMENT, "emitter counts must be positive");
  // belt_tables' bound, ahead of every carve sized from belts
  if (em->belts == 0 || em->belts > 4096) return set_error(BZR_ERR_INVALID_ARGUMENT, "belts must be 1..4096");
  return BZR_OK;
}

// The kernels' BeltTable in device memory: its three rows carved from `st`, then filled (the host tables must
// outlive the copies: the callers synchronise before they return).
void belt_layout(Staging &st, uint32_t belts, BeltTable &bt) {
  bt.belts = belts;
  st.take(bt.cos_lo, belts), st.take(bt.count, belts), st.take(bt.first, belts);
}
struct BeltHost {
  std::vector<float> cos_lo;
  std::vector<uint32_t> count, first;
};
bzr_status upload_belts(bzr_ctx *ctx, const BeltTable &bt, BeltHost &h) {
  if (bzr_status s = belt_tables(bt.belts, h.cos_lo, h.count, h.first)) return s;
  BZR_HIP(hipMemcpyAsync(const_cast<float *>(bt.cos_lo), h.cos_lo.data(), bt.belts * 4, hipMemcpyHostToDevice, ctx->stream));
  BZR_HIP(hipMemcpyAsync(const_cast<uint32_t *>(bt.count), h.count.data(), bt.belts * 4, hipMemcpyHostToDevice, ctx->stream));
  BZR_HIP(hipMemcpyAsync(const_cast<uint32_t *>(bt.first), h.first.data(), bt.belts * 4, hipMemcpyHostToDevice, ctx->stream));
  return BZR_OK;
}
}  // namespace

extern "C" bzr_status bzr_mesh_bounding_sphere(const bzr_mesh *mesh, float out[4]) {
  if (!mesh || !out) return set_error(BZR_ERR_INVALID_ARGUMENT, "null argument");
  for (int k = 0; k < 4; ++k) out[k] = mesh->sphere[k];
  return BZR_OK;
}

extern "C" bzr_status bzr_emit(bzr_ctx *ctx, const bzr_emitter *em, uint64_t first, uint32_t n, float *rays_soa,
                               uint32_t *patch_index, uint32_t flags) {
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (bzr_status s = check_emitter(em)) return s;
  if (n == 0) return BZR_OK;
  if (!rays_soa) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  const bool host = !(flags & BZR_DEVICE_PTRS);
  const size_t rb = (size_t)n * 24, pb = (size_t)n * 4;
  BeltTable bt;
  BeltHost belts;
  float *d_rays = rays_soa;
  uint32_t *d_patch = patch_index;
  if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
        belt_layout(st, em->belts, bt);
        if (host) st.take(d_rays, (size_t)n * 6);
        if (host && patch_index) st.take(d_patch, n);
      }))
    return s;
  if (bzr_status s = upload_belts(ctx, bt, belts)) return s;
  hipLaunchKernelGGL(k_emit<0>, dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream, *em, bt, first, n, n, d_rays, d_patch,
                     (uint32_t *)nullptr, (uint32_t *)nullptr, make_float4(0.0f, 0.0f, 0.0f, 0.0f), (const float4 *)nullptr,
                     0u, (unsigned long long *)nullptr, (float *)nullptr, 0u, (unsigned long long *)nullptr,
                     (uint8_t *)nullptr, 0u);
  BZR_HIP(hipGetLastError());
  if (host) {
    BZR_HIP(hipMemcpyAsync(rays_soa, d_rays, rb, hipMemcpyDeviceToHost, ctx->stream));
    if (patch_index) BZR_HIP(hipMemcpyAsync(patch_index, d_patch, pb, hipMemcpyDeviceToHost, ctx->stream));
  }
  BZR_HIP(hipStreamSynchronize(ctx->stream));  // the staged belt tables must outlive the kernel
  return BZR_OK;
}

// bzr_illuminate (rad and flux null: counts only) and bzr_illuminate_power (rad and flux given, hist optional).
// bzr_illuminate_spectral: nchan > 0, `ri` is the index table [nlens][nchan], and flux, hist, stats and power hold
// nchan maps / rows of four, one per channel (NC below is 1 otherwise).
// bzr_illuminate_tir: spectral with `tir`, the chain that reflects (kModeTir) and what only that call returns.
// bzr_illuminate_media: the same with tir->media, the chain that reflects, refracts between media and absorbs
// (kModeAbsorb); k_land_tir lands its rays as they are (the weights carry everything).
// bzr_illuminate_farfield: the same with tir->far, k_land_far after every batch's chain beside k_land_tir; without a
// target k_land_tir lands on a rectangle of size 0 that no ray meets (its EXITED rows and the ledger are still wanted).
struct IllumFar {
  const bzr_farfield *frame;
  uint64_t *flux;  // [nchan][cells of the frame], host or device memory like the near maps; flux or hist is given
  uint32_t *hist;
  uint64_t *rflux;           // the same for rays that reflected; may be null
  uint64_t *stats, *power;   // [nchan][2], host memory; each may be null
};
extern "C" const char *bzr_internal_farfield_frame(const bzr_farfield *far, uint32_t nchan, float out[13]);  // capi_host.cpp
// k_land_far's combine rounds.  0: plain per-lane atomics -- what the measurement chose (on a 5 degree
// cone into 60 cells every number of rounds was slower than none); bzr_debug_farfield_rounds sets another for an A/B.
constexpr uint32_t kFarRounds = 0;
static bzr_status far_frame(const bzr_farfield *far, uint32_t nchan, FarFrame &f) {
  float v[13];
  if (const char *why = bzr_internal_farfield_frame(far, nchan, v)) return set_error(BZR_ERR_INVALID_ARGUMENT, why);
  for (int k = 0; k < 3; ++k) f.n[k] = v[k], f.au[k] = v[3 + k], f.av[k] = v[6 + k];
  f.r = v[9], f.s = v[10], f.cu = v[11], f.cv = v[12];
  f.bins_u = far->bins_u, f.bins_v = far->bins_v;
  return BZR_OK;
}
struct IllumTir {
  uint32_t max_bounces;
  uint64_t *rflux;          // the stray-light maps [nchan][cells], host or device memory like flux; each may be null
  uint32_t *rhist;
  uint64_t *count, *power;  // the ledger [nchan][BZR_LEDGER_ROWS][BZR_LEDGER_FIELDS], host memory; each may be null
  // bzr_illuminate_media: the chain is kModeAbsorb's, with the gap table [nlens + 1][nchan] and the two absorption
  // tables [nlens][nchan] (host memory, each may be null: vacuum, all zero)
  bool media = false;
  const float *gap = nullptr, *glass_absorb = nullptr, *gap_absorb = nullptr;
  const IllumFar *far = nullptr;  // bzr_illuminate_farfield
  // bzr_illuminate_ghost: the chain is kModeGhost's; ray j of the emitter draws for ray number j
  bool ghost = false;
  uint64_t ghost_seed = 0;
  // bzr_illuminate_bidir: the chain is kModeBidir's (fused only) with ghost_seed and this axis; the BACK rays' two rows
  // [nchan][BZR_LEDGER_ROWS], host memory, each may be null
  bool bidir = false;
  float axis[3] = {0.0f, 0.0f, 0.0f};
  uint64_t *back_count = nullptr, *back_power = nullptr;
  // bzr_illuminate_coated: the chain is kModeCoat's over this coating (checked; null or mask 0: kModeBidir's)
  const bzr_coating *coat = nullptr;
};
static bzr_status illuminate(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri, uint32_t nlens,
                             const bzr_emitter *em, uint64_t total_rays, const bzr_target *tg, const bzr_radiometry *rad,
                             uint64_t *flux, uint32_t *hist, uint64_t *stats, uint64_t *power, uint32_t flags,
                             bool spectral = false, uint32_t nchan = 0, const IllumTir *tir = nullptr) {
  const bool with_power = rad != nullptr;
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (nlens == 0 || nlens > kMaxLenses) return set_error(BZR_ERR_INVALID_ARGUMENT, "nlens must be 1..8");
  if (tir && tir->max_bounces > BZR_MAX_BOUNCES) return set_error(BZR_ERR_INVALID_ARGUMENT, "max_bounces must be 0..8");
  if (spectral)
    if (bzr_status s = check_channels(ri, nchan)) return s;
  const bool media = tir && tir->media;
  if (media) {
    if (bzr_status s = check_gap_table(tir->gap, nlens, nchan)) return s;
    if (bzr_status s = check_absorb_table(tir->glass_absorb, nlens, nchan, "glass_absorb entries must be finite and >= 0"))
      return s;
    if (bzr_status s = check_absorb_table(tir->gap_absorb, nlens, nchan, "gap_absorb entries must be finite and >= 0"))
      return s;
  }
  const uint32_t NC = spectral ? nchan : 1u;
  const IllumFar *const far = tir ? tir->far : nullptr;
  FarFrame ff{};
  const bzr_target nowhere{{0.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}, 0.0f, 0.0f, 1u, 1u};
  const bool landing = tg != nullptr;  // false: far field only (k_land_tir meets `nowhere`)
  if (far) {
    if (bzr_status s = far_frame(far->frame, nchan, ff)) return s;
    if (!far->flux && !far->hist) return set_error(BZR_ERR_INVALID_ARGUMENT, "null far_flux_q32 and far_hist");
    if (!landing) {
      if (flux || hist || tir->rflux || tir->rhist)
        return set_error(BZR_ERR_INVALID_ARGUMENT, "target maps given without a target");
      tg = &nowhere;
    }
  }
  if (!lenses || !ri || !tg || (!with_power && !hist)) return set_error(BZR_ERR_INVALID_ARGUMENT, "null argument");
  if (with_power) {
    if (!flux && landing) return set_error(BZR_ERR_INVALID_ARGUMENT, "null flux_q32");
    if (total_rays >= (1ull << 32)) return set_error(BZR_ERR_INVALID_ARGUMENT, "total_rays must be below 2^32 (64-bit power sums)");
    if (rad->emission > BZR_EMISSION_LAMBERT) return set_error(BZR_ERR_INVALID_ARGUMENT, "unknown emission");
    if (rad->surface > BZR_SURFACE_FRESNEL) return set_error(BZR_ERR_INVALID_ARGUMENT, "unknown surface");
  }
  const bool fresnel = with_power && rad->surface == BZR_SURFACE_FRESNEL;
  if (bzr_status s = check_emitter(em)) return s;
  if (landing && (!tg->bins_u || !tg->bins_v || !(tg->size_u > 0.0f) || !(tg->size_v > 0.0f)))
    return set_error(BZR_ERR_INVALID_ARGUMENT, "target bins and sizes must be positive");
  if (bzr_status s = check_flags(flags)) return s;
  LensSet set{};
  set.count = nlens;
  for (uint32_t l = 0; l < nlens; ++l) {
    if (bzr_status s = check_ctx_mesh(ctx, lenses[l])) return s;
    set.lens[l] = view_of(lenses[l], spectral ? 1.0f : ri[l]);
  }
  const uint32_t nb = max_patches(set);
  DeviceGuard g(ctx->device);
  if (spectral)
    if (bzr_status s = upload_ri_table(ctx, ri, nlens, nchan)) return s;
  if (media) {
    if (bzr_status s = upload_gap_table(ctx, tir->gap, nlens, nchan)) return s;
    if (bzr_status s = upload_absorb_table(ctx, tir->glass_absorb, nlens, nchan, kGlassAbsorbAt, ctx->glass_absorb_host))
      return s;
    if (bzr_status s = upload_absorb_table(ctx, tir->gap_absorb, nlens, nchan, kGapAbsorbAt, ctx->gap_absorb_host))
      return s;
    if (bzr_status s = upload_coat_table(ctx, tir->coat, nlens, nchan)) return s;
  }
  // target plane (normal = axis_u x axis_v normalised, constant = n . origin) and cell sizes, in the
  // oracle's operation order
  const float *au = tg->axis_u, *av = tg->axis_v;
  f3 pn{au[1] * av[2] - au[2] * av[1], au[2] * av[0] - au[0] * av[2], au[0] * av[1] - au[1] * av[0]};
  {
    const float z = pn.x * pn.x + (pn.y * pn.y + pn.z * pn.z);
    if (z > 0.0f) {
      const float s = std::sqrt(z);
      pn = f3{pn.x / s, pn.y / s, pn.z / s};
    }
  }
  const float pc = pn.x * tg->origin[0] + (pn.y * tg->origin[1] + pn.z * tg->origin[2]);
  const float cell_u = tg->size_u / (float)tg->bins_u, cell_v = tg->size_v / (float)tg->bins_v;
  const size_t cells = (size_t)tg->bins_u * tg->bins_v;
  if (spectral && cells >= (1ull << 32)) return set_error(BZR_ERR_INVALID_ARGUMENT, "target of 2^32 cells or more");
  const size_t maps = cells * NC;  // cells of all the channels' maps
  const bool host = !(flags & BZR_DEVICE_PTRS);
  const uint32_t B = chunk_for(ctx, total_rays);
  BeltTable bt;
  BeltHost belts;
  float *d_rays = nullptr, *d_w = nullptr;  // the batch's rays and, with_power, their power
  uint32_t *d_st = nullptr, *d_seg = nullptr, *d_hist = hist;
  unsigned long long *d_stats = nullptr, *d_power = nullptr;  // the four counts and, with_power, the four power sums
  unsigned long long *d_flux = reinterpret_cast<unsigned long long *>(flux);
  uint8_t *d_ch = nullptr;  // spectral: the batch's channel row
  // tir: the batch's bounce row and, staged, the chain's pending row behind it (one memset clears both); the ledger;
  // the stray-light maps of a host caller.  media: the chain's optical path row between the two, under the same
  // memset -- scratch that nothing returns (no glass row: the chain's is optional)
  const size_t ledger = (size_t)BZR_LEDGER_ROWS * BZR_LEDGER_FIELDS * NC;
  const bool bidir = tir && tir->bidir;
  const bool staged = !bidir && use_staged(flags, B, nb);  // (the bidirectional chain is fused only)
  const size_t back_rows = (size_t)BZR_LEDGER_ROWS * NC;
  unsigned long long *d_bcount = nullptr, *d_bpower = nullptr;
  uint32_t *d_bnc = nullptr, *d_pend = nullptr, *d_rhist = tir ? tir->rhist : nullptr;
  float *d_opl = nullptr;
  unsigned long long *d_rflux = tir ? reinterpret_cast<unsigned long long *>(tir->rflux) : nullptr;
  unsigned long long *d_lcount = nullptr, *d_lpower = nullptr;
  // far: the two rows [NC][2] and, for a host caller, the far maps (zeroed, added back like rflux)
  const size_t fmaps = far ? (size_t)ff.bins_u * ff.bins_v * NC : 0;
  unsigned long long *d_fflux = far ? reinterpret_cast<unsigned long long *>(far->flux) : nullptr;
  unsigned long long *d_frflux = far ? reinterpret_cast<unsigned long long *>(far->rflux) : nullptr;
  uint32_t *d_fhist = far ? far->hist : nullptr;
  unsigned long long *d_fstats = nullptr, *d_fpower = nullptr;
  if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
        belt_layout(st, em->belts, bt);
        st.take(d_rays, (size_t)B * 6), st.take(d_st, B), st.take(d_seg, B), st.take(d_stats, 4 * NC);
        if (host && hist) st.take(d_hist, maps);
        if (with_power) st.take(d_w, B), st.take(d_power, 4 * NC);
        if (with_power && host && flux) st.take(d_flux, maps);
        if (spectral) st.take(d_ch, B);
        if (tir) st.take(d_bnc, B);
        if (media) st.take(d_opl, B);
        if (tir && staged) st.take(d_pend, B);
        if (tir) st.take(d_lcount, ledger), st.take(d_lpower, ledger);
        if (bidir) st.take(d_bcount, back_rows), st.take(d_bpower, back_rows);
        if (tir && host && tir->rflux) st.take(d_rflux, maps);
        if (tir && host && tir->rhist) st.take(d_rhist, maps);
        if (far) st.take(d_fstats, 2 * NC), st.take(d_fpower, 2 * NC);
        if (far && host && far->flux) st.take(d_fflux, fmaps);
        if (far && host && far->hist) st.take(d_fhist, fmaps);
        if (far && host && far->rflux) st.take(d_frflux, fmaps);
      }))
    return s;
  if (bzr_status s = upload_belts(ctx, bt, belts)) return s;
  BZR_HIP(hipMemsetAsync(d_stats, 0, 32 * NC, ctx->stream));
  if (host && hist) BZR_HIP(hipMemsetAsync(d_hist, 0, maps * 4, ctx->stream));
  if (with_power) {
    BZR_HIP(hipMemsetAsync(d_power, 0, 32 * NC, ctx->stream));
    if (host && flux) BZR_HIP(hipMemsetAsync(d_flux, 0, maps * 8, ctx->stream));
  }
  if (far) {
    BZR_HIP(hipMemsetAsync(d_fstats, 0, 16 * NC, ctx->stream));
    BZR_HIP(hipMemsetAsync(d_fpower, 0, 16 * NC, ctx->stream));
    if (host && far->flux) BZR_HIP(hipMemsetAsync(d_fflux, 0, fmaps * 8, ctx->stream));
    if (host && far->hist) BZR_HIP(hipMemsetAsync(d_fhist, 0, fmaps * 4, ctx->stream));
    if (host && far->rflux) BZR_HIP(hipMemsetAsync(d_frflux, 0, fmaps * 8, ctx->stream));
  }
  if (tir) {
    BZR_HIP(hipMemsetAsync(d_lcount, 0, ledger * 8, ctx->stream));
    BZR_HIP(hipMemsetAsync(d_lpower, 0, ledger * 8, ctx->stream));
    if (host && tir->rflux) BZR_HIP(hipMemsetAsync(d_rflux, 0, maps * 8, ctx->stream));
    if (host && tir->rhist) BZR_HIP(hipMemsetAsync(d_rhist, 0, maps * 4, ctx->stream));
  }
  if (bidir) {
    BZR_HIP(hipMemsetAsync(d_bcount, 0, back_rows * 8, ctx->stream));
    BZR_HIP(hipMemsetAsync(d_bpower, 0, back_rows * 8, ctx->stream));
  }
  // The in-place job has alive_in set, so the chain has no first stage: nothing in it writes a culled ray's bounce
  // word (either pipeline) or pending word (staged), and a staged bounce stage traces every ray whose pending word is
  // set.  Both rows are therefore cleared before every batch's chain, by one memset on the context's stream (chosen
  // over a store in k_emit, whose instantiations for the other entry points stay as they are).  The media chain's
  // optical path row is in the same case: its first stage would have written every ray's word, later stages add to it.
  const uint32_t *const last_row = staged ? d_pend : media ? reinterpret_cast<uint32_t *>(d_opl) : d_bnc;
  const size_t tir_rows = !tir ? 0 : (size_t)(reinterpret_cast<const char *>(last_row + B) - reinterpret_cast<char *>(d_bnc));
  Work w;
  if (staged)
    if (bzr_status s = ensure_work(ctx, B, nb, w)) return s;
  const float4 sphere = make_float4(lenses[0]->sphere[0], lenses[0]->sphere[1], lenses[0]->sphere[2],
                                    lenses[0]->sphere[3]);
  const uint32_t lambert = with_power && rad->emission == BZR_EMISSION_LAMBERT ? 1u : 0u;
  // the mode, chosen once: the chain's (a lossless surface leaves the weights as emitted: the plain chain; the
  // spectral chain refracts per channel with a lossless surface too: its run-time flag) and the two kernels'
  auto *const chain = (tir && tir->ghost) ? &run_chain<kModeGhost>
                      : media    ? &run_chain<kModeAbsorb>
                      : tir      ? &run_chain<kModeTir>
                      : spectral ? &run_chain<kModeSpectral>
                      : fresnel  ? &run_chain<kModePower>
                                 : &run_chain<kModeStage>;
  auto *const emit = spectral ? &k_emit<2> : with_power ? &k_emit<1> : &k_emit<0>;
  auto *const land = spectral ? &k_land<2> : with_power ? &k_land<1> : &k_land<0>;
  for (uint64_t first = 0; first < total_rays; first += B) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(B, total_rays - first);
    hipLaunchKernelGGL(emit, dim3(grid_for(m)), dim3(kBlock), 0, ctx->stream, *em, bt, first, m, B, d_rays,
                       (uint32_t *)nullptr, d_st, d_seg, sphere, set.lens[0].always, set.lens[0].n_always, d_stats, d_w,
                       lambert, d_power, d_ch, nchan);
    if (tir) BZR_HIP(hipMemsetAsync(d_bnc, 0, tir_rows, ctx->stream));
    TraceJob job{};  // the chain in place over the batch; culled rays (status NONE) are skipped
    job.rays = job.out_rays = d_rays;
    job.alive_in = job.status = d_st;
    job.segments = d_seg;
    job.n = m;
    job.ld = B;
    job.weight_in = job.weight = d_w;
    job.channel = d_ch;
    job.ri_table = ctx->ri_table;
    job.nchan = nchan;
    job.lossless = fresnel ? 0u : 1u;
    job.bounces = d_bnc;
    job.max_bounces = tir ? tir->max_bounces : 0u;
    if (media) {
      job.opl = d_opl;
      job.gap_table = ctx->ri_table + kRiTableFloats;
    }
    if (tir && tir->ghost) {
      job.ghost_base = ghost_base(tir->ghost_seed, first);
    }
    if (bidir) {
      job.ghost_base = ghost_base(tir->ghost_seed, first);
      job.axis_xy[0] = tir->axis[0];
      job.axis_xy[1] = tir->axis[1];
      job.axis_z = tir->axis[2];
      // (a lossless call draws nothing and pays no T: the coating is ignored, the chain is kModeBidir's)
      const uint32_t coat_mask = (tir->coat && !job.lossless) ? tir->coat->mask : 0u;
      if (coat_mask != 0u) {
        job.max_bounces |= coat_mask << 16;
        if (bzr_status s = run_fused<kModeCoat>(ctx, set, job, flags)) return s;
      } else if (bzr_status s = run_fused<kModeBidir>(ctx, set, job, flags)) return s;
      hipLaunchKernelGGL(k_back_rows, dim3(grid_for(m)), dim3(kBlock), 0, ctx->stream, m, (const uint32_t *)d_st,
                         (const uint32_t *)d_seg, (const uint32_t *)d_bnc, (const float *)d_w, (const uint8_t *)d_ch,
                         d_bcount, d_bpower);
    } else if (bzr_status s = chain(ctx, set, job, flags, staged, d_pend, B, w)) return s;
    if (tir)
      hipLaunchKernelGGL(k_land_tir, dim3(grid_for(m)), dim3(kBlock), 0, ctx->stream, *tg,
                         make_float4(pn.x, pn.y, pn.z, pc), cell_u, cell_v, d_rays, B, m, d_st, d_hist, d_stats, d_w, d_flux,
                         d_power, (const uint8_t *)d_ch, (uint32_t)cells,
                         LandTir{d_seg, d_bnc, d_rhist, d_rflux, d_lcount, d_lpower});
    else
      hipLaunchKernelGGL(land, dim3(grid_for(m)), dim3(kBlock), 0, ctx->stream, *tg, make_float4(pn.x, pn.y, pn.z, pc),
                         cell_u, cell_v, d_rays, B, m, d_st, d_hist, d_stats, d_w, d_flux, d_power, (const uint8_t *)d_ch,
                         spectral ? (uint32_t)cells : 0u);
    if (far)
      hipLaunchKernelGGL(k_land_far, dim3(grid_for(m)), dim3(kBlock), 0, ctx->stream, ff, ff.bins_u * ff.bins_v,
                         (const float *)d_rays, B, m, (const uint32_t *)d_st, (const float *)d_w, (const uint8_t *)d_ch,
                         nchan, (const uint32_t *)d_bnc, d_fflux, d_fhist, d_frflux, d_fstats, d_fpower,
                         ctx->far_rounds < 0 ? kFarRounds : (uint32_t)ctx->far_rounds);
    BZR_HIP(hipGetLastError());
  }
  unsigned long long hs[4 * kMaxChannels];
  BZR_HIP(hipMemcpyAsync(hs, d_stats, 32 * NC, hipMemcpyDeviceToHost, ctx->stream));
  std::vector<uint32_t> hh(host && hist ? maps : 0);
  if (host && hist) BZR_HIP(hipMemcpyAsync(hh.data(), d_hist, maps * 4, hipMemcpyDeviceToHost, ctx->stream));
  unsigned long long hp[4 * kMaxChannels] = {};
  std::vector<unsigned long long> hf(host && with_power && flux ? maps : 0);
  if (with_power) {
    BZR_HIP(hipMemcpyAsync(hp, d_power, 32 * NC, hipMemcpyDeviceToHost, ctx->stream));
    if (!hf.empty()) BZR_HIP(hipMemcpyAsync(hf.data(), d_flux, maps * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  unsigned long long hfs[4 * kMaxChannels] = {};  // the far rows: [NC][2] stats, then [NC][2] power
  std::vector<unsigned long long> hff(far && host && far->flux ? fmaps : 0), hfr(far && host && far->rflux ? fmaps : 0);
  std::vector<uint32_t> hfh(far && host && far->hist ? fmaps : 0);
  if (far) {
    BZR_HIP(hipMemcpyAsync(hfs, d_fstats, 16 * NC, hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipMemcpyAsync(hfs + 2 * NC, d_fpower, 16 * NC, hipMemcpyDeviceToHost, ctx->stream));
    if (!hff.empty()) BZR_HIP(hipMemcpyAsync(hff.data(), d_fflux, fmaps * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!hfh.empty()) BZR_HIP(hipMemcpyAsync(hfh.data(), d_fhist, fmaps * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (!hfr.empty()) BZR_HIP(hipMemcpyAsync(hfr.data(), d_frflux, fmaps * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  std::vector<unsigned long long> hrf(tir && host && tir->rflux ? maps : 0), hl(tir ? 2 * ledger : 0);
  std::vector<uint32_t> hrh(tir && host && tir->rhist ? maps : 0);
  if (tir) {
    BZR_HIP(hipMemcpyAsync(hl.data(), d_lcount, ledger * 8, hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipMemcpyAsync(hl.data() + ledger, d_lpower, ledger * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!hrf.empty()) BZR_HIP(hipMemcpyAsync(hrf.data(), d_rflux, maps * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!hrh.empty()) BZR_HIP(hipMemcpyAsync(hrh.data(), d_rhist, maps * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  std::vector<unsigned long long> hb(bidir ? 2 * back_rows : 0);
  if (bidir) {
    BZR_HIP(hipMemcpyAsync(hb.data(), d_bcount, back_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipMemcpyAsync(hb.data() + back_rows, d_bpower, back_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  if (bidir && tir->back_count)
    for (size_t k = 0; k < back_rows; ++k) tir->back_count[k] = hb[k];
  if (bidir && tir->back_power)
    for (size_t k = 0; k < back_rows; ++k) tir->back_power[k] = hb[back_rows + k];
  for (size_t k = 0; k < hrf.size(); ++k) tir->rflux[k] += hrf[k];
  for (size_t k = 0; k < hrh.size(); ++k) tir->rhist[k] += hrh[k];
  if (tir && tir->count)
    for (size_t k = 0; k < ledger; ++k) tir->count[k] = hl[k];
  if (tir && tir->power)
    for (size_t k = 0; k < ledger; ++k) tir->power[k] = hl[ledger + k];
  if (host && hist)
    for (size_t k = 0; k < maps; ++k) hist[k] += hh[k];
  for (size_t k = 0; k < hf.size(); ++k) flux[k] += hf[k];
  for (size_t k = 0; k < hff.size(); ++k) far->flux[k] += hff[k];
  for (size_t k = 0; k < hfh.size(); ++k) far->hist[k] += hfh[k];
  for (size_t k = 0; k < hfr.size(); ++k) far->rflux[k] += hfr[k];
  if (far && far->stats)
    for (uint32_t k = 0; k < 2 * NC; ++k) far->stats[k] = hfs[k];
  if (far && far->power)
    for (uint32_t k = 0; k < 2 * NC; ++k) far->power[k] = hfs[2 * NC + k];
  if (stats)
    for (uint32_t k = 0; k < 4 * NC; ++k) stats[k] = hs[k];
  if (power)
    for (uint32_t k = 0; k < 4 * NC; ++k) power[k] = hp[k];
  return BZR_OK;
}

extern "C" bzr_status bzr_illuminate(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri, uint32_t nlens,
                                     const bzr_emitter *em, uint64_t total_rays, const bzr_target *tg, uint32_t *hist,
                                     uint64_t stats[4], uint32_t flags) {
  return illuminate(ctx, lenses, ri, nlens, em, total_rays, tg, nullptr, nullptr, hist, stats, nullptr, flags);
}

extern "C" bzr_status bzr_illuminate_power(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri, uint32_t nlens,
                                           const bzr_emitter *em, uint64_t total_rays, const bzr_target *tg,
                                           const bzr_radiometry *rad, uint64_t *flux_q32, uint32_t *hist, uint64_t stats[4],
                                           uint64_t power_q32[4], uint32_t flags) {
  if (!rad) return set_error(BZR_ERR_INVALID_ARGUMENT, "null radiometry");
  return illuminate(ctx, lenses, ri, nlens, em, total_rays, tg, rad, flux_q32, hist, stats, power_q32, flags);
}

extern "C" bzr_status bzr_illuminate_spectral(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                              uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                              const bzr_target *tg, const bzr_radiometry *rad, uint64_t *flux_q32,
                                              uint32_t *hist, uint64_t *stats, uint64_t *power_q32, uint32_t flags) {
  if (!rad) return set_error(BZR_ERR_INVALID_ARGUMENT, "null radiometry");
  return illuminate(ctx, lenses, ri_table, nlens, em, total_rays, tg, rad, flux_q32, hist, stats, power_q32, flags, true,
                    nchan);
}

extern "C" bzr_status bzr_illuminate_tir(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table, uint32_t nlens,
                                         uint32_t nchan, const bzr_emitter *em, uint64_t total_rays, const bzr_target *tg,
                                         const bzr_radiometry *rad, uint32_t max_bounces, uint64_t *flux_q32, uint32_t *hist,
                                         uint64_t *reflected_flux_q32, uint32_t *reflected_hist, uint64_t *stats,
                                         uint64_t *power_q32, uint64_t *ledger_count, uint64_t *ledger_power_q32,
                                         uint32_t flags) {
  if (!rad) return set_error(BZR_ERR_INVALID_ARGUMENT, "null radiometry");
  const IllumTir tir{max_bounces, reflected_flux_q32, reflected_hist, ledger_count, ledger_power_q32};
  return illuminate(ctx, lenses, ri_table, nlens, em, total_rays, tg, rad, flux_q32, hist, stats, power_q32, flags, true,
                    nchan, &tir);
}

extern "C" bzr_status bzr_illuminate_media(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                           const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                           uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                           const bzr_target *tg, const bzr_radiometry *rad, uint32_t max_bounces,
                                           uint64_t *flux_q32, uint32_t *hist, uint64_t *reflected_flux_q32,
                                           uint32_t *reflected_hist, uint64_t *stats, uint64_t *power_q32,
                                           uint64_t *ledger_count, uint64_t *ledger_power_q32, uint32_t flags) {
  if (!rad) return set_error(BZR_ERR_INVALID_ARGUMENT, "null radiometry");
  IllumTir tir{max_bounces, reflected_flux_q32, reflected_hist, ledger_count, ledger_power_q32};
  tir.media = true;
  tir.gap = gap_table;
  tir.glass_absorb = glass_absorb;
  tir.gap_absorb = gap_absorb;
  return illuminate(ctx, lenses, ri_table, nlens, em, total_rays, tg, rad, flux_q32, hist, stats, power_q32, flags, true,
                    nchan, &tir);
}

extern "C" bzr_status bzr_illuminate_farfield(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                              const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                              uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                              const bzr_target *tg, const bzr_radiometry *rad, uint32_t max_bounces,
                                              uint64_t *flux_q32, uint32_t *hist, uint64_t *reflected_flux_q32,
                                              uint32_t *reflected_hist, uint64_t *stats, uint64_t *power_q32,
                                              uint64_t *ledger_count, uint64_t *ledger_power_q32, uint32_t flags,
                                              const bzr_farfield *far, uint64_t *far_flux_q32, uint32_t *far_hist,
                                              uint64_t *far_reflected_flux_q32, uint64_t *far_stats,
                                              uint64_t *far_power_q32) {
  if (!rad) return set_error(BZR_ERR_INVALID_ARGUMENT, "null radiometry");
  FarFrame checked{};  // (the frame's own checks need no context: ahead of illuminate()'s)
  if (bzr_status s = far_frame(far, nchan, checked)) return s;
  const IllumFar ifar{far, far_flux_q32, far_hist, far_reflected_flux_q32, far_stats, far_power_q32};
  IllumTir tir{max_bounces, reflected_flux_q32, reflected_hist, ledger_count, ledger_power_q32};
  tir.media = true;
  tir.gap = gap_table;
  tir.glass_absorb = glass_absorb;
  tir.gap_absorb = gap_absorb;
  tir.far = &ifar;
  return illuminate(ctx, lenses, ri_table, nlens, em, total_rays, tg, rad, flux_q32, hist, stats, power_q32, flags, true,
                    nchan, &tir);
}

// bzr_illuminate_farfield with the roulette chain; `far` may be null (bzr_illuminate_media's outputs alone).
extern "C" bzr_status bzr_illuminate_ghost(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                           const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                           uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                           const bzr_target *tg, const bzr_radiometry *rad, uint32_t max_bounces,
                                           uint64_t ghost_seed, uint64_t *flux_q32, uint32_t *hist,
                                           uint64_t *reflected_flux_q32, uint32_t *reflected_hist, uint64_t *stats,
                                           uint64_t *power_q32, uint64_t *ledger_count, uint64_t *ledger_power_q32,
                                           uint32_t flags, const bzr_farfield *far, uint64_t *far_flux_q32,
                                           uint32_t *far_hist, uint64_t *far_reflected_flux_q32, uint64_t *far_stats,
                                           uint64_t *far_power_q32) {
  if (!rad) return set_error(BZR_ERR_INVALID_ARGUMENT, "null radiometry");
  if (!far && (far_flux_q32 || far_hist || far_reflected_flux_q32 || far_stats || far_power_q32))
    return set_error(BZR_ERR_INVALID_ARGUMENT, "far outputs given without a far-field frame");
  if (!far && !tg) return set_error(BZR_ERR_INVALID_ARGUMENT, "neither a target nor a far-field frame");
  if (far) {
    FarFrame checked{};
    if (bzr_status s = far_frame(far, nchan, checked)) return s;
  }
  const IllumFar ifar{far, far_flux_q32, far_hist, far_reflected_flux_q32, far_stats, far_power_q32};
  IllumTir tir{max_bounces, reflected_flux_q32, reflected_hist, ledger_count, ledger_power_q32};
  tir.media = true;
  tir.gap = gap_table;
  tir.glass_absorb = glass_absorb;
  tir.gap_absorb = gap_absorb;
  tir.far = far ? &ifar : nullptr;
  tir.ghost = true;
  tir.ghost_seed = ghost_seed;
  return illuminate(ctx, lenses, ri_table, nlens, em, total_rays, tg, rad, flux_q32, hist, stats, power_q32, flags, true,
                    nchan, &tir);
}

// bzr_illuminate_ghost over the bidirectional chain, with the BACK rays' two rows.
extern "C" bzr_status bzr_illuminate_bidir(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                           const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                           uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                           const bzr_target *tg, const bzr_radiometry *rad, uint32_t max_bounces,
                                           uint64_t ghost_seed, const float axis[3], uint64_t *flux_q32, uint32_t *hist,
                                           uint64_t *reflected_flux_q32, uint32_t *reflected_hist, uint64_t *stats,
                                           uint64_t *power_q32, uint64_t *ledger_count, uint64_t *ledger_power_q32,
                                           uint64_t *back_count, uint64_t *back_power_q32, uint32_t flags,
                                           const bzr_farfield *far, uint64_t *far_flux_q32, uint32_t *far_hist,
                                           uint64_t *far_reflected_flux_q32, uint64_t *far_stats,
                                           uint64_t *far_power_q32) {
  if (!rad) return set_error(BZR_ERR_INVALID_ARGUMENT, "null radiometry");
  if (!far && (far_flux_q32 || far_hist || far_reflected_flux_q32 || far_stats || far_power_q32))
    return set_error(BZR_ERR_INVALID_ARGUMENT, "far outputs given without a far-field frame");
  if (!far && !tg) return set_error(BZR_ERR_INVALID_ARGUMENT, "neither a target nor a far-field frame");
  if (bzr_status s = check_axis(axis)) return s;
  if (bzr_status s = check_bidir_flags(flags)) return s;
  if (far) {
    FarFrame checked{};
    if (bzr_status s = far_frame(far, nchan, checked)) return s;
  }
  const IllumFar ifar{far, far_flux_q32, far_hist, far_reflected_flux_q32, far_stats, far_power_q32};
  IllumTir tir{max_bounces, reflected_flux_q32, reflected_hist, ledger_count, ledger_power_q32};
  tir.media = true;
  tir.gap = gap_table;
  tir.glass_absorb = glass_absorb;
  tir.gap_absorb = gap_absorb;
  tir.far = far ? &ifar : nullptr;
  tir.ghost_seed = ghost_seed;
  tir.bidir = true;
  tir.axis[0] = axis[0], tir.axis[1] = axis[1], tir.axis[2] = axis[2];
  tir.back_count = back_count;
  tir.back_power = back_power_q32;
  return illuminate(ctx, lenses, ri_table, nlens, em, total_rays, tg, rad, flux_q32, hist, stats, power_q32, flags, true,
                    nchan, &tir);
}

// bzr_illuminate_bidir over the coated chain.
extern "C" bzr_status bzr_illuminate_coated(bzr_ctx *ctx, const bzr_mesh *const *lenses, const float *ri_table,
                                            const float *gap_table, const float *glass_absorb, const float *gap_absorb,
                                            uint32_t nlens, uint32_t nchan, const bzr_emitter *em, uint64_t total_rays,
                                            const bzr_target *tg, const bzr_radiometry *rad, uint32_t max_bounces,
                                            uint64_t ghost_seed, const float axis[3], const bzr_coating *coat,
                                            uint64_t *flux_q32, uint32_t *hist, uint64_t *reflected_flux_q32,
                                            uint32_t *reflected_hist, uint64_t *stats, uint64_t *power_q32,
                                            uint64_t *ledger_count, uint64_t *ledger_power_q32, uint64_t *back_count,
                                            uint64_t *back_power_q32, uint32_t flags, const bzr_farfield *far,
                                            uint64_t *far_flux_q32, uint32_t *far_hist, uint64_t *far_reflected_flux_q32,
                                            uint64_t *far_stats, uint64_t *far_power_q32) {
  if (!rad) return set_error(BZR_ERR_INVALID_ARGUMENT, "null radiometry");
  if (!far && (far_flux_q32 || far_hist || far_reflected_flux_q32 || far_stats || far_power_q32))
    return set_error(BZR_ERR_INVALID_ARGUMENT, "far outputs given without a far-field frame");
  if (!far && !tg) return set_error(BZR_ERR_INVALID_ARGUMENT, "neither a target nor a far-field frame");
  if (bzr_status s = check_axis(axis)) return s;
  if (bzr_status s = check_bidir_flags(flags)) return s;
  if (nlens >= 1 && nlens <= kMaxLenses && nchan >= 1 && nchan <= kMaxChannels)
    if (bzr_status s = check_coating(coat, nlens, nchan)) return s;
  if (far) {
    FarFrame checked{};
    if (bzr_status s = far_frame(far, nchan, checked)) return s;
  }
  const IllumFar ifar{far, far_flux_q32, far_hist, far_reflected_flux_q32, far_stats, far_power_q32};
  IllumTir tir{max_bounces, reflected_flux_q32, reflected_hist, ledger_count, ledger_power_q32};
  tir.media = true;
  tir.gap = gap_table;
  tir.glass_absorb = glass_absorb;
  tir.gap_absorb = gap_absorb;
  tir.far = far ? &ifar : nullptr;
  tir.ghost_seed = ghost_seed;
  tir.bidir = true;
  tir.axis[0] = axis[0], tir.axis[1] = axis[1], tir.axis[2] = axis[2];
  tir.back_count = back_count;
  tir.back_power = back_power_q32;
  tir.coat = coat;
  return illuminate(ctx, lenses, ri_table, nlens, em, total_rays, tg, rad, flux_q32, hist, stats, power_q32, flags, true,
                    nchan, &tir);
}

// Host pointers: the rows and zeroed maps are staged in the context's carve, and the call waits (like bzr_emit).
// Device pointers: k_land_far adds straight into the caller's maps; only the two host rows make the call wait.
extern "C" bzr_status bzr_farfield_bin(bzr_ctx *ctx, const bzr_farfield *far, const float *rays_soa, const float *weight,
                                       const uint32_t *status, const uint8_t *channel, uint32_t n, uint32_t nchan,
                                       uint64_t *far_flux_q32, uint32_t *far_hist, uint64_t *far_stats,
                                       uint64_t *far_power_q32, uint32_t flags) {
  if (bzr_status s = check_flags(flags)) return s;
  FarFrame ff{};
  if (bzr_status s = far_frame(far, nchan, ff)) return s;
  if (!far_flux_q32 && !far_hist) return set_error(BZR_ERR_INVALID_ARGUMENT, "null far_flux_q32 and far_hist");
  if (n == 0) return BZR_OK;
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (!rays_soa) return set_error(BZR_ERR_INVALID_ARGUMENT, "null buffer");
  DeviceGuard g(ctx->device);
  const bool host = !(flags & BZR_DEVICE_PTRS), rows = far_stats || far_power_q32;
  const size_t maps = (size_t)ff.bins_u * ff.bins_v * nchan;
  const float *d_rays = rays_soa, *d_w = weight;
  const uint32_t *d_st = status;
  const uint8_t *d_ch = channel;
  unsigned long long *d_flux = reinterpret_cast<unsigned long long *>(far_flux_q32), *d_stats = nullptr, *d_power = nullptr;
  uint32_t *d_hist = far_hist;
  if (host || rows)
    if (bzr_status s = carve_buffer(ctx->scratch, ctx->scratch_bytes, [&](Staging &st) {
          if (rows) st.take(d_stats, 2 * nchan), st.take(d_power, 2 * nchan);
          if (!host) return;
          st.take(d_rays, (size_t)n * 6);
          if (weight) st.take(d_w, n);
          if (status) st.take(d_st, n);
          if (channel) st.take(d_ch, n);
          if (far_flux_q32) st.take(d_flux, maps);
          if (far_hist) st.take(d_hist, maps);
        }))
      return s;
  if (rows) {
    BZR_HIP(hipMemsetAsync(d_stats, 0, 16 * nchan, ctx->stream));
    BZR_HIP(hipMemsetAsync(d_power, 0, 16 * nchan, ctx->stream));
  }
  if (host) {
    BZR_HIP(hipMemcpyAsync(const_cast<float *>(d_rays), rays_soa, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
    if (weight) BZR_HIP(hipMemcpyAsync(const_cast<float *>(d_w), weight, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (status)
      BZR_HIP(hipMemcpyAsync(const_cast<uint32_t *>(d_st), status, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (channel) BZR_HIP(hipMemcpyAsync(const_cast<uint8_t *>(d_ch), channel, n, hipMemcpyHostToDevice, ctx->stream));
    if (far_flux_q32) BZR_HIP(hipMemsetAsync(d_flux, 0, maps * 8, ctx->stream));
    if (far_hist) BZR_HIP(hipMemsetAsync(d_hist, 0, maps * 4, ctx->stream));
  }
  const uint32_t grid = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_land_far, dim3(grid), dim3(kBlock), 0, ctx->stream, ff, ff.bins_u * ff.bins_v, d_rays, n, n, d_st,
                     d_w, d_ch, nchan, (const uint32_t *)nullptr, d_flux, d_hist, (unsigned long long *)nullptr, d_stats,
                     d_power, ctx->far_rounds < 0 ? kFarRounds : (uint32_t)ctx->far_rounds);
  BZR_HIP(hipGetLastError());
  if (!host && !rows) return BZR_OK;
  unsigned long long hs[4 * kMaxChannels] = {};
  std::vector<unsigned long long> hf(host && far_flux_q32 ? maps : 0);
  std::vector<uint32_t> hh(host && far_hist ? maps : 0);
  if (rows) {
    BZR_HIP(hipMemcpyAsync(hs, d_stats, 16 * nchan, hipMemcpyDeviceToHost, ctx->stream));
    BZR_HIP(hipMemcpyAsync(hs + 2 * nchan, d_power, 16 * nchan, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (!hf.empty()) BZR_HIP(hipMemcpyAsync(hf.data(), d_flux, maps * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (!hh.empty()) BZR_HIP(hipMemcpyAsync(hh.data(), d_hist, maps * 4, hipMemcpyDeviceToHost, ctx->stream));
  BZR_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < hf.size(); ++k) far_flux_q32[k] += hf[k];
  for (size_t k = 0; k < hh.size(); ++k) far_hist[k] += hh[k];
  if (far_stats)
    for (uint32_t k = 0; k < 2 * nchan; ++k) far_stats[k] = hs[k];
  if (far_power_q32)
    for (uint32_t k = 0; k < 2 * nchan; ++k) far_power_q32[k] = hs[2 * nchan + k];
  return BZR_OK;
}

extern "C" int32_t bzr_debug_farfield_rounds(void *ctxp, int32_t rounds) {
  bzr_ctx *ctx = static_cast<bzr_ctx *>(ctxp);
  if (!ctx) return set_error(BZR_ERR_INVALID_ARGUMENT, "null context");
  if (rounds > 64) return set_error(BZR_ERR_INVALID_ARGUMENT, "rounds must be at most 64");
  ctx->far_rounds = rounds < 0 ? -1 : rounds;
  return BZR_OK;
}
