// The bidirectional chain through the C++ drop-in: bzr::traceChainBidir against bzr::traceChainAbsorb and the C ABI.
//   CPU part: the signature of both entry points, the refusals that need no context (a zero or NaN axis, max_bounces 9,
//             the staged flag, a table of the wrong size) and bzr_bidir_uniform -- its range check and a restatement of
//             the header's recipe in plain uint64_t at e = 256 + segment.
//   GPU part (when a HIP device is visible): traceChainBidir over cfg2's rays at 64 x 64 with four channels, media,
//             absorption, weights and path in place: at budget 0 traceChainAbsorb's seven outputs bit for bit on every ray
//             that did not leave backward; at budget 4 the same call twice gives the same bits, the C ABI called directly
//             gives them too, another seed does not, rays come BACK, and without absorption a ray with budget left keeps
//             its weight bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "bezierLens.h"
#include "bezierMesh.h"
#include "bzr_debug.h"
#include "mesh.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) {                                                           \
      ++g_fail;                                                              \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                        \
  } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// cfg2's primary rays: plane x = 0, y in [-4.2, 4.2], z in [-2.1, 2.1], along +x
static std::vector<Ray> cfg2_rays(int side) {
  std::vector<Ray> rays;
  for (int i = 0; i < side; ++i)
    for (int j = 0; j < side; ++j)
      rays.emplace_back(Vertex{0.0f, -4.2f + 8.4f * (j + 0.5f) / side, -2.1f + 4.2f * (i + 0.5f) / side}, Vector{1, 0, 0});
  return rays;
}

using CAbi = bzr_status (*)(bzr_ctx *, const bzr_mesh *const *, const float *, const float *, const float *,
                            const float *, uint32_t, uint32_t, const float *, const uint8_t *, const float *,
                            const float *, uint32_t, uint32_t, uint64_t, uint64_t, const float *, float *, float *,
                            uint32_t *, uint32_t *, uint32_t *, float *, float *, uint32_t);
using Cpp = void (*)(std::vector<BezierLens const *> const &, std::vector<float> const &, std::vector<float> const &,
                     std::vector<float> const &, std::vector<float> const &, Ray const *, uint8_t const *, float const *,
                     float const *, std::size_t, uint32_t, uint64_t, uint64_t, float const (&)[3], Ray *, float *,
                     RefractionResult *, float *, float *, uint32_t *, uint32_t *, bzr::Context *);

// include/bzr.h, restated
static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static float draw(uint64_t seed, uint64_t j, uint32_t segment) {
  const uint64_t r = mix64((seed ^ 0x5851F42D4C957F2Dull) + 0x9E3779B97F4A7C15ull * (j + 1));
  const uint64_t h = mix64(r + 0x9E3779B97F4A7C15ull * (256ull + segment + 1));
  return static_cast<float>(h >> 40) / 16777216.0f;
}
static const float kAxis[3] = {1.0f, 0.0f, 0.0f};

static void host_part(BezierMesh const &bezier) {
  CHECK(BZR_ABI_VERSION == 2 && bzr_abi_version() == 2 && BZR_RR_BACK == 4);
  static_assert(std::is_same<decltype(&bzr_trace_chain_bidir), CAbi>::value, "bzr_trace_chain_bidir's signature");
  static_assert(std::is_same<decltype(&bzr::traceChainBidir), Cpp>::value, "bzr::traceChainBidir's signature");
  float opl = 7.0f;
  auto refused = [&](uint32_t budget, const float *axis, uint32_t flags) {
    return bzr_trace_chain_bidir(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr,
                                 nullptr, 1, budget, 0, 0, axis, nullptr, nullptr, nullptr, nullptr, nullptr, &opl, nullptr,
                                 flags) == BZR_ERR_INVALID_ARGUMENT && opl == 7.0f;
  };
  const float zero[3] = {0.0f, -0.0f, 0.0f}, nan[3] = {1.0f, std::nanf(""), 0.0f};
  CHECK(refused(9, kAxis, 0));                      // max_bounces = 9
  CHECK(refused(4, zero, 0) && refused(4, nan, 0) && refused(4, nullptr, 0));
  CHECK(refused(4, kAxis, BZR_PIPELINE_STAGED));    // no staged form
  BezierLens lens(1.3f, bezier);
  Ray ray(Vertex{0.0f, 0.0f, 0.0f}, Vector{1, 0, 0}), out = ray;
  RefractionResult st = RefractionResult::cNone;
  float w = 7.0f;
  bool threw = false;
  try {
    bzr::traceChainBidir({&lens}, {1.3f, 1.5f, 1.8f, 2.4f}, {}, {0.5f, 0.5f, 0.5f}, {}, &ray, nullptr, nullptr, nullptr, 1,
                         4, 1, 2, kAxis, &out, &w, &st, &opl);
  } catch (std::invalid_argument const &) {
    threw = true;
  }
  CHECK(threw && opl == 7.0f && w == 7.0f);
  // the draw
  const uint64_t seeds[3] = {0, 2024, ~0ull}, rays[6] = {0, 1, 0xFFFFFFFFull, 1ull << 32, (1ull << 40) + 5, ~0ull};
  for (uint64_t seed : seeds)
    for (uint64_t j : rays)
      for (uint32_t q = 0; q <= 153; ++q) {
        float u = -1.0f;
        CHECK(bzr_bidir_uniform(seed, j, q, &u) == BZR_OK);
        CHECK(same_bits(u, draw(seed, j, q)) && u >= 0.0f && u < 1.0f);
      }
  float keep = 7.0f;
  CHECK(bzr_bidir_uniform(1, 2, 154, &keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_bidir_uniform(1, 2, 0, nullptr) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(keep == 7.0f);
  std::printf("bidir (host): ABI %d, signatures as declared, the draw is the header's recipe\n", BZR_ABI_VERSION);
}

struct Result {
  std::vector<Ray> out;
  std::vector<RefractionResult> st;
  std::vector<uint32_t> seg, bnc;
  std::vector<float> w, p, glass;
};
static bool same(Result const &a, Result const &b) {
  for (std::size_t i = 0; i < a.out.size(); ++i) {
    if (std::memcmp(a.out[i].mStart.data(), b.out[i].mStart.data(), 12) != 0 ||
        std::memcmp(a.out[i].mDirection.data(), b.out[i].mDirection.data(), 12) != 0)
      return false;
    if (a.st[i] != b.st[i] || a.seg[i] != b.seg[i] || a.bnc[i] != b.bnc[i] || !same_bits(a.w[i], b.w[i]) ||
        !same_bits(a.p[i], b.p[i]) || !same_bits(a.glass[i], b.glass[i]))
      return false;
  }
  return true;
}

static void gpu_part(BezierMesh const &bezier) {
  const std::vector<float> table = {1.3f, 1.5f, 1.8f, 2.4f};
  const std::vector<float> gaps = {1.0f, 1.333f, 1.41f, 1.0f, 1.0f, 1.333f, 1.0f, 1.56f};  // in front, behind
  const std::vector<float> glass_abs = {0.0f, 0.05f, 0.7f, 200.0f}, gap_abs = {0.0f, 0.02f, 0.3f, 0.0f};
  const uint64_t seed = 2024, first = (1ull << 40) + 5;
  BezierLens unread(7.0f, bezier);  // the lens's own index is not read
  std::vector<Ray> rays = cfg2_rays(64);
  const std::size_t n = rays.size();
  std::vector<uint8_t> channel(n);
  std::vector<float> w0(n), p0(n);
  for (std::size_t i = 0; i < n; ++i) {
    channel[i] = static_cast<uint8_t>((i * 7u + i / 64u) % 4u);
    w0[i] = 0.25f + 0.5f * static_cast<float>(i % 7u) / 7.0f;
    p0[i] = 3.0f * static_cast<float>(i % 11u) / 11.0f;
  }
  auto fresh = [&] {
    Result r{std::vector<Ray>(n, rays[0]), std::vector<RefractionResult>(n), std::vector<uint32_t>(n),
             std::vector<uint32_t>(n), w0, p0, std::vector<float>(n, -1.0f)};
    return r;
  };
  auto bidir = [&](uint32_t budget, uint64_t s, bool absorbing = true) {
    Result r = fresh();  // weights and path in place
    const std::vector<float> none;
    bzr::traceChainBidir({&unread}, table, gaps, absorbing ? glass_abs : none, absorbing ? gap_abs : none, rays.data(),
                         channel.data(), r.w.data(), r.p.data(), n, budget, s, first, kAxis, r.out.data(), r.w.data(),
                         r.st.data(), r.p.data(), r.glass.data(), r.seg.data(), r.bnc.data());
    return r;
  };
  auto absorb = [&](uint32_t budget) {
    Result r = fresh();
    bzr::traceChainAbsorb({&unread}, table, gaps, glass_abs, gap_abs, rays.data(), channel.data(), r.w.data(), r.p.data(),
                          n, budget, r.out.data(), r.w.data(), r.st.data(), r.p.data(), r.glass.data(), r.seg.data(),
                          r.bnc.data());
    return r;
  };
  const RefractionResult cBack = static_cast<RefractionResult>(BZR_RR_BACK);
  // budget 0: no draw, traceChainAbsorb bit for bit on every ray that did not leave backward
  {
    const Result z = bidir(0, seed), plain = absorb(0);
    int backward = 0;
    for (std::size_t i = 0; i < n; ++i) {
      if (z.st[i] == cBack) {
        ++backward;
        continue;
      }
      CHECK(std::memcmp(z.out[i].mStart.data(), plain.out[i].mStart.data(), 12) == 0 &&
            std::memcmp(z.out[i].mDirection.data(), plain.out[i].mDirection.data(), 12) == 0);
      CHECK(z.st[i] == plain.st[i] && z.seg[i] == plain.seg[i] && z.bnc[i] == 0 && plain.bnc[i] == 0);
      CHECK(same_bits(z.w[i], plain.w[i]) && same_bits(z.p[i], plain.p[i]) && same_bits(z.glass[i], plain.glass[i]));
    }
    CHECK(backward * 100 < static_cast<int>(n));
  }
  // budget 4: deterministic, seeded, rays come back, and more reflections than total reflection alone
  const Result a = bidir(4, seed), b = bidir(4, seed), c = bidir(4, seed + 1), plain = absorb(4);
  CHECK(same(a, b));
  CHECK(!same(a, c));
  int ghosts = 0, plain_bounced = 0, exits = 0, backs = 0;
  for (std::size_t i = 0; i < n; ++i) {
    ghosts += a.bnc[i] > 0;
    plain_bounced += plain.bnc[i] > 0;
    exits += a.st[i] == RefractionResult::cOutside;
    backs += a.st[i] == cBack;
    CHECK(a.st[i] == RefractionResult::cNone || a.st[i] == RefractionResult::cOutside || a.st[i] == cBack);
    CHECK(a.seg[i] <= 5u * 3u && a.bnc[i] <= 4u);
    if (a.bnc[i] == 0) CHECK(plain.bnc[i] == 0 && plain.w[i] <= a.w[i] && same_bits(a.p[i], plain.p[i]));
  }
  CHECK(exits > 2000 && backs >= 100 && ghosts >= plain_bounced + 100);
  // without absorption a ray that ends with budget left kept its whole weight
  {
    const Result clear = bidir(4, seed, false);
    int kept = 0;
    for (std::size_t i = 0; i < n; ++i) {
      if (clear.bnc[i] < 4u) {
        CHECK(same_bits(clear.w[i], w0[i]));
        ++kept;
      } else {
        CHECK(clear.w[i] <= w0[i]);
      }
    }
    CHECK(kept > 3000);
  }
  // the C ABI on the same context and mesh, [n][6] records
  bzr::Context &ctx = bzr::defaultContext();
  const bzr_mesh *mesh = unread.getMesh().device(ctx);
  std::vector<float> rec(6 * n), orec(6 * n), ow(n), op(n), og(n);
  for (std::size_t i = 0; i < n; ++i) {
    std::memcpy(&rec[6 * i], rays[i].mStart.data(), 12);
    std::memcpy(&rec[6 * i + 3], rays[i].mDirection.data(), 12);
  }
  std::vector<uint32_t> ost(n), oseg(n), obnc(n);
  CHECK(bzr_trace_chain_bidir(ctx.get(), &mesh, table.data(), gaps.data(), glass_abs.data(), gap_abs.data(), 1, 4,
                              rec.data(), channel.data(), w0.data(), p0.data(), static_cast<uint32_t>(n), 4, seed, first,
                              kAxis, orec.data(), ow.data(), ost.data(), oseg.data(), obnc.data(), op.data(), og.data(),
                              BZR_HOST_PTRS | BZR_RAYS_AOS) == BZR_OK);
  for (std::size_t i = 0; i < n; ++i) {
    CHECK(std::memcmp(a.out[i].mStart.data(), &orec[6 * i], 12) == 0 &&
          std::memcmp(a.out[i].mDirection.data(), &orec[6 * i + 3], 12) == 0);
    CHECK(static_cast<uint32_t>(a.st[i]) == ost[i] && a.seg[i] == oseg[i] && a.bnc[i] == obnc[i] && same_bits(a.w[i], ow[i]));
    CHECK(same_bits(a.p[i], op[i]) && same_bits(a.glass[i], og[i]));
  }
  std::printf("hot path: traceChainBidir, %d exits and %d back of %zu rays, %d reflected against %d without the roulette\n",
              exits, backs, n, ghosts, plain_bounced);
}

int main() {
  Mesh mesh;
  mesh.makeEllipsoid(32, 16, Vector(1.0f, 4.0f, 2.0f));
  mesh += Vector{10.0f, 0.0f, 0.0f};
  mesh.standardizeVertices();
  mesh.standardizeNormals();
  BezierMesh bezier(mesh);
  host_part(bezier);
  int32_t devices = 0;
  bzr_device_count(&devices);
  if (devices > 0) gpu_part(bezier);
  else std::printf("no HIP device: hot-path part skipped\n");
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
