// Surface coatings through the C++ drop-in: bzr::traceChainCoated against bzr::traceChainBidir and the C ABI.
//   CPU part: the signature of both entry points, the refusals that need no context (the walk's own, and a coating
//             whose mask names a surface beyond 2 nlens, has no table or holds an entry outside [0, 1] in a masked row),
//             a table of the wrong size, and the two host functions: bzr_coat_transmittance against the header's lookup
//             restated in plain float, bzr_coating_reflectance against the closed forms at normal incidence, and their
//             refusals.
//   GPU part (when a HIP device is visible): traceChainCoated over cfg2's rays at 64 x 64 with four channels, media,
//             absorption, weights and path in place: with mask 0 (a table given, and none) traceChainBidir's seven
//             outputs bit for bit at budgets 0 and 4; with both faces coated by rows of zeros no ray reflects by a draw
//             and fewer rays reflect than on bare glass; with the back face a mirror at budget 1 every cOutside ray has
//             weight 0 and rays come BACK; the C ABI called directly gives the drop-in's bits.
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
                            const float *, uint32_t, uint32_t, uint64_t, uint64_t, const float *, const bzr_coating *,
                            float *, float *, uint32_t *, uint32_t *, uint32_t *, float *, float *, uint32_t);
using Cpp = void (*)(std::vector<BezierLens const *> const &, std::vector<float> const &, std::vector<float> const &,
                     std::vector<float> const &, std::vector<float> const &, Ray const *, uint8_t const *, float const *,
                     float const *, std::size_t, uint32_t, uint64_t, uint64_t, float const (&)[3],
                     std::vector<float> const &, uint32_t, Ray *, float *, RefractionResult *, float *, float *, uint32_t *,
                     uint32_t *, bzr::Context *);

// include/bzr.h's lookup, restated (this file is built with -ffp-contract=off)
static float lookup(const float *row, float mu) {
  mu = mu < 1.0f ? mu : 1.0f;
  const float x = mu * 128.0f;
  int i = static_cast<int>(x);
  i = i < 127 ? i : 127;
  const float f = x - static_cast<float>(i);
  const float d = row[i + 1] - row[i];
  const float p = f * d;
  const float r = row[i] + p;
  return 1.0f - r;
}
static const float kAxis[3] = {1.0f, 0.0f, 0.0f};

static void host_part(BezierMesh const &bezier) {
  CHECK(BZR_ABI_VERSION == 2 && bzr_abi_version() == 2 && BZR_COAT_SAMPLES == 129);
  static_assert(std::is_same<decltype(&bzr_trace_chain_coated), CAbi>::value, "bzr_trace_chain_coated's signature");
  static_assert(std::is_same<decltype(&bzr::traceChainCoated), Cpp>::value, "bzr::traceChainCoated's signature");
  static_assert(sizeof(bzr_coating) == 16 && offsetof(bzr_coating, mask) == 8, "bzr_coating's layout");
  float opl = 7.0f;
  std::vector<float> rows(2 * BZR_COAT_SAMPLES, 0.25f);
  auto refused = [&](uint32_t budget, const float *axis, uint32_t flags, const bzr_coating *coat) {
    return bzr_trace_chain_coated(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr,
                                  nullptr, 1, budget, 0, 0, axis, coat, nullptr, nullptr, nullptr, nullptr, nullptr, &opl,
                                  nullptr, flags) == BZR_ERR_INVALID_ARGUMENT && opl == 7.0f;
  };
  const float zero[3] = {0.0f, -0.0f, 0.0f};
  const bzr_coating good{rows.data(), 3u};
  CHECK(refused(9, kAxis, 0, &good) && refused(4, zero, 0, &good) && refused(4, nullptr, 0, &good));
  CHECK(refused(4, kAxis, BZR_PIPELINE_STAGED, &good) && refused(4, kAxis, BZR_PIPELINE_STAGED, nullptr));
  const bzr_coating beyond{rows.data(), 4u}, no_table{nullptr, 1u};
  CHECK(refused(4, kAxis, 0, &beyond) && std::strstr(bzr_last_error(), "mask"));
  CHECK(refused(4, kAxis, 0, &no_table) && std::strstr(bzr_last_error(), "table"));
  const float bad_values[5] = {std::nanf(""), INFINITY, -INFINITY, -1e-6f, 1.0f + 0x1p-23f};
  for (float v : bad_values) {
    std::vector<float> bad = rows;
    bad[BZR_COAT_SAMPLES + 128] = v;  // the last entry of surface 1's row
    const bzr_coating masked{bad.data(), 2u}, unmasked{bad.data(), 1u};
    CHECK(refused(4, kAxis, 0, &masked) && std::strstr(bzr_last_error(), "[0, 1]"));
    // an unmasked row is not validated: the call gets as far as the null context
    CHECK(refused(4, kAxis, 0, &unmasked) && std::strstr(bzr_last_error(), "context"));
  }
  BezierLens lens(1.3f, bezier);
  Ray ray(Vertex{0.0f, 0.0f, 0.0f}, Vector{1, 0, 0}), out = ray;
  RefractionResult st = RefractionResult::cNone;
  float w = 7.0f;
  bool threw = false;
  try {  // a coating table of another size
    bzr::traceChainCoated({&lens}, {1.3f, 1.5f}, {}, {}, {}, &ray, nullptr, nullptr, nullptr, 1, 4, 1, 2, kAxis,
                          std::vector<float>(2 * BZR_COAT_SAMPLES, 0.0f), 3, &out, &w, &st, &opl);
  } catch (std::invalid_argument const &) {
    threw = true;
  }
  CHECK(threw && opl == 7.0f && w == 7.0f);
  // the lookup
  std::vector<float> row(BZR_COAT_SAMPLES);
  uint32_t lcg = 12345u;
  for (float &v : row) {
    lcg = lcg * 1664525u + 1013904223u;
    v = static_cast<float>(lcg >> 8) / 16777216.0f;
  }
  row[5] = 0.0f, row[6] = 1.0f;
  for (int k = 0; k <= 128 * 64; ++k) {
    const float mu = static_cast<float>(k) / (128.0f * 64.0f) + (k % 3 == 1 ? 0x1p-20f : 0.0f);
    float t = -1.0f;
    CHECK(bzr_coat_transmittance(row.data(), mu, &t) == BZR_OK);
    CHECK(same_bits(t, lookup(row.data(), mu)) && t >= 0.0f && t <= 1.0f);
  }
  float t = 7.0f;
  CHECK(bzr_coat_transmittance(row.data(), 1.0f + 0x1p-23f, &t) == BZR_OK && same_bits(t, 1.0f - row[128]));
  t = 7.0f;
  CHECK(bzr_coat_transmittance(nullptr, 0.5f, &t) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coat_transmittance(row.data(), 0.5f, nullptr) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coat_transmittance(row.data(), std::nanf(""), &t) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coat_transmittance(row.data(), -0.25f, &t) == BZR_ERR_INVALID_ARGUMENT && t == 7.0f);
  // the rows: closed forms at normal incidence
  const double n = 1.5168, nc = 1.38, qw = 0.55 / (4.0 * 1.38);
  float r[BZR_COAT_SAMPLES];
  CHECK(bzr_coating_reflectance(1.0, n, nullptr, nullptr, 0, 0.55, r) == BZR_OK);
  CHECK(r[0] == 1.0f && std::fabs(r[128] - std::pow((n - 1) / (n + 1), 2)) < 1e-8);
  CHECK(bzr_coating_reflectance(1.0, n, &nc, &qw, 1, 0.55, r) == BZR_OK);
  CHECK(r[0] == 1.0f && std::fabs(r[128] - std::pow((n - nc * nc) / (n + nc * nc), 2)) < 1e-8);
  for (int i = 0; i < BZR_COAT_SAMPLES; ++i) CHECK(r[i] >= 0.0f && r[i] <= 1.0f);
  float keep[BZR_COAT_SAMPLES];
  for (float &v : keep) v = 7.0f;
  const double nine[9] = {1.38, 1.38, 1.38, 1.38, 1.38, 1.38, 1.38, 1.38, 1.38}, neg = -1.0, inf = INFINITY;
  CHECK(bzr_coating_reflectance(1.0, n, nine, nine, 9, 0.55, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coating_reflectance(0.0, n, &nc, &qw, 1, 0.55, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coating_reflectance(1.0, inf, &nc, &qw, 1, 0.55, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coating_reflectance(1.0, n, &neg, &qw, 1, 0.55, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coating_reflectance(1.0, n, &nc, &neg, 1, 0.55, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coating_reflectance(1.0, n, &nc, &qw, 1, 0.0, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coating_reflectance(1.0, n, nullptr, &qw, 1, 0.55, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_coating_reflectance(1.0, n, &nc, &qw, 1, 0.55, nullptr) == BZR_ERR_INVALID_ARGUMENT);
  for (float v : keep) CHECK(v == 7.0f);
  std::printf("coat (host): ABI %d, signatures as declared, the lookup is the header's, the rows meet the closed forms\n",
              BZR_ABI_VERSION);
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
  auto coated = [&](uint32_t budget, std::vector<float> const &rows, uint32_t mask) {
    Result r = fresh();  // weights and path in place
    bzr::traceChainCoated({&unread}, table, gaps, glass_abs, gap_abs, rays.data(), channel.data(), r.w.data(), r.p.data(),
                          n, budget, seed, first, kAxis, rows, mask, r.out.data(), r.w.data(), r.st.data(), r.p.data(),
                          r.glass.data(), r.seg.data(), r.bnc.data());
    return r;
  };
  auto bidir = [&](uint32_t budget) {
    Result r = fresh();
    bzr::traceChainBidir({&unread}, table, gaps, glass_abs, gap_abs, rays.data(), channel.data(), r.w.data(), r.p.data(),
                         n, budget, seed, first, kAxis, r.out.data(), r.w.data(), r.st.data(), r.p.data(),
                         r.glass.data(), r.seg.data(), r.bnc.data());
    return r;
  };
  const std::size_t cells = 2 * 4 * BZR_COAT_SAMPLES;
  const std::vector<float> none, zeros(cells, 0.0f), junk(cells, std::nanf(""));
  std::vector<float> mirror(cells, 0.0f);
  for (std::size_t k = cells / 2; k < cells; ++k) mirror[k] = 1.0f;  // surface 1, the back face
  const RefractionResult cBack = static_cast<RefractionResult>(BZR_RR_BACK);
  // mask 0: traceChainBidir bit for bit, with no table and with one that holds NaN
  int bare_bounced = 0;
  for (uint32_t budget : {0u, 4u}) {
    const Result want = bidir(budget);
    CHECK(same(coated(budget, none, 0), want));
    CHECK(same(coated(budget, junk, 0), want));
    if (budget == 4)
      for (std::size_t i = 0; i < n; ++i) bare_bounced += want.bnc[i] > 0;
  }
  // a perfect anti-reflection coating on both faces: what still reflects does so by total reflection
  const Result ar = coated(4, zeros, 3);
  int ar_bounced = 0, exits = 0;
  for (std::size_t i = 0; i < n; ++i) {
    ar_bounced += ar.bnc[i] > 0;
    exits += ar.st[i] == RefractionResult::cOutside;
  }
  CHECK(exits > 2000 && ar_bounced + 100 <= bare_bounced);
  // the back face a mirror, budget 1
  const Result m = coated(1, mirror, 2);
  int backs = 0;
  for (std::size_t i = 0; i < n; ++i) {
    if (m.st[i] == RefractionResult::cOutside) CHECK(m.w[i] == 0.0f);
    backs += m.st[i] == cBack && m.bnc[i] == 1;
  }
  CHECK(backs >= 1000);
  // the C ABI on the same context and mesh, [n][6] records
  bzr::Context &ctx = bzr::defaultContext();
  const bzr_mesh *mesh = unread.getMesh().device(ctx);
  std::vector<float> rec(6 * n), orec(6 * n), ow(n), op(n), og(n);
  for (std::size_t i = 0; i < n; ++i) {
    std::memcpy(&rec[6 * i], rays[i].mStart.data(), 12);
    std::memcpy(&rec[6 * i + 3], rays[i].mDirection.data(), 12);
  }
  std::vector<uint32_t> ost(n), oseg(n), obnc(n);
  const bzr_coating coat{mirror.data(), 2u};
  CHECK(bzr_trace_chain_coated(ctx.get(), &mesh, table.data(), gaps.data(), glass_abs.data(), gap_abs.data(), 1, 4,
                               rec.data(), channel.data(), w0.data(), p0.data(), static_cast<uint32_t>(n), 1, seed, first,
                               kAxis, &coat, orec.data(), ow.data(), ost.data(), oseg.data(), obnc.data(), op.data(),
                               og.data(), BZR_HOST_PTRS | BZR_RAYS_AOS) == BZR_OK);
  for (std::size_t i = 0; i < n; ++i) {
    CHECK(std::memcmp(m.out[i].mStart.data(), &orec[6 * i], 12) == 0 &&
          std::memcmp(m.out[i].mDirection.data(), &orec[6 * i + 3], 12) == 0);
    CHECK(static_cast<uint32_t>(m.st[i]) == ost[i] && m.seg[i] == oseg[i] && m.bnc[i] == obnc[i] && same_bits(m.w[i], ow[i]));
    CHECK(same_bits(m.p[i], op[i]) && same_bits(m.glass[i], og[i]));
  }
  std::printf("hot path: traceChainCoated, mask 0 is traceChainBidir; %d rays reflect on bare glass, %d under a perfect "
              "coating; %d of %zu come back from the mirror\n", bare_bounced, ar_bounced, backs, n);
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
