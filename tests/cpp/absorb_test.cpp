// Beer-Lambert absorption through the C++ drop-in: bzr::traceChainAbsorb against the C ABI's bzr_trace_chain_absorb.
//   CPU part: the signature of both entry points, the table size checks, bzr_debug_attenuation on the host and
//             bzr_absorption_from_transmittance.
//   GPU part (when a HIP device is visible): traceChainAbsorb over cfg2's rays at 64 x 64 with four channels, media on
//             both sides, absorbing glass and an absorbing medium in front, up to four reflections, weights and path in
//             place, against bzr_trace_chain_absorb called directly on the same context and device mesh -- all seven
//             outputs bit for bit; empty absorption tables are traceChainMedia's result, and the tables change only the
//             weights.
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
                            const float *, uint32_t, uint32_t, float *, float *, uint32_t *, uint32_t *, uint32_t *,
                            float *, float *, uint32_t);
using Cpp = void (*)(std::vector<BezierLens const *> const &, std::vector<float> const &, std::vector<float> const &,
                     std::vector<float> const &, std::vector<float> const &, Ray const *, uint8_t const *, float const *,
                     float const *, std::size_t, uint32_t, Ray *, float *, RefractionResult *, float *, float *,
                     uint32_t *, uint32_t *, bzr::Context *);

static void host_part(BezierMesh const &bezier) {
  CHECK(BZR_ABI_VERSION == 2 && bzr_abi_version() == 2);
  static_assert(std::is_same<decltype(&bzr_trace_chain_absorb), CAbi>::value, "bzr_trace_chain_absorb's signature");
  static_assert(std::is_same<decltype(&bzr::traceChainAbsorb), Cpp>::value, "bzr::traceChainAbsorb's signature");
  float opl = 7.0f;
  CHECK(bzr_trace_chain_absorb(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr,
                               nullptr, 1, 4, nullptr, nullptr, nullptr, nullptr, nullptr, &opl,
                               nullptr, 0) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(opl == 7.0f);
  // tables that are neither empty nor [lenses][nchan] are refused before any context is needed
  BezierLens lens(1.3f, bezier);
  Ray ray(Vertex{0.0f, 0.0f, 0.0f}, Vector{1, 0, 0}), out = ray;
  RefractionResult st = RefractionResult::cNone;
  float w = 7.0f;
  for (int which = 0; which < 2; ++which)
    for (std::size_t bad : {std::size_t(1), std::size_t(3), std::size_t(8)}) {
      bool threw = false;
      const std::vector<float> t(bad, 0.5f), none;
      try {
        bzr::traceChainAbsorb({&lens}, {1.3f, 1.5f, 1.8f, 2.4f}, {}, which ? none : t, which ? t : none, &ray, nullptr,
                              nullptr, nullptr, 1, 4, &out, &w, &st, &opl);
      } catch (std::invalid_argument const &) {
        threw = true;
      }
      CHECK(threw);
    }
  CHECK(opl == 7.0f && w == 7.0f);
  // the Beer-Lambert term on the host: 1 at 0, 0 from the cut-off, within 2^-23 (1 + y) of exp(-x) in between
  const float x[6] = {0.0f, 1e-3f, 0.5f, 3.0f, 40.0f, 90.0f};
  float a[6];
  CHECK(bzr_debug_attenuation(nullptr, x, 6, a) == 0);
  CHECK(a[0] == 1.0f && a[5] == 0.0f);
  for (int k = 1; k < 5; ++k) {
    const double want = std::exp(-static_cast<double>(x[k]));
    CHECK(std::fabs(a[k] - want) <= want * std::ldexp(1.0, -23) * (1.0 + x[k] * 1.4426950408889634));
  }
  // a = -ln(T) / d
  const double T[3] = {1.0, 0.98, 0.5};
  float coef[3] = {7.0f, 7.0f, 7.0f};
  CHECK(bzr_absorption_from_transmittance(T, 3, 25.0, coef) == BZR_OK);
  CHECK(coef[0] == 0.0f && coef[1] == static_cast<float>(-std::log(0.98) / 25.0) &&
        coef[2] == static_cast<float>(-std::log(0.5) / 25.0));
  const double bad_t[3] = {0.9, 0.0, 0.5};
  float keep[3] = {7.0f, 7.0f, 7.0f};
  CHECK(bzr_absorption_from_transmittance(bad_t, 3, 25.0, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_absorption_from_transmittance(T, 3, 0.0, keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(keep[0] == 7.0f && keep[1] == 7.0f && keep[2] == 7.0f);
  std::printf("absorb (host): ABI %d, signatures as declared, table sizes checked\n", BZR_ABI_VERSION);
}

static void gpu_part(BezierMesh const &bezier) {
  const std::vector<float> table = {1.3f, 1.5f, 1.8f, 2.4f};
  const std::vector<float> gaps = {1.0f, 1.333f, 1.41f, 1.0f, 1.0f, 1.333f, 1.0f, 1.56f};  // in front, behind
  const std::vector<float> glass_abs = {0.0f, 0.05f, 0.7f, 200.0f}, gap_abs = {0.0f, 0.02f, 0.3f, 0.0f};
  const uint32_t max_bounces = 4;
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
  std::vector<Ray> out(n, rays[0]);
  std::vector<RefractionResult> st(n);
  std::vector<uint32_t> seg(n), bnc(n);
  std::vector<float> w = w0, p = p0, glass(n, -1.0f);
  bzr::traceChainAbsorb({&unread}, table, gaps, glass_abs, gap_abs, rays.data(), channel.data(), w.data(), p.data(), n,
                        max_bounces, out.data(), w.data(), st.data(), p.data(), glass.data(), seg.data(),
                        bnc.data());  // weights and path in place

  // the C ABI on the same context and mesh, [n][6] records
  bzr::Context &ctx = bzr::defaultContext();
  const bzr_mesh *mesh = unread.getMesh().device(ctx);
  std::vector<float> rec(6 * n), orec(6 * n), ow(n), op(n), og(n);
  for (std::size_t i = 0; i < n; ++i) {
    std::memcpy(&rec[6 * i], rays[i].mStart.data(), 12);
    std::memcpy(&rec[6 * i + 3], rays[i].mDirection.data(), 12);
  }
  std::vector<uint32_t> ost(n), oseg(n), obnc(n);
  CHECK(bzr_trace_chain_absorb(ctx.get(), &mesh, table.data(), gaps.data(), glass_abs.data(), gap_abs.data(), 1, 4,
                               rec.data(), channel.data(), w0.data(), p0.data(), static_cast<uint32_t>(n), max_bounces,
                               orec.data(), ow.data(), ost.data(), oseg.data(), obnc.data(), op.data(), og.data(),
                               BZR_HOST_PTRS | BZR_RAYS_AOS) == BZR_OK);
  int exits = 0, bounced = 0, dark = 0;
  for (std::size_t i = 0; i < n; ++i) {
    CHECK(std::memcmp(out[i].mStart.data(), &orec[6 * i], 12) == 0 &&
          std::memcmp(out[i].mDirection.data(), &orec[6 * i + 3], 12) == 0);
    CHECK(static_cast<uint32_t>(st[i]) == ost[i] && seg[i] == oseg[i] && bnc[i] == obnc[i] && same_bits(w[i], ow[i]));
    CHECK(same_bits(p[i], op[i]) && same_bits(glass[i], og[i]));
    CHECK(w[i] >= 0.0f && w[i] <= w0[i]);
    exits += st[i] == RefractionResult::cOutside;
    bounced += bnc[i] > 0;
    dark += w[i] == 0.0f && st[i] == RefractionResult::cOutside;
  }
  CHECK(exits > 2000 && bounced > 200 && dark > 100);

  // empty absorption tables: traceChainMedia's result; the tables above change the weights and nothing else
  std::vector<Ray> mout(n, rays[0]), zout(n, rays[0]);
  std::vector<RefractionResult> mst(n), zst(n);
  std::vector<uint32_t> mseg(n), mbnc(n), zseg(n), zbnc(n);
  std::vector<float> mw(n), mp(n), mg(n), zw(n), zp(n), zg(n);
  bzr::traceChainMedia({&unread}, table, gaps, rays.data(), channel.data(), w0.data(), p0.data(), n, max_bounces,
                       mout.data(), mw.data(), mst.data(), mp.data(), mg.data(), mseg.data(), mbnc.data());
  bzr::traceChainAbsorb({&unread}, table, gaps, {}, {}, rays.data(), channel.data(), w0.data(), p0.data(), n, max_bounces,
                        zout.data(), zw.data(), zst.data(), zp.data(), zg.data(), zseg.data(), zbnc.data());
  int lighter = 0;
  for (std::size_t i = 0; i < n; ++i) {
    CHECK(std::memcmp(zout[i].mStart.data(), mout[i].mStart.data(), 12) == 0 &&
          std::memcmp(zout[i].mDirection.data(), mout[i].mDirection.data(), 12) == 0);
    CHECK(zst[i] == mst[i] && zseg[i] == mseg[i] && zbnc[i] == mbnc[i] && same_bits(zw[i], mw[i]));
    CHECK(same_bits(zp[i], mp[i]) && same_bits(zg[i], mg[i]));
    CHECK(std::memcmp(out[i].mStart.data(), mout[i].mStart.data(), 12) == 0 &&
          std::memcmp(out[i].mDirection.data(), mout[i].mDirection.data(), 12) == 0);
    CHECK(st[i] == mst[i] && seg[i] == mseg[i] && bnc[i] == mbnc[i] && same_bits(p[i], mp[i]) && same_bits(glass[i], mg[i]));
    lighter += !same_bits(w[i], mw[i]);
  }
  CHECK(lighter > 1000);
  std::printf("hot path: traceChainAbsorb, %d exits of %zu rays, %d reflected, %d left with weight 0\n", exits, n, bounced,
              dark);
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
