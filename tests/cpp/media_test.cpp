// Surrounding media through the C++ drop-in: bzr::traceChainMedia against the C ABI's bzr_trace_chain_media.
//   CPU part: the header's constants, the signature of both entry points and the gapTable size check.
//   GPU part (when a HIP device is visible): traceChainMedia over cfg2's rays at 64 x 64 with four channels (indices
//             1.3, 1.5, 1.8, 2.4; water, a gel and vacuum in front, water, vacuum and cement behind), up to four
//             reflections and a path passed in place, against bzr_trace_chain_media called directly on the same
//             context and device mesh -- rays, weights, status, segments, bounces, opl and glass bit for bit; an empty
//             gapTable is traceChainOpl's result, and the media change it; a null outOpl throws.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "bezierLens.h"
#include "bezierMesh.h"
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

using CAbi = bzr_status (*)(bzr_ctx *, const bzr_mesh *const *, const float *, const float *, uint32_t, uint32_t,
                            const float *, const uint8_t *, const float *, const float *, uint32_t, uint32_t, float *,
                            float *, uint32_t *, uint32_t *, uint32_t *, float *, float *, uint32_t);
using Cpp = void (*)(std::vector<BezierLens const *> const &, std::vector<float> const &, std::vector<float> const &,
                     Ray const *, uint8_t const *, float const *, float const *, std::size_t, uint32_t, Ray *, float *,
                     RefractionResult *, float *, float *, uint32_t *, uint32_t *, bzr::Context *);

static void host_part(BezierMesh const &bezier) {
  CHECK(BZR_MAX_BOUNCES == 8);
  CHECK(BZR_ABI_VERSION == 2 && bzr_abi_version() == 2);
  static_assert(std::is_same<decltype(&bzr_trace_chain_media), CAbi>::value, "bzr_trace_chain_media's signature");
  static_assert(std::is_same<decltype(&bzr::traceChainMedia), Cpp>::value, "bzr::traceChainMedia's signature");
  float opl = 7.0f;
  CHECK(bzr_trace_chain_media(nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, 1, 4, nullptr,
                              nullptr, nullptr, nullptr, nullptr, &opl, nullptr, 0) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(opl == 7.0f);
  // a gapTable that is neither empty nor [lenses + 1][nchan] is refused before any context is needed
  BezierLens lens(1.3f, bezier);
  Ray ray(Vertex{0.0f, 0.0f, 0.0f}, Vector{1, 0, 0}), out = ray;
  RefractionResult st = RefractionResult::cNone;
  float w = 7.0f;
  for (std::size_t bad : {std::size_t(1), std::size_t(4), std::size_t(7), std::size_t(12)}) {
    bool threw = false;
    try {
      bzr::traceChainMedia({&lens}, {1.3f, 1.5f, 1.8f, 2.4f}, std::vector<float>(bad, 1.0f), &ray, nullptr, nullptr,
                           nullptr, 1, 4, &out, &w, &st, &opl);
    } catch (std::invalid_argument const &) {
      threw = true;
    }
    CHECK(threw);
  }
  CHECK(opl == 7.0f && w == 7.0f);
  std::printf("media (host): ABI %d, signatures as declared, gapTable sizes checked\n", BZR_ABI_VERSION);
}

static void gpu_part(BezierMesh const &bezier) {
  const std::vector<float> table = {1.3f, 1.5f, 1.8f, 2.4f};
  const std::vector<float> gaps = {1.0f, 1.333f, 1.41f, 1.0f, 1.0f, 1.333f, 1.0f, 1.56f};  // in front, behind
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
  bzr::traceChainMedia({&unread}, table, gaps, rays.data(), channel.data(), w.data(), p.data(), n, max_bounces,
                       out.data(), w.data(), st.data(), p.data(), glass.data(), seg.data(),
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
  CHECK(bzr_trace_chain_media(ctx.get(), &mesh, table.data(), gaps.data(), 1, 4, rec.data(), channel.data(), w0.data(),
                              p0.data(), static_cast<uint32_t>(n), max_bounces, orec.data(), ow.data(), ost.data(),
                              oseg.data(), obnc.data(), op.data(), og.data(), BZR_HOST_PTRS | BZR_RAYS_AOS) == BZR_OK);
  int exits = 0, bounced = 0, with_glass = 0, moved = 0;
  for (std::size_t i = 0; i < n; ++i) {
    CHECK(std::memcmp(out[i].mStart.data(), &orec[6 * i], 12) == 0 &&
          std::memcmp(out[i].mDirection.data(), &orec[6 * i + 3], 12) == 0);
    CHECK(static_cast<uint32_t>(st[i]) == ost[i] && seg[i] == oseg[i] && bnc[i] == obnc[i] && same_bits(w[i], ow[i]));
    CHECK(same_bits(p[i], op[i]) && same_bits(glass[i], og[i]));
    CHECK(p[i] >= p0[i] && glass[i] >= 0.0f);
    exits += st[i] == RefractionResult::cOutside;
    bounced += bnc[i] > 0;
    with_glass += glass[i] > 0.0f;
    moved += !same_bits(p[i], p0[i]);
  }
  CHECK(exits > 2000 && bounced > 200);
  CHECK(with_glass > 2700 && moved >= with_glass);

  // an empty gapTable is vacuum: traceChainOpl's result, which the media above change
  std::vector<Ray> tout(n, rays[0]), vout(n, rays[0]);
  std::vector<RefractionResult> tst(n), vst(n);
  std::vector<uint32_t> tseg(n), tbnc(n), vseg(n), vbnc(n);
  std::vector<float> tw(n), tp(n), tg(n), vw(n), vp(n), vg(n);
  bzr::traceChainOpl({&unread}, table, rays.data(), channel.data(), w0.data(), p0.data(), n, max_bounces, tout.data(),
                     tw.data(), tst.data(), tp.data(), tg.data(), tseg.data(), tbnc.data());
  bzr::traceChainMedia({&unread}, table, {}, rays.data(), channel.data(), w0.data(), p0.data(), n, max_bounces,
                       vout.data(), vw.data(), vst.data(), vp.data(), vg.data(), vseg.data(), vbnc.data());
  int unlike = 0;
  for (std::size_t i = 0; i < n; ++i) {
    CHECK(std::memcmp(vout[i].mStart.data(), tout[i].mStart.data(), 12) == 0 &&
          std::memcmp(vout[i].mDirection.data(), tout[i].mDirection.data(), 12) == 0);
    CHECK(vst[i] == tst[i] && vseg[i] == tseg[i] && vbnc[i] == tbnc[i] && same_bits(vw[i], tw[i]));
    CHECK(same_bits(vp[i], tp[i]) && same_bits(vg[i], tg[i]));
    unlike += !same_bits(p[i], tp[i]) || st[i] != tst[i];
  }
  CHECK(unlike > 1000);

  // without a glass row: the same path
  std::vector<float> p2(n);
  bzr::traceChainMedia({&unread}, table, gaps, rays.data(), channel.data(), w0.data(), p0.data(), n, max_bounces,
                       out.data(), w.data(), st.data(), p2.data());
  for (std::size_t i = 0; i < n; ++i) CHECK(same_bits(p2[i], op[i]));

  bool threw = false;
  try {
    bzr::traceChainMedia({&unread}, table, gaps, rays.data(), channel.data(), nullptr, nullptr, n, max_bounces,
                         out.data(), w.data(), st.data(), nullptr);
  } catch (std::runtime_error const &) {
    threw = true;
  }
  CHECK(threw);
  std::printf("hot path: traceChainMedia, %d exits of %zu rays, %d reflected, %d with a glass path\n", exits, n, bounced,
              with_glass);
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
