// Total internal reflection through the C++ drop-in: bzr::traceChainTir against the C ABI's bzr_trace_chain_tir.
//   CPU part: the header's BZR_MAX_BOUNCES and the ABI version.
//   GPU part (when a HIP device is visible): traceChainTir over cfg2's rays at 64 x 64 with four channels (indices
//             1.3, 1.5, 1.8, 2.4) and up to four reflections against bzr_trace_chain_tir called directly on the same
//             context and device mesh -- rays, weights, status, segments and bounces bit for bit -- and against
//             traceChainSpectral, which must differ on the reflected rays; a budget above the maximum throws.
#include <cstdio>
#include <cstring>
#include <stdexcept>
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

static void host_part() {
  CHECK(BZR_MAX_BOUNCES == 8);
  CHECK(BZR_ABI_VERSION == 2 && bzr_abi_version() == 2);
  std::printf("tir (host): BZR_MAX_BOUNCES = %d\n", BZR_MAX_BOUNCES);
}

static void gpu_part(BezierMesh const &bezier) {
  const std::vector<float> table = {1.3f, 1.5f, 1.8f, 2.4f};
  const uint32_t max_bounces = 4;
  BezierLens unread(7.0f, bezier);  // the lens's own index is not read
  std::vector<Ray> rays = cfg2_rays(64);
  const std::size_t n = rays.size();
  std::vector<uint8_t> channel(n);
  std::vector<float> w0(n);
  for (std::size_t i = 0; i < n; ++i) {
    channel[i] = static_cast<uint8_t>((i * 7u + i / 64u) % 4u);
    w0[i] = 0.25f + 0.5f * static_cast<float>(i % 7u) / 7.0f;
  }
  std::vector<Ray> out(n, rays[0]);
  std::vector<RefractionResult> st(n);
  std::vector<uint32_t> seg(n), bnc(n);
  std::vector<float> w = w0;
  bzr::traceChainTir({&unread}, table, rays.data(), channel.data(), w.data(), n, max_bounces, out.data(), w.data(),
                     st.data(), seg.data(), bnc.data());  // weights in place

  // the C ABI on the same context and mesh, [n][6] records
  bzr::Context &ctx = bzr::defaultContext();
  const bzr_mesh *mesh = unread.getMesh().device(ctx);
  std::vector<float> rec(6 * n), orec(6 * n), ow(n);
  for (std::size_t i = 0; i < n; ++i) {
    std::memcpy(&rec[6 * i], rays[i].mStart.data(), 12);
    std::memcpy(&rec[6 * i + 3], rays[i].mDirection.data(), 12);
  }
  std::vector<uint32_t> ost(n), oseg(n), obnc(n);
  CHECK(bzr_trace_chain_tir(ctx.get(), &mesh, table.data(), 1, 4, rec.data(), channel.data(), w0.data(),
                            static_cast<uint32_t>(n), max_bounces, orec.data(), ow.data(), ost.data(), oseg.data(),
                            obnc.data(), BZR_HOST_PTRS | BZR_RAYS_AOS) == BZR_OK);
  int exits = 0, bounced = 0, bounced_exits = 0;
  for (std::size_t i = 0; i < n; ++i) {
    CHECK(std::memcmp(out[i].mStart.data(), &orec[6 * i], 12) == 0 &&
          std::memcmp(out[i].mDirection.data(), &orec[6 * i + 3], 12) == 0);
    CHECK(static_cast<uint32_t>(st[i]) == ost[i] && seg[i] == oseg[i] && bnc[i] == obnc[i] && same_bits(w[i], ow[i]));
    exits += st[i] == RefractionResult::cOutside;
    bounced += bnc[i] > 0;
    bounced_exits += bnc[i] > 0 && st[i] == RefractionResult::cOutside;
    CHECK(bnc[i] <= max_bounces && seg[i] <= 2 + max_bounces && seg[i] >= 1);
  }
  CHECK(exits > 2000);
  CHECK(bounced > 500 && bounced_exits > 300);

  // without reflections the reflected rays end NONE
  std::vector<Ray> sout(n, rays[0]);
  std::vector<RefractionResult> sst(n);
  std::vector<float> sw(n);
  bzr::traceChainSpectral({&unread}, table, rays.data(), channel.data(), w0.data(), n, sout.data(), sw.data(), sst.data());
  int gained = 0;
  for (std::size_t i = 0; i < n; ++i) {
    if (bnc[i] > 0) CHECK(sst[i] == RefractionResult::cNone);
    else CHECK(sst[i] == st[i] && same_bits(sw[i], w[i]));
    gained += sst[i] == RefractionResult::cNone && st[i] == RefractionResult::cOutside;
  }
  CHECK(gained == bounced_exits);

  bool threw = false;
  try {
    bzr::traceChainTir({&unread}, table, rays.data(), channel.data(), nullptr, n, BZR_MAX_BOUNCES + 1, out.data(), w.data(),
                       st.data());
  } catch (std::runtime_error const &) {
    threw = true;
  }
  CHECK(threw);
  std::printf("hot path: traceChainTir, %d exits of %zu rays, %d reflected, %d of them exit\n", exits, n, bounced,
              bounced_exits);
}

int main() {
  Mesh mesh;
  mesh.makeEllipsoid(32, 16, Vector(1.0f, 4.0f, 2.0f));
  mesh += Vector{10.0f, 0.0f, 0.0f};
  mesh.standardizeVertices();
  mesh.standardizeNormals();
  BezierMesh bezier(mesh);
  host_part();
  int32_t devices = 0;
  bzr_device_count(&devices);
  if (devices > 0) gpu_part(bezier);
  else std::printf("no HIP device: hot-path part skipped\n");
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
