// Ray power through the drop-in classes: BezierLens::refractPower on the host and bzr::traceChainPower on the GPU.
//   CPU part: refractPower returns BezierLens::refract's ray and status bit for bit, and its T is bzr_debug_fresnel
//             of the hit's own values (eta = 1 / ri entering, ri leaving; cos = the hit's mCosIncidence).
//   GPU part (when a HIP device is visible): traceChainPower's rays, status and segments are traceChain's, and each
//             weight is the product, in chain order, of the host path's T for that ray -- bit for bit.
#include <cstdio>
#include <cstring>
#include <tuple>
#include <vector>

#include "bezierLens.h"
#include "bezierMesh.h"
#include "mesh.h"
#include "bzr_debug.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) {                                                           \
      ++g_fail;                                                              \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                        \
  } while (0)

static bool same_ray(Ray const &a, Ray const &b) {
  return std::memcmp(a.mStart.data(), b.mStart.data(), 12) == 0 && std::memcmp(a.mDirection.data(), b.mDirection.data(), 12) == 0;
}
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// cfg2's primary rays: plane x = 0, y in [-4.2, 4.2], z in [-2.1, 2.1], along +x
static std::vector<Ray> cfg2_rays(int side) {
  std::vector<Ray> rays;
  for (int i = 0; i < side; ++i)
    for (int j = 0; j < side; ++j)
      rays.emplace_back(Vertex{0.0f, -4.2f + 8.4f * (j + 0.5f) / side, -2.1f + 4.2f * (i + 0.5f) / side}, Vector{1, 0, 0});
  return rays;
}

// The host chain of one ray through one lens: final ray, status, segments and the weight w0 x T x T.
struct HostChain {
  Ray ray;
  RefractionResult status;
  uint32_t segments;
  float weight;
};
static HostChain host_chain(BezierLens const &lens, Ray const &ray, float w0) {
  HostChain c{ray, RefractionResult::cNone, 0u, w0};
  for (uint32_t j = 0; j < 2u; ++j) {
    auto res = lens.refractPower(c.ray, j == 0 ? RefractionResult::cInside : RefractionResult::cOutside);
    ++c.segments;
    c.status = std::get<1>(res);
    if (c.status == RefractionResult::cNone) break;
    c.ray = std::get<0>(res);
    c.weight = c.weight * std::get<2>(res);
  }
  return c;
}

static void host_part(BezierMesh const &bezier, BezierLens const &lens) {
  const float ri = lens.getRefractiveIndex();
  std::vector<Ray> rays = cfg2_rays(24);
  int refracted = 0, exits = 0;
  for (Ray const &primary : rays) {
    Ray cur = primary;
    for (uint32_t j = 0; j < 2u; ++j) {
      const RefractionResult expect = j == 0 ? RefractionResult::cInside : RefractionResult::cOutside;
      const auto plain = lens.refract(cur, expect);
      const auto power = lens.refractPower(cur, expect);
      CHECK(same_ray(std::get<0>(power), plain.first));
      CHECK(std::get<1>(power) == plain.second);
      if (plain.second == RefractionResult::cNone) {
        CHECK(same_bits(std::get<2>(power), 1.0f));
        break;
      }
      const BezierIntersection hit = bezier.intersect(cur);
      const float eta = j == 0 ? 1.0f / ri : ri, cs = hit.mIntersection.mCosIncidence;
      float want = -1.0f;
      CHECK(bzr_debug_fresnel(&eta, &cs, 1u, &want) == 0);
      CHECK(same_bits(std::get<2>(power), want));
      CHECK(want > 0.0f && want <= 1.0f);
      ++refracted;
      exits += j == 1u;
      cur = plain.first;
    }
  }
  CHECK(refracted > 250 && exits > 100);
  std::printf("refractPower (host): %d refractions, %d exits of %zu rays\n", refracted, exits, rays.size());
}

static void gpu_part(BezierLens const &lens) {
  std::vector<Ray> rays = cfg2_rays(64);
  const std::size_t n = rays.size();
  std::vector<Ray> out(n, rays[0]), plain(n, rays[0]);
  std::vector<RefractionResult> st(n), pst(n);
  std::vector<uint32_t> seg(n), pseg(n);
  std::vector<float> w(n, -1.0f), w2(n);
  bzr::traceChain({&lens}, rays.data(), n, plain.data(), pst.data(), pseg.data());
  bzr::traceChainPower({&lens}, rays.data(), nullptr, n, out.data(), w.data(), st.data(), seg.data());
  for (std::size_t i = 0; i < n; ++i) w2[i] = 0.25f + 0.5f * static_cast<float>(i % 7u) / 7.0f;
  const std::vector<float> w0 = w2;
  std::vector<Ray> out2(n, rays[0]);
  std::vector<RefractionResult> st2(n);
  bzr::traceChainPower({&lens}, rays.data(), w2.data(), n, out2.data(), w2.data(), st2.data());  // weights in place
  int exits = 0;
  for (std::size_t i = 0; i < n; ++i) {
    CHECK(same_ray(out[i], plain[i]) && st[i] == pst[i] && seg[i] == pseg[i]);
    CHECK(same_ray(out2[i], plain[i]) && st2[i] == pst[i]);
    const HostChain a = host_chain(lens, rays[i], 1.0f), b = host_chain(lens, rays[i], w0[i]);
    CHECK(same_ray(a.ray, out[i]) && a.status == st[i] && a.segments == seg[i]);
    CHECK(same_bits(a.weight, w[i]));
    CHECK(same_bits(b.weight, w2[i]));
    exits += st[i] == RefractionResult::cOutside;
  }
  CHECK(exits > 2000);
  std::printf("hot path: traceChainPower, %d exits of %zu rays\n", exits, n);
}

int main() {
  Mesh mesh;
  mesh.makeEllipsoid(32, 16, Vector(1.0f, 4.0f, 2.0f));
  mesh += Vector{10.0f, 0.0f, 0.0f};
  mesh.standardizeVertices();
  mesh.standardizeNormals();
  BezierMesh bezier(mesh);
  BezierLens lens(1.3f, bezier);
  host_part(bezier, lens);
  int32_t devices = 0;
  bzr_device_count(&devices);
  if (devices > 0) gpu_part(lens);
  else std::printf("no HIP device: hot-path part skipped\n");
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
