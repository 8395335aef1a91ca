// Spectral channels through the C++ drop-in: bzr_dispersion_index on the host and bzr::traceChainSpectral on the GPU.
//   CPU part: bzr_dispersion_index (N-BK7's Sellmeier formula at the d line) against the formula in double, and its
//             argument checks.
//   GPU part (when a HIP device is visible): traceChainSpectral with two channels against two traceChainPower calls,
//             one per channel's rays through a lens of that channel's index -- rays, weights, status and segments bit
//             for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
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

static void host_part() {
  const double bk7[6] = {1.03961212, 0.00600069867, 0.231792344, 0.0200179144, 1.01046945, 103.560653};
  const double lambda = 0.5875618, l2 = lambda * lambda;
  double n2 = 1.0;
  for (int k = 0; k < 6; k += 2) n2 += bk7[k] * l2 / (l2 - bk7[k + 1]);
  float ri = -1.0f;
  CHECK(bzr_dispersion_index(BZR_DISPERSION_SELLMEIER, bk7, 6, &lambda, 1, &ri) == BZR_OK);
  CHECK(same_bits(ri, static_cast<float>(std::sqrt(n2))));
  CHECK(std::fabs(ri - 1.51680f) < 5e-5f);
  float keep = 7.0f;
  CHECK(bzr_dispersion_index(2, bk7, 6, &lambda, 1, &keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_dispersion_index(BZR_DISPERSION_CAUCHY, bk7, 4, &lambda, 1, &keep) == BZR_ERR_INVALID_ARGUMENT);
  CHECK(same_bits(keep, 7.0f));
  std::printf("dispersion (host): N-BK7 n_d = %.6f\n", ri);
}

static void gpu_part(BezierMesh const &bezier) {
  const float index[2] = {1.29f, 1.312f};
  BezierLens lens0(index[0], bezier), lens1(index[1], bezier), unread(7.0f, bezier);
  std::vector<Ray> rays = cfg2_rays(64);
  const std::size_t n = rays.size();
  std::vector<uint8_t> channel(n);
  std::vector<float> w0(n);
  for (std::size_t i = 0; i < n; ++i) {
    channel[i] = static_cast<uint8_t>((i * 7u + i / 64u) % 2u);
    w0[i] = 0.25f + 0.5f * static_cast<float>(i % 7u) / 7.0f;
  }
  std::vector<Ray> out(n, rays[0]);
  std::vector<RefractionResult> st(n);
  std::vector<uint32_t> seg(n);
  std::vector<float> w = w0;
  bzr::traceChainSpectral({&unread}, {index[0], index[1]}, rays.data(), channel.data(), w.data(), n, out.data(), w.data(),
                          st.data(), seg.data());  // weights in place; the lens's own index (7) is not read
  int exits = 0, differ = 0;
  for (uint32_t c = 0; c < 2u; ++c) {
    std::vector<Ray> mine, want;
    std::vector<float> wm;
    std::vector<std::size_t> at;
    for (std::size_t i = 0; i < n; ++i)
      if (channel[i] == c) {
        mine.push_back(rays[i]);
        wm.push_back(w0[i]);
        at.push_back(i);
      }
    want.assign(mine.size(), rays[0]);
    std::vector<RefractionResult> ws(mine.size());
    std::vector<uint32_t> wg(mine.size());
    std::vector<float> ww(mine.size()), other(mine.size());
    bzr::traceChainPower({c == 0 ? &lens0 : &lens1}, mine.data(), wm.data(), mine.size(), want.data(), ww.data(), ws.data(),
                         wg.data());
    std::vector<Ray> oo(mine.size(), rays[0]);
    std::vector<RefractionResult> os(mine.size());
    bzr::traceChainPower({c == 0 ? &lens1 : &lens0}, mine.data(), wm.data(), mine.size(), oo.data(), other.data(), os.data());
    for (std::size_t k = 0; k < at.size(); ++k) {
      const std::size_t i = at[k];
      CHECK(same_ray(out[i], want[k]) && st[i] == ws[k] && seg[i] == wg[k]);
      CHECK(same_bits(w[i], ww[k]));
      exits += st[i] == RefractionResult::cOutside;
      differ += !same_ray(want[k], oo[k]);
    }
  }
  CHECK(exits > 2000);
  CHECK(differ > 1000);  // the other channel's index would have given other rays
  std::printf("hot path: traceChainSpectral, %d exits of %zu rays, %d depend on the channel\n", exits, n, differ);
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
