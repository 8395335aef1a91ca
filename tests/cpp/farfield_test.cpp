// Far-field maps through the C++ drop-in: bzr::farfieldBin against bzr_farfield_cell per ray.
//   CPU part: the signatures, the frame checks of bzr_farfield_cell / bzr_farfield_bin / bzr::farfieldBin without a device,
//             the pole's and the centres' cells, bzr_farfield_directions' round trip and bzr_farfield_intensity.
//   GPU part (when a HIP device is visible): farfieldBin over 5 000 directions in three channels with weights and
//             statuses, against a map accumulated on the host from bzr_farfield_cell and q(w) -- flux, counts and the
//             two rows, word for word.
#include <cmath>
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

using CAbi = bzr_status (*)(bzr_ctx *, const bzr_farfield *, const float *, const float *, const uint32_t *, const uint8_t *,
                            uint32_t, uint32_t, uint64_t *, uint32_t *, uint64_t *, uint64_t *, uint32_t);
using Cpp = void (*)(bzr_farfield const &, Ray const *, float const *, RefractionResult const *, uint8_t const *,
                     std::size_t, uint32_t, uint64_t *, uint32_t *, uint64_t *, uint64_t *, bzr::Context *);

static bzr_farfield frame(float extent, uint32_t bu, uint32_t bv) {
  bzr_farfield f{};
  const float u[3] = {0.36f, 0.48f, 0.8f}, v[3] = {0.8f, -0.6f, 0.0f};  // unit, orthogonal, tilted
  std::memcpy(f.axis_u, u, 12);
  std::memcpy(f.axis_v, v, 12);
  f.extent = extent;
  f.bins_u = bu;
  f.bins_v = bv;
  return f;
}

static void host_part() {
  CHECK(BZR_ABI_VERSION == 2 && bzr_abi_version() == 2);
  static_assert(std::is_same<decltype(&bzr_farfield_bin), CAbi>::value, "bzr_farfield_bin's signature");
  static_assert(std::is_same<decltype(&bzr::farfieldBin), Cpp>::value, "bzr::farfieldBin's signature");
  static_assert(sizeof(bzr_farfield) == 36 && BZR_FAR_SEEN == 0 && BZR_FAR_BINNED == 1, "bzr_farfield");
  const bzr_farfield far = frame(1.41421354f, 24, 40);
  std::vector<double> dir(24 * 40 * 3), polar(24 * 40), azimuth(24 * 40);
  CHECK(bzr_farfield_directions(&far, dir.data(), polar.data(), azimuth.data()) == BZR_OK);
  int round_trip = 0;
  for (int c = 0; c < 24 * 40; ++c) {
    const float d[3] = {static_cast<float>(dir[3 * c]), static_cast<float>(dir[3 * c + 1]), static_cast<float>(dir[3 * c + 2])};
    int32_t cell = -2;
    CHECK(bzr_farfield_cell(&far, d, &cell) == BZR_OK);
    round_trip += cell == c;
  }
  CHECK(round_trip == 24 * 40);
  // the pole u x v = (0.48, 0.64, -0.6) lies at the map's centre: with 25 x 41 bins in the middle of cell (iv, iu) =
  // (20, 12); directions beyond its opposite are not binned
  const float pole[3] = {0.48f, 0.64f, -0.6f}, back[3] = {-0.96f, -1.28f, 1.2f}, nan3[3] = {NAN, 0.0f, 0.0f};
  const bzr_farfield odd = frame(1.41421354f, 25, 41);
  int32_t cell = -2;
  CHECK(bzr_farfield_cell(&odd, pole, &cell) == BZR_OK && cell == 20 * 25 + 12);
  CHECK(bzr_farfield_cell(&far, back, &cell) == BZR_OK && cell == -1);  // g = 1 + mu < 0
  CHECK(bzr_farfield_cell(&far, nan3, &cell) == BZR_OK && cell == -1);
  // refused frames, nothing written
  cell = 7;
  for (float extent : {0.0f, -1.0f, 1.5f, NAN, INFINITY}) {
    const bzr_farfield bad = frame(extent, 24, 40);
    CHECK(bzr_farfield_cell(&bad, pole, &cell) == BZR_ERR_INVALID_ARGUMENT && cell == 7);
  }
  const bzr_farfield no_bins = frame(1.0f, 0, 40);
  CHECK(bzr_farfield_cell(&no_bins, pole, &cell) == BZR_ERR_INVALID_ARGUMENT && cell == 7);
  CHECK(bzr_farfield_cell(nullptr, pole, &cell) == BZR_ERR_INVALID_ARGUMENT);
  uint64_t flux[4] = {7, 7, 7, 7};
  uint32_t hist[4] = {7, 7, 7, 7};
  float rays[6] = {0, 0, 0, 1, 0, 0};
  const bzr_farfield small = frame(1.0f, 2, 2);
  CHECK(bzr_farfield_bin(nullptr, &small, rays, nullptr, nullptr, nullptr, 1, 1, flux, hist, nullptr, nullptr, 0) ==
        BZR_ERR_INVALID_ARGUMENT);  // null context
  CHECK(bzr_farfield_bin(nullptr, &small, rays, nullptr, nullptr, nullptr, 0, 1, flux, hist, nullptr, nullptr, 0) == BZR_OK);
  CHECK(bzr_farfield_bin(nullptr, &small, rays, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, 0) ==
        BZR_ERR_INVALID_ARGUMENT);
  CHECK(bzr_farfield_bin(nullptr, &small, rays, nullptr, nullptr, nullptr, 1, 1, flux, hist, nullptr, nullptr,
                         BZR_RAYS_AOS) == BZR_ERR_INVALID_ARGUMENT);
  bool threw = false;
  try {
    const bzr_farfield bad = frame(1.5f, 2, 2);
    bzr::farfieldBin(bad, nullptr, nullptr, nullptr, nullptr, 0, 1, flux, hist);
  } catch (std::runtime_error const &) {
    threw = true;
  }
  CHECK(threw);
  uint64_t rows[2] = {7, 7};
  bzr::farfieldBin(small, nullptr, nullptr, nullptr, nullptr, 0, 1, flux, hist, rows);  // an empty batch needs no device
  CHECK(rows[0] == 0 && rows[1] == 0);
  for (int k = 0; k < 4; ++k) CHECK(flux[k] == 7 && hist[k] == 7);
  // intensity: flux / 2^32 / cell solid angle
  const uint64_t f4[4] = {1ull << 32, 0, 3ull << 31, 5};
  double out[4];
  CHECK(bzr_farfield_intensity(&small, f4, 1, 2.0, out) == BZR_OK);
  CHECK(out[0] == 2.0 && out[1] == 0.0 && out[2] == 3.0 && std::fabs(out[3] - 2.0 * 5 / 4294967296.0) < 1e-24);
  std::printf("farfield (host): ABI %d, signatures as declared, frames checked\n", BZR_ABI_VERSION);
}

static void gpu_part() {
  const bzr_farfield far = frame(1.25f, 24, 40);
  const uint32_t nchan = 3, cells = 24 * 40;
  const std::size_t n = 5000;
  std::vector<Ray> rays;
  std::vector<float> w(n);
  std::vector<RefractionResult> st(n);
  std::vector<uint8_t> ch(n);
  uint64_t s = 12345;
  auto next = [&s] {  // a small generator: uniform in [-1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<float>(static_cast<double>(s >> 11) / 9007199254740992.0 * 2.0 - 1.0);
  };
  for (std::size_t i = 0; i < n; ++i) {
    rays.emplace_back(Vertex{next(), next(), next()}, Vector{next(), next(), next() + 1e-3f});  // the ctor normalises
    w[i] = i % 13 == 0 ? 0.0f : i % 17 == 0 ? 1.0f : 0.5f * (next() + 1.0f);
    st[i] = i % 5 == 0 ? RefractionResult::cNone : i % 7 == 0 ? RefractionResult::cInside : RefractionResult::cOutside;
    ch[i] = static_cast<uint8_t>((i * 7u + i / 64u) % 4u);  // channel 3 is out of range
  }
  std::vector<uint64_t> flux(nchan * cells, 3), want_flux(nchan * cells, 3), rows(2 * nchan), power(2 * nchan);
  std::vector<uint32_t> hist(nchan * cells, 1), want_hist(nchan * cells, 1);
  std::vector<uint64_t> want_rows(2 * nchan, 0), want_power(2 * nchan, 0);
  bzr::farfieldBin(far, rays.data(), w.data(), st.data(), ch.data(), n, nchan, flux.data(), hist.data(), rows.data(),
                   power.data());
  int binned = 0;
  for (std::size_t i = 0; i < n; ++i) {
    if (st[i] != RefractionResult::cOutside || ch[i] >= nchan) continue;
    const uint64_t q = w[i] > 0.0f ? static_cast<uint64_t>(w[i] * 4294967296.0f) : 0;
    int32_t cell = -2;
    CHECK(bzr_farfield_cell(&far, rays[i].mDirection.data(), &cell) == BZR_OK);
    want_rows[2 * ch[i] + BZR_FAR_SEEN] += 1;
    want_power[2 * ch[i] + BZR_FAR_SEEN] += q;
    if (cell < 0) continue;
    ++binned;
    want_rows[2 * ch[i] + BZR_FAR_BINNED] += 1;
    want_power[2 * ch[i] + BZR_FAR_BINNED] += q;
    want_flux[ch[i] * cells + cell] += q;
    want_hist[ch[i] * cells + cell] += 1;
  }
  CHECK(binned > 1000 && binned < 2800);
  CHECK(flux == want_flux && hist == want_hist && rows == want_rows && power == want_power);
  std::printf("hot path: farfieldBin, %d of %zu rays binned\n", binned, n);
}

int main() {
  host_part();
  int32_t devices = 0;
  bzr_device_count(&devices);
  if (devices > 0) gpu_part();
  else std::printf("no HIP device: hot-path part skipped\n");
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
