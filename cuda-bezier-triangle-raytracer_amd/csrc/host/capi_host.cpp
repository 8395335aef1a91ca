// capi_host.cpp -- C ABI over the host preprocessing (Mesh, BezierMesh construction).
// Every entry point catches what the drop-in classes throw (the reference throws
// char const* and std::out_of_range, reference/mesh.cpp:204, bezierMesh.cpp:17-18)
// and reports it as a status code + bzr_last_error() text.
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "bzr/bzr.hpp"
#include "single_ray.hpp"

extern "C" void bzr_internal_set_error(const char *msg);

struct bzr_trimesh {
  Mesh mesh;
};

namespace {
template <typename F>
bzr_status guarded(F &&f) {
  try {
    f();
    return BZR_OK;
  } catch (char const *what) {
    bzr_internal_set_error(what);
    return BZR_ERR_PREPROCESS;
  } catch (std::bad_alloc const &) {
    bzr_internal_set_error("out of memory");
    return BZR_ERR_OUT_OF_MEMORY;
  } catch (std::out_of_range const &e) {
    bzr_internal_set_error((std::string("std::out_of_range: ") + e.what()).c_str());
    return BZR_ERR_PREPROCESS;
  } catch (std::exception const &e) {
    bzr_internal_set_error(e.what());
    return BZR_ERR_PREPROCESS;
  }
}
bzr_status bad(const char *msg) {
  bzr_internal_set_error(msg);
  return BZR_ERR_INVALID_ARGUMENT;
}
}  // namespace

extern "C" {

bzr_status bzr_trimesh_create(bzr_trimesh **out) {
  if (!out) return bad("null out");
  *out = new (std::nothrow) bzr_trimesh();
  return *out ? BZR_OK : BZR_ERR_OUT_OF_MEMORY;
}

bzr_status bzr_trimesh_destroy(bzr_trimesh *m) {
  delete m;
  return BZR_OK;
}

bzr_status bzr_trimesh_copy(const bzr_trimesh *src, bzr_trimesh **out) {
  if (!src || !out) return bad("null argument");
  return guarded([&] { *out = new bzr_trimesh(*src); });
}

bzr_status bzr_trimesh_size(const bzr_trimesh *m, uint32_t *n) {
  if (!m || !n) return bad("null argument");
  *n = static_cast<uint32_t>(m->mesh.size());
  return BZR_OK;
}

bzr_status bzr_trimesh_get(const bzr_trimesh *m, float *xyz) {
  if (!m || (!xyz && m->mesh.size())) return bad("null argument");
  for (uint32_t f = 0; f < m->mesh.size(); ++f)
    for (uint32_t k = 0; k < 3; ++k) std::memcpy(xyz + 9 * f + 3 * k, m->mesh[f][k].data(), 12);
  return BZR_OK;
}

bzr_status bzr_trimesh_set(bzr_trimesh *m, const float *xyz, uint32_t n) {
  if (!m || (!xyz && n)) return bad("null argument");
  return guarded([&] {
    Mesh fresh;
    fresh.reserve(n);
    for (uint32_t f = 0; f < n; ++f) {
      Triangle t;
      for (uint32_t k = 0; k < 3; ++k) t[k] = Vertex(xyz[9 * f + 3 * k], xyz[9 * f + 3 * k + 1], xyz[9 * f + 3 * k + 2]);
      fresh.push_back(t);
    }
    m->mesh = std::move(fresh);
  });
}

bzr_status bzr_trimesh_make_solid_of_revolution(bzr_trimesh *m, int32_t sectors, int32_t belts, int32_t envelope,
                                                float sx, float sy, float sz) {
  if (!m) return bad("null mesh");
  if (sectors < 1 || belts < 1) return bad("sectors and belts must be positive");
  std::function<float(float)> env;
  if (envelope == BZR_ENVELOPE_ELLIPSOID) {
    env = [](float x) { return std::sqrt(1 - x * x); };  // reference/mesh.h:99
  } else if (envelope == BZR_ENVELOPE_TESTLENS) {
    env = [](float x) {  // reference/test.cpp:242-245, 336-339
      float x2 = x * x;
      return std::sqrt(1.0f - x2) + 0.7f * (std::exp(-4.0f) - std::exp(-4.0f * x2));
    };
  } else {
    return bad("unknown envelope");
  }
  return guarded([&] { m->mesh.makeSolidOfRevolution(sectors, belts, env, Vector(sx, sy, sz)); });
}

bzr_status bzr_trimesh_make_ellipsoid(bzr_trimesh *m, int32_t sectors, int32_t belts, float sx, float sy, float sz) {
  if (!m) return bad("null mesh");
  if (sectors < 1 || belts < 1) return bad("sectors and belts must be positive");
  return guarded([&] { m->mesh.makeEllipsoid(sectors, belts, Vector(sx, sy, sz)); });
}

bzr_status bzr_trimesh_read_stl(bzr_trimesh *m, const char *path) {
  if (!m || !path) return bad("null argument");
  return guarded([&] { m->mesh.readMesh(path); });
}

bzr_status bzr_trimesh_write_stl(const bzr_trimesh *m, const char *path) {
  if (!m || !path) return bad("null argument");
  return guarded([&] { m->mesh.writeMesh(path); });
}

bzr_status bzr_trimesh_transform(bzr_trimesh *m, const float t[9], const float d[3]) {
  if (!m || !t || !d) return bad("null argument");
  Transform tr;
  std::memcpy(tr.data(), t, 36);
  return guarded([&] { m->mesh.transform(tr, Vertex(d[0], d[1], d[2])); });
}

bzr_status bzr_trimesh_split(bzr_trimesh *m, int32_t divisor) {
  if (!m) return bad("null mesh");
  if (divisor < 1) return bad("divisor must be >= 1");
  return guarded([&] { m->mesh.splitTriangles(divisor); });
}

bzr_status bzr_trimesh_split_maxside(bzr_trimesh *m, float max_side) {
  if (!m) return bad("null mesh");
  if (!(max_side > 0.0f)) return bad("max_side must be > 0");
  return guarded([&] { m->mesh.splitTriangles(max_side); });
}

bzr_status bzr_trimesh_standardize_vertices(bzr_trimesh *m) {
  if (!m) return bad("null mesh");
  return guarded([&] { m->mesh.standardizeVertices(); });
}

bzr_status bzr_trimesh_standardize_normals(bzr_trimesh *m) {
  if (!m) return bad("null mesh");
  return guarded([&] { m->mesh.standardizeNormals(); });
}

bzr_status bzr_trimesh_neighbours(const bzr_trimesh *m, uint32_t *fellow, uint8_t *start) {
  if (!m || !fellow || !start) return bad("null argument");
  auto const &f2n = m->mesh.getFace2neighbours();
  if (f2n.size() != m->mesh.size()) return bad("mesh is not standardized");
  for (std::size_t f = 0; f < f2n.size(); ++f)
    for (int k = 0; k < 3; ++k) {
      fellow[3 * f + k] = f2n[f].mFellowTriangles[k];
      start[3 * f + k] = f2n[f].mFellowCommonSideStarts[k];
    }
  return BZR_OK;
}

bzr_status bzr_bezier_build(const bzr_trimesh *m, bzr_patch *out) {
  if (!m || (!out && m->mesh.size())) return bad("null argument");
  return guarded([&] {
    BezierMesh bm(m->mesh);
    if (bm.size()) std::memcpy(static_cast<void *>(out), &bm[0], sizeof(bzr_patch) * bm.size());
  });
}

bzr_status bzr_bezier_split_thick(const bzr_trimesh *m, bzr_trimesh *out) {
  if (!m || !out) return bad("null argument");
  return guarded([&] { out->mesh = BezierMesh(m->mesh).splitThickBezierTriangles(); });
}

bzr_status bzr_bezier_interpolate(const bzr_trimesh *m, int32_t divisor, bzr_trimesh *out) {
  if (!m || !out) return bad("null argument");
  if (divisor < 1) return bad("divisor must be >= 1");
  return guarded([&] { out->mesh = BezierMesh(m->mesh).interpolate(divisor); });
}

// include/bzr_debug.h
int32_t bzr_debug_newton_short(const void *patches, uint32_t n, uint32_t stride, const uint32_t *patch,
                               const float *rays, const uint8_t *limit, uint32_t m, float *full, float *skipped) {
  if ((!patches && n) || ((!patch || !rays || !limit || !full || !skipped) && m)) return bad("null argument");
  if (stride < sizeof(bzr_patch) || stride % 4u) return bad("stride");
  for (uint32_t i = 0; i < m; ++i)
    if (patch[i] >= n) return bad("patch index out of range");
  for (uint32_t i = 0; i < m; ++i) {
    const float *rec = reinterpret_cast<const float *>(static_cast<const char *>(patches) + (std::size_t)stride * patch[i]);
    const float ray[6] = {rays[i],
                          rays[(std::size_t)m + i],
                          rays[(std::size_t)2 * m + i],
                          rays[(std::size_t)3 * m + i],
                          rays[(std::size_t)4 * m + i],
                          rays[(std::size_t)5 * m + i]};
    bzr_host::newton_short_pair(rec, ray, limit[i] != 0, full + (std::size_t)12 * i, skipped + (std::size_t)12 * i);
  }
  return BZR_OK;
}

int32_t bzr_debug_fresnel(const float *eta, const float *cs, uint32_t n, float *t_out) {
  if ((!eta || !cs || !t_out) && n) return bad("null argument");
  bzr_host::fresnel_pairs(eta, cs, n, t_out);
  return BZR_OK;
}

// bzr_debug_attenuation's host half (trace.hip holds the entry point and its device half).
void bzr_internal_attenuation_host(const float *x, uint32_t n, float *out) { bzr_host::attenuation(x, n, out); }

// Every value is computed before the first is written: a rejected call leaves out_ri as it was.
bzr_status bzr_dispersion_index(int32_t model, const double *coeff, uint32_t ncoeff, const double *wavelength_um,
                                uint32_t n, float *out_ri) {
  if (model != BZR_DISPERSION_CAUCHY && model != BZR_DISPERSION_SELLMEIER) return bad("unknown dispersion model");
  if (model == BZR_DISPERSION_CAUCHY ? (ncoeff != 2 && ncoeff != 3) : (ncoeff != 2 && ncoeff != 4 && ncoeff != 6))
    return bad("ncoeff: 2 or 3 (Cauchy), 2, 4 or 6 (Sellmeier)");
  if (!coeff || ((!wavelength_um || !out_ri) && n)) return bad("null argument");
  std::vector<float> ri;
  try {
    ri.resize(n);
  } catch (std::bad_alloc const &) {
    bzr_internal_set_error("out of memory");
    return BZR_ERR_OUT_OF_MEMORY;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const double l = wavelength_um[i];
    if (!std::isfinite(l) || !(l > 0.0)) return bad("wavelength must be finite and positive");
    const double l2 = l * l;
    double v;
    if (model == BZR_DISPERSION_CAUCHY) {
      v = coeff[0] + coeff[1] / l2;
      if (ncoeff == 3) v += coeff[2] / (l2 * l2);
    } else {
      double n2 = 1.0;
      for (uint32_t k = 0; k < ncoeff; k += 2) n2 += coeff[k] * l2 / (l2 - coeff[k + 1]);
      if (!(n2 > 0.0)) return bad("Sellmeier n^2 is not positive");
      v = std::sqrt(n2);
    }
    ri[i] = static_cast<float>(v);
    if (!std::isfinite(v) || !std::isfinite(ri[i])) return bad("index is not finite");
  }
  if (n) std::memcpy(out_ri, ri.data(), (std::size_t)n * sizeof(float));
  return BZR_OK;
}

// As above: nothing is written unless every coefficient is good.
bzr_status bzr_absorption_from_transmittance(const double *internal_transmittance, uint32_t n, double thickness,
                                             float *out_a) {
  if (!std::isfinite(thickness) || !(thickness > 0.0)) return bad("thickness must be finite and positive");
  if ((!internal_transmittance || !out_a) && n) return bad("null argument");
  std::vector<float> a;
  try {
    a.resize(n);
  } catch (std::bad_alloc const &) {
    bzr_internal_set_error("out of memory");
    return BZR_ERR_OUT_OF_MEMORY;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const double t = internal_transmittance[i];
    if (!(t > 0.0) || !(t <= 1.0)) return bad("internal transmittance must be in (0, 1]");
    const double v = t == 1.0 ? 0.0 : -std::log(t) / thickness;
    a[i] = static_cast<float>(v);
    if (!std::isfinite(v) || !std::isfinite(a[i])) return bad("absorption coefficient is not finite");
  }
  if (n) std::memcpy(out_a, a.data(), (std::size_t)n * sizeof(float));
  return BZR_OK;
}

// ---- the Fresnel roulette's uniform (include/bzr.h bzr_trace_chain_ghost): the host twin of trace.hip ghost_uniform ----
static uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
bzr_status bzr_ghost_uniform(uint64_t seed, uint64_t ray, uint32_t lens, uint32_t reflections, float *u) {
  if (!u) return bad("null u");
  if (lens > 7u || reflections > BZR_MAX_BOUNCES) return bad("lens must be 0..7 and reflections 0..8");
  const uint64_t e = 16u * lens + reflections;
  const uint64_t r = mix64((seed ^ 0x5851F42D4C957F2Dull) + 0x9E3779B97F4A7C15ull * (ray + 1ull));
  const uint64_t h = mix64(r + 0x9E3779B97F4A7C15ull * (e + 1ull));
  *u = static_cast<float>(static_cast<uint32_t>(h >> 40)) * 0x1p-24f;
  return BZR_OK;
}

// The bidirectional walk's draw (include/bzr.h bzr_trace_chain_bidir): the same function at e = 256 + segment.
bzr_status bzr_bidir_uniform(uint64_t seed, uint64_t ray, uint32_t segment, float *u) {
  if (!u) return bad("null u");
  if (segment > (BZR_MAX_BOUNCES + 1u) * (2u * 8u + 1u)) return bad("segment must be 0..153");
  const uint64_t e = 256u + segment;
  const uint64_t r = mix64((seed ^ 0x5851F42D4C957F2Dull) + 0x9E3779B97F4A7C15ull * (ray + 1ull));
  const uint64_t h = mix64(r + 0x9E3779B97F4A7C15ull * (e + 1ull));
  *u = static_cast<float>(static_cast<uint32_t>(h >> 40)) * 0x1p-24f;
  return BZR_OK;
}

// ---- surface coatings (include/bzr.h bzr_coating) ----
// The lookup's host twin: patch_math_body.inc coat_t, the text the kernels compile.
bzr_status bzr_coat_transmittance(const float *row, float mu, float *t) {
  if (!row || !t) return bad("null argument");
  if (!(mu >= 0.0f)) return bad("mu must be >= 0");
  *t = bzr_host::coat_transmittance(row, mu);
  return BZR_OK;
}

// include/bzr_debug.h: the same lookup over n cosines
int32_t bzr_debug_coat_transmittance(const float *row, const float *mu, uint32_t n, float *out) {
  if ((!row || !mu || !out) && n) return bad("null argument");
  for (uint32_t i = 0; i < n; ++i)
    if (!(mu[i] >= 0.0f)) return bad("mu must be >= 0");
  for (uint32_t i = 0; i < n; ++i) out[i] = bzr_host::coat_transmittance(row, mu[i]);
  return BZR_OK;
}

// One row by the characteristic-matrix method in binary64.  Per polarisation a medium j has the admittance
// y_j = n_j cos_j (s) or n_j / cos_j (p), cos_j = sqrt(1 - (n_gap sin / n_j)^2) a complex root with a non-negative
// imaginary part (evanescent beyond the critical angle); a layer's matrix is [[cos d, -i sin d / y], [-i y sin d, cos d]]
// with d = 2 pi n_j t_j cos_j / lambda; (B, C) = M_1 ... M_k (1, y_glass), r = (y_gap B - C) / (y_gap B + C),
// R = |r|^2.  Every value is computed before the first is written.
namespace {
struct Cx {
  double re, im;
};
inline Cx operator+(Cx a, Cx b) { return {a.re + b.re, a.im + b.im}; }
inline Cx operator-(Cx a, Cx b) { return {a.re - b.re, a.im - b.im}; }
inline Cx operator*(Cx a, Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline Cx operator/(Cx a, Cx b) {
  const double z = b.re * b.re + b.im * b.im;
  return {(a.re * b.re + a.im * b.im) / z, (a.im * b.re - a.re * b.im) / z};
}
// sqrt of a real number: on the positive real or the positive imaginary axis
inline Cx root(double x) { return x >= 0.0 ? Cx{std::sqrt(x), 0.0} : Cx{0.0, std::sqrt(-x)}; }
// cos z and sin z, both divided by e^|Im z|: a layer's matrix may carry any common factor, (B, C) enter r only through
// their ratio, and the scaled pair stays of order 1 where cosh and sinh of a thick evanescent layer would overflow
inline void cx_cos_sin_scaled(Cx z, Cx &c, Cx &s) {
  const double e = std::exp(-2.0 * std::fabs(z.im));
  const double ch = 0.5 * (1.0 + e), sh = (z.im < 0.0 ? -0.5 : 0.5) * (1.0 - e);
  c = {std::cos(z.re) * ch, -std::sin(z.re) * sh};
  s = {std::sin(z.re) * ch, std::cos(z.re) * sh};
}
}  // namespace

bzr_status bzr_coating_reflectance(double n_gap, double n_glass, const double *layer_index,
                                   const double *layer_thickness_um, uint32_t nlayers, double wavelength_um,
                                   float *out_row) {
  constexpr uint32_t kMaxLayers = 8;
  if (!out_row) return bad("null out_row");
  if (nlayers > kMaxLayers) return bad("nlayers must be 0..8");
  if (nlayers && (!layer_index || !layer_thickness_um)) return bad("null layer arrays");
  if (!std::isfinite(n_gap) || !(n_gap > 0.0) || !std::isfinite(n_glass) || !(n_glass > 0.0))
    return bad("indices must be finite and positive");
  if (!std::isfinite(wavelength_um) || !(wavelength_um > 0.0)) return bad("wavelength must be finite and positive");
  for (uint32_t j = 0; j < nlayers; ++j) {
    if (!std::isfinite(layer_index[j]) || !(layer_index[j] > 0.0)) return bad("layer indices must be finite and positive");
    if (!std::isfinite(layer_thickness_um[j]) || !(layer_thickness_um[j] > 0.0))
      return bad("layer thicknesses must be finite and positive");
  }
  float row[BZR_COAT_SAMPLES];
  row[0] = 1.0f;  // (mu = 0: grazing, by definition)
  const double kTwoPi = 6.283185307179586476925286766559;
  for (uint32_t i = 1; i < BZR_COAT_SAMPLES; ++i) {
    const double mu = (double)i / 128.0;
    const double q = n_gap * n_gap * (1.0 - mu * mu);  // (n sin)^2, Snell's invariant
    const double cg2 = 1.0 - q / (n_glass * n_glass);
    if (!(cg2 > 0.0)) {  // the glass is at or beyond its critical angle: a lossless stack sends everything back
      row[i] = 1.0f;
      continue;
    }
    const Cx cg = root(cg2);
    double rsum = 0.0;
    for (int pol = 0; pol < 2; ++pol) {
      const Cx y0 = pol ? Cx{n_gap / mu, 0.0} : Cx{n_gap * mu, 0.0};
      const Cx ys = pol ? Cx{n_glass, 0.0} / cg : Cx{n_glass, 0.0} * cg;
      Cx b{1.0, 0.0}, c = ys;
      for (uint32_t k = nlayers; k-- > 0;) {  // from the glass outwards: (B, C) <- M_k (B, C)
        const double nj = layer_index[k];
        const Cx cj = root(1.0 - q / (nj * nj));
        const double kd = kTwoPi * nj * layer_thickness_um[k] / wavelength_um;
        const Cx mi{0.0, -1.0};
        Cx nb, nc;
        if (cj.re == 0.0 && cj.im == 0.0) {
          // the layer exactly at its critical angle: the matrix's limit for cos_j -> 0.  s (y = n cos_j):
          // sin(kd cos_j) / y -> kd / n and y sin -> 0, [[1, -i kd / n], [0, 1]]; p (y = n / cos_j): sin / y -> 0 and
          // y sin -> n kd, [[1, 0], [-i n kd, 1]]
          nb = b + mi * Cx{pol ? 0.0 : kd / nj, 0.0} * c;
          nc = mi * Cx{pol ? nj * kd : 0.0, 0.0} * b + c;
        } else {
          const Cx yj = pol ? Cx{nj, 0.0} / cj : Cx{nj, 0.0} * cj;
          Cx cd, sd;
          cx_cos_sin_scaled(Cx{kd, 0.0} * cj, cd, sd);
          nb = cd * b + (mi * sd / yj) * c;
          nc = (mi * yj * sd) * b + cd * c;
        }
        b = nb;
        c = nc;
      }
      const Cx r = (y0 * b - c) / (y0 * b + c);
      rsum += r.re * r.re + r.im * r.im;
    }
    double rr = 0.5 * rsum;
    if (!std::isfinite(rr)) return bad("reflectance is not finite");
    if (rr > 1.0) rr = 1.0;  // (an evanescent stack gives 1 up to rounding)
    row[i] = static_cast<float>(rr);
  }
  std::memcpy(out_row, row, sizeof row);
  return BZR_OK;
}

// ---- far field (include/bzr.h bzr_farfield) ----
// The frame's checks and what every user derives from it, stated once: the pole n = axis_u x axis_v normalised as
// illuminate() normalises the target's normal, S = R + R and the cell sizes.  out[13]: n, axis_u, axis_v, R, S, cu,
// cv, as the device's FarFrame holds them (trace.hip calls this too).  Returns NULL, or why the frame is refused.
const char *bzr_internal_farfield_frame(const bzr_farfield *far, uint32_t nchan, float out[13]) {
  if (!far) return "null far-field frame";
  if (!far->bins_u || !far->bins_v) return "far-field bins must be positive";
  if (!std::isfinite(far->extent) || !(far->extent > 0.0f) || !(far->extent <= 1.41421354f))
    return "far-field extent must be in (0, sqrt(2)]";
  if (nchan == 0 || nchan > BZR_MAX_CHANNELS) return "nchan must be 1..64";
  const uint64_t cells = (uint64_t)far->bins_u * far->bins_v;
  if (cells >= (1ull << 32) || cells * nchan >= (1ull << 32)) return "far-field maps of 2^32 cells or more";
  const float *au = far->axis_u, *av = far->axis_v;
  float n[3] = {au[1] * av[2] - au[2] * av[1], au[2] * av[0] - au[0] * av[2], au[0] * av[1] - au[1] * av[0]};
  const float z = n[0] * n[0] + (n[1] * n[1] + n[2] * n[2]);
  if (z > 0.0f) {
    const float s = std::sqrt(z);
    for (float &c : n) c = c / s;
  }
  for (int k = 0; k < 3; ++k) out[k] = n[k], out[3 + k] = au[k], out[6 + k] = av[k];
  const float S = far->extent + far->extent;
  out[9] = far->extent;
  out[10] = S;
  out[11] = S / (float)far->bins_u;
  out[12] = S / (float)far->bins_v;
  return nullptr;
}

namespace {
int64_t farfield_cell_host(const bzr_farfield &far, const float f[13], const float d[3]) {
  const float mu = d[0] * f[0] + (d[1] * f[1] + d[2] * f[2]);
  const float a = d[0] * f[3] + (d[1] * f[4] + d[2] * f[5]), b = d[0] * f[6] + (d[1] * f[7] + d[2] * f[8]);
  const float g = 1.0f + mu;
  const float h = 2.0f / g;
  const float k = std::sqrt(h);
  const float X = a * k, Y = b * k;
  const float u = X + f[9], v = Y + f[9];
  if (!(g > 0.0f && u >= 0.0f && u < f[10] && v >= 0.0f && v < f[10])) return -1;
  uint32_t iu = (uint32_t)(u / f[11]), iv = (uint32_t)(v / f[12]);
  if (iu >= far.bins_u) iu = far.bins_u - 1u;
  if (iv >= far.bins_v) iv = far.bins_v - 1u;
  return (int64_t)iv * far.bins_u + iu;
}
}  // namespace

bzr_status bzr_farfield_cell(const bzr_farfield *far, const float d[3], int32_t *cell) {
  float f[13];
  if (const char *why = bzr_internal_farfield_frame(far, 1, f)) return bad(why);
  if ((uint64_t)far->bins_u * far->bins_v >= (1ull << 31)) return bad("far-field map of 2^31 cells or more");
  if (!d || !cell) return bad("null argument");
  *cell = (int32_t)farfield_cell_host(*far, f, d);
  return BZR_OK;
}

// include/bzr_debug.h: bzr_farfield_cell over n directions [n][3] at once
int32_t bzr_debug_farfield_cells(const void *frame, const float *d_xyz, uint32_t n, int32_t *cell) {
  const bzr_farfield *far = static_cast<const bzr_farfield *>(frame);
  float f[13];
  if (const char *why = bzr_internal_farfield_frame(far, 1, f)) return bad(why);
  if ((uint64_t)far->bins_u * far->bins_v >= (1ull << 31)) return bad("far-field map of 2^31 cells or more");
  if ((!d_xyz || !cell) && n) return bad("null argument");
  for (uint32_t i = 0; i < n; ++i) cell[i] = (int32_t)farfield_cell_host(*far, f, d_xyz + (std::size_t)3 * i);
  return BZR_OK;
}

bzr_status bzr_farfield_directions(const bzr_farfield *far, double *dir_xyz, double *polar_rad, double *azimuth_rad) {
  float f[13];
  if (const char *why = bzr_internal_farfield_frame(far, 1, f)) return bad(why);
  const double R = far->extent;
  for (uint32_t iv = 0; iv < far->bins_v; ++iv)
    for (uint32_t iu = 0; iu < far->bins_u; ++iu) {
      const std::size_t c = (std::size_t)iv * far->bins_u + iu;
      const double X = -R + 2.0 * R * (iu + 0.5) / far->bins_u, Y = -R + 2.0 * R * (iv + 0.5) / far->bins_v;
      const double rho2 = X * X + Y * Y, mu = 1.0 - rho2 / 2.0, w = std::sqrt(std::fmax(1.0 - rho2 / 4.0, 0.0));
      const double a = X * w, b = Y * w;
      if (dir_xyz)
        for (int k = 0; k < 3; ++k) dir_xyz[3 * c + k] = a * f[3 + k] + b * f[6 + k] + mu * f[k];
      if (polar_rad) polar_rad[c] = std::acos(std::fmin(std::fmax(mu, -1.0), 1.0));
      if (azimuth_rad) azimuth_rad[c] = std::atan2(Y, X);
    }
  return BZR_OK;
}

bzr_status bzr_farfield_intensity(const bzr_farfield *far, const uint64_t *flux_q32, uint32_t nmaps, double scale,
                                  double *out) {
  float f[13];
  if (const char *why = bzr_internal_farfield_frame(far, 1, f)) return bad(why);
  if ((!flux_q32 || !out) && nmaps) return bad("null argument");
  if (!std::isfinite(scale)) return bad("scale must be finite");
  const double R = far->extent, omega = (2.0 * R / far->bins_u) * (2.0 * R / far->bins_v);
  const std::size_t total = (std::size_t)far->bins_u * far->bins_v * nmaps;
  for (std::size_t k = 0; k < total; ++k) out[k] = scale * (static_cast<double>(flux_q32[k]) / 4294967296.0) / omega;
  return BZR_OK;
}

}  // extern "C"
