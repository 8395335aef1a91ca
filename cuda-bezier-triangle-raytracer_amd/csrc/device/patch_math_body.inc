// patch_math_body.inc -- the arithmetic of the hot path, included twice by patch_math.hpp:
//   namespace exact   IEEE binary32 in the reference's operation order, no contraction,
//                     correctly rounded div/sqrt: bit-identical to the oracle (BZR_MODE_PARITY)
//   namespace fast    the same expressions with FMA contraction and the hardware's approximate
//                     reciprocal / square root (BZR_MODE_FAST, the Newton stage only)
// Each namespace defines div_rn, sqrt_rn, sqrt_above_hundredth, unit_or_self(a, |a|^2),
// div_heights(hIn, hOut, cos, hIn / cos, hOut / cos), bits_f32(u) (the float with these bits) and rint_even(y)
// (round to the nearest integer, ties to even) before including this file.
//   plane_ray        reference/3dGeomUtil.h:279-296 (+ deviations D1/D2, DESIGN.md)
//   interpolate      reference/bezierTriangle.cpp:105-121
//   surface_normal   reference/bezierTriangle.cpp:197-233
//   newton_tail      reference/bezierTriangle.cpp:132-195
//   fresnel_t        no reference counterpart: the transmittance of a refraction (DESIGN.md (a), ray power)
//   att              no reference counterpart: the Beer-Lambert term of one leg (DESIGN.md (a), absorption)
//   coat_t           no reference counterpart: the transmittance of a coated surface (DESIGN.md (a), surface coatings)
__device__ __forceinline__ f3 add(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 scale(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
__device__ __forceinline__ f3 cross(f3 a, f3 b) {
  return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ f3 normalized(f3 a) {
  float z = dot(a, a);
  return unit_or_self(a, z);
}

// Unpolarised Fresnel transmittance of one refraction (DESIGN.md (a), ray power).  eta, cs and
// s2 = eta^2 (1 - cs^2) < 0.99 are the values Snell's step has (refract_hit): c2 >= 0.1 and eta > 0, so both
// denominators are positive.  The direction-kept branch (s2 <= 1e-12) takes the same formula.
__device__ __forceinline__ float fresnel_t(float eta, float cs, float s2) {
  const float c1 = fabsf(cs), c2 = sqrt_rn(1.0f - s2);
  const float a = eta * c1;
  const float rs = div_rn(a - c2, a + c2);
  const float b = eta * c2;
  const float rp = div_rn(b - c1, b + c1);
  return 1.0f - 0.5f * (rs * rs + rp * rp);
}

// Beer-Lambert attenuation of one leg, att(x) ~ exp(-x) for x = a len >= 0 (DESIGN.md (a), absorption).  No
// correctly rounded expf exists to lean on, so the term is defined by its operations, each rounded once in binary32:
// y = x log2(e); k = rint(y), an integer in 0 .. 125; f = y - k, exact, |f| <= 1/2; 2^-f by a degree-7 Horner
// polynomial with c_j = float((-ln 2)^j / j!); times 2^-k, an exact scaling.  y >= 125 (and a NaN) gives 0, so the
// result is 0 or normal.  c_0 = 1: att(0) = 1.  Not monotone in the last bit.
__device__ __forceinline__ float att(float x) {
  const float y0 = x * bits_f32(0x3FB8AA3Bu);
  const bool live = y0 < 125.0f;
  const float y = live ? y0 : 0.0f;  // (a select, not a branch: the dead lanes run the polynomial on 0)
  const float k = rint_even(y);
  const float f = y - k;
  float p = bits_f32(0xb77fe5feu);
  p = p * f;
  p = p + bits_f32(0x39218489u);
  p = p * f;
  p = p + bits_f32(0xbaaec3ffu);
  p = p * f;
  p = p + bits_f32(0x3c1d955bu);
  p = p * f;
  p = p + bits_f32(0xbd635847u);
  p = p * f;
  p = p + bits_f32(0x3e75fdf0u);
  p = p * f;
  p = p + bits_f32(0xbf317218u);
  p = p * f;
  p = p + 1.0f;
  const float r = p * bits_f32((127u - (uint32_t)(int32_t)k) << 23);
  return live ? r : 0.0f;
}

// Transmittance of a coated surface (DESIGN.md (a), surface coatings; include/bzr.h bzr_coating): the row holds the
// reflectance at the gap-side cosines i / 128, and the lookup is defined by its operations like att.  coat_cell: the
// cell i = min((int)(128 mu'), 127) and the fraction f = 128 mu' - i of mu' = min(mu, 1), both exact (a scaling by a
// power of two, an integer below 2^7, a difference of two floats within a factor of two or with i = 0); the integer
// clamps keep a NaN or a negative mu inside the row.  coat_mix: R = r0 + f (r1 - r0), each operation rounded once, and
// T = 1 - R.  With both entries in [0, 1] so are R and T.
__device__ __forceinline__ int coat_cell(float mu, float &f) {
  const float x = fminf(mu, 1.0f) * 128.0f;
  int i = (int)x;
  i = i < 127 ? i : 127;
  i = i > 0 ? i : 0;
  f = x - (float)i;
  return i;
}
__device__ __forceinline__ float coat_mix(float r0, float r1, float f) {
  const float dr = r1 - r0;
  const float p = f * dr;
  const float r = r0 + p;
  return 1.0f - r;
}
__device__ __forceinline__ float coat_t(const float *row, float mu) {
  float f;
  const int i = coat_cell(mu, f);
  return coat_mix(row[i], row[i + 1], f);
}

template <typename P>
__device__ __forceinline__ f3 matvec(const P &p, f3 v) {  // Eigen row redux over the col-major M
  return mk(p.m(0) * v.x + (p.m(3) * v.y + p.m(6) * v.z), p.m(1) * v.x + (p.m(4) * v.y + p.m(7) * v.z),
            p.m(2) * v.x + (p.m(5) * v.y + p.m(8) * v.z));
}

// Plane::intersect(start, dir) with D1 (point for any t) and D2 (point = start when |cos| < eps)
__device__ __forceinline__ bool plane_ray(f3 n, float c, f3 start, f3 dir, f3 &point, float &cs, float &t) {
  cs = dot(dir, n);
  if (fabsf(cs) >= 0.00001f) {
    t = div_rn(c - dot(n, start), cs);
    point = add(start, scale(dir, t));
    return t > 0.0f;
  }
  t = 0.0f;
  point = start;
  return false;
}

__device__ __forceinline__ float plane_distance(f3 n, float c, f3 p) { return dot(p, n) - c; }
__device__ __forceinline__ f3 plane_project(f3 n, float c, f3 p) { return sub(p, scale(n, dot(p, n) - c)); }

template <typename P>
__device__ __forceinline__ f3 interpolate(const P &p, f3 b) {
  float q0 = b.x * b.x, q1 = b.y * b.y, q2 = b.z * b.z;
#define c(k) p.cp(k)
#define BZR_IP(F)                                                                                      \
  (((((c(0).F * b.x) * q0 + (c(1).F * b.y) * q1) + (c(2).F * b.z) * q2) +                             \
    3.0f * ((((((c(3).F * b.y) * q0 + (c(4).F * b.x) * q1) + (c(5).F * b.z) * q1) + (c(6).F * b.y) * q2) + \
             (c(7).F * b.x) * q2) +                                                                    \
            (c(8).F * b.z) * q0)) +                                                                    \
   (((c(9).F * b.x) * b.y) * b.z) * 6.0f)
  return mk(BZR_IP(x), BZR_IP(y), BZR_IP(z));
#undef BZR_IP
#undef c
}

template <typename P>
__device__ __forceinline__ f3 surface_normal(const P &p, f3 b) {
  float q0 = b.x * b.x, q1 = b.y * b.y, q2 = b.z * b.z;
#define c(k) p.cp(k)
  // control point slots: 300=0 030=1 003=2 210=3 120=4 021=5 012=6 102=7 201=8 111=9
#define BZR_K0(F) (((c(0).F * q0 + c(7).F * q2) + c(4).F * q1) + 2.0f * (((c(8).F * b.x) * b.z + (c(3).F * b.x) * b.y) + (c(9).F * b.z) * b.y))
#define BZR_K1(F) (((c(1).F * q1 + c(6).F * q2) + c(3).F * q0) + 2.0f * (((c(9).F * b.x) * b.z + (c(4).F * b.x) * b.y) + (c(5).F * b.y) * b.z))
#define BZR_K2(F) (((c(2).F * q2 + c(8).F * q0) + c(5).F * q1) + 2.0f * (((c(7).F * b.x) * b.z + (c(6).F * b.y) * b.z) + (c(9).F * b.x) * b.y))
  f3 k0 = mk(BZR_K0(x), BZR_K0(y), BZR_K0(z));
  f3 k1 = mk(BZR_K1(x), BZR_K1(y), BZR_K1(z));
  f3 k2 = mk(BZR_K2(x), BZR_K2(y), BZR_K2(z));
#undef BZR_K0
#undef BZR_K1
#undef BZR_K2
#undef c
  const f3 da = p.da(), db = p.db();
  f3 ca = mk((da.x * k0.x + da.y * k1.x) + da.z * k2.x, (da.x * k0.y + da.y * k1.y) + da.z * k2.y,
             (da.x * k0.z + da.y * k1.z) + da.z * k2.z);
  f3 cb = mk((db.x * k0.x + db.y * k1.x) + db.z * k2.x, (db.x * k0.y + db.y * k1.y) + db.z * k2.y,
             (db.x * k0.z + db.y * k1.z) + db.z * k2.z);
  return normalized(cross(ca, cb));
}

// BezierTriangle::intersect after its planar gate (reference/bezierTriangle.cpp:132-195): bracket,
// secant start, Newton steps, acceptance and the divider-plane classification.  (ic, it) are the
// gate's plane cosine and distance.
// `need` decides whether the last iteration evaluates its surface normal.  That iteration's `middle` is
// the returned h.t, and its normal feeds h.normal and h.cs only -- the acceptance test and the divider
// classification read h.point -- so a caller that knows h.t cannot win (trace.hip trace_segment's vote)
// skips it: h.normal and h.cs are then zero (callers must not rely on that), everything else has the same
// bits.  need(h.t) must be wave-uniform on the device.  NormalAlways (the default) is plain C++: the body
// also compiles for the host.
struct NormalAlways {
  __device__ __forceinline__ bool operator()(float) const { return true; }
};
template <typename P, typename Need = NormalAlways>
__device__ __forceinline__ Hit newton_tail(const P &p, f3 s, f3 d, float ic, float it, Need need = Need()) {
  Hit h;
  h.t = 0.0f;
  h.point = mk(0.0f, 0.0f, 0.0f);
  h.cs = 0.0f;
  h.bary = h.point;
  h.normal = h.point;
  h.what = kNone;
  float din, dout;  // hIn / cos, hOut / cos (correctly rounded; one shared reciprocal where proven, div_heights)
  div_heights(p.hin(), p.hout(), ic, din, dout);
  float closer = it + (ic > 0.0f ? din : dout);
  float further = it + (ic > 0.0f ? dout : din);
  // secant start between the two bounding heights
  f3 por = add(s, scale(d, closer));
  f3 b = matvec(p, plane_project(p.n(), p.c(), por));
  f3 q = interpolate(p, b);
  float diffc = fabsf(plane_distance(p.n(), p.c(), por)) - fabsf(plane_distance(p.n(), p.c(), q));
  por = add(s, scale(d, further));
  b = matvec(p, plane_project(p.n(), p.c(), por));
  q = interpolate(p, b);
  float difff = fabsf(plane_distance(p.n(), p.c(), por)) - fabsf(plane_distance(p.n(), p.c(), q));
  float den = diffc - difff;
  float middle = fabsf(den) < 0.000001f ? div_rn(closer + further, 2.0f)
                                        : div_rn(diffc * further - difff * closer, den);
  f3 pdir = p.n();
#if BZR_NEWTON_UNROLL
#pragma unroll
#endif
  for (int i = 0; i + 1 < BZR_NEWTON_ITERS; ++i) {  // csRootSearchIterations, all but the last
    h.t = middle;
    por = add(s, scale(d, middle));
    f3 pp;
    float pc, pt;
    plane_ray(p.n(), p.c(), por, pdir, pp, pc, pt);
    h.bary = matvec(p, pp);
    h.normal = surface_normal(p, h.bary);
    h.point = interpolate(p, h.bary);
    pdir = normalized(sub(h.point, pp));
    middle = div_rn(dot(sub(h.point, s), h.normal), dot(d, h.normal));
#ifdef BZR_NEWTON_PROBE
    BZR_NEWTON_PROBE(i, middle, pdir);  // host experiments only (scripts/newton_fixpoint.cpp)
#endif
  }
  // The last iteration.  Its Newton step is never taken, so what it leaves is h.t (the t it enters with), the
  // barycentrics, the point and the normal; the normal comes last, behind everything that reads the point, and
  // only when the caller needs it.
  h.t = middle;
  por = add(s, scale(d, middle));
  f3 pp;
  float pc, pt;
  plane_ray(p.n(), p.c(), por, pdir, pp, pc, pt);
  h.bary = matvec(p, pp);
  h.point = interpolate(p, h.bary);
  f3 rel = sub(h.point, s);
  f3 perp = sub(rel, scale(d, dot(rel, d)));
  uint32_t what = kNone;
  if (!(sqrt_above_hundredth(dot(perp, perp)) || h.t < (further - closer) * 1.0f)) {  // norm(perp) > 0.01f: none
    uint32_t out = plane_distance(p.dn(0), p.dc(0), h.point) < 0.0f ? 1u : 0u;
    out |= plane_distance(p.dn(1), p.dc(1), h.point) < 0.0f ? 2u : 0u;
    out |= plane_distance(p.dn(2), p.dc(2), h.point) < 0.0f ? 4u : 0u;
    what = out == 1u ? 0u : (out == 2u ? 1u : (out == 4u ? 2u : kIntersect));
  }
  h.what = what;
  if (need(h.t)) {
    h.normal = surface_normal(p, h.bary);
    if (what == kIntersect) h.cs = dot(d, h.normal);
#ifdef BZR_NEWTON_PROBE
    pdir = normalized(sub(h.point, pp));
    middle = div_rn(dot(sub(h.point, s), h.normal), dot(d, h.normal));
    BZR_NEWTON_PROBE(BZR_NEWTON_ITERS - 1, middle, pdir);
#endif
  } else {
    h.normal = mk(0.0f, 0.0f, 0.0f);  // (not the previous iteration's, which would stay live to here)
  }
  return h;
}
