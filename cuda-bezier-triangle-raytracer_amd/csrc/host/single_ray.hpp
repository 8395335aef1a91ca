// single_ray.hpp -- the drop-in's single-ray hot-path methods on the host (single_ray.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <tuple>
#include <utility>

#include "bzr/bzr.hpp"

namespace bzr_host {
// BezierTriangle::intersect on one 66-word record, twice: whole, and with newton_tail's hook answering "not
// needed" (the last normal skipped).  12 words each: t, point, cos, barycentrics, normal, what.
void newton_short_pair(const float *record, const float ray[6], bool limitNone, float full[12], float skipped[12]);
// The Fresnel transmittance of n (eta, cos) pairs, 0 where Snell's step does not refract (bzr_debug_fresnel).
void fresnel_pairs(const float *eta, const float *cs, uint32_t n, float *t_out);
// The Beer-Lambert term att(x[i]) of n values (bzr_debug_attenuation with a null context).
void attenuation(const float *x, uint32_t n, float *out);
// The coated surface's transmittance coat_t(row, mu), row [BZR_COAT_SAMPLES] (bzr_coat_transmittance).
float coat_transmittance(const float *row, float mu);
}  // namespace bzr_host

namespace bzr {
namespace host {
// BezierTriangle::intersect(ray, limit) (reference/bezierTriangle.cpp:123-195); limitNone = cNone.
BezierIntersection patchIntersect(BezierTriangle const &patch, Ray const &ray, bool limitNone);
// BezierMesh::intersect(ray) (reference/bezierMesh.cpp:206-227); *patch = winning patch, ~0u on a miss.
BezierIntersection meshIntersect(BezierTriangle const *patches, std::size_t n, Ray const &ray, uint32_t *patch);
// BezierLens::refract(ray, expected) (reference/bezierLens.cpp:4-34); the input ray on cNone.
std::pair<Ray, RefractionResult> lensRefract(BezierTriangle const *patches, std::size_t n, float ri, Ray const &ray,
                                             RefractionResult expected);
// The same scan and refraction, with the refraction's Fresnel transmittance T (1 on cNone).
std::tuple<Ray, RefractionResult, float> lensRefractPower(BezierTriangle const *patches, std::size_t n, float ri,
                                                          Ray const &ray, RefractionResult expected);
}  // namespace host
}  // namespace bzr
