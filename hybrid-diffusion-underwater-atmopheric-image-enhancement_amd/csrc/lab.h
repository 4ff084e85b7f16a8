// sRGB -> CIE L*a*b* (D65) in double, shared by uciqe.hip and color_diff.hip: the conversion of tests/_uciqe_def.lab_def (the matrix and
// white point scikit-image uses), every product and sum rounding where the definition's does.  Both files are compiled with
// -ffp-contract=off; black comes out as exactly L = 0, a = 0, b = 0.
#pragma once
#include <math.h>

namespace hdiff {

__device__ __forceinline__ double srgb_to_linear(double v) { return v > 0.04045 ? pow((v + 0.055) / 1.055, 2.4) : v / 12.92; }
__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }

// sr, sg, sb: sRGB components, nominally in [0, 1]
__device__ __forceinline__ void srgb_to_lab(double sr, double sg, double sb, double& L, double& ca, double& cb) {
  const double r = srgb_to_linear(sr), g = srgb_to_linear(sg), b = srgb_to_linear(sb);
  const double fx = lab_f(((0.412453 * r + 0.357580 * g) + 0.180423 * b) / 0.95047);
  const double fy = lab_f(((0.212671 * r + 0.715160 * g) + 0.072169 * b) / 1.0);
  const double fz = lab_f(((0.019334 * r + 0.119193 * g) + 0.950227 * b) / 1.08883);
  L = 116.0 * fy - 16.0;
  ca = 500.0 * (fx - fy);
  cb = 200.0 * (fy - fz);
}

// CIE L*a*b* (D65) -> sRGB in double, NOT clipped: the inverse of srgb_to_lab branch for branch, as tests/_contrast_def.lab_to_srgb_def
// writes it out (contrast.hip).  The inverse matrix is the cofactor form of the nine literals above, each product, difference and
// quotient rounding where the definition's does (the compiler folds them in IEEE double).  sRGB values in (0.04045, 0.0404517] come back
// through the other piece of the transfer curve, 2e-7 off: the published constants do not make the two pieces meet.
__device__ __forceinline__ double lab_f_inverse(double f) {
  const double cube = (f * f) * f;
  return cube > 0.008856 ? cube : (f - 16.0 / 116.0) / 7.787;
}
__device__ __forceinline__ double linear_to_srgb(double v) { return v > 0.0031308 ? 1.055 * pow(v, 1.0 / 2.4) - 0.055 : 12.92 * v; }

__device__ __forceinline__ void lab_to_srgb(double L, double ca, double cb, double& sr, double& sg, double& sb) {
  const double a = 0.412453, b = 0.357580, c = 0.180423, d = 0.212671, e = 0.715160, f = 0.072169, g = 0.019334, h = 0.119193,
               i = 0.950227;
  const double A = (e * i) - (f * h), B = (f * g) - (d * i), C = (d * h) - (e * g);
  const double det = ((a * A) + (b * B)) + (c * C);
  const double fy = (L + 16.0) / 116.0;
  const double fx = fy + (ca / 500.0);
  const double fz = fy - (cb / 200.0);
  const double x = lab_f_inverse(fx) * 0.95047, y = lab_f_inverse(fy) * 1.0, z = lab_f_inverse(fz) * 1.08883;
  sr = linear_to_srgb((((A / det) * x) + ((((c * h) - (b * i)) / det) * y)) + ((((b * f) - (c * e)) / det) * z));
  sg = linear_to_srgb((((B / det) * x) + ((((a * i) - (c * g)) / det) * y)) + ((((c * d) - (a * f)) / det) * z));
  sb = linear_to_srgb((((C / det) * x) + ((((b * g) - (a * h)) / det) * y)) + ((((a * e) - (b * d)) / det) * z));
}

}  // namespace hdiff
