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

}  // namespace hdiff
