// Coefficients of the general-weight register kernels (embed_bwd.hip, embed_w_bwd.hip), float64.
// (1 + xi) Delta_t = F(c_t) - F(c_t - w_t) with F(xi; c) = (1 + xi) sin(2 pi xi c)/(pi xi) and c_t the cumulative normalised weight up
// to and including the element.
#pragma once
#include "fsw_common.h"

namespace fsw {

// F, dF / dxi (series for tiny phases: the two terms of dF cancel there) and h = d F / d c = 2 (1 + xi) cos(2 pi xi c), the factor of
// the weight gradient (embed_generic.hip: H_t = h(c_t) (p_(t) - p_(t+1))), from one sine / cosine pair.
__device__ __forceinline__ void F_dF_h(double xi, double c, double& F, double& dF, double& h) {
  const double x = 2.0 * kPi * xi * c;
  if (fabs(x) < 1e-4) {
    const double q = 1.0 - x * x * (1.0 / 6.0);
    F = (1.0 + xi) * 2.0 * c * q;
    dF = 2.0 * c * q - (1.0 + xi) * 2.0 * c * (2.0 * kPi * c) * (2.0 * kPi * c) * xi * (1.0 / 3.0);
    h = 2.0 * (1.0 + xi) * (1.0 - 0.5 * x * x);      // cos x to x^4 / 24 < 5e-18
    return;
  }
  const double ph = xi * c;
  double s, co;
  sincospi(2.0 * (ph - rint(ph)), &s, &co);
  F = (1.0 + xi) * s / (kPi * xi);
  dF = -s / (kPi * xi * xi) + (1.0 + xi) * 2.0 * c * co / xi;
  h = 2.0 * (1.0 + xi) * co;
}
// the kernels without a weight gradient: h unused, the same F and dF bit for bit
__device__ __forceinline__ void F_dF(double xi, double c, double& F, double& dF) {
  double h;
  F_dF_h(xi, c, F, dF, h);
}

}  // namespace fsw
