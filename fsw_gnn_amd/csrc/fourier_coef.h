// The readout's antiderivative F(xi; c) = (1 + xi) sin(2 pi xi c) / (pi xi) and its xi-derivative, float64: the coefficient of a sorted
// element is F(c_t) - F(c_{t-1}) and the backward kernels of the rows above the register path (embed_wsort_bwd.hip) and of Cartesian
// mode (embed_cart_bwd.hip) evaluate both per (element, frequency).  gfx950.
#pragma once
#include "fsw_common.h"

namespace fsw {

// F and dF/dxi at normalised cumulative weight c, given sin and cos of 2 pi xi c; series for tiny phases (the two terms
// of dF cancel there); xi == 0: F = 2 c, dF = 2 c.  FCoef holds the per-slice factors so that no division is left per element.
struct FCoef {
  double xi, a1, a2, a3;   // a1 = (1 + xi)/(pi xi), a2 = 1/(pi xi^2), a3 = 2 (1 + xi)/xi
  __device__ __forceinline__ explicit FCoef(double x) : xi(x) {
    const double r = x != 0.0 ? 1.0 / x : 0.0;
    a1 = (1.0 + x) * r * (1.0 / kPi);
    a2 = r * r * (1.0 / kPi);
    a3 = 2.0 * (1.0 + x) * r;
  }
};
__device__ __forceinline__ void F_dF_sc(const FCoef& f, double c, double s, double co, double& F, double& dF) {
  const double x = 2.0 * kPi * f.xi * c;
  if (fabs(x) < 1e-4) {
    const double q = 1.0 - x * x * (1.0 / 6.0);
    F = (1.0 + f.xi) * 2.0 * c * q;
    dF = 2.0 * c * q - (1.0 + f.xi) * 2.0 * c * (2.0 * kPi * c) * (2.0 * kPi * c) * f.xi * (1.0 / 3.0);
  } else {
    F = f.a1 * s;
    dF = fma(f.a3 * c, co, -(f.a2 * s));
  }
}
__device__ __forceinline__ void F_dF(const FCoef& f, double c, double& F, double& dF) {
  const double ph = f.xi * c;
  double s, co;
  sincospi(2.0 * (ph - rint(ph)), &s, &co);
  F_dF_sc(f, c, s, co, F, dF);
}

}  // namespace fsw
