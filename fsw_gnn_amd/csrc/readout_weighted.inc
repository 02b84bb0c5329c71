// The general-weight readout of a thread's kMpVT consecutive sorted (key, weight) elements at ONE frequency, included INSIDE the loop
// over the frequencies q of a batch in k_cart_mergepath_w (embed_giant_cart_w.hip) and k_splitw_readout (embed_split_cart_w.hip):
// acc[q] += sum_j (sin(2 pi xi c_j) - sin(2 pi xi c_{j-1})) k_j with c the float64 cumulative weight from cw0 on; xi == 0: sum_j w_j k_j.
// The factor (1 + xi) / (pi xi) is applied once per line by the caller.
// In scope at the point of inclusion: a (freqs), f0, q, kk[kMpVT], ww[kMpVT], acc[], cw0, inv (1 / max(m, tau)) and rho (fsw_common.h:
// pad_residual).
// Text and not a device function: as an inlined function (arrays by reference, the sum returned) k_cart_mergepath_w came out with
// 28132 instead of 30773 instructions and k_splitw_readout with 13274 instead of 13100.  Included text leaves both instruction-identical
// (tools/compare_kernel_asm.py).
  const float xif = a.freqs[f0 + q];
  if (fabsf(xif) < 1e-30f) {   // xi == 0: Delta_t = 2 w_t / max(m, tau)
#pragma unroll
    for (int j = 0; j < kMpVT; ++j) acc[q] = fmaf(ww[j], kk[j], acc[q]);
  } else {
    const double xi = (double)xif;
    double cw = cw0;
    // the element before a key >= 0 is the pad element, or lies behind it, or multiplies a zero key: same residual
    float sprev = sin2pi_rev(xi * ((cw + pad_residual_at(rho, kk[0])) * inv));
#pragma unroll
    for (int j = 0; j < kMpVT; ++j) {
      cw += (double)ww[j];
      const float sn = sin2pi_rev(xi * ((cw + pad_residual_at(rho, kk[j])) * inv));
      acc[q] = fmaf(sn - sprev, kk[j], acc[q]);
      sprev = sn;
    }
  }
