// The general-weight walk of ONE frequency over a thread's VT consecutive sorted elements, included INSIDE the loop over the frequencies
// q of a block of 64 in k_cart_giant_bwd<true> (embed_giant_cart_bwd.hip) and k_splitw_bwd_walk (embed_split_cart_w_bwd.hip): ONE F_dF
// per element at its float64 cumulative weight + one at the thread's lower bound cw0; the key gradients add into G[], the wavefront's
// frequency gradient into lane q's gfl.
// In scope at the point of inclusion: a (freqs, out_scale), grow, fb, q, cw0, inv (1 / max(m, tau)), rho (fsw_common.h: pad_residual), D,
// lane, key[VT], wt[VT], idx[VT], G[VT], gfl and the compile-time constant VT.
// Text like walk_unit.inc, the other branch of k_cart_giant_bwd; included text leaves both kernels instruction-identical.
  const FCoef fc((double)a.freqs[fb + q]);
  const float gi = a.out_scale * grow[fb + q];
  double c = cw0, Fp, dFp;
  F_dF(fc, c * inv, Fp, dFp);   // the lower bound of the thread's first element
  float ds = 0.f;
#pragma unroll
  for (int j = 0; j < VT; ++j) {
    c += (double)wt[j] + (idx[j] == D ? rho : 0.0);
    double Fv, dFv;
    F_dF(fc, c * inv, Fv, dFv);
    G[j] = fmaf(gi, (float)(Fv - Fp), G[j]);
    ds = fmaf((float)(dFv - dFp), key[j], ds);
    Fp = Fv;
    dFp = dFv;
  }
  const float tot = wave_sum(gi * ds);
  if (lane == q) gfl += tot;
