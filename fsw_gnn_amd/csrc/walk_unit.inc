// The unit-weight walk of ONE frequency over a thread's VT consecutive ranks of a sorted line, included INSIDE the loop over the
// frequencies q of a block of 64 in k_cart_giant_bwd<false> (embed_giant_cart_bwd.hip) and k_split_bwd_walk (embed_split_cart_bwd.hip):
// c_t = t / D, F and dF by a float64 rotation restarted from exact values at the thread's first rank r0; the key gradients add into G[],
// the wavefront's frequency gradient into lane q's gfl.
// In scope at the point of inclusion: a (freqs, out_scale), grow, fb, q, inv (1 / D), r0, D, lane, key[VT], G[VT], gfl and the
// compile-time constant VT.
// Text and not a device function: as an inlined function (arrays by reference or as pointers) k_split_bwd_walk goes from 243 to 256
// vector registers with 32 bytes of private memory and k_cart_giant_bwd<false> from 255 to spilling.  Included text leaves both
// instruction-identical (tools/compare_kernel_asm.py).
  const double xi = (double)a.freqs[fb + q];
  const float gi = a.out_scale * grow[fb + q];
  const FCoef fc(xi);
  const double step = xi * inv;   // revolutions per rank
  double sd, cd, sn, cs, Fp, dFp;
  sincospi(2.0 * (step - rint(step)), &sd, &cd);
  const double x0 = step * (double)r0;
  sincospi(2.0 * (x0 - rint(x0)), &sn, &cs);
  F_dF_sc(fc, (double)min(r0, D) * inv, sn, cs, Fp, dFp);
  float ds = 0.f;
#pragma unroll
  for (int j = 0; j < VT; ++j) {
    const double s1 = fma(sn, cd, cs * sd), c1 = fma(cs, cd, -(sn * sd));
    sn = s1;
    cs = c1;
    double Fv, dFv;
    F_dF_sc(fc, (double)min(r0 + j + 1, D) * inv, sn, cs, Fv, dFv);
    if (r0 + j < D) {
      G[j] = fmaf(gi, (float)(Fv - Fp), G[j]);
      ds = fmaf((float)(dFv - dFp), key[j], ds);
    }
    Fp = Fv;
    dFp = dFv;
  }
  const float tot = wave_sum(gi * ds);
  if (lane == q) gfl += tot;
