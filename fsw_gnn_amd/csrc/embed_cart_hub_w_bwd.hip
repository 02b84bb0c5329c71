// Cartesian slice x frequency mode, general weights (w != NULL or tau > 1), lines of 2049 .. FSW_CART_W_MAX_LINE elements: backward
// with respect to the keys and the frequencies (the forward: embed_cart_hub_w.hip; the other classes: embed_cart_bwd.hip).  gfx950.
//
// Modelled on k_cart_bwd_long (embed_cart_hub_bwd.hip) and the diagonal k_embed_wsort_global_bwd<32, true> (embed_wsort_bwd.hip): ONE
// wavefront per (row, slice) line works in its own scratch line of pow2ceil(D + 1) packed (key, entry index) words -- chunks of 2048
// words sorted in registers (WaveLine64), the merge levels above one chunk as element-wise sweeps over the scratch line
// (sweep_pairs_b) with the tail of every level back in registers (merge_chunk).  The reference's pad element (key 0, weight
// max(tau - m, 0)) is element D of the line and carries index D, so it sorts last among keys equal to 0; equal keys keep entry
// order: the project's rule and the generic kernel's.  The weights do not travel through the sort: the walk re-reads them by entry
// index (w[start + idx], the pad weight for idx == D, 0 for the fill elements) and forms the float64 cumulative weights in one pass
// over the sorted line, the carry running across lanes and across chunks.  Every chunk is read out at all F frequencies (g_f and
// xi_f wave-uniform) with ONE F_dF (fourier_coef.h) per (element, frequency), chained as in k_cart_bwd_wave<M, true>: the lower
// bound of a lane's first element is the value at the last element of the lane below, of lane 0 the value the chunk before ended on
// (kept by lane f for frequency f).
//   gkey[e, s]  = sum_f out_scale g[r, s F + f] (F_f(c_rank) - F_f(c_{rank-1}))                      stored for every entry
//   gfreq[f]   += out_scale g[r, s F + f] sum_t (dF_f(c_t) - dF_f(c_{t-1})) p_(t)                     one float atomic per (line, frequency)
// The key gradients pass through the scratch line's second part in entry order, so that the stores to gkey walk the entries; the pad
// element stores nothing.  Lane f carries the line's gfreq sum of frequency f; more than 64 frequencies take another walk per 64.
// Scratch: 12 bytes per element of the padded line and resident wavefront.
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "fourier_coef.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

struct CartBwdLongW {
  const int32_t* rowptr;
  const int32_t* col;
  const float* w;                               // null with tau > 1: every weight is 1
  const int32_t* perm;
  const int32_t* bin_start;
  const float* Xp;
  int64_t ldp;
  const float* freqs;
  int S, F;
  float tau;
  const float* g;
  int64_t ldg;
  int gcol0;
  float out_scale;
  float* gkey;
  int64_t ldk;
  float* gfreq;
};

__global__ void __launch_bounds__(256) k_cart_bwd_long_w(const CartBwdLongW a, int bin, char* __restrict__ scratch, int64_t line_elems,
                                                         int nwaves) {
  constexpr int M = kCartLongM, CAP = kCartMaxLine;
  const int lane = lane_id();
  const int gw = blockIdx.x * 4 + wave_id();
  if (gw >= nwaves) return;                                      // the wavefronts never synchronise with each other
  unsigned long long* se = reinterpret_cast<unsigned long long*>(scratch + (int64_t)gw * line_elems * kCartLineBytes);   // packed (key, index) words
  float* sc = reinterpret_cast<float*>(se + line_elems);                                                     // key gradients, entry order
  const int pbeg = a.bin_start[bin], pend = a.bin_start[bin + 1];
  const int S = a.S, F = a.F;
  const double taud = (double)a.tau;
  const int64_t nlines = (int64_t)(pend - pbeg) * S;
  for (int64_t ln_id = gw; ln_id < nlines; ln_id += nwaves) {
    const int p = pbeg + (int)(ln_id / S), s = (int)(ln_id % S);
    const int node = a.perm[p];
    const int start = a.rowptr[node];
    const int D = a.rowptr[node + 1] - start;
    const int L = D + 1;                                         // with the pad element
    const int Dp = (int)pow2ceil((uint32_t)L);
    if (L <= CAP || L > FSW_CART_W_MAX_LINE || Dp > line_elems) continue;   // not a row of this class (wave-uniform)
    const int32_t* colrow = a.col + start;
    const float* wrow = a.w ? a.w + start : nullptr;
    const float* xs = a.Xp + s;
    // A. chunks: gather (striped: lane-contiguous col and weight reads; the entry index travels with the key), sort, park
    double mpart = 0.0;
    for (int c0 = 0; c0 < Dp; c0 += CAP) {
      WaveLine64<M> ln;
      int c[M];
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const int t = c0 + j * kWave + lane;
        c[j] = t < D ? colrow[t] : -1;
        mpart += (double)(t < D ? (wrow ? wrow[t] : 1.f) : 0.f);
      }
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const int t = c0 + j * kWave + lane;
        // the pad element at x = 0 with index D: last among equal keys; fill elements sort behind the line
        ln.e[j] = pack_key_index(c[j] >= 0 ? xs[(int64_t)c[j] * a.ldp] : (t == D ? 0.f : __builtin_inff()), t);
      }
      ln.sort();
#pragma unroll
      for (int j = 0; j < M; ++j) se[c0 + lane * M + j] = ln.e[j];
    }
    const double m = wave_sum(mpart);
    const double inv = 1.0 / fmax(m, taud);
    const float padw = (float)fmax(taud - m, 0.0);
    const double rho = pad_residual(taud - m, padw);             // what the float wt[] loses of the pad weight: added where the walk passes the pad (fsw_common.h)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    // B. merge levels above one chunk
    for (int size = 2 * CAP; size <= Dp; size <<= 1) {
      sweep_pairs_b(se, Dp, size, 0, true);
      for (int st = size >> 2; st >= CAP; st >>= 1) sweep_pairs_b(se, Dp, size, st, false);
      for (int c0 = 0; c0 < Dp; c0 += CAP) {
        WaveLine64<M> ln;
#pragma unroll
        for (int j = 0; j < M; ++j) ln.e[j] = se[c0 + lane * M + j];
        ln.merge_chunk();
#pragma unroll
        for (int j = 0; j < M; ++j) se[c0 + lane * M + j] = ln.e[j];
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    // C. walk: the lane's ranks r0 .. r0 + M - 1 of every chunk at all frequencies
    const float* grow = a.g + (int64_t)node * a.ldg + a.gcol0 + (int64_t)s * F;
    for (int fb = 0; fb < F; fb += kWave) {
      const int nf = min(kWave, F - fb);
      float gfl = 0.f;                                           // lane q: the line's gfreq sum of frequency fb + q
      double Fc = 0.0, dFc = 0.0;                                // lane q: F and dF of frequency fb + q where the chunk before ended (F(0) = 0)
      double carry = 0.0;                                        // cumulative weight before the chunk
      for (int c0 = 0; c0 < L; c0 += CAP) {
        const int r0 = c0 + lane * M;
        float key[M], G[M], wt[M];
        int idx[M];
        double pre = 0.0;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const unsigned long long e = se[r0 + j];
          key[j] = r0 + j < L ? from_orderable_bits((unsigned int)(e >> 32)) : 0.f;   // fill elements: no inf in the frequency sums
          idx[j] = (int)(unsigned int)e;
          G[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {
          wt[j] = idx[j] < D ? (wrow ? wrow[idx[j]] : 1.f) : (idx[j] == D ? padw : 0.f);
          pre += (double)wt[j] + (idx[j] == D ? rho : 0.0);
        }
        const double cbase = carry + wave_exclusive_scan_f64(pre);
        carry += wave_sum(pre);
        for (int q = 0; q < nf; ++q) {
          const FCoef fc((double)a.freqs[fb + q]);
          const float gi = a.out_scale * grow[fb + q];
          double F0 = 0.0, dF0 = 0.0, Fp = 0.0, dFp = 0.0, c = cbase;
          float ds = 0.f;
#pragma unroll
          for (int j = 0; j < M; ++j) {
            c += (double)wt[j] + (idx[j] == D ? rho : 0.0);
            double Fv, dFv;
            F_dF(fc, c * inv, Fv, dFv);
            if (j == 0) {
              F0 = Fv;
              dF0 = dFv;
            } else {
              G[j] = fmaf(gi, (float)(Fv - Fp), G[j]);
              ds = fmaf((float)(dFv - dFp), key[j], ds);
            }
            Fp = Fv;
            dFp = dFv;
          }
          // the lower bound of this lane's first element: the value at the last element of the lane below; lane 0: where the chunk
          // before ended
          double Fl = __shfl_up(Fp, 1), dFl = __shfl_up(dFp, 1);
          const double Fq = __shfl(Fc, q), dFq = __shfl(dFc, q);
          if (lane == 0) {
            Fl = Fq;
            dFl = dFq;
          }
          const double Fe = __shfl(Fp, kWave - 1), dFe = __shfl(dFp, kWave - 1);
          if (lane == q) {
            Fc = Fe;
            dFc = dFe;
          }
          G[0] = fmaf(gi, (float)(F0 - Fl), G[0]);
          ds = fmaf((float)(dF0 - dFl), key[0], ds);
          const float tot = wave_sum(gi * ds);
          if (lane == q) gfl += tot;
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {
          if (idx[j] < D) sc[idx[j]] = fb == 0 ? G[j] : sc[idx[j]] + G[j];   // the same lane wrote sc[idx] in the walk before
        }
      }
      if (a.gfreq && lane < nf) atomicAdd(a.gfreq + fb + lane, gfl);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (int t = lane; t < D; t += kWave) a.gkey[(int64_t)(start + t) * a.ldk + s] = sc[t];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");       // the next line reuses the scratch
  }
}

}  // namespace

// general weights: the classes of kCartLong[1], one launch per populated bin they touch (embed_cart.h: for_each_cart_line_bin)
int launch_cart_hub_w_bwd(const fsw_cart_args* c, hipStream_t stream) {
  CartBwdLongW t;
  cart_fill_inputs_w(t, c);
  cart_fill_grads(t, c);
  return for_each_cart_line_bin(c, kCartLong[1], [&](int bin, int64_t line_elems, int nwaves) {
    k_cart_bwd_long_w<<<(unsigned)ceil_div(nwaves, 4), 256, 0, stream>>>(t, bin, reinterpret_cast<char*>(c->scratch), line_elems, nwaves);
  });
}

}  // namespace fsw
