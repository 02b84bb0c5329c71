// Cartesian slice x frequency mode, hub rows with unit weights (FSW_LDS_MAX_DEG < in-degree <= FSW_HUB_MAX_DEG): backward with
// respect to the keys and the frequencies (the other classes: embed_cart_bwd.hip).  gfx950.
//
// Modelled on the diagonal k_embed_wsort_global_bwd<32, false> (embed_wsort_bwd.hip): ONE wavefront per (row, slice) line works in
// its own scratch line of packed (key, entry index) words -- chunks of 2048 words sorted in registers (WaveLine64), the merge levels
// above one chunk as element-wise sweeps over the scratch line (sweep_pairs_b) with the tail of every level back in registers
// (merge_chunk).  Equal keys keep entry order: the project's rule and the generic kernel's.  The sorted line is then walked chunk
// by chunk and every chunk is read out at all F frequencies (g_f and xi_f wave-uniform), the unit-weight coefficients
// F(c_{r+1}) - F(c_r) and their xi-derivatives by the float64 rotation of walk_line:
//   gkey[e, s]  = sum_f out_scale g[r, s F + f] (F_f(c_{rank+1}) - F_f(c_rank))                  stored for every entry
//   gfreq[f]   += out_scale g[r, s F + f] sum_t (dF_f(c_{t+1}) - dF_f(c_t)) p_(t)                one float atomic per (line, frequency)
// The key gradients pass through the scratch line's second part in entry order, so that the stores to gkey walk the entries.
// Lane f of the wavefront carries the line's gfreq sum of frequency f; more than 64 frequencies take another walk per 64.
// Scratch: 12 bytes per element of the padded line (next power of two >= the bin's longest row) and resident wavefront.
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "fourier_coef.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

struct CartBwdLong {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* perm;
  const int32_t* bin_start;
  const float* Xp;
  int64_t ldp;
  const float* freqs;
  int S, F;
  const float* g;
  int64_t ldg;
  int gcol0;
  float out_scale;
  float* gkey;
  int64_t ldk;
  float* gfreq;
};

__global__ void __launch_bounds__(256) k_cart_bwd_long(const CartBwdLong a, int bin, char* __restrict__ scratch, int64_t line_elems,
                                                       int nwaves) {
  constexpr int M = kCartLongM, CAP = kCartMaxLine;
  const int lane = lane_id();
  const int gw = blockIdx.x * 4 + wave_id();
  if (gw >= nwaves) return;                                      // the wavefronts never synchronise with each other
  unsigned long long* se = reinterpret_cast<unsigned long long*>(scratch + (int64_t)gw * line_elems * kCartLineBytes);   // packed (key, index) words
  float* sc = reinterpret_cast<float*>(se + line_elems);                                                     // key gradients, entry order
  const int pbeg = a.bin_start[bin], pend = a.bin_start[bin + 1];
  const int S = a.S, F = a.F;
  const int64_t nlines = (int64_t)(pend - pbeg) * S;
  for (int64_t ln_id = gw; ln_id < nlines; ln_id += nwaves) {
    const int p = pbeg + (int)(ln_id / S), s = (int)(ln_id % S);
    const int node = a.perm[p];
    const int start = a.rowptr[node];
    const int D = a.rowptr[node + 1] - start;
    const int Dp = (int)pow2ceil((uint32_t)D);
    if (D <= CAP || Dp > line_elems) continue;                   // not a row of this class (wave-uniform)
    const int32_t* colrow = a.col + start;
    const float* xs = a.Xp + s;
    // A. chunks: gather (striped: lane-contiguous col reads; the entry index travels with the key), sort, park
    for (int c0 = 0; c0 < Dp; c0 += CAP) {
      {
        constexpr bool RUN_PAD = false;
        unsigned long long* const run_line = se;
#include "sorted_run.inc"
      }
    }
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
    const double inv = 1.0 / (double)D;
    const float* grow = a.g + (int64_t)node * a.ldg + a.gcol0 + (int64_t)s * F;
    for (int fb = 0; fb < F; fb += kWave) {
      const int nf = min(kWave, F - fb);
      float gfl = 0.f;                                           // lane q: the line's gfreq sum of frequency fb + q
      for (int c0 = 0; c0 < D; c0 += CAP) {
        const int r0 = c0 + lane * M;
        float key[M], G[M];
        int idx[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const unsigned long long e = se[r0 + j];
          key[j] = r0 + j < D ? from_orderable_bits((unsigned int)(e >> 32)) : 0.f;   // fill elements: no inf in the frequency sums
          idx[j] = (int)(unsigned int)e;
          G[j] = 0.f;
        }
        for (int q = 0; q < nf; ++q) {
          const double xi = (double)a.freqs[fb + q];
          const float gi = a.out_scale * grow[fb + q];
          const FCoef fc(xi);
          const double step = xi * inv;                          // revolutions per rank
          double sd, cd, sn, cs, Fp, dFp;
          sincospi(2.0 * (step - rint(step)), &sd, &cd);
          const double x0 = step * (double)r0;
          sincospi(2.0 * (x0 - rint(x0)), &sn, &cs);
          F_dF_sc(fc, (double)r0 * inv, sn, cs, Fp, dFp);
          float ds = 0.f;
#pragma unroll
          for (int j = 0; j < M; ++j) {
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
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {
          if (r0 + j < D) sc[idx[j]] = fb == 0 ? G[j] : sc[idx[j]] + G[j];   // the same lane wrote sc[idx] in the walk before
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

// unit weights with tau <= 1: the classes of kCartLong[0], one launch per populated hub bin (embed_cart.h: for_each_cart_line_bin)
int launch_cart_hub_bwd(const fsw_cart_args* c, hipStream_t stream) {
  CartBwdLong t;
  cart_fill_inputs(t, c);
  cart_fill_grads(t, c);
  return for_each_cart_line_bin(c, kCartLong[0], [&](int bin, int64_t line_elems, int nwaves) {
    k_cart_bwd_long<<<(unsigned)ceil_div(nwaves, 4), 256, 0, stream>>>(t, bin, reinterpret_cast<char*>(c->scratch), line_elems, nwaves);
  });
}

}  // namespace fsw
