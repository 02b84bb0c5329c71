// Backward of the fused neighbourhood kernel WITH the gradient of the weights, rows above kWSortMaxDeg = 1024 neighbours, scratch-line
// form.  gfx950.
//
// The structure is that of k_embed_wsort_global_bwd<M, true> (embed_wsort_bwd.hip): one wavefront per line in a scratch line in global
// memory, the line of D + 1 elements -- the pad element (key 0, weight max(tau - m, 0) in float64) is element D -- as packed (key,
// element index) words, ties by element index; chunks of 64 M words sorted in registers, merged by sweeps over the scratch line
// (wave_sort.h: sweep_pairs_b), the last merge level walked chunk by chunk with the cumulative weight carried from chunk to chunk.
// gkey and gfreq come from F and dF/dxi on the cumulative weight with the expressions of k_embed_wsort_w_bwd (embed_w_sort_bwd.hip).
//
// The gradient of the weights needs, at rank t, the sum of q over the LATER ranks; a forward walk over the chunks has the earlier ones.
// Total minus prefix: with h(c) = 2 (1 + xi) cos(2 pi xi c), c1_t = cum_t / M, c0_t = c1_{t-1},
//     q_t   = (h(c1_t) - h(c0_t)) key_t
//     P_t   = sum_{v <= t} q_v            in-lane prefix + float64 wave exclusive scan of the lanes' sums + carry over the chunks
//     e_t   = h(c1_t) key_t - P_t
//     Qtot  = P_last,   HC = sum_t (h(c1_t) c1_t - h(c0_t) c0_t) key_t
//     R(t)  = e_t + Qtot                  (= h(c1_t) key_t + sum_{v > t} q_v of embed_w_sort_bwd.hip)
//     gw_j(s) = gd_s (e_rank(j) + K'_s),  gd_s = out_scale g[row, s] / M
//     K'_s  = -e_pad (m < tau: Qtot cancels)   |   -e_pad - HC (m == tau)   |   Qtot - HC (m > tau)
// so one forward pass over the chunks suffices: the per-element part e_t is known when the chunk is walked, the line constant K'_s
// when the line ends.  The lane keeps h(c1_t) key_t - (in-lane prefix) of the chunk's M ranks until the scan of the lanes' sums is known.
//
// Sum over slices: a wavefront's task is (row, kWLongSlices consecutive slices).  Its scratch line holds, next to the packed words [Dp]
// and the float key-gradient line, a float64 accumulator in element order: 8 + 8 + 4 = 20 bytes per element of the padded line (Dp =
// the next power of two of the bin's longest D + 1).  For every slice of the task the lane that holds rank(j) does a plain
// acc[j] += gd_s e_t (an element occurs once per line: no atomic), the line constants are summed in a wave-uniform Ksum += gd_s K'_s,
// and after the last slice the wave issues ONE float32 atomic per entry, acc[j] + Ksum, to consecutive addresses of gw (none for an
// exactly zero value).  An entry receives ceil(S / kWLongSlices) float32 adds.
// The weights are read as (double)w + (double)w_lo wherever a weight is read (w_lo nullable: include/fsw_hip.h,
// fsw_embed_backward_w_lo_f32): the row mass, 1 / max(m, tau), the pad weight and every cumulative weight.
// A line whose output gradient is zero writes zeros to its gkey column, skips the sort and adds nothing to gfreq or gw.
// No workgroup barrier: the wavefronts of a workgroup are independent, surplus ones return at once.  Fences: workgroup scope orders a
// wave's scratch stores before its own later loads (same CU, same L1; embed_wsort.hip) -- the words between the sweeps, the key
// gradients before they are copied out, and the accumulator, whose element j is updated by another lane in every slice.
#include <algorithm>
#include "embed_launch.h"
#include "sortnet.h"
#include "wave_sort.h"
#include "weighted_coef.h"

namespace fsw {

constexpr int kWLongBytesPerElem = 8 + 8 + 4;   // packed word, accumulator, key gradient
constexpr int kWLongBatch = 8;                  // accumulator updates in flight per lane

template <int M>
__global__ void __launch_bounds__(256) k_embed_w_long_bwd(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ w, const float* __restrict__ w_lo,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ bin_start, int bin, const float* __restrict__ Xp, int64_t ldp, int S,
    const float* __restrict__ freqs, float tau, const float* __restrict__ g, int64_t ldg, int gcol0, float out_scale,
    float* __restrict__ gfreq, float* __restrict__ gkey, int64_t ldk, float* __restrict__ gwt, char* __restrict__ scratch,
    int64_t line_elems, int nwaves) {
  constexpr int CAP = M * kWave;
  constexpr int G = kWLongSlices;
  static_assert(M % kWLongBatch == 0, "ranks per lane: a multiple of the update batch");
  const int lane = lane_id();
  const int wid = blockIdx.x * 4 + wave_id();
  if (wid >= nwaves) return;                              // this wavefront has no scratch line
  char* base = scratch + (int64_t)wid * line_elems * kWLongBytesPerElem;
  unsigned long long* se = reinterpret_cast<unsigned long long*>(base);   // [line_elems] packed (key, index) words
  double* acc = reinterpret_cast<double*>(base + 8 * line_elems);          // [line_elems] sum over the task's slices, element order
  float* sc = reinterpret_cast<float*>(base + 16 * line_elems);            // [line_elems] key gradients of the line, element order
  const int pbeg = bin_start[bin], pend = bin_start[bin + 1];
  const int ngroups = (S + G - 1) / G;
  const int64_t ntasks = (int64_t)(pend - pbeg) * ngroups;
  const double taud = (double)tau;
  for (int64_t task = wid; task < ntasks; task += nwaves) {
    const int p = pbeg + (int)(task / ngroups), k0 = (int)(task % ngroups) * G;
    const int node = perm[p];
    const int start = rowptr[node];
    const int D = rowptr[node + 1] - start;
    const int Dtot = D + 1;
    if ((int64_t)Dtot > line_elems) continue;             // longer than the scratch line (the launcher sizes it by the bin's longest row)
    const int Dp = (int)pow2ceil((uint32_t)Dtot);
    auto weight_at = [&](int t) -> double { return (double)w[start + t] + (w_lo ? (double)w_lo[start + t] : 0.0); };
    double part = 0.0;
    for (int t = lane; t < D; t += kWave) {
      part += weight_at(t);
      acc[t] = 0.0;                                       // (ordered before the first update by the fence behind the chunk sort)
    }
    const double m = wave_sum(part);
    const double inv = 1.0 / fmax(m, taud);
    const double padd = fmax(taud - m, 0.0);              // the pad weight in float64 (fsw_common.h: pad_residual)
    // (id > D: a filler ahead of a NaN key; it reads nothing)
    auto weight_of = [&](int id) -> double { return id < D ? weight_at(id) : (id == D ? padd : 0.0); };
    double Ksum = 0.0;                                    // sum over the slices of gd_s K'_s (wave-uniform)

    for (int k = k0; k < min(k0 + G, S); ++k) {
      const float graw = g[(int64_t)node * ldg + gcol0 + k];
      const float gi = out_scale * graw;
      if (graw == 0.f) {                                  // zero key gradients, nothing else (wave-uniform)
        for (int t = lane; t < D; t += kWave) gkey[(int64_t)(start + t) * ldk + k] = 0.f;
        continue;
      }
      const double xi = (double)freqs[k];
      const double gd = (double)out_scale * (double)graw * inv;
      for (int c0 = 0; c0 < Dp; c0 += CAP) {
        WaveLine64<M> ln;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const int t = c0 + lane * M + j;
          float key = __builtin_inff();
          if (t < D) key = Xp[(int64_t)col[start + t] * ldp + k];
          else if (t == D) key = 0.f;
          ln.e[j] = pack_key_index(key, t);
        }
        ln.sort();
#pragma unroll
        for (int j = 0; j < M; ++j) se[c0 + lane * M + j] = ln.e[j];
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      double gf = 0.0, HC = 0.0, epad = 0.0;
      double carry = 0.0, Pcarry = 0.0;                   // cumulative weight and sum of q of the chunks walked so far
      // a line of one chunk (D + 1 <= 64 M) is sorted already: its only "level" is the walk
      for (int size = Dp > CAP ? 2 * CAP : CAP; size <= Dp; size <<= 1) {
        const bool merge = size > CAP;
        if (merge) {
          sweep_pairs_b(se, Dp, size, 0, true);
          for (int st = size >> 2; st >= CAP; st >>= 1) sweep_pairs_b(se, Dp, size, st, false);
        }
        const bool last = size == Dp;
        for (int c0 = 0; c0 < Dp; c0 += CAP) {
          if (last && c0 >= Dtot) break;                  // only fillers from here on
          WaveLine64<M> ln;
#pragma unroll
          for (int j = 0; j < M; ++j) ln.e[j] = se[c0 + lane * M + j];
          if (merge) ln.merge_chunk();
          if (!last) {
#pragma unroll
            for (int j = 0; j < M; ++j) se[c0 + lane * M + j] = ln.e[j];
            continue;
          }
          const int r0 = c0 + lane * M;
          double lanew = 0.0;   // (the lane's weights: a copy of the loop in k_embed_wsort_bwd)
#pragma unroll
          for (int j = 0; j < M; ++j) lanew += (r0 + j < Dtot) ? weight_of(ln.index(j)) : 0.0;
          const double cstart = carry + wave_exclusive_scan_f64(lanew);
          carry += wave_sum(lanew);
          // forward over the lane's ranks, as k_embed_wsort_w_bwd: gkey into the element's place of the key-gradient line, gfreq, the
          // lane's sums of q and of the HC terms, and h(c1) key - (in-lane prefix of q) of every rank
          double c = cstart, c0n = c * inv, Fp, dFp, hp;
          F_dF_h(xi, c0n, Fp, dFp, hp);
          double el[M];
          double Q = 0.0;
#pragma unroll
          for (int j = 0; j < M; ++j) {
            const int id = ln.index(j);
            const bool valid = r0 + j < Dtot;
            c += valid ? weight_of(id) : 0.0;
            const double c1 = c * inv;
            double F, dF, h;
            F_dF_h(xi, c1, F, dF, h);
            const double kd = valid ? (double)ln.key(j) : 0.0;   // the +inf fillers beyond the line: weight 0, key taken as 0
            if (valid) {
              if (id < D) sc[id] = gi * (float)(F - Fp);          // the pad element (id == D) has no source row
              gf = fma((double)gi * (dF - dFp), kd, gf);
            }
            Q += (h - hp) * kd;
            HC += (h * c1 - hp * c0n) * kd;
            el[j] = h * kd - Q;
            Fp = F;
            dFp = dF;
            hp = h;
            c0n = c1;
          }
          // P_t = (chunks before) + (lanes below) + (in-lane prefix)
          const double Pbase = Pcarry + wave_exclusive_scan_f64(Q);
          Pcarry += wave_sum(Q);
#pragma unroll
          for (int j0 = 0; j0 < M; j0 += kWLongBatch) {  // the loads of a batch first: one round trip per batch, not per element
            double a[kWLongBatch];
#pragma unroll
            for (int u = 0; u < kWLongBatch; ++u) {
              const int id = ln.index(j0 + u);
              a[u] = (r0 + j0 + u < Dtot && id < D) ? acc[id] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kWLongBatch; ++u) {
              const int id = ln.index(j0 + u);
              const double e = el[j0 + u] - Pbase;
              if (r0 + j0 + u < Dtot) {
                if (id < D) acc[id] = a[u] + gd * e;
                else epad = e;
              }
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      }
      gf = wave_sum(gf);
      if (lane == 0 && gfreq) atomicAdd(gfreq + k, (float)gf);
      HC = wave_sum(HC);
      epad = wave_sum(epad);                              // one lane holds element D
      Ksum += gd * (m < taud ? -epad : (m == taud ? -epad - HC : Pcarry - HC));
      for (int t = lane; t < D; t += kWave) gkey[(int64_t)(start + t) * ldk + k] = sc[t];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the next line reuses the scratch; another lane updates acc[j]
    }
    for (int t = lane; t < D; t += kWave) {
      const double v = acc[t] + Ksum;
      if (v != 0.0) atomicAdd(gwt + start + t, (float)v);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");     // the next task zeroes the accumulator
  }
}

// Rows above kWSortMaxDeg neighbours: one launch per non-empty degree bin, the longest rows first, the scratch line sized by the bin's
// own longest row (as launch_embed_long_bwd(global = true), embed_wsort_bwd.hip).  The largest bin comes first and needs the longest
// line: when the buffer does not hold one wave's line of it, the call fails before any launch.
int launch_embed_w_long_bwd(const fsw_embed_args& a, const float* w_lo, int64_t max_degree, const float* g, int64_t ldg, float* gkey,
                            int64_t ldk, float* gfreq, float* gw, void* scratch, size_t scratch_bytes, hipStream_t stream) {
  static_assert(kWSortLastBin + 1 == FSW_BIN_LDS0 + 2 && FSW_BIN_LDS0 + 3 == FSW_BIN_HUB0 && FSW_BIN_HUB0 + 4 == FSW_BIN_GLOBAL,
                "the bins above the wave-sort class: 1025 .. 2048, four hub bins, the rest");
  const int64_t ngroups = ceil_div(a.S, kWLongSlices);
  for (int bin = FSW_BIN_GLOBAL; bin > kWSortLastBin; --bin) {
    const int64_t rows = bin_rows_or(a, bin, bin, a.num_rows);
    if (rows <= 0) continue;
    const int64_t bin_lo = (int64_t)kWSortMaxDeg << (bin - kWSortLastBin - 1);   // the bin holds bin_lo + 1 .. 2 bin_lo (the last: above)
    if (max_degree <= bin_lo) continue;                   // no row of the graph reaches this bin
    const int64_t bin_max = bin == FSW_BIN_GLOBAL ? max_degree : std::min<int64_t>(max_degree, 2 * bin_lo);
    const int64_t line_elems = (int64_t)pow2ceil((uint32_t)(bin_max + 1));
    const int64_t wave_bytes = line_elems * kWLongBytesPerElem;
    const int64_t nwaves = std::min<int64_t>(std::min<int64_t>(scratch ? (int64_t)(scratch_bytes / (size_t)wave_bytes) : 0, 2048), rows * ngroups);
    FSW_REQUIRE(nwaves >= 1, "fsw_embed_backward_w_f32: scratch buffer too small for rows above %d neighbours (one line of %lld bytes; "
                "fsw_embed_backward_w_scratch_bytes suffices)", kWSortMaxDeg, (long long)wave_bytes);
    k_embed_w_long_bwd<kWLongRanks><<<(unsigned)ceil_div(nwaves, 4), 256, 0, stream>>>(
        a.rowptr, a.col, a.w, w_lo, a.perm, a.bin_start, bin, a.Xp, a.ldp, a.S, a.freqs, a.tau, g, ldg, a.has_mass, a.out_scale, gfreq, gkey,
        ldk, gw, reinterpret_cast<char*>(scratch), line_elems, (int)nwaves);
    FSW_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace fsw
