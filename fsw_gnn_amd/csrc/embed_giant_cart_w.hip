// Cartesian slice x frequency mode, general weights (w != NULL or tau > 1), lines of more than FSW_CART_W_MAX_LINE elements (any
// length): forward.  gfx950.
//
// The composition of the diagonal k_embed_mergepath_w (embed_hub.hip) with the readout of k_cart_hub_w (embed_cart_hub_w.hip).  One
// workgroup of four wavefronts takes ONE (recipient row, slice) line of L = D + 1 elements at a time (persistent, XCD-aware line
// loop): the D neighbours (key, weight) and the reference's pad element (key 0, weight max(tau - m, 0), fsw_embedding.py:1000-1017)
// as element D.
//   A. every block of kMpBlk elements is gathered, sorted in the workgroup's registers (WaveLine<32, true>, two exchange levels
//      through LDS) and parked in the workgroup's scratch lines; the row's mass m is summed in float64 while the blocks load, so the
//      pad element, which lies in the last block, costs no pass of its own;
//   B. the levels above one block are merge-path passes (merge_path.h: merge_path_levels<true>) between the ping and the pong line;
//      the last pass parks its output too, in the line it would have written next.  Ties leave in any order: the readout is
//      invariant under that;
//   C. the sorted line is read out at all F frequencies in batches of kFB.  Per batch the workgroup walks the parked line in tiles
//      of 256 threads x 16 consecutive ranks: the float64 cumulative weight before a thread's first element comes from a workgroup
//      scan and carries from tile to tile, then every frequency of the batch adds its sine differences
//        out[r, s F + f] = (1 + xi) / (pi xi) sum_t (sin(2 pi xi c_t) - sin(2 pi xi c_{t-1})) p_(t),   xi = 0: 2 sum_t w_(t) p_(t) / max(m, tau),
//      phase in float64, sine in float32 (sin2pi_rev), into the thread's kFB sums.  One workgroup reduction per batch as in
//      k_cart_hub_w: wave sums into a double-buffered LDS table, ONE barrier, lanes 0 .. kFB - 1 of wavefront 0 store a contiguous run.
// The order of summation of a line is fixed, so the output does not depend on how many workgroups share the rows.
// Unit weights: embed_giant_cart.hip.  The classes and the scratch lines: embed_cart.h.
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "hub_line.h"
#include "merge_path.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

struct CartGiantW {
  const int32_t* rowptr;
  const int32_t* col;
  const float* w;                 // null with tau > 1: every weight is 1
  const int32_t* perm;
  const int32_t* bin_start;
  const float* Xp;
  int64_t ldp;
  const float* freqs;
  int S, F;
  float tau;
  float* out;
  int64_t ldo;
  const float* bias;
  float out_scale;
  int has_mass, mass_fn;
  float mass_scale;
  float* scratch;
  int64_t line_cap;         // elements of each of a workgroup's four scratch lines: a multiple of kMpBlk, > the longest row
  int bin, min_degree;      // the rows: perm[bin_start[bin] ..] with at least min_degree neighbours
};

static_assert(kCartGiantWBlk == kMpBlk, "the block of embed_cart.h is the block of merge_path.h");

__global__ void __launch_bounds__(kMpNT, 2) k_cart_mergepath_w(const CartGiantW a) {
  constexpr int NW = 4, M = kCartLongM, CAP = M * kWave;
  static_assert(NW * CAP == kMpBlk && NW * kWave == kMpNT, "block = one workgroup's registers");
  extern __shared__ __attribute__((aligned(16))) float xsm[];   // phase A: keys [NW][CAP] | weights [NW][CAP]; levels: tiles | boundaries
  __shared__ double redd[NW];             // wavefront totals of the weights
  __shared__ float red[2][kFB][NW];       // wave sums of a batch of frequencies, double-buffered
  float* xk = xsm;
  float* xw = xsm + NW * CAP;
  float* tk = xsm;
  float* tw = xsm + kMpTileLds;
  int* part = reinterpret_cast<int*>(xsm + 2 * kMpTileLds);
  const int pbeg = a.bin_start[a.bin], nrows = a.bin_start[FSW_NUM_BINS] - pbeg;
  const int lane = lane_id(), w = wave_id();
  const int S = a.S, F = a.F;
  const int blk = xcd_first_line();
  float* k0 = a.scratch + (int64_t)blk * 4 * a.line_cap;
  float* k1 = k0 + a.line_cap;
  float* w0 = k1 + a.line_cap;
  float* w1 = w0 + a.line_cap;
  const int64_t nlines = (int64_t)nrows * S;
  const double taud = (double)a.tau;
  MpStamps st{};                                            // phase stamps of merge_path_levels (compiled out: merge_path.h)
  st.start();
  for (int64_t line = blk; line < nlines; line += gridDim.x) {
    const int node = a.perm[pbeg + (int)(line / S)], s = (int)(line % S);
    const int start = a.rowptr[node];
    const int D = a.rowptr[node + 1] - start;
    const int Dtot = D + 1;                                 // with the pad element
    const int nb = (Dtot + kMpBlk - 1) / kMpBlk;
    // a row of another class in this bin, or one longer than the host's max_degree, which sized the lines (workgroup-uniform)
    if (D < a.min_degree || (int64_t)nb * kMpBlk > a.line_cap) continue;
    // A. blocks; the row's mass from the weights as the blocks load them (the pad element is element D = in the LAST block)
    double pm = 0.0, m = 0.0;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
      WaveLine<M, true> ln;
      const int t0 = b * kMpBlk + w * CAP;
#pragma unroll
      for (int h = 0; h < M; h += 16) {                     // two batches of 16 gathers: the index registers are the budget
        int c[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int t = t0 + (h + j) * kWave + lane;
          c[j] = t < D ? a.col[start + t] : -1;
          ln.w[h + j] = t < D ? (a.w ? a.w[start + t] : 1.f) : 0.f;
          pm += (double)ln.w[h + j];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) ln.k[h + j] = c[j] >= 0 ? a.Xp[(int64_t)c[j] * a.ldp + s] : __builtin_inff();
      }
      if (b == nb - 1) {                                   // every weight of the row has been read: its mass, then the pad element
        pm = wave_sum(pm);
        if (lane == 0) redd[w] = pm;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NW; ++q) m += redd[q];
        __syncthreads();
        const float padw = (float)fmax(taud - m, 0.0);     // zero weight unless the row is deficient (its residual: below)
#pragma unroll
        for (int j = 0; j < M; ++j)
          if (t0 + j * kWave + lane == D) {
            ln.k[j] = 0.f;
            ln.w[j] = padw;
          }
      }
      ln.sort();
#pragma unroll
      for (int size = 2; size <= NW; size <<= 1) {
        wave_exchange_w<M>(ln, xk, xw, w, lane, w ^ (size - 1), true, (w & (size >> 1)) == 0);
        for (int stride = size >> 2; stride >= 1; stride >>= 1) wave_exchange_w<M>(ln, xk, xw, w, lane, w ^ stride, false, (w & stride) == 0);
        ln.merge_chunk();
      }
      const int64_t o = (int64_t)b * kMpBlk + w * CAP + lane * M;
#pragma unroll
      for (int j = 0; j < M; j += 4) {
        *reinterpret_cast<float4*>(k0 + o + j) = make_float4(ln.k[j], ln.k[j + 1], ln.k[j + 2], ln.k[j + 3]);
        *reinterpret_cast<float4*>(w0 + o + j) = make_float4(ln.w[j], ln.w[j + 1], ln.w[j + 2], ln.w[j + 3]);
      }
    }
    const double inv = 1.0 / fmax(m, taud);
    // must be the float that phase A stored as the pad element's weight (padw above: the same expression of the same m)
    const double rho = pad_residual(taud - m, (float)fmax(taud - m, 0.0));   // what the float line loses of the pad weight (fsw_common.h)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    // B. merge-path levels; level i reads the line that level i - 1 wrote, so the last of `levels` writes the pong line when levels is odd
    int levels = 0;
    for (int r = 1; r < nb; r <<= 1) ++levels;              // nb >= 2: lines of this class have more than one block
    float* fk = (levels & 1) ? k1 : k0;
    float* fw = (levels & 1) ? w1 : w0;
    merge_path_levels<true>(k0, k1, w0, w1, nb, tk, tw, part, [&](int r0, const float* ok, const float* ow) {
#pragma unroll
      for (int j = 0; j < kMpVT; j += 4) {
        *reinterpret_cast<float4*>(fk + r0 + j) = make_float4(ok[j], ok[j + 1], ok[j + 2], ok[j + 3]);
        *reinterpret_cast<float4*>(fw + r0 + j) = make_float4(ow[j], ow[j + 1], ow[j + 2], ow[j + 3]);
      }
    }, st);
    // C. readout: thread tid of tile i reads the ranks i * kMpTile + tid * kMpVT .. + kMpVT - 1 -- the places it stored itself
    float* orow = a.out + (int64_t)node * a.ldo;
    const int64_t c0 = (int64_t)a.has_mass + (int64_t)s * F;
    const int ntiles = (Dtot + kMpTile - 1) / kMpTile;      // the tiles beyond hold fill elements only (key +inf, weight 0)
    int buf = 0;
    for (int f0 = 0; f0 < F; f0 += kFB, buf ^= 1) {
      const int nf = min(kFB, F - f0);
      float acc[kFB];
#pragma unroll
      for (int q = 0; q < kFB; ++q) acc[q] = 0.f;
      double carry = 0.0;                                   // the cumulative weight before the tile
#pragma unroll 1
      for (int i = 0; i < ntiles; ++i) {
        const int r0 = i * kMpTile + (int)threadIdx.x * kMpVT;
        float kk[kMpVT], ww[kMpVT];
#pragma unroll
        for (int j = 0; j < kMpVT; j += 4) {
          const float4 x = *reinterpret_cast<const float4*>(fk + r0 + j);
          const float4 y = *reinterpret_cast<const float4*>(fw + r0 + j);
          kk[j] = x.x; kk[j + 1] = x.y; kk[j + 2] = x.z; kk[j + 3] = x.w;
          ww[j] = y.x; ww[j + 1] = y.y; ww[j + 2] = y.z; ww[j + 3] = y.w;
        }
        double lsum = 0.0;
#pragma unroll
        for (int j = 0; j < kMpVT; ++j) {
          if (r0 + j >= Dtot) kk[j] = 0.f;                  // fill elements: weight 0, and no inf in the sums
          lsum += (double)ww[j];
        }
        double cw0 = wave_exclusive_scan_f64(lsum);
        const double wtot = __shfl(cw0 + lsum, kWave - 1);  // this wavefront's total
        if (lane == 0) redd[w] = wtot;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < NW; ++q) {
          if (q < w) cw0 += redd[q];
          tot += redd[q];
        }
        __syncthreads();                                    // redd is rewritten by the next tile
        cw0 += carry;
        carry += tot;
#pragma unroll
        for (int q = 0; q < kFB; ++q) {
          if (q < nf) {
#include "readout_weighted.inc"
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kFB; ++q) {
        if (q < nf) {
          const float tot = wave_sum(acc[q]);
          if (lane == 0) red[buf][q][w] = tot;
        }
      }
      __syncthreads();
      // the batch before the previous one used this buffer: every wavefront has passed a barrier since wavefront 0 read it
      if (w == 0 && lane < nf) {
        float val = 0.f;
#pragma unroll
        for (int u = 0; u < NW; ++u) val += red[buf][lane][u];
        const float xif = a.freqs[f0 + lane];
        const double xi = (double)xif;
        val *= fabsf(xif) < 1e-30f ? 2.f * (float)inv : (float)((1.0 + xi) / (kPi * xi));
        const int64_t c = c0 + f0 + lane;
        orow[c] = a.out_scale * (val + (a.bias ? a.bias[c] : 0.f));
      }
    }
    if (a.has_mass && s == 0 && w == 0 && lane == 0) orow[0] = mass_column((float)m, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
    // the next line's blocks overwrite the scratch lines that other threads' merge tiles read: every wavefront has left the levels
    __syncthreads();
  }
}

}  // namespace

// general weights: the rows of the giant class of kCartLong[1], as many workgroups as c->scratch holds lines
int launch_cart_giant_w(const fsw_cart_args* c, hipStream_t stream) {
  const CartLongMode& m = kCartLong[1];
  int64_t nwg;
  size_t line_bytes;
  if (const int rc = cart_giant_plan(c, m, &nwg, &line_bytes)) return rc;
  if (nwg == 0) return 0;
  CartGiantW t;
  cart_fill_inputs_w(t, c);
  cart_fill_outputs(t, c);
  t.scratch = (float*)c->scratch; t.line_cap = (int64_t)(line_bytes / (4 * sizeof(float)));
  t.bin = m.giant_bin; t.min_degree = m.giant_min_degree;
  const size_t lds = sizeof(float) * 2 * 4 * kCartLongM * kWave;   // phase A's (key, weight) exchange buffers; the tiles + boundaries fit inside
  static_assert(sizeof(float) * 2 * kMpTileLds + sizeof(int) * (kMpParts + 1) <= sizeof(float) * 2 * 4 * kCartLongM * kWave, "LDS of the merge levels");
  FSW_SET_MAX_LDS_ONCE((&k_cart_mergepath_w), lds);        // 64 KB of dynamic LDS + the kernel's static words
  k_cart_mergepath_w<<<(unsigned)nwg, kMpNT, lds, stream>>>(t);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace fsw
