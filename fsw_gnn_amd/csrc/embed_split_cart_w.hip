// Cartesian slice x frequency mode, general weights (w != NULL or tau > 1), lines of more than FSW_CART_W_MAX_LINE elements: the forward of
// k_cart_mergepath_w (embed_giant_cart_w.hip) with ONE (row, slice) line split over many workgroups.  gfx950.
//
// k_cart_mergepath_w gives a line to one workgroup of four wavefronts, which sorts the line's blocks of kMpBlk (key, weight) elements one
// after the other, merges them level by level and reads the sorted line out: one point cloud at S = 16 keeps 16 workgroups of the chip
// busy.  Here every phase is a launch of its own whose grid covers (line, piece), from the same building blocks (hub_line.h, wave_sort.h,
// merge_path.h):
//   k_splitw_mass     (row, block): the float64 sum of the block's weights into mass[row][b]; the row's mass m is the sum of its pieces in
//                     block order (w == NULL: every weight is 1).  m does not depend on the slice.  The one-workgroup kernel has m "for
//                     free" once it has loaded every block; here the last block of a line needs it before it is sorted, for the pad element
//   k_splitw_sort     (line, block): phase A of k_cart_mergepath_w -- 16 gathers in flight per batch, WaveLine<32, true>, two exchange
//                     levels -- and the block parked in the line's ping region.  The line's last block places the pad element (key 0, weight
//                     max(tau - m, 0)) as element D
//   k_splitw_level    one launch per merge level, (span of tiles, line): level k merges runs of kMpBlk << k elements from the ping region
//                     into the pong region (k even) or back (k odd).  A workgroup finds the boundaries of its own tiles of kMpTile outputs
//                     (merge_path_split in the level's SOURCE region), stages and merges them as merge_path_levels<true> does and copies its
//                     share of a run without a partner.  A line of nb blocks runs ceil(log2 nb) levels and ends in ping when that number is
//                     even, in pong when it is odd.  At a line's LAST level a tile also leaves the float64 sum of its weights in
//                     tsum[line][tile]
//   k_splitw_readout  (tile, line): the cumulative weight before the tile = the sum of the earlier tiles' sums in tile order (float64),
//                     then phase C of k_cart_mergepath_w on the tile at all F frequencies in batches of kFB -- phase in float64, sine in
//                     float32 (sin2pi_rev), the xi = 0 branch, fill ranks >= L contribute nothing -- into partial[line][tile][f]
//   k_splitw_finish   (line, f): the partial sums in tile order, the factor (1 + xi) / (pi xi) or 2 / max(m, tau), bias, out_scale; the
//                     mass column once per row (s == 0)
// Consecutive launches in the caller's stream are the only synchronisation between workgroups: no spin barrier, no cooperative launch,
// no flag in memory, no float atomic.  The grids are sized by the longest row; a workgroup whose block, span, level or tile does not
// exist for ITS line leaves at once (workgroup-uniform, before any barrier), and so does one whose row belongs to the class below, which
// shares the degree bin (k_cart_hub_w has written that row).  Every line owns its regions of the scratch and every word a phase reads was
// written by an earlier phase of the same call, so a line's output depends on the line only: not on S, the other rows, the grid, the span
// or what the scratch held.
// NOT bit-identical to k_cart_mergepath_w: there a thread carries its float32 sums over all tiles of the line and the workgroup adds them
// once; here the float32 sums are formed per tile and added in tile order (and the float64 mass and cumulative weights are added in another
// order).  Both are within the project's bound of the float64 embedding (tests/test_hip_cart_split_w.py).
// The scratch and its query: embed_cart.h (CartSplitWPlan), include/fsw_hip.h (fsw_embed_cart_split_w_scratch_bytes).
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "hub_line.h"
#include "merge_path.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

constexpr int kSplitWMaxSpan = 16;             // tile slots a level workgroup takes at most: boundaries held in LDS
constexpr int kSplitWLevelWg = 1024;           // workgroups a level aims at when it chooses the span (four resident per CU of 256)
constexpr int kSplitWFinishNT = 256;
static_assert(kCartGiantWBlk == kMpBlk && kCartSplitWTile == kMpTile, "the block and the tile of embed_cart.h are those of merge_path.h");

struct CartSplitW {
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
  float* scratch;           // [nlines][4][cap]: keys ping, keys pong, weights ping, weights pong
  int64_t cap;              // a multiple of kMpBlk, > the longest row
  double* tsum;             // [nlines][tiles]
  float* partial;           // [nlines][tiles][F]
  double* mass;             // [rows][nbmax]
  int nbmax, tiles;
  int64_t nlines;
  int bin, min_degree;      // the rows: perm[bin_start[bin] ..] with at least min_degree neighbours
};

struct SplitWRow { int node, start, D, nb; };
// the row (embed_cart.h: cart_row_at) with the blocks of its line of D + 1 elements; false for a row that k_cart_mergepath_w skips too
__device__ __forceinline__ bool splitw_row(const CartSplitW& a, int64_t row, SplitWRow& l) {
  cart_row_at(a, a.bin_start[a.bin] + (int)row, l);
  l.nb = (l.D + 1 + kMpBlk - 1) / kMpBlk;
  return l.D >= a.min_degree && (int64_t)l.nb * kMpBlk <= a.cap;
}
// the row's mass: its pieces in block order
__device__ __forceinline__ double splitw_mass(const CartSplitW& a, int64_t row, int nb) {
  const double* p = a.mass + row * a.nbmax;
  double m = 0.0;
  for (int b = 0; b < nb; ++b) m += p[b];
  return m;
}
// merge levels of a line of nb blocks; the line ends in the pong region when the number is odd
__device__ __forceinline__ int splitw_levels(int nb) {
  int levels = 0;
  for (int r = 1; r < nb; r <<= 1) ++levels;
  return levels;
}

// grid (nbmax, rows)
__global__ void __launch_bounds__(kMpNT) k_splitw_mass(const CartSplitW a) {
  __shared__ double redd[kMpNT / kWave];
  const int b = blockIdx.x;
  const int64_t row = blockIdx.y;
  SplitWRow l;
  if (!splitw_row(a, row, l) || b >= l.nb) return;
  const int t0 = b * kMpBlk, n = max(0, min(l.D - t0, kMpBlk));
  double* dst = a.mass + row * a.nbmax + b;
  if (!a.w) {                                                // kernel-uniform
    if (threadIdx.x == 0) *dst = (double)n;
    return;
  }
  const float* wr = a.w + l.start + t0;
  double pm = 0.0;
#pragma unroll 8
  for (int i = 0; i < kMpBlk / kMpNT; ++i) {
    const int t = i * kMpNT + (int)threadIdx.x;
    pm += t < n ? (double)wr[t] : 0.0;
  }
  pm = wave_sum(pm);
  if (lane_id() == 0) redd[wave_id()] = pm;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = 0.0;
#pragma unroll
    for (int q = 0; q < kMpNT / kWave; ++q) m += redd[q];
    *dst = m;
  }
}

// grid (nbmax, nlines)
__global__ void __launch_bounds__(kMpNT, 2) k_splitw_sort(const CartSplitW a) {
  constexpr int NW = 4, M = kCartLongM, CAP = M * kWave;
  static_assert(NW * CAP == kMpBlk && NW * kWave == kMpNT, "block = one workgroup's registers");
  extern __shared__ __attribute__((aligned(16))) float xsm[];   // keys [NW][CAP] | weights [NW][CAP]
  float* xk = xsm;
  float* xw = xsm + NW * CAP;
  const int b = blockIdx.x;
  const int64_t line = blockIdx.y;
  const int64_t row = line / a.S;
  const int s = (int)(line - row * a.S);
  SplitWRow l;
  if (!splitw_row(a, row, l) || b >= l.nb) return;
  const int lane = lane_id(), w = wave_id();
  const int D = l.D;
  WaveLine<M, true> ln;
  const int t0 = b * kMpBlk + w * CAP;
#pragma unroll
  for (int h = 0; h < M; h += 16) {                          // two batches of 16 gathers: the index registers are the budget
    int c[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int t = t0 + (h + j) * kWave + lane;
      c[j] = t < D ? a.col[l.start + t] : -1;
      ln.w[h + j] = t < D ? (a.w ? a.w[l.start + t] : 1.f) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) ln.k[h + j] = c[j] >= 0 ? a.Xp[(int64_t)c[j] * a.ldp + s] : __builtin_inff();
  }
  if (b == l.nb - 1) {                                       // the pad element is element D = in the LAST block (workgroup-uniform)
    const float padw = (float)fmax((double)a.tau - splitw_mass(a, row, l.nb), 0.0);   // zero weight unless the row is deficient
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
  float* k0 = a.scratch + line * 4 * a.cap;
  float* w0 = k0 + 2 * a.cap;
  const int64_t o = (int64_t)b * kMpBlk + w * CAP + lane * M;
#pragma unroll
  for (int j = 0; j < M; j += 4) {
    *reinterpret_cast<float4*>(k0 + o + j) = make_float4(ln.k[j], ln.k[j + 1], ln.k[j + 2], ln.k[j + 3]);
    *reinterpret_cast<float4*>(w0 + o + j) = make_float4(ln.w[j], ln.w[j + 1], ln.w[j + 2], ln.w[j + 3]);
  }
}

// grid (ceil(2 nbmax / span), nlines): tile slots sp * span .. + span - 1 of level `level` (runs of R = kMpBlk << level elements)
__global__ void __launch_bounds__(kMpNT, 4) k_splitw_level(const CartSplitW a, int level, int span) {
  __shared__ __attribute__((aligned(16))) float tk[kMpTileLds];
  __shared__ __attribute__((aligned(16))) float tw[kMpTileLds];
  __shared__ int part[kSplitWMaxSpan + 1];
  __shared__ double redd[kMpNT / kWave];
  const int64_t line = blockIdx.y;
  SplitWRow l;
  if (!splitw_row(a, line / a.S, l)) return;
  const int total = l.nb * kMpBlk;                            // <= cap <= 2^27
  const int64_t R64 = (int64_t)kMpBlk << level;
  if (R64 >= total) return;                                   // not a level of this line
  const int R = (int)R64;
  const int slots = total / kMpTile;
  const int64_t s064 = (int64_t)blockIdx.x * span;
  if (s064 >= slots) return;                                  // the span lies past the line
  const int s0 = (int)s064, s1 = min(s0 + span, slots);
  const int nruns = (total + R - 1) / R;                      // >= 2
  const bool last = nruns == 2;
  const int covered = (int)min((int64_t)total, (int64_t)(nruns >> 1) * 2 * R);   // elements that belong to a pair of runs
  const unsigned pair_mask = 2u * (unsigned)R - 1u;
  const int ntiles = covered / kMpTile;
  const int g0 = min(s0, ntiles), cnt = min(s1, ntiles) - g0;   // the span's merge tiles g0 .. g0 + cnt - 1
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  float* base = a.scratch + line * 4 * a.cap;
  const bool odd = level & 1;                                 // level k reads what level k - 1 wrote: ping at even levels
  const float* sk = base + (odd ? a.cap : 0);
  float* dk = base + (odd ? 0 : a.cap);
  const float* sw = sk + 2 * a.cap;
  float* dw = dk + 2 * a.cap;
  if (cnt > 0) {                                              // workgroup-uniform
    // elements of A before the start of tiles g0 .. g0 + cnt (0 at the first tile of a pair)
    if (tid <= cnt) {
      const int pos = (g0 + tid) * kMpTile;
      int v = 0;
      if (pos < covered) {
        const int pb = (int)((unsigned)pos & ~pair_mask), d = pos - pb;
        if (d) v = merge_path_split(sk + pb, R, sk + pb + R, min(R, total - pb - R), d);
      }
      part[tid] = v;
    }
    __syncthreads();
    struct TileGeo {
      int pos, pb, a0, b0, na;
    };
    auto geometry = [&](int i) {
      TileGeo t;
      t.pos = (g0 + i) * kMpTile;
      t.pb = (int)((unsigned)t.pos & ~pair_mask);
      const int d0 = t.pos - t.pb;
      const int nB = min(R, total - t.pb - R);
      t.a0 = part[i];
      const int a1 = (d0 + kMpTile >= R + nB) ? R : part[i + 1];   // the pair ends with this tile: all of A is before its end
      t.b0 = d0 - t.a0;
      t.na = a1 - t.a0;
      return t;
    };
    // the tile's elements (A-part, then B-part), element tid + u * 256 in register u: the loads of tile i + 1 are issued before tile i
    // is merged out of LDS
    float pk[kMpVT], pw[kMpVT];
    auto fetch = [&](const TileGeo& t) {
#pragma unroll
      for (int u = 0; u < kMpVT; ++u) {
        const int e = tid + u * kMpNT;
        const int src = e < t.na ? t.pb + t.a0 + e : t.pb + R + t.b0 + (e - t.na);
        pk[u] = sk[src];
        pw[u] = sw[src];
      }
    };
    fetch(geometry(0));
    for (int i = 0; i < cnt; ++i) {
      const TileGeo g = geometry(i);
      const int na = g.na, nbb = kMpTile - g.na;
#pragma unroll
      for (int u = 0; u < kMpVT; ++u) {
        tk[mp_pad(tid + u * kMpNT)] = pk[u];
        tw[mp_pad(tid + u * kMpNT)] = pw[u];
      }
      __syncthreads();
      if (i + 1 < cnt) fetch(geometry(i + 1));
      const int dd = tid * kMpVT;
      int ia = merge_path_split_tile(tk, na, nbb, dd);
      int ib = dd - ia;
      float ok[kMpVT], ow[kMpVT];
      float ka = tk[mp_pad(min(ia, kMpTile - 1))], kb = tk[mp_pad(min(na + ib, kMpTile - 1))];
      float wa = tw[mp_pad(min(ia, kMpTile - 1))], wb = tw[mp_pad(min(na + ib, kMpTile - 1))];
#pragma unroll
      for (int j = 0; j < kMpVT; ++j) {
        const bool ta = ia < na && (ib >= nbb || ka <= kb);     // a value read past the end of its part is never compared
        ok[j] = ta ? ka : kb;
        ow[j] = ta ? wa : wb;
        ia += ta ? 1 : 0;
        ib += ta ? 0 : 1;
        const int nx = mp_pad(min(ta ? ia : na + ib, kMpTile - 1));   // the next element of the part that gave this output
        const float kn = tk[nx], wn = tw[nx];
        ka = ta ? kn : ka;
        kb = ta ? kb : kn;
        wa = ta ? wn : wa;
        wb = ta ? wb : wn;
      }
      float4* ok4 = reinterpret_cast<float4*>(dk + g.pos + dd);
      float4* ow4 = reinterpret_cast<float4*>(dw + g.pos + dd);
#pragma unroll
      for (int j = 0; j < kMpVT; j += 4) {
        ok4[j >> 2] = make_float4(ok[j], ok[j + 1], ok[j + 2], ok[j + 3]);
        ow4[j >> 2] = make_float4(ow[j], ow[j + 1], ow[j + 2], ow[j + 3]);
      }
      if (last) {                                             // the line is sorted: the tile's weight for the readout's cumulative sums
        double lsum = 0.0;
#pragma unroll
        for (int j = 0; j < kMpVT; ++j) lsum += (double)ow[j];
        lsum = wave_sum(lsum);
        if (lane == 0) redd[w] = lsum;
      }
      __syncthreads();                                        // the tile buffers are overwritten next
      if (last && tid == 0) {                                 // redd is rewritten after the next tile's staging barrier
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < kMpNT / kWave; ++q) tot += redd[q];
        a.tsum[line * a.tiles + (g0 + i)] = tot;
      }
    }
  }
  // the span's share of a run without a partner moves on unchanged
  const int c0 = max(s0, ntiles) * kMpTile, c1 = max(s1, ntiles) * kMpTile;
  for (int e = c0 + tid * 4; e < c1; e += kMpNT * 4) {
    *reinterpret_cast<float4*>(dk + e) = *reinterpret_cast<const float4*>(sk + e);
    *reinterpret_cast<float4*>(dw + e) = *reinterpret_cast<const float4*>(sw + e);
  }
}

// grid (tiles, nlines): thread tid reads the ranks i * kMpTile + tid * kMpVT .. + kMpVT - 1 of the sorted line
__global__ void __launch_bounds__(kMpNT, 2) k_splitw_readout(const CartSplitW a) {
  constexpr int NW = kMpNT / kWave;
  static_assert(NW <= kFB, "wavefront 0 sums a batch's wave sums");
  __shared__ double redd[NW];             // wavefront totals of the weights
  __shared__ float red[2][kFB][NW];       // wave sums of a batch of frequencies, double-buffered
  const int i = blockIdx.x;
  const int64_t line = blockIdx.y;
  const int64_t row = line / a.S;
  SplitWRow l;
  if (!splitw_row(a, row, l)) return;
  const int Dtot = l.D + 1;
  if ((int64_t)i * kMpTile >= Dtot) return;                   // the tiles beyond hold fill elements only (key +inf, weight 0)
  const int lane = lane_id(), w = wave_id();
  const int F = a.F;
  const bool odd = splitw_levels(l.nb) & 1;
  const float* fk = a.scratch + line * 4 * a.cap + (odd ? a.cap : 0);
  const float* fw = fk + 2 * a.cap;
  const double m = splitw_mass(a, row, l.nb);
  const double inv = 1.0 / fmax(m, (double)a.tau);
  // must be the float that k_splitw_sort stored as the pad element's weight (padw there: the same expression of the same splitw_mass)
  const double rho = pad_residual((double)a.tau - m, (float)fmax((double)a.tau - m, 0.0));   // what the float line loses of the pad weight (fsw_common.h)
  const double* ts = a.tsum + line * a.tiles;
  double carry = 0.0;                                         // the cumulative weight before the tile
  for (int q = 0; q < i; ++q) carry += ts[q];
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
    if (r0 + j >= Dtot) kk[j] = 0.f;                          // fill elements: weight 0, and no inf in the sums
    lsum += (double)ww[j];
  }
  double cw0 = wave_exclusive_scan_f64(lsum);
  const double wtot = __shfl(cw0 + lsum, kWave - 1);          // this wavefront's total
  if (lane == 0) redd[w] = wtot;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NW; ++q)
    if (q < w) cw0 += redd[q];
  cw0 += carry;
  float* prow = a.partial + (line * a.tiles + i) * (int64_t)F;
  int buf = 0;
  for (int f0 = 0; f0 < F; f0 += kFB, buf ^= 1) {
    const int nf = min(kFB, F - f0);
    float acc[kFB];
#pragma unroll
    for (int q = 0; q < kFB; ++q) {
      acc[q] = 0.f;
      if (q < nf) {
#include "readout_weighted.inc"
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
      prow[f0 + lane] = val;
    }
  }
}

// one thread per (line, f)
__global__ void __launch_bounds__(kSplitWFinishNT) k_splitw_finish(const CartSplitW a) {
  const int64_t idx = (int64_t)blockIdx.x * kSplitWFinishNT + threadIdx.x;
  if (idx >= a.nlines * a.F) return;
  const int64_t line = idx / a.F;
  const int f = (int)(idx - line * a.F);
  const int64_t row = line / a.S;
  const int s = (int)(line - row * a.S);
  SplitWRow l;
  if (!splitw_row(a, row, l)) return;
  const int ntiles = (l.D + 1 + kMpTile - 1) / kMpTile;
  const float* p = a.partial + line * a.tiles * (int64_t)a.F + f;
  float val = 0.f;
  for (int i = 0; i < ntiles; ++i) val += p[(int64_t)i * a.F];
  const double m = splitw_mass(a, row, l.nb);
  const double inv = 1.0 / fmax(m, (double)a.tau);
  const float xif = a.freqs[f];
  const double xi = (double)xif;
  val *= fabsf(xif) < 1e-30f ? 2.f * (float)inv : (float)((1.0 + xi) / (kPi * xi));
  float* orow = a.out + (int64_t)l.node * a.ldo;
  const int64_t c = (int64_t)a.has_mass + (int64_t)s * a.F + f;
  orow[c] = a.out_scale * (val + (a.bias ? a.bias[c] : 0.f));
  if (a.has_mass && s == 0 && f == 0) orow[0] = mass_column((float)m, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
}

}  // namespace

// general weights: the rows of the giant class of kCartLong[1], every line in its own regions of c->scratch
int launch_cart_split_w(const fsw_cart_args* c, const CartSplitWPlan& p, hipStream_t stream) {
  const CartLongMode& m = kCartLong[1];
  if (p.lines <= 0) return 0;
  CartSplitW t;
  cart_fill_inputs_w(t, c);
  cart_fill_outputs(t, c);
  t.scratch = (float*)c->scratch; t.cap = p.cap;
  t.tsum = (double*)((char*)c->scratch + p.tsum_offset);
  t.partial = (float*)((char*)c->scratch + p.partial_offset);
  t.mass = (double*)((char*)c->scratch + p.mass_offset);
  t.nbmax = p.nbmax; t.tiles = p.tiles; t.nlines = p.lines;
  t.bin = m.giant_bin; t.min_degree = m.giant_min_degree;
  // lines * cap * 16 <= 2 GiB with cap >= 3 blocks: lines <= 5461, nbmax <= 16384, tiles <= 32768 -- every grid dimension fits
  k_splitw_mass<<<dim3((unsigned)p.nbmax, (unsigned)p.rows), kMpNT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  const size_t lds = sizeof(float) * 2 * 4 * kCartLongM * kWave;   // the (key, weight) exchange buffers
  FSW_SET_MAX_LDS_ONCE((&k_splitw_sort), lds);                // 64 KB of dynamic LDS
  k_splitw_sort<<<dim3((unsigned)p.nbmax, (unsigned)p.lines), kMpNT, lds, stream>>>(t);
  FSW_LAUNCH_CHECK();
  // the span does not change what a level writes (every tile's boundaries are those of its own diagonals), only how many workgroups share it
  const int span = (int)std::min<int64_t>(kSplitWMaxSpan, std::max<int64_t>(1, p.lines * p.tiles / kSplitWLevelWg));
  const dim3 spans((unsigned)ceil_div(p.tiles, span), (unsigned)p.lines);
  for (int level = 0; ((int64_t)kMpBlk << level) < p.cap; ++level) {
    k_splitw_level<<<spans, kMpNT, 0, stream>>>(t, level, span);
    FSW_LAUNCH_CHECK();
  }
  k_splitw_readout<<<dim3((unsigned)p.tiles, (unsigned)p.lines), kMpNT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  k_splitw_finish<<<(unsigned)ceil_div(p.lines * c->F, kSplitWFinishNT), kSplitWFinishNT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace fsw
