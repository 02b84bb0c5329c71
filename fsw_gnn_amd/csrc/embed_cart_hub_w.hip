// Cartesian slice x frequency mode, general weights (w != NULL or tau > 1), lines of 2049 .. FSW_CART_W_MAX_LINE elements: forward.  gfx950.
//
// The weighted counterpart of k_cart_hub (embed_cart_hub.hip), built from the diagonal k_embed_hub_w (embed_hub.hip; building blocks
// in hub_line.h and wave_sort.h): one workgroup of NW = 2, 4 or 8 wavefronts takes ONE (recipient row, slice) line of
// L = D + 1 <= NW * 2048 elements -- the D neighbours (key, weight) and the reference's pad element (key 0, weight max(tau - m, 0),
// fsw_embedding.py:1000-1017) as element D -- and keeps it in registers as WaveLine<32, true>.  Every wavefront gathers and sorts its
// chunk, the merge levels above one chunk exchange keys and weights through LDS (wave_exchange_w).  The sort is paid once per slice:
// the float64 cumulative weight before each lane's first element is formed once per line (lane sum -> wave scan -> wavefront
// offsets) and the lane's 32 elements are then read out at all F frequencies in the sine-difference form of k_embed_hub_w,
//   out[r, s F + f] = (1 + xi) / (pi xi) sum_t (sin(2 pi xi c_t) - sin(2 pi xi c_{t-1})) p_(t),   xi = 0: 2 sum_t w_(t) p_(t) / max(m, tau),
// phase in float64, sine in float32 (sin2pi_rev).  The F sums of a line are reduced over the workgroup as in k_cart_hub: batches of
// kFB frequencies per barrier in a double-buffered LDS table, lanes 0 .. kFB - 1 of wavefront 0 store a contiguous run of outputs.
// Nothing of the line goes to global memory and the kernel needs no scratch.
// The classes follow the line length, not the degree bins (cut at D = 2048, 4096, ...): each class is launched over the two bins it
// touches with a workgroup-uniform dlo < D <= dhi filter, as launch_hub_w does.  Rows of FSW_CART_W_MAX_LINE neighbours and more: the
// giant class (embed_cart.h; embed_giant_cart_w.hip, backward embed_giant_cart_bwd.hip).
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "hub_line.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

struct CartHubW {
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
};

// rows perm[bin_start[bin_lo] .. bin_start[bin_hi + 1] - 1] with dlo < D <= dhi; dhi + 1 <= NW * M * 64
template <int NW, int M>
__global__ void __launch_bounds__(NW* kWave, 2) k_cart_hub_w(const CartHubW a, int bin_lo, int bin_hi, int dlo, int dhi) {
  static_assert(NW >= 2 && NW <= kFB, "one line across 2 .. 16 wavefronts");
  constexpr int CAP = M * kWave;
  extern __shared__ __attribute__((aligned(16))) float xsm[];   // exchange buffers: keys [NW][CAP] | weights [NW][CAP]
  float* xk = xsm;
  float* xw = xsm + NW * CAP;
  __shared__ double redd[NW];             // wavefront totals of the weights
  __shared__ float red[2][kFB][NW];       // wave sums of a batch of frequencies, double-buffered
  const int pbeg = a.bin_start[bin_lo], nrows = a.bin_start[bin_hi + 1] - pbeg;
  const int lane = lane_id(), w = wave_id();
  const int S = a.S, F = a.F;
  const double taud = (double)a.tau;
  const int xcd = blockIdx.x & 7;
  for (int64_t vb = blockIdx.x;; vb += gridDim.x) {
    const auto [r, s] = hub_virtual_line(vb, xcd, 1, S);
    if (r >= nrows) return;                 // the whole workgroup leaves
    const int node = a.perm[pbeg + r];
    const int start = a.rowptr[node];
    const int D = a.rowptr[node + 1] - start;
    if (D <= dlo || D > dhi) continue;      // not a row of this class (workgroup-uniform)
    const int Dtot = D + 1;                 // with the pad element; Dtot <= NW * CAP by the class bounds

    // gather (striped: element t0 + j * 64 + lane), total mass, pad element: as k_embed_hub_w
    WaveLine<M, true> ln;
    const int t0 = w * CAP;
    {
      int c[M];
      double part = 0.0;
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const int t = t0 + j * kWave + lane;
        c[j] = t < D ? a.col[start + t] : -1;
        ln.w[j] = t < D ? (a.w ? a.w[start + t] : 1.f) : 0.f;
        part += (double)ln.w[j];
      }
#pragma unroll
      for (int j = 0; j < M; ++j) ln.k[j] = c[j] >= 0 ? a.Xp[(int64_t)c[j] * a.ldp + s] : __builtin_inff();
      part = wave_sum(part);
      if (lane == 0) redd[w] = part;
    }
    __syncthreads();
    double m = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) m += redd[q];
    __syncthreads();
    const double inv = 1.0 / fmax(m, taud);
    const float padw = (float)fmax(taud - m, 0.0);             // zero weight unless the row is deficient
    const double rho = pad_residual(taud - m, padw);           // what the float line loses of it (fsw_common.h)
    {
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
      for (int st = size >> 2; st >= 1; st >>= 1) wave_exchange_w<M>(ln, xk, xw, w, lane, w ^ st, false, (w & st) == 0);
      ln.merge_chunk();
    }
    // element (w, lane, j) has rank r0 + j; cw0: the cumulative weight before the lane's first element, once per line
    const int r0 = w * CAP + lane * M;
    double lsum = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) lsum += (double)ln.w[j];
    double cw0 = wave_exclusive_scan_f64(lsum);
    {
      const double wtot = __shfl(cw0 + lsum, kWave - 1);       // this wavefront's total
      if (lane == 0) redd[w] = wtot;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NW; ++q)
        if (q < w) cw0 += redd[q];
      // redd is next written by the following line, after the barriers of this readout and of its own exchanges
    }
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (r0 + j >= Dtot) ln.k[j] = 0.f;                        // fill elements: weight 0, and no inf in the sums

    float* orow = a.out + (int64_t)node * a.ldo;
    const int64_t c0 = (int64_t)a.has_mass + (int64_t)s * F;
    int buf = 0;
    for (int f0 = 0; f0 < F; f0 += kFB, buf ^= 1) {
      const int nf = min(kFB, F - f0);
      for (int q = 0; q < nf; ++q) {
        const float xif = a.freqs[f0 + q];
        float acc = 0.f;
        if (fabsf(xif) < 1e-30f) {                                     // xi == 0: Delta_t = 2 w_t / max(m, tau)
#pragma unroll
          for (int j = 0; j < M; ++j) acc = fmaf(ln.w[j], ln.k[j], acc);
        } else {
          const double xi = (double)xif;
          double cw = cw0;
          // the element before a key >= 0 is the pad element, or lies behind it, or multiplies a zero key: same residual
          float sprev = sin2pi_rev(xi * ((cw + pad_residual_at(rho, ln.k[0])) * inv));
#pragma unroll
          for (int j = 0; j < M; ++j) {
            cw += (double)ln.w[j];
            const float sn = sin2pi_rev(xi * ((cw + pad_residual_at(rho, ln.k[j])) * inv));
            acc = fmaf(sn - sprev, ln.k[j], acc);
            sprev = sn;
          }
        }
        const float tot = wave_sum(acc);
        if (lane == 0) red[buf][q][w] = tot;
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
    // the next line's mass reduction (a barrier pair) separates its first batch from this line's last two
  }
}

template <int NW>
int launch_cart_hub_w_class(const CartHubW& t, const CartLongClass& k, int64_t rows, hipStream_t stream) {
  constexpr int M = kCartLongM;
  const size_t lds = sizeof(float) * 2 * NW * M * kWave;
  if (lds + 2048 > 64 * 1024) FSW_SET_MAX_LDS_ONCE((&k_cart_hub_w<NW, M>), lds);   // the kernel's static LDS comes on top of the 64 KB default
  k_cart_hub_w<NW, M><<<cart_hub_grid(rows, t.S), NW * kWave, lds, stream>>>(t, k.bin_lo, k.bin_hi, k.dlo, k.dhi);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// general weights: one launch per class of kCartLong[1] that the graph can have rows of
int launch_cart_hub_w(const fsw_cart_args* c, hipStream_t stream) {
  const int32_t* bs = c->bin_start_host;
  CartHubW t;
  cart_fill_inputs_w(t, c);
  cart_fill_outputs(t, c);
  constexpr decltype(&launch_cart_hub_w_class<2>) launch[] = {launch_cart_hub_w_class<2>, launch_cart_hub_w_class<4>,
                                                              launch_cart_hub_w_class<8>};   // class i: 2 << i wavefronts
  const CartLongMode& m = kCartLong[1];
  for (int i = 0; i < m.num; ++i) {
    const int64_t rows = (int64_t)bs[m.cls[i].bin_hi + 1] - bs[m.cls[i].bin_lo];
    if (rows <= 0 || c->max_degree <= m.cls[i].dlo) continue;
    if (const int rc = launch[i](t, m.cls[i], rows, stream)) return rc;
  }
  return 0;
}

}  // namespace fsw
