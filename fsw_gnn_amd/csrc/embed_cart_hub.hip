// Cartesian slice x frequency mode, hub rows with unit weights (FSW_LDS_MAX_DEG < in-degree <= FSW_HUB_MAX_DEG): forward.  gfx950.
//
// The line-in-registers structure of the diagonal hub kernels (embed_hub.hip, building blocks in hub_line.h): one workgroup of
// NW = 2, 4, 8 or 16 wavefronts takes ONE (recipient row, slice) line of up to NW * 2048 keys, wavefront w holds elements
// w * 2048 .. (w + 1) * 2048 - 1 (32 per lane), every wavefront gathers and sorts its chunk and the merge levels above one chunk
// exchange registers through LDS.  The sort is paid once per slice; the sorted registers are then read out at all F frequencies
// (unit_readout: one float64 FMA per key and frequency).  The F sums of a line are reduced over the workgroup in batches of kFB
// frequencies per barrier: every wavefront drops its kFB wave sums into an LDS table, ONE barrier, then lane f of the batch adds
// the NW partials and the batch's outputs leave as one contiguous run.  The table is double-buffered, so no second barrier frees
// it.  Nothing of the line goes to global memory and the kernel needs no scratch.
// The rows above FSW_HUB_MAX_DEG: the giant class (embed_cart.h; embed_giant_cart.hip); general weights: embed_cart_hub_w.hip.
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "hub_line.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

struct CartHub {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* perm;
  const int32_t* bin_start;
  const float* Xp;
  int64_t ldp;
  const float* freqs;
  int S, F;
  float* out;
  int64_t ldo;
  const float* bias;
  float out_scale;
  int has_mass, mass_fn;
  float mass_scale;
};

template <int NW, int M>
__global__ void __launch_bounds__(NW* kWave, 4) k_cart_hub(const CartHub a, int bin) {
  static_assert(NW >= 2 && NW <= kFB, "one line across 2 .. 16 wavefronts");
  constexpr int CAP = M * kWave;
  __shared__ float xbuf[NW * CAP];        // exchange buffer: element (lane, j) of wavefront w at xbuf[w * CAP + j * 64 + lane]
  __shared__ float red[2][kFB][NW];       // wave sums of a batch of frequencies, double-buffered
  const int pbeg = a.bin_start[bin], nrows = a.bin_start[bin + 1] - pbeg;
  const int lane = lane_id(), w = wave_id();
  const int S = a.S, F = a.F;
  const int xcd = blockIdx.x & 7;
  for (int64_t vb = blockIdx.x;; vb += gridDim.x) {
    const auto [r, s] = hub_virtual_line(vb, xcd, 1, S);
    if (r >= nrows) return;                 // the whole workgroup leaves
    const int node = a.perm[pbeg + r];
    const int start = a.rowptr[node];
    const int D = a.rowptr[node + 1] - start;
    if (D <= 0 || D > NW * CAP) continue;   // not a row of this class (workgroup-uniform)
    WaveLine<M, false> ln;
    gather_chunk<M>(ln, a.col + start, w * CAP, D, a.Xp, a.ldp, s, lane);
    ln.sort();
    workgroup_merge_levels<NW, M>(ln, xbuf, w, lane);
    const int r0 = w * CAP + lane * M;      // rank of the lane's first key
    float* orow = a.out + (int64_t)node * a.ldo;
    const int64_t c0 = (int64_t)a.has_mass + (int64_t)s * F;
    int buf = 0;
    for (int f0 = 0; f0 < F; f0 += kFB, buf ^= 1) {
      const int nf = min(kFB, F - f0);
      for (int q = 0; q < nf; ++q) {
        const float tot = wave_sum(unit_readout<M>(ln, r0, D, a.freqs[f0 + q]));
        if (lane == 0) red[buf][q][w] = tot;
      }
      __syncthreads();
      // the batch before the previous one used this buffer: every wavefront has passed a barrier since wavefront 0 read it
      if (w == 0 && lane < nf) {
        float val = 0.f;
#pragma unroll
        for (int u = 0; u < NW; ++u) val += red[buf][lane][u];
        const int64_t c = c0 + f0 + lane;
        orow[c] = a.out_scale * (val + (a.bias ? a.bias[c] : 0.f));
      }
    }
    if (a.has_mass && s == 0 && w == 0 && lane == 0) orow[0] = mass_column((float)D, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
    // the next line's exchanges (at least one barrier pair) separate its first batch from this line's last two
  }
}

template <int NW>
int launch_cart_hub_class(const CartHub& t, const CartLongClass& k, int64_t rows, hipStream_t stream) {
  k_cart_hub<NW, kCartLongM><<<cart_hub_grid(rows, t.S), NW * kWave, 0, stream>>>(t, k.bin_lo);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// unit weights with tau <= 1: one launch per populated class of kCartLong[0] (one hub bin each)
int launch_cart_hub(const fsw_cart_args* c, hipStream_t stream) {
  const int32_t* bs = c->bin_start_host;
  CartHub t;
  cart_fill_inputs(t, c);
  cart_fill_outputs(t, c);
  constexpr decltype(&launch_cart_hub_class<2>) launch[] = {launch_cart_hub_class<2>, launch_cart_hub_class<4>, launch_cart_hub_class<8>,
                                                            launch_cart_hub_class<16>};   // class i: 2 << i wavefronts
  const CartLongMode& m = kCartLong[0];
  for (int i = 0; i < m.num; ++i) {
    const int64_t rows = (int64_t)bs[m.cls[i].bin_hi + 1] - bs[m.cls[i].bin_lo];
    if (rows <= 0) continue;
    if (const int rc = launch[i](t, m.cls[i], rows, stream)) return rc;
  }
  return 0;
}

}  // namespace fsw
