// Cartesian slice x frequency mode, hub rows with unit weights (FSW_LDS_MAX_DEG < in-degree <= FSW_HUB_MAX_DEG): forward.  gfx950.
//
// The line-in-registers structure of the diagonal hub kernels (embed_hub.hip, building blocks in hub_line.h): one workgroup of
// NW = 2, 4, 8 or 16 wavefronts takes ONE (recipient row, slice) line of up to NW * 2048 keys, wavefront w holds elements
// w * 2048 .. w * 2048 + 2047 (32 per lane), every wavefront gathers and sorts its chunk and the merge levels above one chunk
// exchange registers through LDS.  The sort is paid once per slice; the sorted registers are then read out at all F frequencies
// (unit_readout: one float64 FMA per key and frequency).  The F sums of a line are reduced over the workgroup in batches of kFB
// frequencies per barrier: every wavefront drops its kFB wave sums into an LDS table, ONE barrier, then lane f of the batch adds
// the NW partials and the batch's outputs leave as one contiguous run.  The table is double-buffered, so no second barrier frees
// it.  Nothing of the line goes to global memory and the kernel needs no scratch.
// The rows above FSW_HUB_MAX_DEG stay on the generic kernel (embed_cart.h); general weights: embed_cart_hub_w.hip.
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "hub_line.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

constexpr int kCartHubM = 32;     // keys per lane
constexpr int kFB = 16;           // frequencies per synchronisation of the readout

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
  // virtual block -> (row, slice) as in k_embed_hub: the blocks b, b + 8, b + 16, ... (one XCD under round-robin dispatch) take the
  // slices 0 .. S - 1 of row xcd, then of row xcd + 8, ...; the grid is capped, a multiple of 8, and strides over the virtual blocks
  const int xcd = blockIdx.x & 7;
  for (int64_t vb = blockIdx.x;; vb += gridDim.x) {
    const int64_t i = vb >> 3;
    const int64_t rl = i / S;
    const int s = (int)(i - rl * S);
    const int64_t r = rl * 8 + xcd;
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
int launch_cart_hub_bin(const CartHub& t, int bin, int64_t rows, hipStream_t stream) {
  if (rows <= 0) return 0;
  // virtual blocks = (rows rounded up to 8) x slices; the launched grid is capped at 2^20 workgroups and strides
  const int64_t nvirtual = ceil_div(rows, 8) * t.S * 8;
  const int64_t nblocks = std::min<int64_t>(nvirtual, 1ll << 20);
  k_cart_hub<NW, kCartHubM><<<(unsigned)nblocks, NW * kWave, 0, stream>>>(t, bin);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// unit weights with tau <= 1: the rows of the four hub bins, one launch per populated bin (bin FSW_BIN_HUB0 + i: NW = 2 << i)
int launch_cart_hub(const fsw_cart_args* c, hipStream_t stream) {
  const int32_t* bs = c->bin_start_host;
  CartHub t;
  t.rowptr = c->rowptr; t.col = c->col; t.perm = c->perm; t.bin_start = c->bin_start;
  t.Xp = (const float*)c->Xp; t.ldp = c->ldp; t.freqs = (const float*)c->freqs; t.S = c->S; t.F = c->F;
  t.out = (float*)c->out; t.ldo = c->ldo; t.bias = (const float*)c->bias; t.out_scale = (float)c->out_scale;
  t.has_mass = c->has_mass; t.mass_fn = c->mass_fn; t.mass_scale = (float)c->mass_scale;
  int rc;
  if ((rc = launch_cart_hub_bin<2>(t, FSW_BIN_HUB0, (int64_t)bs[FSW_BIN_HUB0 + 1] - bs[FSW_BIN_HUB0], stream))) return rc;
  if ((rc = launch_cart_hub_bin<4>(t, FSW_BIN_HUB0 + 1, (int64_t)bs[FSW_BIN_HUB0 + 2] - bs[FSW_BIN_HUB0 + 1], stream))) return rc;
  if ((rc = launch_cart_hub_bin<8>(t, FSW_BIN_HUB0 + 2, (int64_t)bs[FSW_BIN_HUB0 + 3] - bs[FSW_BIN_HUB0 + 2], stream))) return rc;
  return launch_cart_hub_bin<16>(t, FSW_BIN_HUB0 + 3, (int64_t)bs[FSW_BIN_HUB0 + 4] - bs[FSW_BIN_HUB0 + 3], stream);
}

}  // namespace fsw
