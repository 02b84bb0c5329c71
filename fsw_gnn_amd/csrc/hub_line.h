// Building blocks of the kernels that keep ONE (row, slice) line of a hub row (FSW_LDS_MAX_DEG < in-degree) in the registers of the
// NW wavefronts of a workgroup: the striped gather of a wavefront's chunk, the register exchange between wavefronts through LDS, the
// bitonic merge levels above one chunk and the unit-weight readout of a lane's keys; for lines longer than the registers, the parked
// blocks of a scratch line and the line loop per XCD.  Shared by the diagonal kernels of embed_hub.hip (k_embed_hub, k_embed_hub_q4,
// k_embed_giant; general weights: k_embed_hub_w, k_embed_mergepath_w) and embed_wsort.hip (k_embed_wsort_global) and the Cartesian ones
// of embed_cart_hub.hip (k_cart_hub), embed_cart_hub_w.hip (k_cart_hub_w), embed_giant_cart.hip (k_cart_giant), embed_split_cart.hip
// (k_split_sort, k_split_sweep, k_split_tail), embed_giant_cart_w.hip (k_cart_mergepath_w), embed_split_cart_w.hip (k_splitw_sort) and
// embed_giant_cart_bwd.hip (k_cart_giant_bwd).  gfx950.
#pragma once
#include "fsw_common.h"
#include "wave_sort.h"

namespace fsw {

#ifndef FSW_HUB_ABL
#define FSW_HUB_ABL 0   // timing experiments (tools/exp_hub.sh): 1 no gather, 2 no wave sort, 4 no cross-wave merge, 8 no readout
#endif

// register exchange between the wavefronts of a workgroup through xbuf [NW][CAP]: this wavefront keeps, element by
// element, the smaller (lower) or larger key of (its own, wavefront `partner`'s -- same element, or mirrored)
template <int M>
__device__ __forceinline__ void wave_exchange(WaveLine<M, false>& ln, float* __restrict__ xbuf, int w, int lane, int partner,
                                              bool mirrored, bool lower) {
  constexpr int CAP = M * kWave;
  // one base register per side and immediate offsets j * 256 B: the asm statements keep the compiler from folding the lane
  // term into 32 separate per-element addresses (v_bitop3 of lane ^ constant), which it then hoists out of loops and spills.
  // The OFFSET is laundered, not the pointer: an opaque pointer loses its LDS address space and every access became a
  // flat_load / flat_store (72 of each in k_embed_hub<4, 24>: the flat path counts on vmcnt AND lgkmcnt, so each exchange also
  // waited for the wavefront's outstanding gathers)
  int moff = w * CAP + lane;
  asm volatile("" : "+v"(moff));
  float* mine = xbuf + moff;
#pragma unroll
  for (int j = 0; j < M; ++j) mine[j * kWave] = ln.k[j];
  __syncthreads();
  int toff = partner * CAP + (mirrored ? kWave - 1 - lane : lane);
  asm volatile("" : "+v"(toff));
  const float* theirs = xbuf + toff;
  const float lim = lower ? -__builtin_inff() : __builtin_inff();   // wave-uniform: min below the partner, max above it
#pragma unroll
  for (int j = 0; j < M; ++j) ln.k[j] = minmax_by_limit(ln.k[j], theirs[(mirrored ? M - 1 - j : j) * kWave], lim);
  __syncthreads();   // everybody has read: the buffer may be overwritten by the next exchange
}

// the same exchange for a (key, weight) line through xk | xw [NW][CAP] each: the weight follows its key (embed_hub.hip: k_embed_hub_w,
// k_embed_mergepath_w; embed_cart_hub_w.hip: k_cart_hub_w; embed_giant_cart_w.hip: k_cart_mergepath_w)
template <int M>
__device__ __forceinline__ void wave_exchange_w(WaveLine<M, true>& ln, float* __restrict__ xk, float* __restrict__ xw, int w, int lane,
                                                int partner, bool mirrored, bool lower) {
  constexpr int CAP = M * kWave;
  int moff = w * CAP + lane;                               // the offset is laundered, not the pointers (see wave_exchange)
  asm volatile("" : "+v"(moff));
  float* mk = xk + moff;
  float* mw = xw + moff;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    mk[j * kWave] = ln.k[j];
    mw[j * kWave] = ln.w[j];
  }
  __syncthreads();
  int off = partner * CAP + (mirrored ? kWave - 1 - lane : lane);
  asm volatile("" : "+v"(off));
  const float* tk = xk + off;
  const float* tw = xw + off;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int jj = (mirrored ? M - 1 - j : j) * kWave;
    const float ok = tk[jj], ow = tw[jj];
    const bool take = lower ? (ok < ln.k[j]) : (ok > ln.k[j]);   // ties: both wavefronts keep their own element
    ln.k[j] = take ? ok : ln.k[j];
    ln.w[j] = take ? ow : ln.w[j];
  }
  __syncthreads();
}

// NW sorted chunks (one per wavefront, after WaveLine::sort) -> the workgroup's NW * CAP keys sorted; element (lane, j) of
// wavefront w then has rank w * CAP + lane * M + j
template <int NW, int M>
__device__ __forceinline__ void workgroup_merge_levels(WaveLine<M, false>& ln, float* __restrict__ xbuf, int w, int lane) {
#pragma unroll
  for (int size = 2; size <= ((FSW_HUB_ABL & 4) ? 0 : NW); size <<= 1) {
    wave_exchange<M>(ln, xbuf, w, lane, w ^ (size - 1), true, (w & (size >> 1)) == 0);        // element E against E ^ (size * CAP - 1)
    for (int st = size >> 2; st >= 1; st >>= 1) wave_exchange<M>(ln, xbuf, w, lane, w ^ st, false, (w & st) == 0);
    ln.merge_chunk();
  }
}

// the workgroup's NW * CAP keys form a bitonic sequence whose halves were separated elsewhere: finish the merge
template <int NW, int M>
__device__ __forceinline__ void workgroup_merge_block(WaveLine<M, false>& ln, float* __restrict__ xbuf, int w, int lane) {
#pragma unroll
  for (int st = NW >> 1; st >= 1; st >>= 1) wave_exchange<M>(ln, xbuf, w, lane, w ^ st, false, (w & st) == 0);
  ln.merge_chunk();
}

// unit-weight readout of the lane's M keys of ranks r0 .. r0 + M - 1 in a neighbourhood of D: coefficients
// (1 + xi) [sin(2 pi xi (r + 1) / D) - sin(2 pi xi r / D)] / (pi xi) (reference fsw_embedding.py:1047-1075, 1109 with
// weights 1 / D) = B cos(2 pi xi (r + 1/2) / D) by the one-FMA float64 recurrence of UnitCoef (fsw_common.h) started at the
// lane's first rank.  Returns the lane's partial sum.
template <int M, class Line>
__device__ __forceinline__ float unit_readout(const Line& ln, int r0, int D, float xif) {
  const double xi = (double)xif;
  const double inv = 1.0 / (double)D;
  float acc = 0.f;
  if (fabsf(xif) < 1e-30f) {                       // xi == 0: Delta_t = 2 w_t
#pragma unroll
    for (int j = 0; j < M; ++j) acc += (r0 + j < D) ? ln.k[j] : 0.f;
    return acc * 2.f * (float)inv;
  }
  if constexpr (FSW_HUB_ABL & 8) {
#pragma unroll
    for (int j = 0; j < M; ++j) acc += (r0 + j < D) ? ln.k[j] : 0.f;
    return acc;
  }
  UnitCoef uc;
  uc.start(xi, D, r0);
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const float cj = uc.next();
    acc += (r0 + j < D) ? cj * ln.k[j] : 0.f;
  }
  return acc * uc.B;
}

// gather elements t0 + j * 64 + lane (j < M; striped: lane-contiguous col reads -- the chunk is sorted next) of slice k
template <int M>
__device__ __forceinline__ void gather_chunk(WaveLine<M, false>& ln, const int32_t* __restrict__ colrow, int t0, int D,
                                             const float* __restrict__ Xp, int64_t ldp, int k, int lane) {
  int c[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int t = t0 + j * kWave + lane;
    c[j] = t < D ? colrow[t] : -1;
  }
#pragma unroll
  for (int j = 0; j < M; ++j)
    ln.k[j] = c[j] >= 0 ? ((FSW_HUB_ABL & 1) ? (float)((c[j] * 2654435761u) >> 8) : Xp[(int64_t)c[j] * ldp + k]) : __builtin_inff();
}

// Virtual block vb -> (row r of the launch's bins, first slice): the workgroups b, b + 8, b + 16, ... (one XCD under round-robin
// dispatch) walk the slices of row xcd = b & 7, lines_per_block at a time, then those of row xcd + 8, ...  The launched grid is capped, a
// multiple of 8 and strides (vb += gridDim.x), so a workgroup stays on its residue and leaves at its first row past the bins.
struct HubLineId { int64_t r; int s; };
__device__ __forceinline__ HubLineId hub_virtual_line(int64_t vb, int xcd, int lines_per_block, int S) {
  const int64_t i = (vb >> 3) * lines_per_block;
  const int64_t rl = i / S;
  const int s = (int)(i - rl * S);
  return {rl * 8 + xcd, s};
}

// ---- steps of the kernels that keep a line LONGER than the workgroup's registers in a scratch line (k_embed_giant and the giant and
// split forms of Cartesian mode).  Loops, unroll pragmas, readfirstlane and barriers stay with the callers: they are each kernel's tuning.

// First line of a persistent workgroup that strides by gridDim.x: the workgroups of one XCD take consecutive lines (slices of the same
// row) when the grid is a multiple of 8
__device__ __forceinline__ int xcd_first_line() {
  return (gridDim.x & 7) ? (int)blockIdx.x : (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3));
}

// park / fetch the lane's M keys at 16 bytes per access
template <int M>
__device__ __forceinline__ void park_keys(const WaveLine<M, false>& ln, float* dst) {
#pragma unroll
  for (int j = 0; j < M; j += 4) *reinterpret_cast<float4*>(dst + j) = make_float4(ln.k[j], ln.k[j + 1], ln.k[j + 2], ln.k[j + 3]);
}
template <int M>
__device__ __forceinline__ void fetch_keys(WaveLine<M, false>& ln, const float* src) {
#pragma unroll
  for (int j = 0; j < M; j += 4) {
    const float4 v = *reinterpret_cast<const float4*>(src + j);
    ln.k[j] = v.x; ln.k[j + 1] = v.y; ln.k[j + 2] = v.z; ln.k[j + 3] = v.w;
  }
}

// one 16-byte access of an element-wise exchange between two parked blocks of BLK keys: lo[e .. e + 3] against hi[e .. e + 3], or, the
// flip, against hi[BLK - 1 - e ..] mirrored; the smaller keys stay in lo
template <int BLK>
__device__ __forceinline__ void sweep_block_pair(float* lo, float* hi, int e, bool flip) {
  const float4 x = *reinterpret_cast<const float4*>(lo + e);
  float4 y;
  if (flip) {
    const float4 t = *reinterpret_cast<const float4*>(hi + (BLK - 4 - e));
    y = make_float4(t.w, t.z, t.y, t.x);
  } else {
    y = *reinterpret_cast<const float4*>(hi + e);
  }
  const float4 mn = make_float4(fminf(x.x, y.x), fminf(x.y, y.y), fminf(x.z, y.z), fminf(x.w, y.w));
  const float4 mx = make_float4(fmaxf(x.x, y.x), fmaxf(x.y, y.y), fmaxf(x.z, y.z), fmaxf(x.w, y.w));
  *reinterpret_cast<float4*>(lo + e) = mn;
  if (flip) *reinterpret_cast<float4*>(hi + (BLK - 4 - e)) = make_float4(mx.w, mx.z, mx.y, mx.x);
  else *reinterpret_cast<float4*>(hi + e) = mx;
}

}  // namespace fsw
