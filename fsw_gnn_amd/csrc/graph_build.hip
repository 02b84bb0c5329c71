// Edge list -> CSR by recipient + degree bins.  gfx950.
//
// Replaces FSW_conv.edge_index_to_adj (reference fsw_conv.py:384-447) and the sp.get_slice_info sorts of
// FSW_embedding.forward (reference fsw_embedding.py:778-821).  The reference coalesces and stable-sorts E
// int64 COO keys with torch.sort; here the edges are grouped by recipient with a hand-written stable LSD
// radix sort on the recipient index only (ceil(log2(rows+1)) bits, 7-8 bits per pass):
//   upsweep    per 4096-edge tile: digit histogram (wave-aggregated LDS atomics)
//   scan       exclusive scan of the digit-major [digit][tile] count table = global base of every (tile, digit)
//   downsweep  wave64 match ranking (ballot per digit bit), per-wave digit counters in LDS, tile-local
//              reorder through LDS so the global writes are runs of consecutive addresses per digit
// The first pass reads the int64 edge_index directly (and validates it), later passes move int32 pairs.
// The sort is stable, so every CSR row keeps its senders in edge-list order: the build is deterministic.
// rowptr comes from the boundaries of the sorted keys; rows are then bucketed by in-degree so the fused
// neighbourhood kernels run exact-size sorting networks on runs of equal-degree rows.
// Scratch: one workspace buffer of fsw_graph_workspace_bytes(rows, edges) bytes, laid out by graph_ws.h (key / value ping-pong, the
// count table of a pass, the block sums of the device-wide scan -- sized for the longest scan of any entry point, and the scan checks
// the capacity it is given --, bucket starts, bin counters).
// (A first version used one global int atomic per edge for the histogram and one for the scatter:
//  1.13 ms at 10M edges against ~0.3 ms for the sort -- profiles/r01_v1_bench_kernel_stats.csv.)
#include <algorithm>
#include <atomic>
#include "fsw_common.h"
#include "graph_bins.h" // the device-wide scan and the degree bins, shared with graph_import.hip
#include "graph_ws.h"   // the workspace layout and the tile constants it depends on (host only: also built into a CPU test)
#include "graph_plan.h" // the packed edge word and the plan of the two-level build (host helpers: also built into a CPU test)

namespace fsw {

#ifndef FSW_RS_THREADS
#define FSW_RS_THREADS 512   // 8 wavefronts x 8 rounds per 4096-edge tile (256 x 16: 0.273 -> 0.253 ms for the build at config 3)
#endif
constexpr int kRsThreads = FSW_RS_THREADS;
constexpr int kRsItems = kRsTile / kRsThreads;                   // rounds of 64 consecutive edges per wave (kRsTile = 4096: graph_ws.h)
static_assert(kRsThreads * kRsItems == kRsTile, "a tile is a whole number of rounds");
constexpr int kRsWaves = kRsThreads / kWave;

// Lanes of the wavefront whose digit equals this lane's (wave64 "match any" from one ballot per digit bit).  The lanes that
// differ from me in some bit are accumulated in two 32-bit halves -- per bit one v_bfe, one v_cmp and two or/xor pairs, no
// 64-bit selects and no branches (bits above the digit width are zero in every lane and change nothing).  Inactive lanes
// (ok == false) form a group of their own.
template <int MAXB>
__device__ __forceinline__ unsigned long long match_digit(uint32_t d, bool ok) {
  uint32_t dlo = 0u, dhi = 0u;
#pragma unroll
  for (int b = 0; b < MAXB; ++b) {
    const uint32_t bit = (d >> b) & 1u;
    const unsigned long long bb = __ballot(bit != 0u);
    const uint32_t m = 0u - bit;
    dlo |= (uint32_t)bb ^ m;
    dhi |= (uint32_t)(bb >> 32) ^ m;
  }
  const unsigned long long okm = __ballot(ok);
  const unsigned long long same = ~(((unsigned long long)dhi << 32) | (unsigned long long)dlo);
  return ok ? (same & okm) : ~okm;
}

// ---- radix sort by recipient ----------------------------------------------------------------------------
// Key of edge e: its recipient, or `num_rows` (a sentinel that sorts last) when an endpoint is out of range.
template <bool FIRST>
__device__ __forceinline__ uint32_t load_key(const int64_t* __restrict__ recipients, const int64_t* __restrict__ senders,
                                             const uint32_t* __restrict__ keys_in, int64_t e, int64_t num_rows,
                                             int64_t num_cols, int& flags) {
  if constexpr (FIRST) {
    const int64_t r = recipients[e], c = senders[e];
    if (r < 0 || r >= num_rows || c < 0 || c >= num_cols) {
      flags |= FSW_FLAG_INDEX_RANGE;
      return (uint32_t)num_rows;
    }
    return (uint32_t)r;
  } else {
    return keys_in[e];
  }
}

template <bool FIRST>
__global__ void __launch_bounds__(kRsThreads) k_rs_upsweep(const int64_t* __restrict__ recipients,
                                                           const int64_t* __restrict__ senders,
                                                           const float* __restrict__ edge_w,
                                                           const uint32_t* __restrict__ keys_in, int64_t num_edges,
                                                           int64_t num_rows, int64_t num_cols, int shift, int ndigits,
                                                           int32_t* __restrict__ counts /* [ndigits][ntiles] */, int64_t ntiles,
                                                           int32_t* __restrict__ stats) {
  __shared__ int hist[kRsMaxDigits];
  for (int d = threadIdx.x; d < ndigits; d += kRsThreads) hist[d] = 0;
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * kRsTile;
  const uint32_t mask = (uint32_t)ndigits - 1;
  int flags = 0;
  // half a tile's loads in flight, then its LDS atomics
  constexpr int kHalf = kRsItems / 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint32_t key[kHalf];
#pragma unroll
    for (int i = 0; i < kHalf; ++i) {
      const int64_t e = tile0 + (int64_t)(h * kHalf + i) * kRsThreads + threadIdx.x;
      key[i] = 0xffffffffu;
      if (e < num_edges) {
        key[i] = load_key<FIRST>(recipients, senders, keys_in, e, num_rows, num_cols, flags);
        if (FIRST && edge_w) {
          const float w = edge_w[e];
          if (!(fabsf(w) <= 3.402823466e38f)) flags |= FSW_FLAG_W_NONFINITE;
          if (w < 0.f) flags |= FSW_FLAG_W_NEGATIVE;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kHalf; ++i)
      if (tile0 + (int64_t)(h * kHalf + i) * kRsThreads + threadIdx.x < num_edges) atomicAdd(&hist[(key[i] >> shift) & mask], 1);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < ndigits; d += kRsThreads) counts[(int64_t)d * ntiles + blockIdx.x] = hist[d];
  if (FIRST && flags) atomicOr(&stats[FSW_STAT_FLAGS], flags);
}

// VAL = uint32_t (sender) for unit weights, uint64_t (sender | weight bits << 32) when weights are carried
template <bool FIRST, class VAL, bool EID = false>   // EID: carry the edge id instead of the sender
__global__ void __launch_bounds__(kRsThreads) k_rs_downsweep(const int64_t* __restrict__ recipients,
                                                             const int64_t* __restrict__ senders,
                                                             const float* __restrict__ edge_w,
                                                             const uint32_t* __restrict__ keys_in,
                                                             const VAL* __restrict__ vals_in, int64_t num_edges,
                                                             int64_t num_rows, int64_t num_cols, int shift, int nbits,
                                                             const int32_t* __restrict__ bases /* scanned [ndigits][ntiles] */,
                                                             int64_t ntiles, uint32_t* __restrict__ keys_out,
                                                             VAL* __restrict__ vals_out) {
  __shared__ int wcnt[kRsWaves][kRsMaxDigits];   // per-wave digit counters, then exclusive wave bases
  __shared__ int dstart[kRsMaxDigits];           // tile-local exclusive start of each digit
  __shared__ int gbase[kRsMaxDigits];            // global base of (this tile, digit)
  __shared__ uint32_t skey[kRsTile];
  __shared__ VAL sval[kRsTile];
  const int ndigits = 1 << nbits;
  const uint32_t mask = (uint32_t)ndigits - 1;
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  for (int d = threadIdx.x; d < ndigits; d += kRsThreads) {
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) wcnt[w][d] = 0;
    gbase[d] = bases[(int64_t)d * ntiles + blockIdx.x];
  }
  __syncthreads();

  // wave wv owns tile elements [wv*1024, wv*1024 + 1024) as 16 rounds of 64 consecutive edges (stable order)
  const int64_t wave0 = (int64_t)blockIdx.x * kRsTile + (int64_t)wv * (kRsItems * kWave);
  uint32_t key[kRsItems];
  VAL val[kRsItems];
  int rank[kRsItems];
  int dummy = 0;
  // two half-tiles of 8 rounds: all loads of a half are issued before its first match (the matches are ~60 vector
  // instructions a round; with the loads inside the rounds every round waited for its own HBM access)
  constexpr int kHalf = kRsItems / 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = h * kHalf; i < (h + 1) * kHalf; ++i) {
      const int64_t e = wave0 + (int64_t)i * kWave + lane;
      const bool ok = e < num_edges;
      key[i] = 0xffffffffu;
      val[i] = VAL(0);
      if (ok) {
        key[i] = load_key<FIRST>(recipients, senders, keys_in, e, num_rows, num_cols, dummy);
        if constexpr (FIRST && EID) {
          val[i] = (VAL)(uint32_t)e;
        } else if constexpr (FIRST) {
          const uint32_t s = (uint32_t)senders[e];
          if constexpr (sizeof(VAL) == 8)
            val[i] = (VAL)s | ((VAL)__float_as_uint(edge_w[e]) << 32);
          else
            val[i] = (VAL)s;
        } else {
          val[i] = vals_in[e];
        }
      }
    }
#pragma unroll
    for (int i = h * kHalf; i < (h + 1) * kHalf; ++i) {
      const bool ok = wave0 + (int64_t)i * kWave + lane < num_edges;
      const uint32_t d = (key[i] >> shift) & mask;
      const unsigned long long peers = match_digit<9>(d, ok);
      const int leader = __ffsll((long long)peers) - 1;
      const int below = __popcll(peers & ((1ull << lane) - 1ull));
      int prev = 0;
      if (ok && lane == leader) {
        prev = wcnt[wv][d];
        wcnt[wv][d] = prev + __popcll(peers);
      }
      prev = __shfl(prev, leader);
      rank[i] = prev + below;
    }
  }
  __syncthreads();
  // per digit: exclusive bases across waves and the tile-local digit start
  for (int d = threadIdx.x; d < ndigits; d += kRsThreads) {
    int acc = 0;
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) {
      const int c = wcnt[w][d];
      wcnt[w][d] = acc;
      acc += c;
    }
    dstart[d] = acc;  // tile total for now
  }
  __syncthreads();
  if (threadIdx.x < kWave) {  // exclusive scan of the tile totals over the digits (<= kRsMaxDigits = 8 per lane)
    constexpr int kPer = kRsMaxDigits / kWave;
    int v[kPer], s = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int d = lane * kPer + j;
      v[j] = d < ndigits ? dstart[d] : 0;
      s += v[j];
    }
    int ex = wave_inclusive_scan(s) - s;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int d = lane * kPer + j;
      if (d < ndigits) dstart[d] = ex;
      ex += v[j];
    }
  }
  __syncthreads();
  // tile-local reorder through LDS
#pragma unroll
  for (int i = 0; i < kRsItems; ++i) {
    const int64_t e = wave0 + (int64_t)i * kWave + lane;
    if (e < num_edges) {
      const uint32_t d = (key[i] >> shift) & mask;
      const int lpos = dstart[d] + wcnt[wv][d] + rank[i];
      skey[lpos] = key[i];
      sval[lpos] = val[i];
    }
  }
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * kRsTile;
  const int count = (int)min((int64_t)kRsTile, num_edges - tile0);
  for (int i = threadIdx.x; i < count; i += kRsThreads) {
    const uint32_t k = skey[i];
    const uint32_t d = (k >> shift) & mask;
    const int64_t pos = (int64_t)gbase[d] + (i - dstart[d]);
    keys_out[pos] = k;
    vals_out[pos] = sval[i];
  }
}

// ---- packed partition pass: the only pass of the unit-weight two-level build when an edge fits one word (graph_plan.h) ----------
// The kernels above with two differences: a tile is kPackTile edges, and the downsweep writes ONE uint32 per edge -- the low rb row
// bits and the sender -- into runs that are twice as long.  The digit (= bucket, the row bits from rb upwards) is not part of the
// word, so the tile-local reorder keeps it beside the word in LDS (16 bits).
constexpr int kPackItems = kPackTile / kRsThreads;   // rounds of 64 consecutive edges per wave
constexpr int kPackAhead = 8;                        // rounds whose loads are in flight together
static_assert(kRsThreads * kPackItems == kPackTile && kPackItems % kPackAhead == 0, "a packed tile is a whole number of load groups");
static_assert(kRsMaxDigits <= (1 << 16), "the digit of an edge is kept in 16 bits");
constexpr size_t kPackLdsBytes = sizeof(int) * (size_t)(kRsWaves + 2) * kRsMaxDigits + (sizeof(uint32_t) + sizeof(uint16_t)) * (size_t)kPackTile;

// key of one edge from its two endpoints (load_key<true> on values already loaded)
__device__ __forceinline__ uint32_t key_of(int64_t r, int64_t c, int64_t num_rows, int64_t num_cols, int& flags) {
  if (r < 0 || r >= num_rows || c < 0 || c >= num_cols) {
    flags |= FSW_FLAG_INDEX_RANGE;
    return (uint32_t)num_rows;
  }
  return (uint32_t)r;
}

// VEC: both endpoint arrays are 16-byte aligned (a tile starts at an even edge): a lane reads two consecutive edges with one 16-byte
// load per array.  The histogram needs no order, so which lane counts which edge does not matter.
template <bool VEC>
__global__ void __launch_bounds__(kRsThreads) k_pack_upsweep(const int64_t* __restrict__ recipients, const int64_t* __restrict__ senders,
                                                             int64_t num_edges, int64_t num_rows, int64_t num_cols, int shift, int ndigits,
                                                             int32_t* __restrict__ counts /* [ndigits][ntiles] */, int64_t ntiles,
                                                             int32_t* __restrict__ stats) {
  __shared__ int hist[kRsMaxDigits];
  for (int d = threadIdx.x; d < ndigits; d += kRsThreads) hist[d] = 0;
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * kPackTile;
  const uint32_t mask = (uint32_t)ndigits - 1;
  int flags = 0;
  if constexpr (VEC) {
    constexpr int kPairs = kPackItems / 2, kPairsAhead = kPackAhead / 2;
    static_assert(kPackItems % 2 == 0 && kPairs % kPairsAhead == 0, "pairs of edges in whole load groups");
#pragma unroll
    for (int h = 0; h < kPairs / kPairsAhead; ++h) {
      uint32_t key[kPairsAhead][2];
#pragma unroll
      for (int i = 0; i < kPairsAhead; ++i) {
        const int64_t e = tile0 + 2 * ((int64_t)(h * kPairsAhead + i) * kRsThreads + threadIdx.x);
        key[i][0] = key[i][1] = 0xffffffffu;
        if (e + 1 < num_edges) {
          const longlong2 r = *reinterpret_cast<const longlong2*>(recipients + e);
          const longlong2 c = *reinterpret_cast<const longlong2*>(senders + e);
          key[i][0] = key_of(r.x, c.x, num_rows, num_cols, flags);
          key[i][1] = key_of(r.y, c.y, num_rows, num_cols, flags);
        } else if (e < num_edges) {
          key[i][0] = key_of(recipients[e], senders[e], num_rows, num_cols, flags);
        }
      }
#pragma unroll
      for (int i = 0; i < kPairsAhead; ++i) {
        const int64_t e = tile0 + 2 * ((int64_t)(h * kPairsAhead + i) * kRsThreads + threadIdx.x);
        if (e < num_edges) atomicAdd(&hist[(key[i][0] >> shift) & mask], 1);
        if (e + 1 < num_edges) atomicAdd(&hist[(key[i][1] >> shift) & mask], 1);
      }
    }
  } else {
#pragma unroll
    for (int h = 0; h < kPackItems / kPackAhead; ++h) {
      uint32_t key[kPackAhead];
#pragma unroll
      for (int i = 0; i < kPackAhead; ++i) {
        const int64_t e = tile0 + (int64_t)(h * kPackAhead + i) * kRsThreads + threadIdx.x;
        key[i] = 0xffffffffu;
        if (e < num_edges) key[i] = key_of(recipients[e], senders[e], num_rows, num_cols, flags);
      }
#pragma unroll
      for (int i = 0; i < kPackAhead; ++i)
        if (tile0 + (int64_t)(h * kPackAhead + i) * kRsThreads + threadIdx.x < num_edges) atomicAdd(&hist[(key[i] >> shift) & mask], 1);
    }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < ndigits; d += kRsThreads) counts[(int64_t)d * ntiles + blockIdx.x] = hist[d];
  if (flags) atomicOr(&stats[FSW_STAT_FLAGS], flags);
}

__global__ void __launch_bounds__(kRsThreads) k_pack_downsweep(const int64_t* __restrict__ recipients, const int64_t* __restrict__ senders,
                                                               int64_t num_edges, int64_t num_rows, int64_t num_cols, int rb, int cb,
                                                               int nbits, const int32_t* __restrict__ bases /* scanned [ndigits][ntiles] */,
                                                               int64_t ntiles, uint32_t* __restrict__ words_out) {
  extern __shared__ int psm[];   // wcnt[kRsWaves][kRsMaxDigits] | dstart[kRsMaxDigits] | gbase[kRsMaxDigits] | sword[kPackTile] | sdig[kPackTile]
  int* wcnt = psm;                                       // per-wave digit counters, then exclusive wave bases
  int* dstart = psm + kRsWaves * kRsMaxDigits;           // tile-local exclusive start of each digit
  int* gbase = dstart + kRsMaxDigits;                    // global base of (this tile, digit)
  uint32_t* sword = reinterpret_cast<uint32_t*>(gbase + kRsMaxDigits);
  uint16_t* sdig = reinterpret_cast<uint16_t*>(sword + kPackTile);
  const int ndigits = 1 << nbits;
  const uint32_t mask = (uint32_t)ndigits - 1, rmask = (1u << rb) - 1u;
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  int* mine = wcnt + wv * kRsMaxDigits;
  for (int d = threadIdx.x; d < ndigits; d += kRsThreads) {
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) wcnt[w * kRsMaxDigits + d] = 0;
    gbase[d] = bases[(int64_t)d * ntiles + blockIdx.x];
  }
  __syncthreads();

  // wave wv owns kPackItems rounds of 64 consecutive edges (stable order)
  const int64_t wave0 = (int64_t)blockIdx.x * kPackTile + (int64_t)wv * (kPackItems * kWave);
  uint32_t word[kPackItems];
  int dig[kPackItems], rank[kPackItems];
  int dummy = 0;
#pragma unroll
  for (int h = 0; h < kPackItems / kPackAhead; ++h) {
    uint32_t key[kPackAhead], snd[kPackAhead];
#pragma unroll
    for (int u = 0; u < kPackAhead; ++u) {
      const int64_t e = wave0 + (int64_t)(h * kPackAhead + u) * kWave + lane;
      key[u] = 0xffffffffu;
      snd[u] = 0u;
      if (e < num_edges) {
        key[u] = load_key<true>(recipients, senders, nullptr, e, num_rows, num_cols, dummy);
        snd[u] = (uint32_t)senders[e];
      }
    }
#pragma unroll
    for (int u = 0; u < kPackAhead; ++u) {
      const int i = h * kPackAhead + u;
      const bool ok = wave0 + (int64_t)i * kWave + lane < num_edges;
      const uint32_t d = (key[u] >> rb) & mask;
      // an edge with an endpoint out of range: the sentinel row, sender 0 (its sender may hold anything)
      word[i] = pack_edge(key[u], rmask, cb, (int64_t)key[u] < num_rows ? snd[u] : 0u);
      dig[i] = (int)d;
      const unsigned long long peers = match_digit<9>(d, ok);
      const int leader = __ffsll((long long)peers) - 1;
      const int below = __popcll(peers & ((1ull << lane) - 1ull));
      int prev = 0;
      if (ok && lane == leader) {
        prev = mine[d];
        mine[d] = prev + __popcll(peers);
      }
      prev = __shfl(prev, leader);
      rank[i] = prev + below;
    }
  }
  __syncthreads();
  // per digit: exclusive bases across waves and the tile-local digit start
  for (int d = threadIdx.x; d < ndigits; d += kRsThreads) {
    int acc = 0;
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) {
      const int c = wcnt[w * kRsMaxDigits + d];
      wcnt[w * kRsMaxDigits + d] = acc;
      acc += c;
    }
    dstart[d] = acc;  // tile total for now
  }
  __syncthreads();
  if (threadIdx.x < kWave) {  // exclusive scan of the tile totals over the digits (<= kRsMaxDigits = 8 per lane)
    constexpr int kPer = kRsMaxDigits / kWave;
    int v[kPer], s = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int d = lane * kPer + j;
      v[j] = d < ndigits ? dstart[d] : 0;
      s += v[j];
    }
    int ex = wave_inclusive_scan(s) - s;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int d = lane * kPer + j;
      if (d < ndigits) dstart[d] = ex;
      ex += v[j];
    }
  }
  __syncthreads();
  // tile-local reorder through LDS
#pragma unroll
  for (int i = 0; i < kPackItems; ++i) {
    const int64_t e = wave0 + (int64_t)i * kWave + lane;
    if (e < num_edges) {
      const int lpos = dstart[dig[i]] + mine[dig[i]] + rank[i];
      sword[lpos] = word[i];
      sdig[lpos] = (uint16_t)dig[i];
    }
  }
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * kPackTile;
  const int count = (int)min((int64_t)kPackTile, num_edges - tile0);
  for (int i = threadIdx.x; i < count; i += kRsThreads) {
    const int d = sdig[i];
    words_out[(int64_t)gbase[d] + (i - dstart[d])] = sword[i];
  }
}

// ---- rowptr from the sorted keys, col / w from the sorted values --------------------------------------------
template <class VAL>
__global__ void __launch_bounds__(256) k_finish_csr(const uint32_t* __restrict__ keys, const VAL* __restrict__ vals,
                                                    int64_t num_edges, int64_t num_rows, int32_t* __restrict__ rowptr,
                                                    int32_t* __restrict__ col, float* __restrict__ w) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= num_edges; i += (int64_t)gridDim.x * blockDim.x) {
    // key sequence extended with -1 in front and num_rows behind; invalid edges carry key == num_rows
    const int64_t prev = i == 0 ? -1 : (int64_t)keys[i - 1];
    const int64_t cur = i == num_edges ? num_rows : (int64_t)keys[i];
    for (int64_t r = prev + 1; r <= cur && r <= num_rows; ++r) rowptr[r] = (int32_t)i;
    if (i < num_edges && cur < num_rows) {
      const VAL v = vals[i];
      col[i] = (int32_t)(uint32_t)v;
      if constexpr (sizeof(VAL) == 8) w[i] = __uint_as_float((uint32_t)(v >> 32));
    }
  }
}

// LSD radix sort of E (key, value) pairs.  first_a / first_b: the int64 arrays the FIRST pass reads directly
// (key = first_a[e], valid when 0 <= first_a[e] < range_a and 0 <= first_b[e] < range_b; invalid edges get the
// sentinel key range_a and sort last).  keys_in != NULL: pre-built uint32 keys instead (values from g.vals[*cur]).
// On return *cur selects the ping-pong buffer that holds the result.  (key_bits: graph_plan.h -- values 0 .. range_a, the sentinel, must fit.)
// lo_bit > 0: only the key bits from lo_bit upwards are sorted (the two-level build finishes the low bits bucket by bucket),
// in passes of up to max_bits bits.
template <class VAL, bool EID>
static int radix_sort_pairs(const int64_t* first_a, const int64_t* first_b, const float* edge_w, bool from_keys,
                            int64_t num_edges, int64_t range_a, int64_t range_b, int32_t* stats, GraphWs& g, int* cur_io,
                            hipStream_t stream, int lo_bit = 0, int max_bits = 8, int* last_bits = nullptr) {
  const int keybits = key_bits(range_a) - lo_bit;
  const int npass = (keybits + max_bits - 1) / max_bits;
  const int bits = (keybits + npass - 1) / npass;
  if (last_bits) *last_bits = bits;
  const int64_t ntiles = ceil_div(num_edges, kRsTile);
  int cur = *cur_io;
  for (int pass = 0; pass < npass; ++pass) {
    const int shift = lo_bit + pass * bits;
    const int ndigits = 1 << bits;
    const bool first = (pass == 0) && !from_keys;
    const uint32_t* kin = g.keys[cur];
    const VAL* vin = reinterpret_cast<const VAL*>(g.vals[cur]);
    uint32_t* kout = g.keys[cur ^ 1];
    VAL* vout = reinterpret_cast<VAL*>(g.vals[cur ^ 1]);
    if (first)
      k_rs_upsweep<true><<<(unsigned)ntiles, kRsThreads, 0, stream>>>(first_a, first_b, edge_w, nullptr, num_edges, range_a,
                                                                      range_b, shift, ndigits, g.counts, ntiles, stats);
    else
      k_rs_upsweep<false><<<(unsigned)ntiles, kRsThreads, 0, stream>>>(nullptr, nullptr, nullptr, kin, num_edges, range_a,
                                                                       range_b, shift, ndigits, g.counts, ntiles, stats);
    FSW_LAUNCH_CHECK();
    int rc = exclusive_scan_i32(g.counts, (int64_t)ndigits * ntiles, g.block_sums, g.block_sums_cap, stream);
    if (rc) return rc;
    if (first)
      k_rs_downsweep<true, VAL, EID><<<(unsigned)ntiles, kRsThreads, 0, stream>>>(first_a, first_b, edge_w, nullptr, nullptr, num_edges,
                                                                                  range_a, range_b, shift, bits, g.counts, ntiles, kout, vout);
    else
      k_rs_downsweep<false, VAL, EID><<<(unsigned)ntiles, kRsThreads, 0, stream>>>(nullptr, nullptr, nullptr, kin, vin, num_edges, range_a,
                                                                                   range_b, shift, bits, g.counts, ntiles, kout, vout);
    FSW_LAUNCH_CHECK();
    cur ^= 1;
  }
  *cur_io = cur;
  return 0;
}

template <class VAL>
static int sort_and_finish(const int64_t* recipients, const int64_t* senders, const float* edge_w, int64_t num_edges,
                           int64_t num_rows, int64_t num_cols, int32_t* rowptr, int32_t* col, float* w, int32_t* stats,
                           GraphWs& g, hipStream_t stream) {
  int cur = 0;
  int rc = radix_sort_pairs<VAL, false>(recipients, senders, edge_w, false, num_edges, num_rows, num_cols, stats, g, &cur, stream);
  if (rc) return rc;
  const int blocks = (int)std::min<int64_t>(ceil_div(num_edges + 1, 256), 256 * 32);
  k_finish_csr<VAL><<<blocks, 256, 0, stream>>>(g.keys[cur], reinterpret_cast<const VAL*>(g.vals[cur]), num_edges, num_rows, rowptr, col, w);
  FSW_LAUNCH_CHECK();
  return 0;
}

// ---- coalescing build (edge features; exact reference adjacency) ----------------------------------------------------
// Sort by (recipient, sender) = stable sort by sender, then stable sort by recipient, carrying the edge id; a run of equal
// (recipient, sender) pairs becomes ONE CSR entry whose weight and feature vector are the sums over the run -- what
// torch.sparse_coo_tensor(...).coalesce() does to adj and X_edge in the reference (fsw_conv.py:397-398, 436-437).
__global__ void __launch_bounds__(256) k_gather_keys(const int64_t* __restrict__ recipients, const uint32_t* __restrict__ eid,
                                                     const uint32_t* __restrict__ sender_keys, int64_t num_edges, int64_t num_rows,
                                                     int64_t num_cols, uint32_t* __restrict__ keys_out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < num_edges; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = recipients[eid[i]];
    // an edge whose sender was out of range carries the sentinel sender key: keep it invalid
    keys_out[i] = (r < 0 || r >= num_rows || sender_keys[i] >= (uint32_t)num_cols) ? (uint32_t)num_rows : (uint32_t)r;
  }
}

__global__ void __launch_bounds__(256) k_mark_heads(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ eid,
                                                    const int64_t* __restrict__ senders, int64_t num_edges, int64_t num_rows,
                                                    int32_t* __restrict__ head) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < num_edges; i += (int64_t)gridDim.x * blockDim.x) {
    const bool valid = keys[i] < (uint32_t)num_rows;
    const bool differs = i == 0 || keys[i] != keys[i - 1] || senders[eid[i]] != senders[eid[i - 1]];
    head[i] = (valid && differs) ? 1 : 0;
  }
}

// pos = exclusive scan of head.  One thread per run head sums the run (duplicates are rare and short) in edge-list order.
__global__ void __launch_bounds__(256) k_emit_coalesced(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ eid,
                                                        const int32_t* __restrict__ head, const int32_t* __restrict__ pos,
                                                        const int64_t* __restrict__ senders, const float* __restrict__ edge_w,
                                                        const float* __restrict__ edge_feat, int d_edge, int64_t num_edges,
                                                        int64_t num_rows, uint32_t* __restrict__ keyc, int32_t* __restrict__ col,
                                                        float* __restrict__ w, float* __restrict__ ef,
                                                        int32_t* __restrict__ slot_of_edge, int32_t* __restrict__ nnz_out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < num_edges; i += (int64_t)gridDim.x * blockDim.x) {
    if (i == num_edges - 1) *nnz_out = pos[i] + head[i];
    if (!head[i]) continue;
    const int p = pos[i];
    double wsum = 0.0;
    for (int q = 0; q < d_edge; ++q) ef[(int64_t)p * d_edge + q] = 0.f;
    for (int64_t j = i; j < num_edges && (j == i || (!head[j] && keys[j] < (uint32_t)num_rows)); ++j) {
      const uint32_t e = eid[j];
      wsum += edge_w ? (double)edge_w[e] : 1.0;
      for (int q = 0; q < d_edge; ++q) ef[(int64_t)p * d_edge + q] += edge_feat[(int64_t)e * d_edge + q];
      if (slot_of_edge) slot_of_edge[e] = p;
    }
    keyc[p] = keys[i];
    col[p] = (int32_t)senders[eid[i]];
    w[p] = (float)wsum;
  }
}

__global__ void __launch_bounds__(256) k_rowptr_from_keys(const uint32_t* __restrict__ keyc, const int32_t* __restrict__ nnz_ptr,
                                                          int64_t num_rows, int32_t* __restrict__ rowptr) {
  const int64_t nnz = *nnz_ptr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nnz; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t prev = i == 0 ? -1 : (int64_t)keyc[i - 1];
    const int64_t cur = i == nnz ? num_rows : (int64_t)keyc[i];
    for (int64_t r = prev + 1; r <= cur && r <= num_rows; ++r) rowptr[r] = (int32_t)i;
  }
}

// ---- two-level build: one partition pass over the high key bits, then every bucket of 2^rb rows finished by ONE workgroup ----
// The LSD build above moves every edge three times at 1M rows (3 x 7 bits) and pays 3 x (upsweep, three scan launches,
// downsweep).  Here one pass (same kernels, up to 9 bits) groups the edges by bucket = row >> rb, stably; a bucket then holds
// ~E / buckets edges of 2^rb <= 2048 consecutive rows, and one workgroup finishes it without further global passes:
//   1. every wave histograms ITS contiguous part of the bucket over the 2^rb rows (wave-private LDS table),
//   2. exclusive scan over the waves per row (= where each wave's entries of a row start inside the row) and over the rows
//      (= rowptr of the bucket's rows: the bucket's start is already the number of edges of all smaller rows),
//   3. every wave walks its part again in order: wave64 match on the row bits gives the rank among the round's 64 edges, the
//      wave-private cursor the rest -> col[] / w[] written in place, in edge-list order inside every row (stable, deterministic).
// The scattered 4-byte stores of step 3 land in the bucket's own window of col[] (80 KB at config 3) from one workgroup, i.e. one
// L2: they merge there and reach HBM as whole lines.  A bucket of any size is handled (the workgroup just loops longer), so the
// result never depends on the edge distribution -- but a hub-heavy bucket serialises on its workgroup, which is why the host
// side keeps the LSD build for skewed graphs (graph.py).
// kBucketWaves = 8 wavefronts per bucket, kBucketMaxRowBits = 11 row bits: graph_ws.h (LDS: (kBucketWaves + 1) * 2^bits ints, 72 KB at 11)
constexpr int kBucketAhead = 8;                          // rounds of 64 edges whose loads are in flight together

template <class VAL>
__global__ void __launch_bounds__(kBucketWaves * kWave) k_bucket_rows(const uint32_t* __restrict__ keys, const VAL* __restrict__ vals,
                                                                      const int32_t* __restrict__ bstart, int64_t bstride, int ntable,
                                                                      int64_t num_edges, int64_t num_rows, int rb,
                                                                      int32_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                                                      float* __restrict__ w, int stage_cap) {
  extern __shared__ int bsm[];   // wcnt[kBucketWaves][R] | tot[R] | stage[stage_cap] values (VAL)
  const int R = 1 << rb;
  const uint32_t rmask = (uint32_t)R - 1u;
  int* wcnt = bsm;
  int* tot = bsm + kBucketWaves * R;
  VAL* stage = reinterpret_cast<VAL*>(bsm + (kBucketWaves + 1) * R);
  __shared__ int wsum[kBucketWaves];
  const int b = blockIdx.x, lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t s = bstart[(int64_t)b * bstride];
  const int64_t e = b + 1 < ntable ? (int64_t)bstart[(int64_t)(b + 1) * bstride] : num_edges;
  for (int i = threadIdx.x; i < kBucketWaves * R; i += blockDim.x) wcnt[i] = 0;
  __syncthreads();
  // the wave's contiguous part of the bucket, a whole number of 64-edge rounds
  const int64_t L = ceil_div(e - s, (int64_t)kBucketWaves * kWave) * kWave;
  const int64_t w0 = min(s + wv * L, e), w1 = min(w0 + L, e);
  int* mine = wcnt + wv * R;
  // a bucket that fits the staging tile is put in order in LDS and leaves as whole lines; a larger one scatters its 4-byte
  // stores over its window of col[] (8x the write traffic when 500 buckets' windows compete for the L2s: PMC WRITE_SIZE)
  const bool staged = e - s <= stage_cap;
  {  // kBucketAhead loads in flight (the next group's issued before this group's LDS atomics)
    uint32_t kn[kBucketAhead];
#pragma unroll
    for (int u = 0; u < kBucketAhead; ++u) kn[u] = w0 + lane + u * kWave < w1 ? keys[w0 + lane + u * kWave] : 0u;
    for (int64_t i = w0 + lane; i < w1; i += kBucketAhead * kWave) {
      uint32_t kk[kBucketAhead];
#pragma unroll
      for (int u = 0; u < kBucketAhead; ++u) kk[u] = kn[u];
      const int64_t nx = i + kBucketAhead * kWave;
      if (nx - lane < w1) {
#pragma unroll
        for (int u = 0; u < kBucketAhead; ++u) kn[u] = nx + u * kWave < w1 ? keys[nx + u * kWave] : 0u;
      }
#pragma unroll
      for (int u = 0; u < kBucketAhead; ++u)
        if (i + u * kWave < w1) atomicAdd(&mine[kk[u] & rmask], 1);
    }
  }
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    int acc = 0;
#pragma unroll
    for (int q = 0; q < kBucketWaves; ++q) {
      const int c = wcnt[q * R + r];
      wcnt[q * R + r] = acc;
      acc += c;
    }
    tot[r] = acc;
  }
  __syncthreads();
  {  // exclusive scan of tot[0..R) in place: thread t owns R / blockDim.x consecutive rows
    constexpr int kPerMax = (1 << kBucketMaxRowBits) / (kBucketWaves * kWave);
    const int per = max(R / (int)blockDim.x, 1);
    const int r0 = threadIdx.x * per;
    int v[kPerMax], sum = 0;
#pragma unroll
    for (int j = 0; j < kPerMax; ++j) {
      v[j] = (j < per && r0 + j < R) ? tot[r0 + j] : 0;
      sum += v[j];
    }
    const int inc = wave_inclusive_scan(sum);
    if (lane == kWave - 1) wsum[wv] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int q = 0; q < kBucketWaves; ++q)
      if (q < wv) base += wsum[q];
    int ex = base + inc - sum;
#pragma unroll
    for (int j = 0; j < kPerMax; ++j)
      if (j < per && r0 + j < R) {
        tot[r0 + j] = ex;
        const int64_t row = (int64_t)b * R + r0 + j;
        if (row <= num_rows) rowptr[row] = (int32_t)(s + ex);   // row == num_rows: the run of invalid edges (sentinel key) = nnz
        ex += v[j];
      }
  }
  __syncthreads();
  // the next group's loads are issued before the current group is ranked (two wavefronts per SIMD do not hide an HBM round
  // trip per group on their own)
  uint32_t keyn[kBucketAhead];
  VAL valn[kBucketAhead];
  auto load_group = [&](int64_t g) {
#pragma unroll
    for (int u = 0; u < kBucketAhead; ++u) {
      const int64_t i = g + u * kWave + lane;
      keyn[u] = i < w1 ? keys[i] : 0xffffffffu;
      valn[u] = i < w1 ? vals[i] : VAL(0);
    }
  };
  load_group(w0);
  for (int64_t g0 = w0; g0 < w1; g0 += kBucketAhead * kWave) {
    uint32_t keyv[kBucketAhead];
    VAL valv[kBucketAhead];
#pragma unroll
    for (int u = 0; u < kBucketAhead; ++u) {
      keyv[u] = keyn[u];
      valv[u] = valn[u];
    }
    if (g0 + kBucketAhead * kWave < w1) load_group(g0 + kBucketAhead * kWave);
#pragma unroll
    for (int u = 0; u < kBucketAhead; ++u) {
      if (g0 + u * kWave >= w1) break;                       // wave-uniform
      const bool ok = g0 + u * kWave + lane < w1;
      const uint32_t key = keyv[u];
      const uint32_t k = key & rmask;
      const unsigned long long peers = match_digit<kBucketMaxRowBits>(k, ok);
      const int leader = __ffsll((long long)peers) - 1;
      const int below = __popcll(peers & ((1ull << lane) - 1ull));
      int prev = 0;
      if (ok && lane == leader) {
        prev = mine[k];
        mine[k] = prev + __popcll(peers);
      }
      prev = __shfl(prev, leader);
      if (ok && (int64_t)key < num_rows) {
        const int lpos = tot[k] + prev + below;
        if (staged) {
          stage[lpos] = valv[u];
        } else {
          col[s + lpos] = (int32_t)(uint32_t)valv[u];
          if constexpr (sizeof(VAL) == 8) w[s + lpos] = __uint_as_float((uint32_t)(valv[u] >> 32));
        }
      }
    }
  }
  if (staged) {
    __syncthreads();
    // valid entries of the bucket: everything below the run of the sentinel row (invalid edges), if that row lives here
    const int64_t sent = num_rows - (int64_t)b * R;
    const int nvalid = (sent >= 0 && sent < R) ? tot[sent] : (int)(e - s);
    for (int i = threadIdx.x; i < nvalid; i += blockDim.x) {
      const VAL v = stage[i];
      col[s + i] = (int32_t)(uint32_t)v;
      if constexpr (sizeof(VAL) == 8) w[s + i] = __uint_as_float((uint32_t)(v >> 32));
    }
  }
}

// The bucket kernel of the packed path (graph_plan.h): one word per edge -- row inside the bucket and sender -- read twice instead of a
// key read twice and a sender; the row of a word is b * R + its row field, which is what the `key < num_rows` test above becomes.
// Its scan step holds the degree of every row of the bucket in registers, so it also counts the rows' degree bins and the maximal
// degree (what k_bin_count re-reads rowptr for): one LDS table, then at most one global atomic per non-empty bin.  A bucket is
// FSW_BIN_BLOCK_ROWS rows, the granularity of a row chunk, so it lies inside ONE chunk; the sentinel row num_rows is never counted.
static_assert((1 << kBucketMaxRowBits) == FSW_BIN_BLOCK_ROWS, "a bucket of the two-level build is one bin block: it never straddles a row chunk");

__global__ void __launch_bounds__(kBucketWaves * kWave) k_bucket_rows_packed(const uint32_t* __restrict__ words, const int32_t* __restrict__ bstart,
                                                                             int64_t bstride, int ntable, int64_t num_edges, int64_t num_rows,
                                                                             int rb, int cb, int32_t* __restrict__ rowptr,
                                                                             int32_t* __restrict__ col, int stage_cap, int64_t chunk_rows,
                                                                             int32_t* __restrict__ bin_count, int32_t* __restrict__ stats) {
  extern __shared__ int bsm[];   // wcnt[kBucketWaves][R] | tot[R] | stage[stage_cap] senders
  const int R = 1 << rb;
  int* wcnt = bsm;
  int* tot = bsm + kBucketWaves * R;
  uint32_t* stage = reinterpret_cast<uint32_t*>(bsm + (kBucketWaves + 1) * R);
  __shared__ int wsum[kBucketWaves];
  __shared__ int lbin[FSW_NUM_BINS];
  __shared__ int lmax;
  const int b = blockIdx.x, lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t s = bstart[(int64_t)b * bstride];
  const int64_t e = b + 1 < ntable ? (int64_t)bstart[(int64_t)(b + 1) * bstride] : num_edges;
  for (int i = threadIdx.x; i < kBucketWaves * R; i += blockDim.x) wcnt[i] = 0;
  if (threadIdx.x < FSW_NUM_BINS) lbin[threadIdx.x] = 0;
  if (threadIdx.x == 0) lmax = 0;
  __syncthreads();
  // the wave's contiguous part of the bucket, a whole number of 64-edge rounds
  const int64_t L = ceil_div(e - s, (int64_t)kBucketWaves * kWave) * kWave;
  const int64_t w0 = min(s + wv * L, e), w1 = min(w0 + L, e);
  int* mine = wcnt + wv * R;
  const bool staged = e - s <= stage_cap;   // as in k_bucket_rows: a bucket that fits the staging tile leaves as whole lines
  {  // kBucketAhead loads in flight (the next group's issued before this group's LDS atomics)
    uint32_t kn[kBucketAhead];
#pragma unroll
    for (int u = 0; u < kBucketAhead; ++u) kn[u] = w0 + lane + u * kWave < w1 ? words[w0 + lane + u * kWave] : 0u;
    for (int64_t i = w0 + lane; i < w1; i += kBucketAhead * kWave) {
      uint32_t kk[kBucketAhead];
#pragma unroll
      for (int u = 0; u < kBucketAhead; ++u) kk[u] = kn[u];
      const int64_t nx = i + kBucketAhead * kWave;
      if (nx - lane < w1) {
#pragma unroll
        for (int u = 0; u < kBucketAhead; ++u) kn[u] = nx + u * kWave < w1 ? words[nx + u * kWave] : 0u;
      }
#pragma unroll
      for (int u = 0; u < kBucketAhead; ++u)
        if (i + u * kWave < w1) atomicAdd(&mine[edge_row(kk[u], cb)], 1);
    }
  }
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    int acc = 0;
#pragma unroll
    for (int q = 0; q < kBucketWaves; ++q) {
      const int c = wcnt[q * R + r];
      wcnt[q * R + r] = acc;
      acc += c;
    }
    tot[r] = acc;
  }
  __syncthreads();
  {  // exclusive scan of tot[0..R) in place: thread t owns R / blockDim.x consecutive rows; v[j] is the degree of row b * R + r0 + j
    constexpr int kPerMax = (1 << kBucketMaxRowBits) / (kBucketWaves * kWave);
    const int per = max(R / (int)blockDim.x, 1);
    const int r0 = threadIdx.x * per;
    int v[kPerMax], sum = 0, mx = 0;
#pragma unroll
    for (int j = 0; j < kPerMax; ++j) {
      v[j] = (j < per && r0 + j < R) ? tot[r0 + j] : 0;
      sum += v[j];
      // rows below num_rows only: the sentinel row's run (invalid edges) is no degree
      const bool valid = j < per && r0 + j < R && (int64_t)b * R + r0 + j < num_rows;
      const int bin = degree_bin(valid ? v[j] : 0);
      if (valid) mx = max(mx, v[j]);
      const unsigned long long peers = match_bin(bin, valid);
      if (valid && lane == __ffsll((long long)peers) - 1) atomicAdd(&lbin[bin], __popcll(peers));   // one LDS atomic per bin and wave
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
    if (lane == 0 && mx) atomicMax(&lmax, mx);
    const int inc = wave_inclusive_scan(sum);
    if (lane == kWave - 1) wsum[wv] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int q = 0; q < kBucketWaves; ++q)
      if (q < wv) base += wsum[q];
    int ex = base + inc - sum;
#pragma unroll
    for (int j = 0; j < kPerMax; ++j)
      if (j < per && r0 + j < R) {
        tot[r0 + j] = ex;
        const int64_t row = (int64_t)b * R + r0 + j;
        if (row <= num_rows) rowptr[row] = (int32_t)(s + ex);   // row == num_rows: the run of invalid edges (sentinel key) = nnz
        ex += v[j];
      }
    // the barrier above also ordered the LDS atomics on lbin / lmax.  A bucket without a row below num_rows (the sentinel row alone)
    // has empty bins and touches no counter -- its chunk index may lie behind the last chunk.
    const int64_t chunk = ((int64_t)b * R) / chunk_rows;
    if (threadIdx.x < FSW_NUM_BINS && lbin[threadIdx.x]) atomicAdd(&bin_count[chunk * FSW_NUM_BINS + threadIdx.x], lbin[threadIdx.x]);
    if (threadIdx.x == 0 && lmax) atomicMax(&stats[FSW_STAT_MAX_DEGREE], lmax);
  }
  __syncthreads();
  // the next group's loads are issued before the current group is ranked
  uint32_t wordn[kBucketAhead];
  auto load_group = [&](int64_t g) {
#pragma unroll
    for (int u = 0; u < kBucketAhead; ++u) {
      const int64_t i = g + u * kWave + lane;
      wordn[u] = i < w1 ? words[i] : 0u;
    }
  };
  load_group(w0);
  const int64_t rows_here = num_rows - (int64_t)b * R;   // rows of this bucket below num_rows (<= 0: none, > R: all)
  for (int64_t g0 = w0; g0 < w1; g0 += kBucketAhead * kWave) {
    uint32_t wordv[kBucketAhead];
#pragma unroll
    for (int u = 0; u < kBucketAhead; ++u) wordv[u] = wordn[u];
    if (g0 + kBucketAhead * kWave < w1) load_group(g0 + kBucketAhead * kWave);
#pragma unroll
    for (int u = 0; u < kBucketAhead; ++u) {
      if (g0 + u * kWave >= w1) break;                       // wave-uniform
      const bool ok = g0 + u * kWave + lane < w1;
      const uint32_t k = edge_row(wordv[u], cb);
      const unsigned long long peers = match_digit<kBucketMaxRowBits>(k, ok);
      const int leader = __ffsll((long long)peers) - 1;
      const int below = __popcll(peers & ((1ull << lane) - 1ull));
      int prev = 0;
      if (ok && lane == leader) {
        prev = mine[k];
        mine[k] = prev + __popcll(peers);
      }
      prev = __shfl(prev, leader);
      if (ok && (int64_t)k < rows_here) {
        const int lpos = tot[k] + prev + below;
        const uint32_t sender = edge_sender(wordv[u], cb);
        if (staged)
          stage[lpos] = sender;
        else
          col[s + lpos] = (int32_t)sender;
      }
    }
  }
  if (staged) {
    __syncthreads();
    // valid entries of the bucket: everything below the run of the sentinel row (invalid edges), if that row lives here
    const int nvalid = (rows_here >= 0 && rows_here < R) ? tot[rows_here] : (int)(e - s);
    for (int i = threadIdx.x; i < nvalid; i += blockDim.x) col[s + i] = (int32_t)stage[i];
  }
}

// first index of every bucket in the sorted keys (buckets = key >> rb): the multi-pass case of the two-level build
__global__ void __launch_bounds__(256) k_bucket_starts(const uint32_t* __restrict__ keys, int64_t num_edges, int rb, int64_t nbuckets,
                                                       int32_t* __restrict__ bstart) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= num_edges; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t prev = i == 0 ? -1 : (int64_t)(keys[i - 1] >> rb);
    const int64_t cur = i == num_edges ? nbuckets : (int64_t)(keys[i] >> rb);
    for (int64_t q = prev + 1; q <= cur && q <= nbuckets; ++q) bstart[q] = (int32_t)i;
  }
}

// two_level_ok (graph_ws.h) and two_level_plan (graph_plan.h) decide what the build does with a shape, for the build and for fsw_graph_build_plan.
static_assert(kPartitionBits == 9, "graph_ws.h: the literal handed to radix_sort_pairs below");
template <class VAL>
static int sort_and_finish_two_level(const int64_t* recipients, const int64_t* senders, const float* edge_w, int64_t num_edges,
                                     int64_t num_rows, int64_t num_cols, int32_t* rowptr, int32_t* col, float* w, int32_t* stats,
                                     GraphWs& g, hipStream_t stream, const TwoLevelPlan& p) {
  const int rb = p.rb;
  const int64_t nbuckets = p.nbuckets;
  const int64_t ntiles = ceil_div(num_edges, kRsTile);
  int cur = 0, bits = 0;
  int rc = radix_sort_pairs<VAL, false>(recipients, senders, edge_w, false, num_edges, num_rows, num_cols, stats, g, &cur, stream, rb, 9, &bits);
  if (rc) return rc;
  FSW_REQUIRE(bits == p.bits, "fsw_graph_build_two_level: the partition ran passes of %d bits, the plan says %d", bits, p.bits);
  const int32_t* bstart = g.counts;     // single pass: the scanned [digit][tile] table, digit = bucket
  int64_t bstride = ntiles;
  int ntable = 1 << bits;
  if (bits != p.upper) {                // several passes: bucket boundaries from the sorted keys
    const int blocks = (int)std::min<int64_t>(ceil_div(num_edges + 1, 256), 256 * 32);
    k_bucket_starts<<<blocks, 256, 0, stream>>>(g.keys[cur], num_edges, rb, nbuckets, g.block_sums_big);
    FSW_LAUNCH_CHECK();
    bstart = g.block_sums_big;
    bstride = 1;
    ntable = (int)nbuckets + 1;
  }
  FSW_SET_MAX_LDS_ONCE((&k_bucket_rows<VAL>), 160 * 1024 - 1024);
  k_bucket_rows<VAL><<<(unsigned)nbuckets, kBucketWaves * kWave, p.lds, stream>>>(g.keys[cur], reinterpret_cast<const VAL*>(g.vals[cur]), bstart,
                                                                                bstride, ntable, num_edges, num_rows, rb, rowptr, col, w,
                                                                                p.stage_cap);
  FSW_LAUNCH_CHECK();
  return 0;
}

// The packed path (graph_plan.h): upsweep, scan and downsweep over tiles of kPackTile edges, one word per edge into keys[1]; the bucket
// kernel unpacks it and counts the degree bins, so finish_bins skips k_bin_count.
static int sort_and_finish_packed(const int64_t* recipients, const int64_t* senders, int64_t num_edges, int64_t num_rows, int64_t num_cols,
                                  int64_t chunk_rows, int32_t* rowptr, int32_t* col, int32_t* stats, GraphWs& g, hipStream_t stream,
                                  const TwoLevelPlan& p) {
  const int ndigits = 1 << p.bits;
  FSW_REQUIRE(p.packed && ndigits <= kRsMaxDigits && (int64_t)ndigits * p.ntiles <= (int64_t)kRsMaxDigits * ceil_div(num_edges, kRsTile),
              "fsw_graph_build_two_level: the packed count table does not fit the workspace");
  uint32_t* words = g.keys[1];
  if (((reinterpret_cast<uintptr_t>(recipients) | reinterpret_cast<uintptr_t>(senders)) & 15) == 0)
    k_pack_upsweep<true><<<(unsigned)p.ntiles, kRsThreads, 0, stream>>>(recipients, senders, num_edges, num_rows, num_cols, p.rb, ndigits,
                                                                       g.counts, p.ntiles, stats);
  else
    k_pack_upsweep<false><<<(unsigned)p.ntiles, kRsThreads, 0, stream>>>(recipients, senders, num_edges, num_rows, num_cols, p.rb, ndigits,
                                                                        g.counts, p.ntiles, stats);
  FSW_LAUNCH_CHECK();
  if ((int64_t)ndigits * p.ntiles <= kScanTile) {
    k_scan_one<<<1, kScanThreads, 0, stream>>>(g.counts, (int64_t)ndigits * p.ntiles);
    FSW_LAUNCH_CHECK();
  } else if (int rc = exclusive_scan_i32(g.counts, (int64_t)ndigits * p.ntiles, g.block_sums, g.block_sums_cap, stream)) {
    return rc;
  }
  FSW_SET_MAX_LDS_ONCE((&k_pack_downsweep), kPackLdsBytes);
  k_pack_downsweep<<<(unsigned)p.ntiles, kRsThreads, kPackLdsBytes, stream>>>(recipients, senders, num_edges, num_rows, num_cols, p.rb, p.cb,
                                                                             p.bits, g.counts, p.ntiles, words);
  FSW_LAUNCH_CHECK();
  FSW_SET_MAX_LDS_ONCE((&k_bucket_rows_packed), 160 * 1024 - 1024);
  k_bucket_rows_packed<<<(unsigned)p.nbuckets, kBucketWaves * kWave, p.lds, stream>>>(words, g.counts, p.ntiles, ndigits, num_edges, num_rows,
                                                                                     p.rb, p.cb, rowptr, col, p.stage_cap,
                                                                                     one_chunk_if_zero(num_rows, chunk_rows), g.bin_count, stats);
  FSW_LAUNCH_CHECK();
  return 0;
}

// keys = the sender of every CSR entry, values = the entry's position: the input of the sender-major sort (fsw_graph_transpose)
__global__ void __launch_bounds__(256) k_entry_keys(const int32_t* __restrict__ col, int64_t nnz, int64_t num_cols,
                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = col[i];
    keys[i] = (c < 0 || c >= num_cols) ? (uint32_t)num_cols : (uint32_t)c;
    vals[i] = (uint32_t)i;
  }
}

}  // namespace fsw

using namespace fsw;

extern "C" size_t fsw_graph_workspace_bytes(int64_t num_rows, int64_t num_edges) {
  GraphWs g = carve(nullptr, num_edges, num_rows);
  return g.total;
}

static int graph_build_impl(const int64_t* recipients, const int64_t* senders, const float* edge_w, int64_t num_edges,
                            int64_t num_rows, int64_t num_cols, int64_t chunk_rows, int32_t* rowptr, int32_t* col, float* w,
                            int32_t* perm, int32_t* invperm, int32_t* bin_start, int32_t* stats, void* workspace,
                            size_t workspace_bytes, fsw_stream_t stream_, bool two_level) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  FSW_REQUIRE(num_rows >= 1 && num_rows < (1ll << 31) - 1 && num_cols >= 1 && num_cols < (1ll << 31) && num_edges >= 0 &&
                  num_edges < (1ll << 31) - kRsTile,
              "fsw_graph_build: sizes must satisfy 1 <= rows, cols < 2^31 and 0 <= edges < 2^31 (got %lld, %lld, %lld)",
              (long long)num_rows, (long long)num_cols, (long long)num_edges);
  FSW_REQUIRE(workspace && workspace_bytes >= fsw_graph_workspace_bytes(num_rows, num_edges),
              "fsw_graph_build: workspace too small");
  FSW_REQUIRE(rowptr && perm && bin_start && stats && (num_edges == 0 || (col && recipients && senders)),
              "fsw_graph_build: null pointer");
  FSW_REQUIRE(!edge_w || w, "fsw_graph_build: edge_w given but w is null");
  if (int rc = check_chunks(num_rows, chunk_rows)) return rc;
  GraphWs g = carve(workspace, num_edges, num_rows);

  FSW_CHECK_HIP(hipMemsetAsync(g.bin_count, 0, kBinTableBytes, stream));
  FSW_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(int32_t) * FSW_NUM_STATS, stream));
  const bool try_two = two_level && num_edges > 0 && two_level_ok(num_rows, num_edges);
  const TwoLevelPlan p = try_two ? two_level_plan(num_rows, num_cols, num_edges, edge_w != nullptr) : TwoLevelPlan{};
  const bool counted = try_two && p.packed;   // the degree bins are counted by the bucket kernel
  if (num_edges == 0) {
    FSW_CHECK_HIP(hipMemsetAsync(rowptr, 0, sizeof(int32_t) * (size_t)(num_rows + 1), stream));
  } else if (try_two) {
    int rc = p.packed ? sort_and_finish_packed(recipients, senders, num_edges, num_rows, num_cols, chunk_rows, rowptr, col, stats, g, stream, p)
             : edge_w ? sort_and_finish_two_level<unsigned long long>(recipients, senders, edge_w, num_edges, num_rows, num_cols, rowptr, col, w, stats, g, stream, p)
                      : sort_and_finish_two_level<uint32_t>(recipients, senders, edge_w, num_edges, num_rows, num_cols, rowptr, col, w, stats, g, stream, p);
    if (rc) return rc;
  } else {
    int rc = edge_w ? sort_and_finish<unsigned long long>(recipients, senders, edge_w, num_edges, num_rows, num_cols, rowptr, col, w, stats, g, stream)
                    : sort_and_finish<uint32_t>(recipients, senders, edge_w, num_edges, num_rows, num_cols, rowptr, col, w, stats, g, stream);
    if (rc) return rc;
  }
  return finish_bins(rowptr, num_rows, chunk_rows, perm, invperm, bin_start, stats, g.bin_count, g.bin_cursor, stream, counted);
}

// Host only: what fsw_graph_build_two_level does with a shape (GraphPlanWord of graph_plan.h), from the functions the build itself calls.
extern "C" int fsw_graph_build_plan(int64_t num_rows, int64_t num_cols, int64_t num_edges, int weighted, int32_t* out) {
  FSW_REQUIRE(out && num_rows >= 1 && num_rows < (1ll << 31) - 1 && num_cols >= 1 && num_cols < (1ll << 31) && num_edges >= 0 &&
                  num_edges < (1ll << 31) - kRsTile,
              "fsw_graph_build_plan: null pointer or sizes outside 1 <= rows, cols < 2^31, 0 <= edges < 2^31");
  graph_plan_words(num_rows, num_cols, num_edges, weighted != 0, out);
  return 0;
}

extern "C" int fsw_graph_build(const int64_t* recipients, const int64_t* senders, const float* edge_w, int64_t num_edges,
                               int64_t num_rows, int64_t num_cols, int64_t chunk_rows, int32_t* rowptr, int32_t* col, float* w,
                               int32_t* perm, int32_t* invperm, int32_t* bin_start, int32_t* stats, void* workspace,
                               size_t workspace_bytes, fsw_stream_t stream) {
  return graph_build_impl(recipients, senders, edge_w, num_edges, num_rows, num_cols, chunk_rows, rowptr, col, w, perm, invperm, bin_start,
                          stats, workspace, workspace_bytes, stream, false);
}

// Same contract and same result, bit for bit; the edges are grouped by a single partition pass + one workgroup per bucket of 2048
// rows (above) when the shape suits that (>= 32768 rows, <= 65536 edges per bucket on average), by the LSD passes otherwise.
extern "C" int fsw_graph_build_two_level(const int64_t* recipients, const int64_t* senders, const float* edge_w, int64_t num_edges,
                                         int64_t num_rows, int64_t num_cols, int64_t chunk_rows, int32_t* rowptr, int32_t* col, float* w,
                                         int32_t* perm, int32_t* invperm, int32_t* bin_start, int32_t* stats, void* workspace,
                                         size_t workspace_bytes, fsw_stream_t stream) {
  return graph_build_impl(recipients, senders, edge_w, num_edges, num_rows, num_cols, chunk_rows, rowptr, col, w, perm, invperm, bin_start,
                          stats, workspace, workspace_bytes, stream, true);
}

extern "C" int fsw_graph_build_coalesced(const int64_t* recipients, const int64_t* senders, const float* edge_w,
                                         const float* edge_feat, int d_edge, int64_t num_edges, int64_t num_rows, int64_t num_cols,
                                         int32_t* rowptr, int32_t* col, float* w, float* ef, int32_t* slot_of_edge, int32_t* perm,
                                         int32_t* invperm, int32_t* bin_start, int32_t* stats, void* workspace,
                                         size_t workspace_bytes, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  FSW_REQUIRE(num_rows >= 1 && num_rows < (1ll << 31) - 1 && num_cols >= 1 && num_cols < (1ll << 31) - 1 && num_edges >= 0 &&
                  num_edges < (1ll << 31) - kRsTile,
              "fsw_graph_build_coalesced: sizes must satisfy 1 <= rows, cols < 2^31 and 0 <= edges < 2^31");
  FSW_REQUIRE(workspace && workspace_bytes >= fsw_graph_workspace_bytes(num_rows, num_edges),
              "fsw_graph_build_coalesced: workspace too small");
  FSW_REQUIRE(rowptr && perm && bin_start && stats && w && (num_edges == 0 || (col && recipients && senders)),
              "fsw_graph_build_coalesced: null pointer");
  FSW_REQUIRE(d_edge >= 0 && (d_edge == 0 || (edge_feat && ef)), "fsw_graph_build_coalesced: edge features need edge_feat and ef");
  GraphWs g = carve(workspace, num_edges, num_rows);
  FSW_CHECK_HIP(hipMemsetAsync(g.bin_count, 0, kBinTableBytes, stream));
  FSW_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(int32_t) * FSW_NUM_STATS, stream));
  if (num_edges == 0) {
    FSW_CHECK_HIP(hipMemsetAsync(rowptr, 0, sizeof(int32_t) * (size_t)(num_rows + 1), stream));
    return finish_bins(rowptr, num_rows, 0, perm, invperm, bin_start, stats, g.bin_count, g.bin_cursor, stream);
  }
  if (slot_of_edge) FSW_CHECK_HIP(hipMemsetAsync(slot_of_edge, 0xff, sizeof(int32_t) * (size_t)num_edges, stream));
  const int edge_blocks = (int)std::min<int64_t>(ceil_div(num_edges, 256), 256 * 16);
  int cur = 0, rc;
  // 1. stable sort by sender, carrying the edge id (validates both endpoints and the weights)
  if ((rc = radix_sort_pairs<uint32_t, true>(senders, recipients, edge_w, false, num_edges, num_cols, num_rows, stats, g, &cur, stream))) return rc;
  // 2. stable sort by recipient: (recipient, sender) order
  k_gather_keys<<<edge_blocks, 256, 0, stream>>>(recipients, reinterpret_cast<const uint32_t*>(g.vals[cur]), g.keys[cur], num_edges,
                                                 num_rows, num_cols, g.keys[cur ^ 1]);
  FSW_LAUNCH_CHECK();
  {  // the gathered keys live in the other key buffer: make it the current one, values stay where they are
    uint32_t* t = g.keys[cur];
    g.keys[cur] = g.keys[cur ^ 1];
    g.keys[cur ^ 1] = t;
  }
  if ((rc = radix_sort_pairs<uint32_t, true>(nullptr, nullptr, nullptr, true, num_edges, num_rows, num_cols, stats, g, &cur, stream))) return rc;
  // 3. runs of equal (recipient, sender) -> one entry each
  const uint32_t* keys = g.keys[cur];
  const uint32_t* eid = reinterpret_cast<const uint32_t*>(g.vals[cur]);
  int32_t* head = reinterpret_cast<int32_t*>(g.vals[cur ^ 1]);
  int32_t* pos = head + num_edges;
  uint32_t* keyc = g.keys[cur ^ 1];
  k_mark_heads<<<edge_blocks, 256, 0, stream>>>(keys, eid, senders, num_edges, num_rows, head);
  FSW_LAUNCH_CHECK();
  FSW_CHECK_HIP(hipMemcpyAsync(pos, head, sizeof(int32_t) * (size_t)num_edges, hipMemcpyDeviceToDevice, stream));
  if ((rc = exclusive_scan_i32(pos, num_edges, g.block_sums, g.block_sums_cap, stream))) return rc;
  int32_t* nnz_dev = stats + FSW_STAT_NNZ;
  k_emit_coalesced<<<edge_blocks, 256, 0, stream>>>(keys, eid, head, pos, senders, edge_w, edge_feat, d_edge, num_edges, num_rows,
                                                    keyc, col, w, ef, slot_of_edge, nnz_dev);
  FSW_LAUNCH_CHECK();
  k_rowptr_from_keys<<<edge_blocks, 256, 0, stream>>>(keyc, nnz_dev, num_rows, rowptr);
  FSW_LAUNCH_CHECK();
  return finish_bins(rowptr, num_rows, 0, perm, invperm, bin_start, stats, g.bin_count, g.bin_cursor, stream);
}

// Sender-major view of a built graph: cptr[j] .. cptr[j + 1] index the entries of `order` that list, in CSR order, the CSR
// positions e with col[e] == j.  The backward pass sums the stored key gradients over it (fsw_segment_sum_rows_f32) instead of
// scattering them with float atomics.  A stable LSD sort of (col[e], e): the CSR build's own passes.
extern "C" int fsw_graph_transpose(const int32_t* col, int64_t nnz, int64_t num_cols, int32_t* cptr, int32_t* order, void* workspace,
                                   size_t workspace_bytes, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  FSW_REQUIRE(num_cols >= 1 && num_cols < (1ll << 31) - 1 && nnz >= 0 && nnz < (1ll << 31) - kRsTile,
              "fsw_graph_transpose: sizes must satisfy 1 <= cols < 2^31 and 0 <= nnz < 2^31");
  FSW_REQUIRE(cptr && workspace && workspace_bytes >= fsw_graph_workspace_bytes(num_cols, nnz) && (nnz == 0 || (col && order)),
              "fsw_graph_transpose: null pointer or workspace too small");
  if (nnz == 0) {
    FSW_CHECK_HIP(hipMemsetAsync(cptr, 0, sizeof(int32_t) * (size_t)(num_cols + 1), stream));
    return 0;
  }
  GraphWs g = carve(workspace, nnz, num_cols);
  const int blocks = (int)std::min<int64_t>(ceil_div(nnz + 1, 256), 256 * 32);
  k_entry_keys<<<blocks, 256, 0, stream>>>(col, nnz, num_cols, g.keys[0], reinterpret_cast<uint32_t*>(g.vals[0]));
  FSW_LAUNCH_CHECK();
  int cur = 0;
  if (int rc = radix_sort_pairs<uint32_t, true>(nullptr, nullptr, nullptr, true, nnz, num_cols, num_cols, nullptr, g, &cur, stream)) return rc;
  k_finish_csr<uint32_t><<<blocks, 256, 0, stream>>>(g.keys[cur], reinterpret_cast<const uint32_t*>(g.vals[cur]), nnz, num_cols, cptr, order,
                                                     nullptr);
  FSW_LAUNCH_CHECK();
  return 0;
}
