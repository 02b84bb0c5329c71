// What the CSR build (graph_build.hip) and the CSR import (graph_import.hip) share: the device-wide exclusive scan of int32 and the
// degree bins of a finished rowptr (bin_start, perm, invperm and the stats words).  Both translation units include this header, so
// the kernels have internal linkage (static): each unit gets its own copy of the code, nothing is defined twice in the library.
#pragma once
#include "fsw_common.h"
#include "graph_ws.h"

namespace fsw {

// ---- generic device-wide exclusive scan of int32 (three launches) ----------------------------------
__device__ __forceinline__ int wave_inclusive_scan(int v) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    int t = __shfl_up(v, off);
    if (lane_id() >= off) v += t;
  }
  return v;
}

__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
  __shared__ int wsum[kScanThreads / kWave];
  int inc = wave_inclusive_scan(v);
  int w = threadIdx.x >> 6;
  if (lane_id() == kWave - 1) wsum[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kScanThreads / kWave; ++i) {
    int s = wsum[i];
    if (i < w) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

static __global__ void __launch_bounds__(kScanThreads) k_scan_partial(const int32_t* __restrict__ in, int64_t n,
                                                                      int32_t* __restrict__ block_sums) {
  int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int s = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i)
    if (base + i < n) s += in[base + i];
  int tot;
  block_exclusive_scan(s, &tot);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

static __global__ void __launch_bounds__(kScanThreads) k_scan_block_sums(int32_t* __restrict__ block_sums, int64_t nb) {
  int carry = 0;
  for (int64_t a = 0; a < nb; a += kScanThreads) {
    int64_t i = a + threadIdx.x;
    int v = i < nb ? block_sums[i] : 0;
    int tot;
    int ex = block_exclusive_scan(v, &tot);
    if (i < nb) block_sums[i] = carry + ex;
    carry += tot;
  }
}

static __global__ void __launch_bounds__(kScanThreads) k_scan_apply(int32_t* __restrict__ data, int64_t n,
                                                                    const int32_t* __restrict__ block_sums) {
  int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int v[kScanItems];
  int s = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    v[i] = base + i < n ? data[base + i] : 0;
    s += v[i];
  }
  int tot;
  int ex = block_exclusive_scan(s, &tot) + block_sums[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    if (base + i < n) data[base + i] = ex;
    ex += v[i];
  }
}

// A table of at most kScanTile elements (the count table of a packed partition pass over a small graph): one workgroup, one launch.
static __global__ void __launch_bounds__(kScanThreads) k_scan_one(int32_t* __restrict__ data, int64_t n) {
  const int64_t base = (int64_t)threadIdx.x * kScanItems;
  int v[kScanItems];
  int s = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    v[i] = base + i < n ? data[base + i] : 0;
    s += v[i];
  }
  int tot;
  int ex = block_exclusive_scan(s, &tot);
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    if (base + i < n) data[base + i] = ex;
    ex += v[i];
  }
}

// block_sums holds block_sums_cap entries; one per kScanTile elements is needed.  A longer input is refused before any launch.
static int exclusive_scan_i32(int32_t* data, int64_t n, int32_t* block_sums, int64_t block_sums_cap, hipStream_t stream) {
  const int64_t nb = ceil_div(n, kScanTile);
  FSW_REQUIRE(nb <= block_sums_cap, "exclusive_scan_i32: %lld elements need %lld block sums, the workspace holds %lld",
              (long long)n, (long long)nb, (long long)block_sums_cap);
  k_scan_partial<<<(unsigned)nb, kScanThreads, 0, stream>>>(data, n, block_sums);
  FSW_LAUNCH_CHECK();
  k_scan_block_sums<<<1, kScanThreads, 0, stream>>>(block_sums, nb);
  FSW_LAUNCH_CHECK();
  k_scan_apply<<<(unsigned)nb, kScanThreads, 0, stream>>>(data, n, block_sums);
  FSW_LAUNCH_CHECK();
  return 0;
}

// ---- degree bins ----------------------------------------------------------------------------------------------
// Most rows of a graph share a handful of degrees, so per-thread LDS atomics on the bin counters serialise (48 us for
// 1M rows).  Rows are matched inside the wavefront instead (one ballot per bit of the bin id): one LDS atomic per
// distinct bin and wave, and the lane's rank among its peers for free.
__device__ __forceinline__ unsigned long long match_bin(int bin, bool valid) {
  unsigned long long peers = __ballot(valid);
  if (!valid) peers = ~peers;
  static_assert(FSW_NUM_BINS <= 64, "bin ids must fit 6 bits");
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const unsigned long long bb = __ballot((bin >> b) & 1);
    peers &= ((bin >> b) & 1) ? bb : ~bb;
  }
  return peers;
}

// Row chunks: with chunk_rows > 0 the rows are binned separately inside every chunk of chunk_rows consecutive rows
// (a multiple of kBinRowsPerBlock, so a workgroup never straddles two chunks): perm lists chunk 0's rows by degree bin, then
// chunk 1's, ..., and bin_start holds one row of FSW_NUM_BINS + 1 offsets per chunk.  A kernel handed chunk c's row of
// bin_start visits exactly the recipients [c * chunk_rows, (c + 1) * chunk_rows) -- that is how the multi-GPU path
// overlaps the collective of one node range with the kernels of the next (dist.py).
constexpr int kBinItems = 8;
constexpr int kBinRowsPerBlock = 256 * kBinItems;
static_assert(kBinRowsPerBlock == FSW_BIN_BLOCK_ROWS, "include/fsw_hip.h documents the chunk granularity");

static __global__ void __launch_bounds__(256) k_bin_count(const int32_t* __restrict__ rowptr, int64_t n, int64_t chunk_rows,
                                                          int32_t* __restrict__ bin_count, int32_t* __restrict__ stats) {
  __shared__ int lbin[FSW_NUM_BINS];
  __shared__ int lmax;
  if (threadIdx.x < FSW_NUM_BINS) lbin[threadIdx.x] = 0;
  if (threadIdx.x == 0) lmax = 0;
  __syncthreads();
  int mx = 0;
  const int64_t r0 = (int64_t)blockIdx.x * kBinRowsPerBlock + threadIdx.x;
#pragma unroll
  for (int i = 0; i < kBinItems; ++i) {
    const int64_t r = r0 + (int64_t)i * 256;
    const bool valid = r < n;
    const int deg = valid ? rowptr[r + 1] - rowptr[r] : 0;
    const int bin = degree_bin(deg);
    mx = max(mx, deg);
    const unsigned long long peers = match_bin(bin, valid);
    if (valid && lane_id() == __ffsll((long long)peers) - 1) atomicAdd(&lbin[bin], __popcll(peers));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
  if (lane_id() == 0) atomicMax(&lmax, mx);
  __syncthreads();
  const int64_t chunk = ((int64_t)blockIdx.x * kBinRowsPerBlock) / chunk_rows;
  if (threadIdx.x < FSW_NUM_BINS && lbin[threadIdx.x]) atomicAdd(&bin_count[chunk * FSW_NUM_BINS + threadIdx.x], lbin[threadIdx.x]);
  if (threadIdx.x == 0 && lmax) atomicMax(&stats[FSW_STAT_MAX_DEGREE], lmax);
}

static __global__ void __launch_bounds__(kMaxRowChunks) k_bin_offsets(const int32_t* __restrict__ bin_count, int32_t* __restrict__ bin_start,
                                                                      int32_t* __restrict__ bin_cursor, int32_t* __restrict__ stats,
                                                                      int num_chunks, const int32_t* __restrict__ rowptr, int64_t num_rows) {
  __shared__ int ctot[kMaxRowChunks];
  const int c = threadIdx.x;
  if (c == 0) stats[FSW_STAT_NNZ] = rowptr[num_rows];   // CSR entries in use (invalid edges dropped, parallel edges merged or not)
  int tot = 0;
  if (c < num_chunks)
    for (int b = 0; b < FSW_NUM_BINS; ++b) tot += bin_count[c * FSW_NUM_BINS + b];
  ctot[c] = tot;
  __syncthreads();
  if (c == 0) {
    int acc = 0;
    for (int i = 0; i < num_chunks; ++i) {
      const int t = ctot[i];
      ctot[i] = acc;
      acc += t;
    }
  }
  __syncthreads();
  if (c < num_chunks) {
    int acc = ctot[c], reg = 0, mid = 0;
    const int32_t* cnt = bin_count + c * FSW_NUM_BINS;
    int32_t* bs = bin_start + c * (FSW_NUM_BINS + 1);
    for (int b = 0; b < FSW_NUM_BINS; ++b) {
      bs[b] = acc;
      bin_cursor[c * FSW_NUM_BINS + b] = acc;
      if (b >= 1 && b <= FSW_REG_MAX_DEG) reg += cnt[b];
      if (b >= FSW_BIN_MID0 && b < FSW_BIN_HUB0) mid += cnt[b];
      acc += cnt[b];
    }
    bs[FSW_NUM_BINS] = acc;
    if (cnt[0]) atomicAdd(&stats[FSW_STAT_NUM_ZERO_DEG], cnt[0]);
    if (reg) atomicAdd(&stats[FSW_STAT_NUM_REG], reg);
    if (mid) atomicAdd(&stats[FSW_STAT_NUM_LDS], mid);
    int glob = 0;
    for (int b = FSW_BIN_HUB0; b <= FSW_BIN_GLOBAL; ++b) glob += cnt[b];
    if (glob) atomicAdd(&stats[FSW_STAT_NUM_GLOBAL], glob);
  }
}

// k_bin_offsets without its serial walk (the packed path): one wavefront per chunk.  Lane b holds the count of bin b, a wave scan gives
// the bin's offset inside the chunk, and the chunk's base is the sum of all counters of the chunks before it (coalesced loads, a
// wave reduction) -- no thread walks 50 dependent loads, and the chunks do not wait for one thread's scan over them.
static_assert(FSW_NUM_BINS <= kWave, "one lane per bin");
static __global__ void __launch_bounds__(kWave) k_bin_offsets_wave(const int32_t* __restrict__ bin_count, int32_t* __restrict__ bin_start,
                                                                   int32_t* __restrict__ bin_cursor, int32_t* __restrict__ stats,
                                                                   const int32_t* __restrict__ rowptr, int64_t num_rows) {
  const int c = blockIdx.x, b = threadIdx.x;
  if (c == 0 && b == 0) stats[FSW_STAT_NNZ] = rowptr[num_rows];
  int before = 0;
  for (int i = b; i < c * FSW_NUM_BINS; i += kWave) before += bin_count[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
  const int cnt = b < FSW_NUM_BINS ? bin_count[c * FSW_NUM_BINS + b] : 0;
  const int inc = wave_inclusive_scan(cnt);
  if (b < FSW_NUM_BINS) {
    bin_start[c * (FSW_NUM_BINS + 1) + b] = before + inc - cnt;
    bin_cursor[c * FSW_NUM_BINS + b] = before + inc - cnt;
  }
  if (b == FSW_NUM_BINS - 1) bin_start[c * (FSW_NUM_BINS + 1) + FSW_NUM_BINS] = before + inc;
  // the stats words: sums of the counters over classes of bins
  int reg = (b >= 1 && b <= FSW_REG_MAX_DEG) ? cnt : 0;
  int mid = (b >= FSW_BIN_MID0 && b < FSW_BIN_HUB0) ? cnt : 0;
  int glob = (b >= FSW_BIN_HUB0 && b <= FSW_BIN_GLOBAL) ? cnt : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    reg += __shfl_xor(reg, off);
    mid += __shfl_xor(mid, off);
    glob += __shfl_xor(glob, off);
  }
  if (b == 0) {
    if (cnt) atomicAdd(&stats[FSW_STAT_NUM_ZERO_DEG], cnt);
    if (reg) atomicAdd(&stats[FSW_STAT_NUM_REG], reg);
    if (mid) atomicAdd(&stats[FSW_STAT_NUM_LDS], mid);
    if (glob) atomicAdd(&stats[FSW_STAT_NUM_GLOBAL], glob);
  }
}

// A workgroup places kBinRowsPerBlock consecutive rows: per-bin counts accumulate in LDS over the rounds (a lane's rank
// is the running count before its round + its rank among its wave peers), then ONE global atomic per bin claims the
// workgroup's range -- the cursors of a chunk are shared by all its workgroups, so same-address atomics are the cost to
// keep low.
static __global__ void __launch_bounds__(256) k_bin_rows(const int32_t* __restrict__ rowptr, int64_t n, int64_t chunk_rows,
                                                         int32_t* __restrict__ bin_cursor, int32_t* __restrict__ perm,
                                                         int32_t* __restrict__ invperm) {
  __shared__ int lcount[FSW_NUM_BINS];
  __shared__ int lbase[FSW_NUM_BINS];
  if (threadIdx.x < FSW_NUM_BINS) lcount[threadIdx.x] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kBinRowsPerBlock + threadIdx.x;
  int bin[kBinItems], rank[kBinItems];
#pragma unroll
  for (int i = 0; i < kBinItems; ++i) {
    const int64_t r = r0 + (int64_t)i * 256;
    const bool valid = r < n;
    bin[i] = valid ? degree_bin(rowptr[r + 1] - rowptr[r]) : 0;
    const unsigned long long peers = match_bin(bin[i], valid);
    const int leader = __ffsll((long long)peers) - 1;
    int prev = 0;
    if (valid && lane_id() == leader) prev = atomicAdd(&lcount[bin[i]], __popcll(peers));   // one LDS atomic per bin and wave
    rank[i] = __shfl(prev, leader) + __popcll(peers & ((1ull << lane_id()) - 1ull));
  }
  __syncthreads();
  const int64_t chunk = ((int64_t)blockIdx.x * kBinRowsPerBlock) / chunk_rows;
  if (threadIdx.x < FSW_NUM_BINS && lcount[threadIdx.x])
    lbase[threadIdx.x] = atomicAdd(&bin_cursor[chunk * FSW_NUM_BINS + threadIdx.x], lcount[threadIdx.x]);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kBinItems; ++i) {
    const int64_t r = r0 + (int64_t)i * 256;
    if (r < n) {
      const int pos = lbase[bin[i]] + rank[i];
      perm[pos] = (int32_t)r;
      if (invperm) invperm[r] = pos;
    }
  }
}

// chunk_rows == 0: one chunk of all rows
static int64_t one_chunk_if_zero(int64_t num_rows, int64_t chunk_rows) {
  return chunk_rows > 0 ? chunk_rows : ceil_div(num_rows, kBinRowsPerBlock) * kBinRowsPerBlock;
}

// bin_count (zeroed by the caller), bin_cursor: [kMaxRowChunks][FSW_NUM_BINS] int32 each.  wave_offsets: k_bin_offsets_wave after a
// k_bin_count of its own (the import; the builds keep the kernels they were measured with)
static int finish_bins(int32_t* rowptr, int64_t num_rows, int64_t chunk_rows, int32_t* perm, int32_t* invperm, int32_t* bin_start,
                       int32_t* stats, int32_t* bin_count, int32_t* bin_cursor, hipStream_t stream, bool counted = false,
                       bool wave_offsets = false) {
  chunk_rows = one_chunk_if_zero(num_rows, chunk_rows);
  const int num_chunks = (int)ceil_div(num_rows, chunk_rows);
  const int row_blocks = (int)ceil_div(num_rows, kBinRowsPerBlock);
  if (!counted) {   // counted: bin_count and the maximal degree came from the bucket kernel of the packed two-level build
    k_bin_count<<<row_blocks, 256, 0, stream>>>(rowptr, num_rows, chunk_rows, bin_count, stats);
    FSW_LAUNCH_CHECK();
  }
  if (counted || wave_offsets)
    k_bin_offsets_wave<<<num_chunks, kWave, 0, stream>>>(bin_count, bin_start, bin_cursor, stats, rowptr, num_rows);
  else
    k_bin_offsets<<<1, kMaxRowChunks, 0, stream>>>(bin_count, bin_start, bin_cursor, stats, num_chunks, rowptr, num_rows);
  FSW_LAUNCH_CHECK();
  k_bin_rows<<<row_blocks, 256, 0, stream>>>(rowptr, num_rows, chunk_rows, bin_cursor, perm, invperm);
  FSW_LAUNCH_CHECK();
  return 0;
}

static int check_chunks(int64_t num_rows, int64_t chunk_rows) {
  FSW_REQUIRE(chunk_rows >= 0 && chunk_rows % kBinRowsPerBlock == 0,
              "fsw_graph_build: chunk_rows must be 0 or a positive multiple of %d", kBinRowsPerBlock);
  FSW_REQUIRE(chunk_rows == 0 || ceil_div(num_rows, chunk_rows) <= kMaxRowChunks, "fsw_graph_build: more than %d row chunks",
              kMaxRowChunks);
  return 0;
}

}  // namespace fsw
