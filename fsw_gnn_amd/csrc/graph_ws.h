// Workspace of the CSR build (graph_build.hip): which scratch regions a build of (num_rows, num_edges) needs and where they lie.
// Host only, plain C++ without HIP types: tests/native/test_graph_ws.cpp sweeps the layout on the CPU with the functions the library
// calls.  Callers: fsw_graph_workspace_bytes and every entry point of graph_build.hip (carve).
//
// One buffer, carved into regions that start on 256-byte boundaries (E = max(num_edges, 1), ntiles = ceil(E / kRsTile)):
//   keys[2]         4 E bytes each   ping-pong of the uint32 sort keys
//   vals[2]         8 E bytes each   ping-pong of the values: uint32 sender / edge id, or uint64 sender | weight bits.  The coalescing
//                                    build reuses the idle one as head[E] | pos[E] (two int32 per edge: exactly 8 E bytes)
//   counts          [kRsMaxDigits][ntiles] int32: the digit-major count table of one radix pass
//   block_sums      block_sums_cap int32: the block totals of exclusive_scan_i32, one per kScanTile scanned elements.  Sized for the
//                   LARGEST scan any caller runs: the count table of a 9-bit pass (kRsMaxDigits * ntiles elements) and the head flags
//                   of the coalescing build (E elements, i.e. ntiles blocks -- 8 x the former from two tiles on).  The scan is told the
//                   capacity and refuses a longer input with a status code before it launches anything.
//   block_sums_big  bucket starts of the two-level build (multi-pass case): rows / 2^11 + 2 entries
//   bin_count, bin_cursor   [kMaxRowChunks][FSW_NUM_BINS] int32 each
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/fsw_hip.h"

namespace fsw {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 16;
constexpr int kScanTile = kScanThreads * kScanItems;   // elements per workgroup of exclusive_scan_i32 = per entry of block_sums
constexpr int kRsTile = 4096;                          // edges per tile of the radix passes
constexpr int kRsMaxDigits = 512;                      // 9 bits: the bucket pass of the two-level build
constexpr int kMaxRowChunks = 256;
constexpr size_t kBinTableBytes = sizeof(int32_t) * kMaxRowChunks * FSW_NUM_BINS;
constexpr size_t kWsAlign = 256;
static_assert(kMaxRowChunks == FSW_MAX_ROW_CHUNKS, "include/fsw_hip.h documents the number of row chunks");

inline size_t ws_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t ws_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

enum GraphWsRegion {
  kWsKeys0, kWsKeys1, kWsVals0, kWsVals1, kWsCounts, kWsBlockSums, kWsBlockSumsBig, kWsBinCount, kWsBinCursor, kWsNumRegions
};

struct GraphWsLayout {
  size_t off[kWsNumRegions];     // byte offset of every region, a multiple of kWsAlign
  size_t bytes[kWsNumRegions];   // bytes the region is used for (its slot is rounded up to kWsAlign)
  int64_t block_sums_cap;        // entries of block_sums
  size_t total;
};

inline GraphWsLayout graph_ws_layout(int64_t num_edges, int64_t num_rows) {
  const size_t E = (size_t)(num_edges > 1 ? num_edges : 1);
  const size_t ntiles = ws_ceil_div(E, kRsTile);
  const size_t rows = (size_t)(num_rows > 0 ? num_rows : 0);
  GraphWsLayout l;
  const size_t radix_blocks = ws_ceil_div((size_t)kRsMaxDigits * ntiles, kScanTile);   // scan of the count table
  const size_t edge_blocks = ntiles;                                                    // scan of one int per edge
  static_assert(kScanTile == kRsTile, "edge_blocks = ceil(E / kScanTile)");
  l.block_sums_cap = (int64_t)((radix_blocks > edge_blocks ? radix_blocks : edge_blocks) + 1);
  l.bytes[kWsKeys0] = l.bytes[kWsKeys1] = 4 * E;
  l.bytes[kWsVals0] = l.bytes[kWsVals1] = 8 * E;
  l.bytes[kWsCounts] = 4 * (size_t)kRsMaxDigits * ntiles;
  l.bytes[kWsBlockSums] = 4 * (size_t)l.block_sums_cap;
  l.bytes[kWsBlockSumsBig] = 4 * ((rows >> 10) + 3);
  l.bytes[kWsBinCount] = l.bytes[kWsBinCursor] = kBinTableBytes;
  size_t p = 0;
  for (int r = 0; r < kWsNumRegions; ++r) {
    l.off[r] = p;
    p += ws_align_up(l.bytes[r], kWsAlign);
  }
  l.total = p;
  return l;
}

struct GraphWs {
  uint32_t* keys[2];
  void* vals[2];
  int32_t* counts;      // [ndigits][ntiles]
  int32_t* block_sums;  // scan scratch, block_sums_cap entries
  int64_t block_sums_cap;
  int32_t* block_sums_big;  // bucket starts of the two-level build (multi-pass case): rows / 2^11 + 2 entries
  int32_t* bin_count;
  int32_t* bin_cursor;
  size_t total;
};

inline GraphWs carve(void* ws, int64_t num_edges, int64_t num_rows = 0) {
  const GraphWsLayout l = graph_ws_layout(num_edges, num_rows);
  char* base = reinterpret_cast<char*>(ws);
  auto at = [&](int r) -> void* { return base ? base + l.off[r] : nullptr; };   // no arithmetic on a null base (size query)
  GraphWs g;
  g.keys[0] = reinterpret_cast<uint32_t*>(at(kWsKeys0));
  g.keys[1] = reinterpret_cast<uint32_t*>(at(kWsKeys1));
  g.vals[0] = at(kWsVals0);
  g.vals[1] = at(kWsVals1);
  g.counts = reinterpret_cast<int32_t*>(at(kWsCounts));
  g.block_sums = reinterpret_cast<int32_t*>(at(kWsBlockSums));
  g.block_sums_cap = l.block_sums_cap;
  g.block_sums_big = reinterpret_cast<int32_t*>(at(kWsBlockSumsBig));
  g.bin_count = reinterpret_cast<int32_t*>(at(kWsBinCount));
  g.bin_cursor = reinterpret_cast<int32_t*>(at(kWsBinCursor));
  g.total = l.total;
  return g;
}

// ---- constants of the two-level build that decide which path a shape takes (graph_plan.h: two_level_plan) ----
constexpr int kBucketWaves = 8;
#ifndef FSW_BUCKET_ROW_BITS
#define FSW_BUCKET_ROW_BITS 11
#endif
constexpr int kBucketMaxRowBits = FSW_BUCKET_ROW_BITS;   // LDS: (kBucketWaves + 1) * 2^bits ints (72 KB at 11, 144 KB at 12)
constexpr int kPartitionBits = 9;                        // bits of a partition pass

// shapes the two-level build is meant for: enough rows for a partition pass, buckets that one workgroup finishes quickly
static bool two_level_ok(int64_t num_rows, int64_t num_edges) {
  if (num_rows < (1 << 15) || num_edges < (1 << 18)) return false;
  const int64_t nbuckets = (num_rows + 1 + ((int64_t)1 << kBucketMaxRowBits) - 1) >> kBucketMaxRowBits;
  return num_edges / nbuckets <= (1 << 16);
}

// LDS of the bucket kernel that is left for a staging tile beside its tables
inline size_t bucket_stage_room(size_t tables) {
  const size_t room = (size_t)160 * 1024 - 1024 - tables;                      // 1 KB for the static arrays
  return room;
}

}  // namespace fsw
