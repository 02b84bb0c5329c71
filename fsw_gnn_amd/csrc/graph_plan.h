// Packed edge word of the two-level CSR build (graph_build.hip) and what that build does with a shape.
// Host helpers in plain C++ (tests/native/test_graph_plan.cpp runs them on the CPU); pack_edge / edge_row / edge_sender are the
// functions the kernels call as well.
//
// The partition pass of the unit-weight two-level build groups the edges by bucket = row >> rb.  Inside a bucket only the low rb row
// bits still matter, and a sender needs cb = key_bits(num_cols - 1) bits, so when rb + cb <= 32 an edge travels as ONE uint32
//   word = (row & (2^rb - 1)) << cb | sender
// instead of a (key, sender) pair: the partition pass writes 4 bytes per edge instead of 8 and the bucket kernel reads 8 instead of
// 12.  An edge with an endpoint out of range keeps its sentinel row num_rows (it sorts behind every valid edge) and carries sender 0.
// With one word per edge the partition pass reorders kPackTile = 2 x kRsTile edges in the LDS the pair kernels need for kRsTile:
// runs of 16 edges per digit instead of 8 at 512 digits, and a count table of half as many tiles.
#pragma once
#include <stdint.h>
#include "graph_ws.h"

#if defined(__HIPCC__)
#define FSW_PLAN_HD __host__ __device__ inline
#else
#define FSW_PLAN_HD inline
#endif

namespace fsw {

// edges per tile of the packed partition pass.  Measured at config 3 (1M rows, 10M edges; whole build, the pair path 0.246-0.253 ms):
// 4096 0.218-0.224 ms, 8192 0.203-0.211 ms, 16384 0.223-0.231 ms (214 VGPRs and 116 KB of LDS: one workgroup per CU).
constexpr int kPackTile = 8192;
static_assert(kPackTile % kRsTile == 0, "the packed count table ([digits][tiles of kPackTile]) fits the region sized for kRsTile");

// number of bits that hold every value 0 .. range (range itself included: the sentinel key of the sorts)
inline int key_bits(int64_t range) {
  int keybits = 1;
  while ((1ll << keybits) <= range) ++keybits;
  return keybits;
}

FSW_PLAN_HD uint32_t pack_edge(uint32_t row, uint32_t rmask, int cb, uint32_t sender) { return ((row & rmask) << cb) | sender; }
FSW_PLAN_HD uint32_t edge_row(uint32_t word, int cb) { return word >> cb; }                       // the low rb bits of the row
FSW_PLAN_HD uint32_t edge_sender(uint32_t word, int cb) { return word & ((1u << cb) - 1u); }

// bits of a sender 0 .. num_cols - 1
inline int sender_bits(int64_t num_cols) { return key_bits(num_cols > 1 ? num_cols - 1 : 0); }

// The packed path: unit weights, ONE partition pass (its digit is the bucket, so the dropped upper row bits are the bucket index), and
// a word that holds both fields.  rb >= 1 and cb >= 1, so cb < 32 and every shift above is defined.
inline bool packed_ok(bool weighted, int pass_bits, int upper_bits, int rb, int cb) {
  return !weighted && pass_bits == upper_bits && rb + cb <= 32;
}

// fsw_graph_build_plan's out[] (int32)
enum GraphPlanWord {
  kPlanTwoLevel,     // 1: partition pass + bucket kernel; 0: the LSD passes (every other word is then 0)
  kPlanPacked,       // 1: one packed word per edge
  kPlanTile,         // edges per tile of the partition pass
  kPlanStageCap,     // entries of the bucket kernel's LDS staging tile (0: no staging)
  kPlanPasses,       // partition passes
  kPlanRowBits,      // rb: a bucket is 2^rb rows
  kPlanSenderBits,   // cb
  kPlanBuckets,
  kPlanNumWords
};

static_assert(kPlanNumWords == FSW_GRAPH_PLAN_WORDS, "include/fsw_hip.h documents the words of the plan");

struct TwoLevelPlan {
  int rb, upper, passes, bits, cb;
  bool packed;
  int tile;
  int64_t ntiles, nbuckets;
  int stage_cap;
  size_t tables, lds;
};

// What the two-level build does with a shape that two_level_ok (graph_ws.h) accepts -- the one place that decides it, for the build
// and for fsw_graph_build_plan.
inline TwoLevelPlan two_level_plan(int64_t num_rows, int64_t num_cols, int64_t num_edges, bool weighted) {
  TwoLevelPlan p;
  const int kb = key_bits(num_rows);
  p.rb = kBucketMaxRowBits < kb ? kBucketMaxRowBits : kb;
  p.nbuckets = (num_rows + 1 + ((int64_t)1 << p.rb) - 1) >> p.rb;
  p.upper = kb - p.rb;
  p.passes = (p.upper + kPartitionBits - 1) / kPartitionBits;   // how radix_sort_pairs splits the upper bits
  p.bits = p.passes ? (p.upper + p.passes - 1) / p.passes : 0;
  p.cb = sender_bits(num_cols);
  p.packed = p.passes == 1 && packed_ok(weighted, p.bits, p.upper, p.rb, p.cb);
  p.tile = p.packed ? kPackTile : kRsTile;
  p.ntiles = (int64_t)ws_ceil_div((size_t)num_edges, (size_t)p.tile);
  // LDS: the tables, and -- when the average bucket (+ 3 %) fits what is left of 160 KB -- a staging tile for the bucket's values
  // (one workgroup per CU then); without it two workgroups share a CU
  const size_t vsize = weighted ? sizeof(unsigned long long) : sizeof(uint32_t);
  const size_t tables = sizeof(int) * (size_t)(kBucketWaves + 1) * ((size_t)1 << p.rb);
  const size_t room = bucket_stage_room(tables);
  const int64_t avg = (num_edges + p.nbuckets - 1) / p.nbuckets;
  const int64_t want = avg + avg / 32 + 256;   // random graphs: max bucket ~ avg + 4 sqrt(avg); a larger bucket scatters
  p.stage_cap = (want * (int64_t)vsize <= (int64_t)room) ? (int)(room / vsize) : 0;
  p.tables = tables;
  p.lds = tables + (size_t)p.stage_cap * vsize;
  return p;
}

// fsw_graph_build_plan's out[]: zeros for a shape that takes the LSD passes
inline void graph_plan_words(int64_t num_rows, int64_t num_cols, int64_t num_edges, bool weighted, int32_t* out) {
  for (int i = 0; i < kPlanNumWords; ++i) out[i] = 0;
  if (num_edges == 0 || !two_level_ok(num_rows, num_edges)) return;
  const TwoLevelPlan p = two_level_plan(num_rows, num_cols, num_edges, weighted);
  out[kPlanTwoLevel] = 1;
  out[kPlanPacked] = p.packed;
  out[kPlanTile] = p.tile;
  out[kPlanStageCap] = p.stage_cap;
  out[kPlanPasses] = p.passes;
  out[kPlanRowBits] = p.rb;
  out[kPlanSenderBits] = p.cb;
  out[kPlanBuckets] = (int32_t)p.nbuckets;
}

// digits x tiles of the partition pass and the block sums of its scan fit the workspace of graph_ws.h
inline bool plan_fits_workspace(const TwoLevelPlan& p, const GraphWsLayout& l) {
  const size_t n = ((size_t)1 << p.bits) * (size_t)p.ntiles;
  return sizeof(int32_t) * n <= l.bytes[kWsCounts] && (int64_t)ws_ceil_div(n, kScanTile) <= l.block_sums_cap;
}

}  // namespace fsw
