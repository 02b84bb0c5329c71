// Host-side checks of the packed path of the two-level CSR build (fsw_gnn_amd/csrc/graph_plan.h), with the functions the library and
// its kernels call: the packed edge word round-trips at sender widths 1, 20, 21 and 22 (row field at its widest for each), the packed
// path is taken exactly for unit weights, one partition pass and rb + cb <= 32, two_level_ok / two_level_plan / graph_plan_words --
// what the build and fsw_graph_build_plan call -- give the expected path at every boundary, and for the 6 x 10 (rows, edges) pairs of
// test_graph_ws.cpp the count table of a packed partition pass (any digit width up to 9 bits) and the block sums of its scan fit the
// regions carve() hands out -- the last entry of both is written, so the sanitizers watch.
#include <cstdio>
#include <cstdlib>
#include "../../fsw_gnn_amd/csrc/graph_plan.h"

using namespace fsw;

static int bad = 0;
static long long ctx_a = 0, ctx_b = 0;
#define CHECK(cond)                                                                                              \
  do {                                                                                                           \
    if (!(cond)) {                                                                                               \
      if (bad < 20) printf("line %d: (%lld, %lld): %s\n", __LINE__, ctx_a, ctx_b, #cond);                       \
      ++bad;                                                                                                     \
    }                                                                                                            \
  } while (0)

int main() {
  // key_bits / sender_bits: values 0 .. range fit
  CHECK(key_bits(0) == 1 && key_bits(1) == 1 && key_bits(2) == 2 && key_bits(2047) == 11 && key_bits(2048) == 12);
  CHECK(key_bits(32768) == 16 && key_bits((1ll << 20) - 1) == 20 && key_bits(1ll << 20) == 21 && key_bits((1ll << 31) - 2) == 31);
  CHECK(sender_bits(1) == 1 && sender_bits(2) == 1 && sender_bits(3) == 2 && sender_bits(1 << 20) == 20 && sender_bits((1 << 20) + 1) == 21);
  CHECK(sender_bits(1 << 21) == 21 && sender_bits((1 << 21) + 1) == 22 && sender_bits((1ll << 31) - 1) == 31);

  // the word: row field and sender come back, at the widest row field that still fits beside cb sender bits
  const int kCb[] = {1, 20, 21, 22};
  for (int cb : kCb) {
    const int rb = 32 - cb < 11 ? 32 - cb : 11;
    const uint32_t rmask = (1u << rb) - 1u, smax = (1u << cb) - 1u;
    ctx_a = cb;
    const uint32_t rows[] = {0u, 1u, rmask - 1u, rmask, rmask + 1u, 0x7ffffffeu, 0x12345678u};
    const uint32_t snds[] = {0u, 1u, smax / 2u, smax - 1u, smax};
    for (uint32_t row : rows)
      for (uint32_t snd : snds) {
        ctx_b = row;
        const uint32_t w = pack_edge(row, rmask, cb, snd);
        CHECK(edge_row(w, cb) == (row & rmask));
        CHECK(edge_sender(w, cb) == snd);
        // the bucket kernel's validity test: b * R + row field < num_rows, for the row itself and for a sentinel one above it
        const int64_t b = row >> rb;
        CHECK(b * ((int64_t)1 << rb) + edge_row(w, cb) == (int64_t)row);
      }
    // order inside a bucket is the order of the row fields: a larger row field gives a larger word whatever the senders
    CHECK(pack_edge(5, rmask, cb, 0) > pack_edge(4, rmask, cb, smax));
  }

  // which shapes are packed (rb = 11 on every two-level shape)
  ctx_a = ctx_b = 0;
  CHECK(packed_ok(false, 9, 9, 11, 21) && packed_ok(false, 5, 5, 11, 1) && packed_ok(false, 9, 9, 11, 20));
  CHECK(!packed_ok(false, 9, 9, 11, 22));     // 33 bits
  CHECK(!packed_ok(true, 9, 9, 11, 20));      // weights travel with the sender
  CHECK(!packed_ok(false, 5, 10, 11, 20));    // two partition passes: the digit of the last pass is not the bucket
  CHECK(packed_ok(false, 9, 9, 10, 22) && !packed_ok(false, 9, 9, 10, 23));

  // the plan itself, with the functions the build calls, at the boundaries of its paths: rows, cols, edges, weights ->
  // two-level, packed, edges per tile, sender bits, partition passes
  struct Shape { int64_t rows, cols, edges; bool weighted; int two, packed, tile, cb, passes; };
  const Shape kShapes[] = {
      {32768, 32768, 262144, false, 1, 1, kPackTile, 15, 1},
      {32767, 32768, 262144, false, 0, 0, 0, 0, 0},
      {32768, 32768, 262143, false, 0, 0, 0, 0, 0},
      {32768, (int64_t)1 << 21, 262144, false, 1, 1, kPackTile, 21, 1},
      {32768, ((int64_t)1 << 21) + 1, 262144, false, 1, 0, kRsTile, 22, 1},
      {32768, 32768, 262144, true, 1, 0, kRsTile, 15, 1},
      {1000000, 1000000, 10000000, false, 1, 1, kPackTile, 20, 1},
      {((int64_t)1 << 20) - 1, (int64_t)1 << 20, 2000000, false, 1, 1, kPackTile, 20, 1},
      {(int64_t)1 << 20, (int64_t)1 << 20, 2000000, false, 1, 0, kRsTile, 20, 2},
      {40000, 40000, 1400000, false, 0, 0, 0, 0, 0},
      {40000, 40000, 0, false, 0, 0, 0, 0, 0},
  };
  for (const Shape& sh : kShapes) {
    ctx_a = sh.rows;
    ctx_b = sh.edges;
    int32_t w[kPlanNumWords];
    graph_plan_words(sh.rows, sh.cols, sh.edges, sh.weighted, w);
    CHECK(w[kPlanTwoLevel] == sh.two && w[kPlanPacked] == sh.packed && w[kPlanTile] == sh.tile && w[kPlanSenderBits] == sh.cb);
    CHECK(w[kPlanPasses] == sh.passes);
    CHECK((sh.edges > 0 && two_level_ok(sh.rows, sh.edges)) == (sh.two == 1));
    if (sh.two) {
      const TwoLevelPlan p = two_level_plan(sh.rows, sh.cols, sh.edges, sh.weighted);
      CHECK(p.rb == 11 && w[kPlanRowBits] == 11 && p.nbuckets == (sh.rows + 1 + 2047) / 2048 && w[kPlanBuckets] == p.nbuckets);
      CHECK(p.ntiles == (sh.edges + p.tile - 1) / p.tile && (p.packed ? p.bits == p.upper : true));
      CHECK(p.nbuckets <= ((int64_t)1 << p.upper));                           // the bucket kernel indexes the count table by bucket
      // 8-byte values: the average bucket of the weighted shape (15 421 edges) does not fit the staging tile of 11 136 entries
      CHECK(p.stage_cap == (sh.weighted ? 0 : 22272) && p.lds == p.tables + (size_t)p.stage_cap * (sh.weighted ? 8 : 4));
      CHECK(p.lds <= (size_t)160 * 1024 - 1024);
      CHECK(plan_fits_workspace(p, graph_ws_layout(sh.edges, sh.rows)));
    }
  }
  ctx_a = ctx_b = 0;

  // the count table and the scan of a packed pass inside the workspace
  const int64_t kRows[] = {1, 1000, 62463, 62464, 200000, (int64_t)1 << 24};
  const int64_t kEdges[] = {0, 1, 4096, 4097, 262144, 262145, 524289, 1310721, 5000000, ((int64_t)1 << 31) - 4097};
  int cells = 0;
  for (int64_t rows : kRows)
    for (int64_t E : kEdges) {
      ctx_a = rows;
      ctx_b = E;
      const GraphWsLayout l = graph_ws_layout(E, rows);
      const int64_t En = E > 1 ? E : 1;
      if (E > 0 && two_level_ok(rows, E)) {   // the shapes of the sweep the two-level build takes: their own plan
        const TwoLevelPlan p = two_level_plan(rows, rows, E, false);
        CHECK(plan_fits_workspace(p, l));
        CHECK(p.packed == (p.passes == 1 && p.rb + p.cb <= 32));
      }
      for (int bits = 1; bits <= 9; ++bits) {
        TwoLevelPlan p = {};
        p.bits = bits;
        p.tile = kPackTile;
        p.ntiles = (En + kPackTile - 1) / kPackTile;
        CHECK(plan_fits_workspace(p, l));
        CHECK(p.ntiles <= (En + kRsTile - 1) / kRsTile);
      }
      {  // the check can fail: a 9-bit table of one tile more than the region is sized for (tiles of kRsTile)
        TwoLevelPlan p = {};
        p.bits = 9;
        p.ntiles = (En + kRsTile - 1) / kRsTile + 1;
        CHECK(!plan_fits_workspace(p, l));
      }
      if (l.total <= ((size_t)64 << 20)) {
        char* buf = static_cast<char*>(malloc(l.total));
        CHECK(buf != nullptr);
        if (buf) {
          const GraphWs g = carve(buf, E, rows);
          const int64_t ntiles = (En + kPackTile - 1) / kPackTile;
          const int64_t n = (int64_t)kRsMaxDigits * ntiles;
          g.counts[n - 1] = 1;                                               // [digit 511][last tile]
          g.block_sums[(n + kScanTile - 1) / kScanTile - 1] = 1;             // the scan's last block total
          g.keys[1][En - 1] = 1;                                             // the last packed word
          CHECK((char*)(g.counts + n) <= buf + l.off[kWsCounts] + l.bytes[kWsCounts]);
          CHECK((n + kScanTile - 1) / kScanTile <= g.block_sums_cap);
          free(buf);
        }
      }
      ++cells;
    }
  ctx_a = ctx_b = 0;
  CHECK(cells == 60);
  printf("%d cells, %d failed checks\n%s\n", cells, bad, bad ? "FAILED" : "OK");
  return bad ? 1 : 0;
}
