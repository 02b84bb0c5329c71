// Host-side sweep of the CSR build's workspace layout (fsw_gnn_amd/csrc/graph_ws.h), with the functions the library calls.
// For every (rows, edges) pair: block_sums holds one entry per kScanTile elements of BOTH scans the build runs (the count table of a
// 9-bit radix pass and the per-edge head flags of the coalescing build), head[E] | pos[E] of the coalescing build fit the idle value
// buffer, and the regions are disjoint, 256-byte aligned, in order and inside `total`.  carve() maps the layout onto a base pointer
// region by region and touches no pointer when the base is null (the size query).
#include <cstdio>
#include <cstdlib>
#include "../../fsw_gnn_amd/csrc/graph_ws.h"

using namespace fsw;

static int bad = 0;
#define CHECK(cond)                                                                                   \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      if (bad < 20) printf("line %d: rows %lld edges %lld: %s\n", __LINE__, (long long)rows, (long long)E, #cond); \
      ++bad;                                                                                          \
    }                                                                                                 \
  } while (0)

int main() {
  const int64_t kRows[] = {1, 1000, 62463, 62464, 200000, (int64_t)1 << 24};
  const int64_t kEdges[] = {0, 1, 4096, 4097, 262144, 262145, 524289, 1310721, 5000000, ((int64_t)1 << 31) - 4097};
  int cells = 0;
  for (int64_t rows : kRows)
    for (int64_t E : kEdges) {
      const GraphWsLayout l = graph_ws_layout(E, rows);
      const int64_t En = E > 1 ? E : 1;
      const int64_t ntiles = (En + kRsTile - 1) / kRsTile;
      // the two scans
      CHECK(l.block_sums_cap >= (E + kScanTile - 1) / kScanTile);
      CHECK(l.block_sums_cap >= ((int64_t)kRsMaxDigits * ntiles + kScanTile - 1) / kScanTile);
      CHECK(l.bytes[kWsBlockSums] >= 4 * (size_t)l.block_sums_cap);
      // head | pos of the coalescing build live in vals[cur ^ 1], either one
      CHECK(l.bytes[kWsVals0] >= 2 * sizeof(int32_t) * (size_t)E && l.bytes[kWsVals1] >= 2 * sizeof(int32_t) * (size_t)E);
      CHECK(l.bytes[kWsVals0] == 8 * (size_t)En && l.bytes[kWsKeys0] >= 4 * (size_t)En && l.bytes[kWsKeys1] >= 4 * (size_t)En);
      // what the kernels index: the count table, the bucket starts (ceil((rows + 1) / 2048) + 1 entries), the bin tables
      CHECK(l.bytes[kWsCounts] >= sizeof(int32_t) * (size_t)kRsMaxDigits * (size_t)ntiles);
      CHECK(l.bytes[kWsBlockSumsBig] >= sizeof(int32_t) * (size_t)((rows + 1 + 2047) / 2048 + 1));
      CHECK(l.bytes[kWsBinCount] == kBinTableBytes && l.bytes[kWsBinCursor] == kBinTableBytes);
      // disjoint, aligned, inside total
      size_t end = 0;
      for (int r = 0; r < kWsNumRegions; ++r) {
        CHECK(l.off[r] % kWsAlign == 0);
        CHECK(l.off[r] >= end);
        CHECK(l.bytes[r] > 0);
        end = l.off[r] + l.bytes[r];
        CHECK(end <= l.total);
      }
      for (int a = 0; a < kWsNumRegions; ++a)
        for (int b = a + 1; b < kWsNumRegions; ++b)
          CHECK(l.off[a] + l.bytes[a] <= l.off[b] || l.off[b] + l.bytes[b] <= l.off[a]);
      // the size query (null base) and the pointers of a real base
      const GraphWs q = carve(nullptr, E, rows);
      CHECK(q.total == l.total && q.block_sums_cap == l.block_sums_cap && q.block_sums == nullptr && q.keys[0] == nullptr);
      if (l.total <= ((size_t)64 << 20)) {
        char* buf = static_cast<char*>(malloc(l.total));
        CHECK(buf != nullptr);
        if (buf) {
          const GraphWs g = carve(buf, E, rows);
          CHECK((char*)g.keys[0] == buf + l.off[kWsKeys0] && (char*)g.keys[1] == buf + l.off[kWsKeys1]);
          CHECK((char*)g.vals[0] == buf + l.off[kWsVals0] && (char*)g.vals[1] == buf + l.off[kWsVals1]);
          CHECK((char*)g.counts == buf + l.off[kWsCounts] && (char*)g.block_sums == buf + l.off[kWsBlockSums]);
          CHECK((char*)g.block_sums_big == buf + l.off[kWsBlockSumsBig]);
          CHECK((char*)g.bin_count == buf + l.off[kWsBinCount] && (char*)g.bin_cursor == buf + l.off[kWsBinCursor]);
          CHECK(g.total == l.total && g.block_sums_cap == l.block_sums_cap);
          // the last entry of both scans and of the bin tables is writable memory of the buffer (the sanitizers watch)
          g.block_sums[l.block_sums_cap - 1] = 1;
          g.bin_cursor[kMaxRowChunks * FSW_NUM_BINS - 1] = 1;
          reinterpret_cast<int32_t*>(g.vals[1])[2 * En - 1] = 1;
          free(buf);
        }
      }
      ++cells;
    }
  const int64_t rows = 0, E = 0;
  CHECK(cells == 60);
  // the workspace grows with the edges and never shrinks with the rows
  CHECK(graph_ws_layout(262145, 1000).total >= graph_ws_layout(262144, 1000).total);
  CHECK(graph_ws_layout(5000, 200000).total >= graph_ws_layout(5000, 1000).total);
  printf("%d cells, %d failed checks\n%s\n", cells, bad, bad ? "FAILED" : "OK");
  return bad ? 1 : 0;
}
