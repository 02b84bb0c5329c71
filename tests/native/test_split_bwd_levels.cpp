// Host-side run of the merge levels of the split backward (fsw_gnn_amd/csrc/embed_split_cart_bwd.hip: k_split_bwd_level) with the
// kernel's own span helpers (fsw_gnn_amd/csrc/merge_path64_span.h) and the tile helpers of merge_path64.h.  Every level is a set of
// spans; a span is what one workgroup does: the boundaries of its own merge tiles by binary search in the level's SOURCE region, its
// tiles merged into the other region, its share of the run without a partner copied.  The spans of every level run in REVERSED and in
// shuffled order: a span that read another span's output of the same level would see a word that is not yet written (the destination
// is poisoned before every level).  Every word of the destination is written exactly once per level.  Lines of 2048 x {1, 2, 3, 17, 32,
// 33, 49, 69} distinct random words; the result is compared word for word with std::sort, in the region that the parity of the level
// count names (ping after an even number of levels, pong after an odd number).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../fsw_gnn_amd/csrc/merge_path64_span.h"

using namespace fsw;

static int bad = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (bad < 20) printf("line %d: %s\n", __LINE__, #cond);             \
      ++bad;                                                              \
    }                                                                     \
  } while (0)

static const mp64_t kPoison = 0x5555555555555555ull;

// one span as the workgroup runs it: src -> dst; written counts the stores to every word of dst
static void run_span(const mp64_t* src, mp64_t* dst, int total, const Mp64Level& lv, int span, int sp, std::vector<int>& written) {
  Mp64Span s;
  if (!mp64_span(total, lv, span, sp, s)) return;
  CHECK(s.nt >= 0 && s.nt <= span && s.nt <= kMp64MaxSpan && s.t0 >= 0 && s.t0 + s.nt <= lv.ntiles);
  CHECK(s.c0 <= s.c1 && s.c0 >= lv.covered && s.c1 <= total && (s.c1 - s.c0) % kMp64Tile == 0);
  CHECK(s.nt + (s.c1 - s.c0) / kMp64Tile > 0);
  std::vector<mp64_t> tk(kMp64TileLds);
  std::vector<int> part(kMp64MaxSpan + 1);
  if (s.nt > 0) {
    for (int tid = 0; tid < kMp64NT; ++tid)
      for (int i = tid; i <= s.nt; i += kMp64NT) part[i] = mp64_boundary(src, total, lv, (s.t0 + i) * kMp64Tile);
    for (int i = 0; i < s.nt; ++i) {
      const Mp64TileGeo g = mp64_tile_geo(total, lv, s.t0 + i, part[i], part[i + 1]);
      const int nbb = kMp64Tile - g.na;
      CHECK(g.na >= 0 && g.na <= kMp64Tile && g.pos + kMp64Tile <= lv.covered);
      std::fill(tk.begin(), tk.end(), ~0ull);
      for (int tid = 0; tid < kMp64NT; ++tid)
        for (int u = 0; u < kMp64VT; ++u) {
          const int e = tid + u * kMp64NT, from = mp64_tile_src(g, lv.R, e);
          CHECK(from >= 0 && from < total);
          if (from < 0 || from >= total) continue;
          tk[mp64_pad(e)] = src[from];
        }
      for (int tid = 0; tid < kMp64NT; ++tid) {
        const int dd = tid * kMp64VT;
        mp64_t out[kMp64VT];
        mp64_merge_serial(tk.data(), g.na, nbb, dd, mp64_split_tile(tk.data(), g.na, nbb, dd), out);
        for (int j = 0; j < kMp64VT; ++j) {
          dst[g.pos + dd + j] = out[j];
          ++written[g.pos + dd + j];
        }
      }
    }
  }
  // its share of the run without a partner
  for (int tid = 0; tid < kMp64NT; ++tid) mp64_copy_run(src, dst, s.c0, s.c1, tid);
  for (int e = s.c0; e < s.c1; ++e) {
    CHECK(dst[e] == src[e]);
    ++written[e];
  }
}

enum Order { REVERSED, SHUFFLED };

static void check_line(int nruns, int span, Order order, unsigned seed) {
  const int total = nruns * kMp64Run;
  std::mt19937_64 rng(seed);
  std::vector<mp64_t> line(total);
  for (int t = 0; t < total; ++t) line[t] = (rng() & ~0xffffffffull) | (unsigned)t;   // distinct: the index is the low half
  std::shuffle(line.begin(), line.end(), rng);
  std::vector<mp64_t> region[2] = {line, std::vector<mp64_t>(total, kPoison)};          // ping, pong
  for (int r = 0; r < nruns; ++r) std::sort(region[0].begin() + r * kMp64Run, region[0].begin() + (r + 1) * kMp64Run);   // k_split_bwd_runs
  const int nspans = mp64_num_spans(total, span);
  CHECK(nspans * span >= total / kMp64Tile && (nspans - 1) * span < total / kMp64Tile);
  int k = 0;
  for (; mp64_level_run(k) < (int64_t)total; ++k) {
    const Mp64Level lv = mp64_level(total, (int)mp64_level_run(k));
    const std::vector<mp64_t>& src = region[k & 1];
    std::vector<mp64_t>& dst = region[(k + 1) & 1];
    std::fill(dst.begin(), dst.end(), kPoison);
    std::vector<int> written(total, 0), spans(nspans + 2);                              // two spans past the line: they must leave at once
    for (int i = 0; i < nspans + 2; ++i) spans[i] = i;
    if (order == REVERSED) std::reverse(spans.begin(), spans.end());
    else std::shuffle(spans.begin(), spans.end(), rng);
    for (int sp : spans) run_span(src.data(), dst.data(), total, lv, span, sp, written);
    for (int e = 0; e < total; ++e) CHECK(written[e] == 1);
  }
  CHECK(k == mp64_num_levels(total));
  std::sort(line.begin(), line.end());
  CHECK(region[k & 1] == line);                      // ping after an even number of levels, pong after an odd number
}

int main() {
  static_assert(kMp64Tile == kMp64Run, "a tile slot is a run");
  const int runs[] = {1, 2, 3, 17, 32, 33, 49, 69};
  const int spans[] = {1, 3, 4, kMp64MaxSpan};
  unsigned seed = 1;
  for (int nruns : runs)
    for (int span : spans)
      for (Order order : {REVERSED, SHUFFLED}) check_line(nruns, span, order, seed++);
  if (bad) {
    printf("FAILED: %d checks\n", bad);
    return 1;
  }
  printf("OK\n");
  return 0;
}
