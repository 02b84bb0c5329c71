// Host-side run of the merge levels of fsw_gnn_amd/csrc/merge_path64.h: the levels are emulated tile by tile and thread by thread with
// the helpers the kernel calls (level and tile geometry, diagonal split, serial merge, copy of a run without a partner).
// Lines of packed (key, entry index) words with many equal keys (-0 and +0 among them), the pad element (key 0, index D) and fill
// elements (key +inf), run counts 2, 3, 4, 5, 16, 17, 32, 33 and 69 with a last run that is full, one element long and one short of
// full.  After every level the line equals std::sort of the words of every pair of runs, at the end std::sort of the line, which is
// the stable order by key with the pad element last among the zeros.  Every staged tile holds exactly kMp64Tile words, every word of
// the paired runs is staged exactly once and no index leaves the line.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "../../fsw_gnn_amd/csrc/merge_path64.h"

using namespace fsw;

static int bad = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (bad < 20) printf("line %d: %s\n", __LINE__, #cond);             \
      ++bad;                                                              \
    }                                                                     \
  } while (0)

// one level as the workgroup runs it: src -> dst
static void run_level(const std::vector<mp64_t>& src, std::vector<mp64_t>& dst, int total, int R) {
  const Mp64Level lv = mp64_level(total, R);
  CHECK(lv.nruns >= 2 && lv.covered % kMp64Tile == 0 && lv.covered <= total && lv.covered % 2 == 0 && total % 2 == 0);
  std::vector<mp64_t> tk(kMp64TileLds);
  std::vector<int> part(kMp64Parts + 1), staged(total, 0);
  for (int g0 = 0; g0 < lv.ntiles; g0 += kMp64Parts) {
    const int cnt = mp64_min(kMp64Parts, lv.ntiles - g0);
    for (int tid = 0; tid < kMp64NT; ++tid)
      for (int i = tid; i <= cnt; i += kMp64NT) part[i] = mp64_boundary(src.data(), total, lv, (g0 + i) * kMp64Tile);
    for (int i = 0; i < cnt; ++i) {
      const Mp64TileGeo g = mp64_tile_geo(total, lv, g0 + i, part[i], part[i + 1]);
      const int nB = mp64_min(lv.R, total - g.pb - lv.R), nbb = kMp64Tile - g.na;
      CHECK(g.pos == (g0 + i) * kMp64Tile && g.pb % (2 * R) == 0 && g.pb <= g.pos && g.pos + kMp64Tile <= lv.covered);
      CHECK(g.na >= 0 && g.na <= kMp64Tile && g.a0 >= 0 && g.a0 + g.na <= lv.R);          // the A-part lies in run A
      CHECK(nbb >= 0 && g.b0 >= 0 && g.b0 + nbb <= nB);                                    // the B-part lies in run B
      std::fill(tk.begin(), tk.end(), ~0ull);
      int count = 0;
      for (int tid = 0; tid < kMp64NT; ++tid)
        for (int u = 0; u < kMp64VT; ++u) {
          const int e = tid + u * kMp64NT, from = mp64_tile_src(g, lv.R, e);
          CHECK(from >= 0 && from < total);
          if (from < 0 || from >= total) continue;
          CHECK(mp64_pad(e) < kMp64TileLds);
          ++staged[from];
          tk[mp64_pad(e)] = src[from];
          ++count;
        }
      CHECK(count == kMp64Tile);
      for (int tid = 0; tid < kMp64NT; ++tid) {
        const int dd = tid * kMp64VT;
        const int ia = mp64_split_tile(tk.data(), g.na, nbb, dd);
        CHECK(ia >= 0 && ia <= g.na && dd - ia >= 0 && dd - ia <= nbb);
        mp64_t out[kMp64VT];
        mp64_merge_serial(tk.data(), g.na, nbb, dd, ia, out);
        for (int j = 0; j < kMp64VT; ++j) dst[g.pos + dd + j] = out[j];
      }
    }
  }
  if (lv.nruns & 1)
    for (int tid = 0; tid < kMp64NT; ++tid) mp64_copy_run(src.data(), dst.data(), lv.covered, total, tid);
  else
    CHECK(lv.covered == total);
  for (int e = 0; e < total; ++e) CHECK(staged[e] == (e < lv.covered ? 1 : 0));
}

static void check_line(int nruns, int last, bool pad_element, unsigned seed) {
  const int total = nruns * kMp64Run;
  const int L = (nruns - 1) * kMp64Run + last;          // elements of the line; with pad_element the last one is the pad
  const int D = pad_element ? L - 1 : L;
  static const float vals[] = {-3.5f, -1.f, -0.f, 0.f, 0.f, 0.25f, 0.75f, 0.75f, 2.f, 1e30f};
  srand(seed);
  std::vector<float> key(total);
  std::vector<mp64_t> line(total);
  for (int t = 0; t < total; ++t) {
    key[t] = t < D ? (rand() % 4 ? vals[rand() % 10] : (float)(rand() % 1000) / 64.f - 8.f)
                   : (t == D && pad_element ? 0.f : std::numeric_limits<float>::infinity());
    line[t] = pack_key_index(key[t], t);
  }
  std::vector<mp64_t> ref = line, a = line, b(total, 0);
  for (int r = 0; r < nruns; ++r) std::sort(a.begin() + r * kMp64Run, a.begin() + (r + 1) * kMp64Run);   // what phase A parks
  int levels = 0;
  for (long long R = kMp64Run; R < total; R <<= 1, ++levels) {
    std::fill(b.begin(), b.end(), 0ull);
    run_level(a, b, total, (int)R);
    std::vector<mp64_t> want = line;
    for (long long p = 0; p < total; p += 2 * R) std::sort(want.begin() + p, want.begin() + std::min<long long>(p + 2 * R, total));
    CHECK(b == want);
    a.swap(b);
  }
  CHECK(levels == mp64_num_levels(total));
  std::sort(ref.begin(), ref.end());
  CHECK(a == ref);
  // the order of the words is the project's rule: stable by key value (-0 == +0), the pad element last among the zeros, fill last
  std::vector<int> order(total);
  for (int t = 0; t < total; ++t) order[t] = t;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] < key[y]; });
  for (int t = 0; t < total; ++t) CHECK((int)(unsigned)a[t] == order[t]);
}

int main() {
  static_assert(kMp64Run % kMp64Tile == 0 && kMp64Tile == kMp64NT * kMp64VT, "tile geometry");
  const int runs[] = {2, 3, 4, 5, 16, 17, 32, 33, 69};
  const int lasts[] = {kMp64Run, 1, kMp64Run - 1};
  unsigned seed = 1;
  for (int nruns : runs)
    for (int last : lasts)
      for (int pad = nruns > 17 ? 1 : 0; pad < 2; ++pad) check_line(nruns, last, pad != 0, seed++);   // without the pad element: up to 17 runs
  check_line(1, 7, true, 99);                            // one run: no level
  CHECK(mp64_num_levels(kMp64Run) == 0 && mp64_num_levels(2 * kMp64Run) == 1 && mp64_num_levels(3 * kMp64Run) == 2);
  if (bad) {
    printf("FAILED: %d checks\n", bad);
    return 1;
  }
  printf("OK\n");
  return 0;
}
