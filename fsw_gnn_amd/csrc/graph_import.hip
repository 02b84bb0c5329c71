// CSR adjacency in, the library's CSR + degree bins out: fsw_graph_import_csr.  gfx950.
//
// For callers that already hold the adjacency by recipient (a torch.sparse_csr tensor, PyG's adj_t.csr() triple, batch.ptr): nothing
// is sorted.  The result equals, entry for entry, what the builds of graph_build.hip produce from the corresponding edge list
// (include/fsw_hip.h states the semantics); the degree bins come from the kernels the builds use (graph_bins.h).
//
//   k_csr_check   one pass over rowptr_in and the entries, 4 consecutive elements per lane (16-byte accesses): validates both, and in
//                 the plain mode (no self loops, no 'gcn') narrows and copies them in the same pass -- reads 8 (nnz + rows) bytes of
//                 int64 input once and writes 4 (nnz + rows), the whole import apart from the bins.  col_in / w_in are indexed by the
//                 entry number e < nnz only, rowptr_in by the row number: in bounds whatever the arrays hold.
//   k_csr_diag    (strict self loops) per row the place of the diagonal entry by binary search; an exclusive scan of "row has none"
//                 gives the number of inserted loops before every row.
//   k_csr_rows    (self loops and / or 'gcn') row-cooperative copy: 8 lanes per row, and a row above kLongRow entries by the whole
//                 workgroup afterwards, so a hub row is neither one lane's nor one wavefront's job.  Appends or merges the loop,
//                 writes slot_of_entry, and for 'gcn' the square root of the row's weight sum (float64 partial sums of a fixed lane
//                 pattern, reduced in a fixed tree: the same bits on every run).
//                 A second launch of the same walk (RowGcn) then writes w / sqrt(deg[row]) / sqrt(deg[col]) over the output entries.
//   k_csr_void    MALFORMED, INDEX_RANGE or COL_ORDER: rowptr all 0 = the empty graph.  Every kernel after k_csr_check reads the flag
//                 word (and the descent counter of the column-order check) on the device and leaves at once, so a value of rowptr_in
//                 is used as an index only after the whole array passed the check.
// Column order (strict_cols) is checked entry-parallel too: k_csr_check counts the positions e with col[e - 1] >= col[e] over ALL
// entries and subtracts those that lie on the start of a non-empty row; what is left are descents inside rows.
#include "graph_bins.h"

namespace fsw {

constexpr int kCsrBad = FSW_FLAG_CSR_MALFORMED | FSW_FLAG_INDEX_RANGE | FSW_FLAG_CSR_COL_ORDER;
constexpr int kLongRow = 2048;      // entries from which on a row is walked by the whole workgroup
constexpr int kRowGroup = 8;        // lanes per row below that
constexpr int kRowThreads = 256;
constexpr int kRowsPerBlock = kRowThreads / kRowGroup;

// ---- workspace: per-row scratch only (nothing per entry) ---------------------------------------------------------------------
struct ImportWs {
  int32_t* bin_count;
  int32_t* bin_cursor;
  int32_t* block_sums;
  int64_t block_sums_cap;
  int32_t* shift;      // [rows + 1] strict self loops: 1 where the row has no diagonal entry, then its exclusive scan
  int32_t* diag;       // [rows]     strict self loops: input position of the diagonal entry / of the place it is inserted at
  float* sqrt_deg;     // [rows]     'gcn'
  int32_t* descents;   // [1]        column-order check
  size_t total;
};

inline ImportWs carve_import(void* ws, int64_t num_rows) {
  const size_t rows = (size_t)(num_rows > 0 ? num_rows : 0);
  char* base = reinterpret_cast<char*>(ws);
  size_t p = 0;
  auto take = [&](size_t bytes) -> void* {
    void* at = base ? base + p : nullptr;
    p += ws_align_up(bytes, kWsAlign);
    return at;
  };
  ImportWs g;
  g.bin_count = reinterpret_cast<int32_t*>(take(kBinTableBytes));
  g.bin_cursor = reinterpret_cast<int32_t*>(take(kBinTableBytes));
  g.block_sums_cap = (int64_t)ws_ceil_div(rows + 1, kScanTile) + 1;
  g.block_sums = reinterpret_cast<int32_t*>(take(4 * (size_t)g.block_sums_cap));
  g.shift = reinterpret_cast<int32_t*>(take(4 * (rows + 1)));
  g.diag = reinterpret_cast<int32_t*>(take(4 * rows));
  g.sqrt_deg = reinterpret_cast<float*>(take(4 * rows));
  g.descents = reinterpret_cast<int32_t*>(take(16));
  g.total = p;
  return g;
}

// MALFORMED / INDEX_RANGE / COL_ORDER as of the end of k_csr_check (COL_ORDER itself is set by k_csr_void, from the same counter)
__device__ __forceinline__ bool import_bad(const int32_t* __restrict__ stats, const int32_t* __restrict__ descents) {
  return (stats[FSW_STAT_FLAGS] & kCsrBad) != 0 || *descents != 0;
}

__device__ __forceinline__ int weight_flags(float w) {
  int f = 0;
  if (!(fabsf(w) <= 3.402823466e38f)) f |= FSW_FLAG_W_NONFINITE;
  if (w < 0.f) f |= FSW_FLAG_W_NEGATIVE;
  return f;
}

__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off);
  return v;
}

// 4 consecutive indices from a 16-byte aligned position
__device__ __forceinline__ void load4(const int64_t* __restrict__ p, int64_t v[4]) {
  const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
  v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
}
__device__ __forceinline__ void load4(const int32_t* __restrict__ p, int64_t v[4]) {
  const int4 a = *reinterpret_cast<const int4*>(p);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
}

// VEC: every array is 16-byte aligned, so a lane's 4 consecutive elements are one 16-byte access per 4-byte array.
// COPY: the plain mode -- col / w / rowptr / slot_of_entry leave in this pass (the final weights are the input weights: their flags too).
template <class IDX, bool VEC, bool COPY>
static __global__ void __launch_bounds__(256) k_csr_check(const IDX* __restrict__ rowptr_in, const IDX* __restrict__ col_in,
                                                          const float* __restrict__ w_in, int64_t num_rows, int64_t num_cols, int64_t nnz,
                                                          int strict, int32_t* __restrict__ rowptr_out, int32_t* __restrict__ col_out,
                                                          float* __restrict__ w_out, int32_t* __restrict__ slot,
                                                          int32_t* __restrict__ descents, int32_t* __restrict__ stats) {
  const int64_t nquads = ceil_div(nnz > num_rows + 1 ? nnz : num_rows + 1, 4);
  int flags = 0, desc = 0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquads; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = 4 * q;
    // ---- entries i0 .. i0 + 3
    if (i0 < nnz) {
      const bool full = VEC && i0 + 3 < nnz;
      const int cnt = (int)min((int64_t)4, nnz - i0);
      int64_t c[4] = {i0, i0 + 1, i0 + 2, i0 + 3};   // col_in == NULL: the identity
      if (col_in) {
        if (full) {
          load4(col_in + i0, c);
        } else {
          for (int j = 0; j < cnt; ++j) c[j] = (int64_t)col_in[i0 + j];
        }
        for (int j = 0; j < cnt; ++j)
          if (c[j] < 0 || c[j] >= num_cols) flags |= FSW_FLAG_INDEX_RANGE;
        if (strict) {
          if (i0 > 0 && (int64_t)col_in[i0 - 1] >= c[0]) ++desc;
          for (int j = 1; j < cnt; ++j)
            if (c[j - 1] >= c[j]) ++desc;
        }
      }
      float w[4] = {1.f, 1.f, 1.f, 1.f};
      if (w_in) {
        if (full) {
          const float4 t = *reinterpret_cast<const float4*>(w_in + i0);
          w[0] = t.x, w[1] = t.y, w[2] = t.z, w[3] = t.w;
        } else {
          for (int j = 0; j < cnt; ++j) w[j] = w_in[i0 + j];
        }
        for (int j = 0; j < cnt; ++j) {
          if (w[j] != 1.f) flags |= FSW_FLAG_W_NONUNIT;
          if (COPY) flags |= weight_flags(w[j]);
        }
      }
      if constexpr (COPY) {
        if (full) {
          *reinterpret_cast<int4*>(col_out + i0) = make_int4((int)c[0], (int)c[1], (int)c[2], (int)c[3]);
          if (w_in) *reinterpret_cast<float4*>(w_out + i0) = make_float4(w[0], w[1], w[2], w[3]);
          if (slot) *reinterpret_cast<int4*>(slot + i0) = make_int4((int)i0, (int)i0 + 1, (int)i0 + 2, (int)i0 + 3);
        } else {
          for (int j = 0; j < cnt; ++j) {
            col_out[i0 + j] = (int32_t)c[j];
            if (w_in) w_out[i0 + j] = w[j];
            if (slot) slot[i0 + j] = (int32_t)(i0 + j);
          }
        }
      }
    }
    // ---- rowptr_in[i0 .. i0 + 3] (indices 0 .. num_rows) and the element behind them
    if (i0 <= num_rows) {
      const bool full = VEC && i0 + 3 <= num_rows;
      const int cnt = (int)min((int64_t)4, num_rows + 1 - i0);
      int64_t v[5] = {0, 0, 0, 0, 0};
      if (full) {
        load4(rowptr_in + i0, v);
      } else {
        for (int j = 0; j < cnt; ++j) v[j] = (int64_t)rowptr_in[i0 + j];
      }
      const bool has_next = i0 + cnt <= num_rows;          // v[cnt] = rowptr_in[i0 + cnt] exists
      if (has_next) v[cnt] = (int64_t)rowptr_in[i0 + cnt];
      for (int j = 0; j < cnt; ++j) {
        const int64_t i = i0 + j;
        bool bad = v[j] < 0 || (i == 0 && v[j] != 0) || (i == num_rows && v[j] != nnz);
        if (j + 1 < cnt || has_next) bad = bad || v[j + 1] < v[j];
        if (bad) flags |= FSW_FLAG_CSR_MALFORMED;
        // the start of a non-empty row is no descent inside a row (the value is used as an index only between 1 and nnz - 1)
        if (strict && col_in && i < num_rows && v[j] > 0 && v[j] < nnz && v[j + 1] > v[j] &&
            (int64_t)col_in[v[j] - 1] >= (int64_t)col_in[v[j]])
          --desc;
      }
      if constexpr (COPY) {
        if (full) {
          *reinterpret_cast<int4*>(rowptr_out + i0) = make_int4((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
        } else {
          for (int j = 0; j < cnt; ++j) rowptr_out[i0 + j] = (int32_t)v[j];
        }
      }
    }
  }
  flags = wave_or(flags);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) desc += __shfl_xor(desc, off);
  if (lane_id() == 0) {
    if (flags) atomicOr(&stats[FSW_STAT_FLAGS], flags);
    if (desc) atomicAdd(descents, desc);
  }
}

// One launch instead of three memsets: the bin counters, the descent counter and the stats words start at 0.
static __global__ void __launch_bounds__(256) k_csr_init(int32_t* __restrict__ bin_count, int32_t* __restrict__ descents,
                                                         int32_t* __restrict__ stats) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kMaxRowChunks * FSW_NUM_BINS) bin_count[i] = 0;
  if (i < FSW_NUM_STATS) stats[i] = 0;
  if (i == 0) *descents = 0;
}

// The empty graph for an input that failed the check; also turns the descent counter into its flag.
static __global__ void __launch_bounds__(256) k_csr_void(int32_t* __restrict__ rowptr_out, int64_t num_rows, const int32_t* __restrict__ descents,
                                                         int32_t* __restrict__ stats) {
  const bool order = *descents != 0;
  if (order && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&stats[FSW_STAT_FLAGS], FSW_FLAG_CSR_COL_ORDER);
  if (!order && !(stats[FSW_STAT_FLAGS] & kCsrBad)) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= num_rows; i += (int64_t)gridDim.x * blockDim.x) rowptr_out[i] = 0;
}

// shift[r] = 1 when row r has no diagonal entry (a loop is inserted), diag[r] = the input position of the diagonal entry or of the
// first entry with a larger column (= where the loop goes).  Columns are strictly increasing inside the row (checked).
template <class IDX>
static __global__ void __launch_bounds__(256) k_csr_diag(const IDX* __restrict__ rowptr_in, const IDX* __restrict__ col_in, int64_t num_rows,
                                                         int32_t* __restrict__ shift, int32_t* __restrict__ diag,
                                                         const int32_t* __restrict__ descents, const int32_t* __restrict__ stats) {
  if (import_bad(stats, descents)) return;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= num_rows; r += (int64_t)gridDim.x * blockDim.x) {
    if (r == num_rows) {
      shift[r] = 0;
      continue;
    }
    const int64_t a = (int64_t)rowptr_in[r], b = (int64_t)rowptr_in[r + 1];
    int64_t lo = a, hi = b;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      const int64_t c = col_in ? (int64_t)col_in[mid] : mid;
      if (c < r) lo = mid + 1; else hi = mid;
    }
    const bool has = lo < b && (col_in ? (int64_t)col_in[lo] : lo) == r;
    diag[r] = (int32_t)lo;
    shift[r] = has ? 0 : 1;
  }
}

// sum over the G lanes that walk one row, the same value in all of them; a fixed tree, so the same bits on every run
template <int G>
__device__ __forceinline__ double row_sum(double v, double* lds) {
  if constexpr (G == kRowGroup) {
#pragma unroll
    for (int off = kRowGroup / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
  } else {
    v = wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kRowThreads / kWave; ++i) s += lds[i];
    return s;
  }
}

enum { kLoopNone = 0, kLoopAppend = 1, kLoopStrict = 2 };

template <class IDX>
struct RowCopy {
  const IDX* rowptr_in;
  const IDX* col_in;
  const float* w_in;
  int loop;            // kLoop*
  float loop_w;
  int gcn;
  const int32_t* shift;
  const int32_t* diag;
  int32_t* rowptr_out;
  int32_t* col_out;
  float* w_out;
  int32_t* slot;
  float* sqrt_deg;
  int64_t num_rows;

  __device__ __forceinline__ int64_t length(int64_t r) const { return (int64_t)rowptr_in[r + 1] - (int64_t)rowptr_in[r]; }

  template <int G>
  __device__ __forceinline__ int row(int64_t r, int lane, double* lds) const {
    const int64_t a = (int64_t)rowptr_in[r], b = (int64_t)rowptr_in[r + 1];
    int64_t o = a, p = b;         // output start of the row; strict: input position of the diagonal entry / of the inserted loop
    bool has = false;
    if (loop == kLoopAppend) o = a + r;
    if (loop == kLoopStrict) {
      o = a + shift[r];
      p = diag[r];
      has = shift[r + 1] == shift[r];
    }
    const bool insert = loop == kLoopStrict && !has;
    int flags = 0;
    double sum = 0.0;
    for (int64_t e = a + lane; e < b; e += G) {
      const int64_t pos = o + (e - a) + ((insert && e >= p) ? 1 : 0);
      float w = w_in ? w_in[e] : 1.f;
      if (has && e == p) w = (float)((double)w + (double)loop_w);   // the coalesced sum of the entry and the loop
      col_out[pos] = (int32_t)(col_in ? (int64_t)col_in[e] : e);
      w_out[pos] = w;
      if (slot) slot[e] = (int32_t)pos;
      sum += (double)w;
      if (!gcn) flags |= weight_flags(w);
    }
    const int64_t end = o + (b - a) + ((loop == kLoopAppend || insert) ? 1 : 0);
    if (lane == 0) {
      if (loop == kLoopAppend || insert) {
        const int64_t pos = loop == kLoopAppend ? o + (b - a) : o + (p - a);
        col_out[pos] = (int32_t)r;
        w_out[pos] = loop_w;
        if (!gcn) flags |= weight_flags(loop_w);
      }
      rowptr_out[r] = (int32_t)o;
      if (r == num_rows - 1) rowptr_out[num_rows] = (int32_t)end;
    }
    if (gcn) {
      double s = row_sum<G>(sum, lds);
      if (loop == kLoopAppend || insert) s += (double)loop_w;
      if (lane == 0) sqrt_deg[r] = sqrtf((float)s);
    }
    return flags;
  }
};

// the 'gcn' weights of the finished rows: w / sqrt(deg[row]) / sqrt(deg[col]), the expression and order of the edge-list path
struct RowGcn {
  const int32_t* rowptr_out;
  const int32_t* col_out;
  float* w_out;
  const float* sqrt_deg;

  __device__ __forceinline__ int64_t length(int64_t r) const { return (int64_t)rowptr_out[r + 1] - (int64_t)rowptr_out[r]; }

  template <int G>
  __device__ __forceinline__ int row(int64_t r, int lane, double*) const {
    const int64_t a = rowptr_out[r], b = rowptr_out[r + 1];
    const float dr = sqrt_deg[r];
    int flags = 0;
    for (int64_t j = a + lane; j < b; j += G) {
      const float w = w_out[j] / dr / sqrt_deg[col_out[j]];
      w_out[j] = w;
      flags |= weight_flags(w);
    }
    return flags;
  }
};

// kRowGroup lanes per row; the rows above kLongRow entries of a workgroup's kRowsPerBlock rows are then walked by all its lanes
template <class F>
static __global__ void __launch_bounds__(kRowThreads) k_csr_rows(F f, int64_t num_rows, const int32_t* __restrict__ descents,
                                                                 int32_t* __restrict__ stats) {
  __shared__ int long_rows[kRowsPerBlock];
  __shared__ int nlong;
  __shared__ double lds[kRowThreads / kWave];
  if (import_bad(stats, descents)) return;
  const int grp = threadIdx.x / kRowGroup, gl = threadIdx.x % kRowGroup;
  int flags = 0;
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < num_rows; base += (int64_t)gridDim.x * kRowsPerBlock) {
    if (threadIdx.x == 0) nlong = 0;
    __syncthreads();
    const int64_t r = base + grp;
    if (r < num_rows) {
      if (f.length(r) > kLongRow) {
        if (gl == 0) long_rows[atomicAdd(&nlong, 1)] = grp;
      } else {
        flags |= f.template row<kRowGroup>(r, gl, lds);
      }
    }
    __syncthreads();
    const int n = nlong;
    for (int i = 0; i < n; ++i) flags |= f.template row<kRowThreads>(base + long_rows[i], (int)threadIdx.x, lds);
    __syncthreads();
  }
  flags = wave_or(flags);
  if (flags && lane_id() == 0) atomicOr(&stats[FSW_STAT_FLAGS], flags);
}

static int grid_for(int64_t items, int per_block) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(items, per_block), 1), 1 << 20); }

template <class IDX>
static int import_impl(const IDX* rowptr_in, const IDX* col_in, const float* w_in, int64_t nnz, int64_t num_rows, int64_t num_cols,
                       int64_t chunk_rows, float loop_w, int gcn, int strict, int32_t* rowptr, int32_t* col, float* w, int32_t* slot,
                       int32_t* perm, int32_t* invperm, int32_t* bin_start, int32_t* stats, ImportWs& g, hipStream_t stream) {
  const int loop = loop_w == 0.f ? kLoopNone : strict ? kLoopStrict : kLoopAppend;
  const bool plain = loop == kLoopNone && !gcn;
  const uintptr_t all = reinterpret_cast<uintptr_t>(rowptr_in) | reinterpret_cast<uintptr_t>(col_in) | reinterpret_cast<uintptr_t>(w_in) |
                        reinterpret_cast<uintptr_t>(rowptr) | reinterpret_cast<uintptr_t>(col) | reinterpret_cast<uintptr_t>(w) |
                        reinterpret_cast<uintptr_t>(slot);
  const bool vec = (all & 15) == 0;
  const int blocks = grid_for(ceil_div(std::max(nnz, num_rows + 1), 4), 256);
#define FSW_CSR_CHECK(VEC, COPY)                                                                                                      \
  k_csr_check<IDX, VEC, COPY><<<blocks, 256, 0, stream>>>(rowptr_in, col_in, w_in, num_rows, num_cols, nnz, strict, rowptr, col, w, slot, \
                                                          g.descents, stats)
  if (vec && plain) FSW_CSR_CHECK(true, true);
  else if (vec) FSW_CSR_CHECK(true, false);
  else if (plain) FSW_CSR_CHECK(false, true);
  else FSW_CSR_CHECK(false, false);
#undef FSW_CSR_CHECK
  FSW_LAUNCH_CHECK();
  if (!plain) {
    if (loop == kLoopStrict) {
      k_csr_diag<IDX><<<grid_for(num_rows + 1, 256), 256, 0, stream>>>(rowptr_in, col_in, num_rows, g.shift, g.diag, g.descents, stats);
      FSW_LAUNCH_CHECK();
      // an input that failed the check leaves shift unwritten: its scan is then never read (every later kernel leaves at once)
      if (int rc = exclusive_scan_i32(g.shift, num_rows + 1, g.block_sums, g.block_sums_cap, stream)) return rc;
    }
    const RowCopy<IDX> f{rowptr_in, col_in, w_in, loop, loop_w, gcn, g.shift, g.diag, rowptr, col, w, slot, g.sqrt_deg, num_rows};
    k_csr_rows<<<grid_for(num_rows, kRowsPerBlock), kRowThreads, 0, stream>>>(f, num_rows, g.descents, stats);
    FSW_LAUNCH_CHECK();
    if (gcn) {
      const RowGcn h{rowptr, col, w, g.sqrt_deg};
      k_csr_rows<<<grid_for(num_rows, kRowsPerBlock), kRowThreads, 0, stream>>>(h, num_rows, g.descents, stats);
      FSW_LAUNCH_CHECK();
    }
  }
  k_csr_void<<<grid_for(num_rows + 1, 256), 256, 0, stream>>>(rowptr, num_rows, g.descents, stats);
  FSW_LAUNCH_CHECK();
  return finish_bins(rowptr, num_rows, chunk_rows, perm, invperm, bin_start, stats, g.bin_count, g.bin_cursor, stream, false, true);
}

}  // namespace fsw

using namespace fsw;

extern "C" size_t fsw_graph_import_workspace_bytes(int64_t num_rows, int64_t nnz) {
  (void)nnz;   // per-row scratch only
  return carve_import(nullptr, num_rows).total;
}

extern "C" int fsw_graph_import_csr(const void* rowptr_in, const void* col_in, const float* w_in, int index_bytes, int64_t nnz,
                                    int64_t num_rows, int64_t num_cols, int64_t chunk_rows, float self_loop_weight, int gcn,
                                    int strict_cols, int32_t* rowptr, int32_t* col, float* w, int32_t* slot_of_entry, int32_t* perm,
                                    int32_t* invperm, int32_t* bin_start, int32_t* stats, void* workspace, size_t workspace_bytes,
                                    fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  FSW_REQUIRE(index_bytes == 4 || index_bytes == 8, "fsw_graph_import_csr: index_bytes must be 4 or 8 (got %d)", index_bytes);
  FSW_REQUIRE(num_rows >= 1 && num_rows < (1ll << 31) - 1 && num_cols >= 1 && num_cols < (1ll << 31) && nnz >= 0 &&
                  nnz + num_rows < (1ll << 31) - kRsTile,
              "fsw_graph_import_csr: sizes must satisfy 1 <= rows, cols < 2^31 and 0 <= nnz, nnz + rows < 2^31 (got %lld, %lld, %lld)",
              (long long)num_rows, (long long)num_cols, (long long)nnz);
  FSW_REQUIRE((gcn == 0 || gcn == 1) && (strict_cols == 0 || strict_cols == 1), "fsw_graph_import_csr: gcn and strict_cols are 0 or 1");
  FSW_REQUIRE(self_loop_weight >= 0.f && self_loop_weight <= 3.402823466e38f, "fsw_graph_import_csr: self_loop_weight must be finite and >= 0");
  const bool loops = self_loop_weight != 0.f;
  FSW_REQUIRE(!(loops || gcn) || num_rows == num_cols, "fsw_graph_import_csr: self loops and 'gcn' weights need a square adjacency");
  FSW_REQUIRE(col_in || num_cols >= nnz, "fsw_graph_import_csr: col_in == NULL (col[e] = e) needs num_cols >= nnz");
  FSW_REQUIRE(workspace && workspace_bytes >= fsw_graph_import_workspace_bytes(num_rows, nnz), "fsw_graph_import_csr: workspace too small");
  FSW_REQUIRE(rowptr_in && rowptr && perm && bin_start && stats && (nnz + (loops ? num_rows : 0) == 0 || col),
              "fsw_graph_import_csr: null pointer");
  FSW_REQUIRE(!(w_in || loops || gcn) || w, "fsw_graph_import_csr: the imported graph carries weights but w is null");
  if (int rc = check_chunks(num_rows, chunk_rows)) return rc;
  ImportWs g = carve_import(workspace, num_rows);
  static_assert(kBinTableBytes == sizeof(int32_t) * kMaxRowChunks * FSW_NUM_BINS, "k_csr_init zeroes the whole table");
  k_csr_init<<<(kMaxRowChunks * FSW_NUM_BINS + 255) / 256, 256, 0, stream>>>(g.bin_count, g.descents, stats);
  FSW_LAUNCH_CHECK();
  if (index_bytes == 8)
    return import_impl<int64_t>(reinterpret_cast<const int64_t*>(rowptr_in), reinterpret_cast<const int64_t*>(col_in), w_in, nnz, num_rows,
                                num_cols, chunk_rows, self_loop_weight, gcn, strict_cols, rowptr, col, w, slot_of_entry, perm, invperm,
                                bin_start, stats, g, stream);
  return import_impl<int32_t>(reinterpret_cast<const int32_t*>(rowptr_in), reinterpret_cast<const int32_t*>(col_in), w_in, nnz, num_rows,
                              num_cols, chunk_rows, self_loop_weight, gcn, strict_cols, rowptr, col, w, slot_of_entry, perm, invperm,
                              bin_start, stats, g, stream);
}
