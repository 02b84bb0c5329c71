/* fsw_hip.h -- C ABI of libfsw_hip.so: the MI355X (gfx950) native hot path of FSW_conv / FSW_embedding.
 *
 * Drop-in boundary.  The reference's only native code is libfsw_embedding.so, loaded with ctypes
 * (reference fsw_embedding.py:94-99, 195-206) and called with raw tensor.data_ptr() device pointers
 * from segcumsum_cuda (fsw_embedding.py:2878-3012).  This library is loaded the same way and keeps the
 * same conventions -- plain pointers and sizes, caller-owned pre-allocated buffers, no torch types --
 * with three deliberate changes:
 *   - every entry point is stream-ordered (takes a hipStream_t) and never device-synchronises
 *     (the reference wrappers cudaDeviceSynchronize() before and after each launch,
 *      fsw_embedding.cu:197, 208, 215, 227, and use the default stream);
 *   - every entry point returns an int status (0 = ok); nothing prints-and-exit(1)s
 *     (fsw_embedding.cu:20-27).  fsw_last_error() returns the message of the last failure;
 *   - besides the segmented cumsum, the whole chain the reference builds out of ~15 E*S-sized COO
 *     tensors (fsw_embedding.py:894-1112: projection, per-slice sort, weight permutation, segmented
 *     cumsum, sinc/cos readout, reduction) is exported as fused kernels on a CSR adjacency.
 *
 * The three legacy symbols at the end keep the reference's exact signatures, so the reference's own
 * fsw_embedding.py can dlopen this library in place of libfsw_embedding.so unchanged.
 *
 * All pointers are DEVICE pointers unless stated otherwise.  Index type is int32: num_rows, num_cols
 * and num_edges must each be < 2^31.
 */
#ifndef FSW_HIP_H
#define FSW_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fsw_stream_t; /* a hipStream_t (torch.cuda.current_stream().cuda_stream) */

#define FSW_ABI_VERSION 6

/* Degree classes of the fused neighbourhood kernels.  Rows are binned by in-degree:
 *   bin b, 0 <= b <= FSW_REG_MAX_DEG : rows of degree exactly b (register path, one wave per row and
 *                                      64-slice chunk, exact-size sorting network)
 *   bin FSW_BIN_MID0 + i             : fsw_mid_size(i-1) < degree <= fsw_mid_size(i), i < FSW_NUM_MID_BINS
 *                                      (register path with the network of size fsw_mid_size(i), +inf padding)
 *   bin FSW_BIN_LDS0 + i             : 256 << i < degree <= 512 << i, i < FSW_NUM_LDS_BINS (wave-sort path: the
 *                                      neighbourhood is transposed through LDS, every wavefront sorts one slice's
 *                                      line held across its lanes' registers)
 *   bin FSW_BIN_HUB0 + i             : 2048 << i < degree <= 4096 << i, i < FSW_NUM_HUB_BINS (hub path: a workgroup of 2 << i
 *                                      wavefronts holds ONE slice's line in its registers, 2048 keys per wavefront; the merge
 *                                      levels above one wavefront exchange registers through LDS)
 *   bin FSW_BIN_GLOBAL               : degree > FSW_HUB_MAX_DEG (global-scratch bitonic path, any degree)
 * General (non-unit) weights carry a weight next to every key and a line holds one more element (the reference's pad element), so
 * their per-lane register path ends at FSW_MID_MAX_DEG_WEIGHTED; above it (key, weight) lines of 64 x {3 .. 32} keys per lane on
 * one, two or four wavefronts take rows of up to 8191 neighbours, sorted blocks of 8192 + merge-path levels the rest
 * (csrc/embed_hub.hip, csrc/merge_path.h); with edge features the LDS-staged / scratch-line kernels of csrc/embed_wsort.hip.      */
#define FSW_REG_MAX_DEG 32
#define FSW_NUM_MID_BINS 9
#define FSW_MID_SIZES {40, 48, 64, 80, 96, 128, 160, 192, 256}
#define FSW_MID_MAX_DEG 256
#define FSW_MID_MAX_DEG_WEIGHTED 128
#define FSW_LDS_MAX_DEG 2048
#define FSW_HUB_MAX_DEG 32768
#define FSW_CART_W_MAX_LINE 16384 /* Cartesian mode, general weights: longest line (D + 1 elements) of the tuned classes */
#define FSW_BIN_MID0 (FSW_REG_MAX_DEG + 1)
#define FSW_NUM_LDS_BINS 3
#define FSW_BIN_LDS0 (FSW_BIN_MID0 + FSW_NUM_MID_BINS)
#define FSW_NUM_HUB_BINS 4
#define FSW_BIN_HUB0 (FSW_BIN_LDS0 + FSW_NUM_LDS_BINS)
#define FSW_BIN_GLOBAL (FSW_BIN_HUB0 + FSW_NUM_HUB_BINS)
#define FSW_NUM_BINS (FSW_BIN_GLOBAL + 1)

/* stats[] words written by fsw_graph_build / fsw_project_f32 (device int32[FSW_NUM_STATS]) */
#define FSW_STAT_FLAGS 0        /* OR of FSW_FLAG_* */
#define FSW_STAT_MAX_DEGREE 1
#define FSW_STAT_NUM_ZERO_DEG 2
#define FSW_STAT_NUM_REG 3      /* rows with 1 <= degree <= FSW_REG_MAX_DEG */
#define FSW_STAT_NUM_LDS 4      /* rows with FSW_REG_MAX_DEG < degree <= FSW_LDS_MAX_DEG (mid bins + LDS bin) */
#define FSW_STAT_NUM_GLOBAL 5   /* rows with degree > FSW_LDS_MAX_DEG (hub bins + global bin) */
#define FSW_STAT_NNZ 6          /* number of CSR entries in use = rowptr[num_rows] (after coalescing, without invalid edges) */
#define FSW_STAT_USER 7         /* never written by the library after the build zeroes it: the Python side parks the bits of
                                   the total-mass scale here so that ONE device->host copy per forward fetches everything */
#define FSW_NUM_STATS 8

#define FSW_FLAG_INDEX_RANGE 1   /* an edge endpoint outside [0, num_rows) x [0, num_cols) */
#define FSW_FLAG_W_NONFINITE 2   /* reference assert fsw_embedding.py:678-679 */
#define FSW_FLAG_W_NEGATIVE 4    /* reference assert fsw_embedding.py:680 */
#define FSW_FLAG_X_NONFINITE 8   /* reference assert fsw_embedding.py:652-653 */

int fsw_abi_version(void);
const char* fsw_arch(void);       /* "gfx950" */
const char* fsw_last_error(void); /* host string, valid until the next failing call on this thread */

/* ---- adjacency: edge list -> CSR by recipient, plus degree bins ---------------------------------
 * Replaces FSW_conv.edge_index_to_adj (reference fsw_conv.py:384-447: torch.sparse_coo_tensor().coalesce()
 * + sp.get_slice_info) and the sp.get_slice_info(W, -1) / concat_sparse sorts of FSW_embedding.forward
 * (fsw_embedding.py:778-821).  Parallel edges are kept as separate elements: k parallel unit edges
 * j->i contribute exactly what the reference's single coalesced entry of weight k contributes, because
 * the Fourier readout telescopes over equal projections (DESIGN.md "duplicates").
 *   recipients/senders : int64[num_edges]  (edge_index row 1 / row 0; COO indices row 0 / row 1)
 *   edge_w             : float[num_edges] or NULL for unit weights
 *   rowptr int32[num_rows+1], col int32[num_edges], w float[num_edges] (ignored if edge_w NULL)
 *   perm int32[num_rows]  rows ordered by degree bin; bin_start int32[FSW_NUM_BINS+1] offsets into perm
 *   invperm int32[num_rows] or NULL: position of every row in perm (perm[invperm[r]] == r)
 *   stats int32[FSW_NUM_STATS] (zeroed by this call)
 *   chunk_rows : 0, or a positive multiple of FSW_BIN_BLOCK_ROWS.  With chunk_rows > 0 the rows are binned separately
 *                inside every chunk of chunk_rows consecutive rows: perm lists chunk 0's rows by degree bin, then chunk
 *                1's, ...; bin_start then holds ceil(num_rows / chunk_rows) (<= FSW_MAX_ROW_CHUNKS) rows of
 *                FSW_NUM_BINS + 1 offsets.  Passing row c of bin_start (and num_rows = chunk_rows) to fsw_embed_f32 /
 *                fsw_conv_fused_f32 restricts that call to the recipients of chunk c -- the multi-GPU path overlaps
 *                the collective of one node range with the kernels of the next this way.                          */
#define FSW_BIN_BLOCK_ROWS 2048
#define FSW_MAX_ROW_CHUNKS 256
/* workspace: one scratch buffer of fsw_graph_workspace_bytes(num_rows, num_edges) bytes for the three builds below (and, with
 * (num_cols, nnz), for fsw_graph_transpose).  About 24 bytes per edge: key and value ping-pong, the count table of a radix pass,
 * the block sums of the device-wide scan (sized for the longest scan of any entry point: one int per 4096 edges), bucket starts
 * and bin counters -- csrc/graph_ws.h.  Query it for every call; a smaller buffer is refused with a status.                    */
size_t fsw_graph_workspace_bytes(int64_t num_rows, int64_t num_edges);
int fsw_graph_build(const int64_t* recipients, const int64_t* senders, const float* edge_w,
                    int64_t num_edges, int64_t num_rows, int64_t num_cols, int64_t chunk_rows,
                    int32_t* rowptr, int32_t* col, float* w, int32_t* perm, int32_t* invperm, int32_t* bin_start,
                    int32_t* stats, void* workspace, size_t workspace_bytes, fsw_stream_t stream);
/* The same build with the same arguments and the same result, entry for entry; one partition pass over the high row bits +
 * one workgroup per bucket of 2048 rows instead of three LSD passes when the shape suits it (>= 32768 rows, <= 65536 edges
 * per bucket on average; the LSD passes otherwise).  Faster on graphs without hub rows (0.38 -> ~0.2 ms at 1M rows / 10M
 * edges); a bucket that holds hub rows serialises on its workgroup, so callers keep fsw_graph_build for skewed graphs.   */
int fsw_graph_build_two_level(const int64_t* recipients, const int64_t* senders, const float* edge_w,
                    int64_t num_edges, int64_t num_rows, int64_t num_cols, int64_t chunk_rows,
                    int32_t* rowptr, int32_t* col, float* w, int32_t* perm, int32_t* invperm, int32_t* bin_start,
                    int32_t* stats, void* workspace, size_t workspace_bytes, fsw_stream_t stream);
/* Host only (no device call): what fsw_graph_build_two_level does with a shape, computed by the code the build runs.
 * out int32[FSW_GRAPH_PLAN_WORDS]: [0] 1 = partition pass + bucket kernel, 0 = the LSD passes (all other words are then 0);
 * [1] 1 = one packed uint32 per edge (unit weights, one partition pass, row bits of a bucket + sender bits <= 32);
 * [2] edges per tile of the partition pass; [3] entries of the bucket kernel's LDS staging tile (0: none);
 * [4] partition passes; [5] row bits of a bucket; [6] sender bits; [7] buckets.                                          */
#define FSW_GRAPH_PLAN_WORDS 8
int fsw_graph_build_plan(int64_t num_rows, int64_t num_cols, int64_t num_edges, int weighted, int32_t* out);

/* Coalescing variant: entries sorted by (recipient, sender), parallel edges merged into ONE entry whose
 * weight (edge_w or 1 per edge) and edge-feature vector are the sums over the duplicates -- exactly what
 * torch.sparse_coo_tensor(...).coalesce() does to adj and X_edge in the reference (fsw_conv.py:397-398,
 * 436-437).  Required with edge features (the key of an element then depends on its feature vector, so
 * parallel edges are no longer equivalent to separate elements).  col/w/ef are sized for num_edges
 * entries, the first stats[FSW_STAT_NNZ] are used.  slot_of_edge int32[num_edges] (nullable): CSR
 * position of every input edge (-1 for rejected edges) -- the backward routes feature gradients with it. */
int fsw_graph_build_coalesced(const int64_t* recipients, const int64_t* senders, const float* edge_w,
                              const float* edge_feat, int d_edge, int64_t num_edges, int64_t num_rows, int64_t num_cols,
                              int32_t* rowptr, int32_t* col, float* w, float* ef, int32_t* slot_of_edge, int32_t* perm,
                              int32_t* invperm, int32_t* bin_start, int32_t* stats, void* workspace, size_t workspace_bytes,
                              fsw_stream_t stream);

/* ---- adjacency: CSR in, the same CSR + degree bins out (no sort) ---------------------------------
 * For callers that hold the adjacency by recipient already (torch.sparse_csr, PyG's adj_t.csr(), batch.ptr).  Row i of the
 * input lists the senders to recipient i.  The outputs are those of fsw_graph_build (rowptr / col / w as int32 / int32 / float,
 * perm, optional invperm, bin_start, stats, chunk_rows with the same meaning) and equal, entry for entry, what the builds above
 * produce from the edge list (recipient = row of e, sender = col_in[e]) in CSR order.
 *   rowptr_in [num_rows + 1], col_in [nnz] : int32 (index_bytes 4) or int64 (index_bytes 8); col_in NULL = the identity
 *                col[e] = e (segments of consecutive vertices: a readout's ptr), which needs num_cols >= nnz
 *   w_in float[nnz] or NULL for unit weights
 *   col / w / slot_of_entry : sized for nnz entries, and for nnz + num_rows when self_loop_weight != 0; w may be NULL when the
 *                result is unit (w_in NULL, no self loops, no gcn); slot_of_entry int32[nnz] (nullable) receives the output
 *                position of every input entry
 *   self_loop_weight : 0 = none (finite, >= 0; needs num_rows == num_cols).  strict_cols 0: one entry (r, r, self_loop_weight) is
 *                appended as the LAST entry of every row, whether or not the row has a diagonal entry (what appending the loops
 *                to the edge list and the stable build give); a unit input becomes weighted with w = 1 on its entries.
 *                strict_cols 1 (the coalesced adjacency, used with edge features): the columns of every row must be strictly
 *                increasing; the loop's weight is ADDED to the diagonal entry where there is one (float64 sum rounded to
 *                float), otherwise a new entry is inserted at its sorted place -- fsw_graph_build_coalesced of the edge list
 *                with the loops appended.  The caller scatters its feature rows with slot_of_entry; new entries carry zeros.
 *   gcn 1      : deg[r] = sum of row r's final weights (float64 partial sums in a fixed order: reproducible), then
 *                w = w / sqrt(deg[row]) / sqrt(deg[col]) in float32; needs num_rows == num_cols.
 * Entries keep their order inside a row; repeated columns stay separate elements (strict_cols 0).
 * stats: FSW_FLAG_W_NONFINITE / FSW_FLAG_W_NEGATIVE describe the FINAL weights; FSW_FLAG_INDEX_RANGE a column outside
 * [0, num_cols); and
 *   FSW_FLAG_CSR_MALFORMED  rowptr_in[0] != 0, a negative or decreasing pair, or rowptr_in[num_rows] != nnz
 *   FSW_FLAG_CSR_COL_ORDER  strict_cols only: two neighbouring columns of a row are not strictly increasing
 *   FSW_FLAG_W_NONUNIT      informational: some input weight is not exactly 1
 * Safety: given only that the arrays have the stated lengths, every device access of the import is in bounds for ANY contents
 * (col_in / w_in are indexed by e < nnz; a value of rowptr_in becomes an index only after the whole array passed the check).
 * With MALFORMED, INDEX_RANGE or COL_ORDER set the imported graph is EMPTY -- rowptr all 0, stats[FSW_STAT_NNZ] 0, every row in the
 * zero-degree bin (the kernels of the import read the flag word on the device) -- so no later kernel can index out of range before
 * the host has seen the flag.  Stream-ordered: no host wait, no allocation.  Sizes with nnz + num_rows >= 2^31, index_bytes other
 * than 4 or 8 and a workspace below fsw_graph_import_workspace_bytes (per-row scratch only, about 12 bytes a row) are refused
 * with a status before any launch.                                                                                          */
#define FSW_FLAG_CSR_MALFORMED 16
#define FSW_FLAG_CSR_COL_ORDER 32
#define FSW_FLAG_W_NONUNIT 64
size_t fsw_graph_import_workspace_bytes(int64_t num_rows, int64_t nnz);
int fsw_graph_import_csr(const void* rowptr_in, const void* col_in, const float* w_in, int index_bytes, int64_t nnz,
                         int64_t num_rows, int64_t num_cols, int64_t chunk_rows, float self_loop_weight, int gcn, int strict_cols,
                         int32_t* rowptr, int32_t* col, float* w, int32_t* slot_of_entry, int32_t* perm, int32_t* invperm,
                         int32_t* bin_start, int32_t* stats, void* workspace, size_t workspace_bytes, fsw_stream_t stream);

/* ---- projection: Xp[n, ldp] = X[n, ldx] . V[S, ldv]^T on the matrix cores -------------------------
 * Default: every operand split into three bf16 planes (x = x1 + x2 + x3 carries fp32's 24 significand bits), six
 * v_mfma_f32_32x32x16_bf16 per k-step with fp32 accumulation: < 5e-7 against float64, 2.7x fewer matrix cycles than the exact
 * fp32 MFMA (v_mfma_f32_32x32x2_f32), which FSW_PROJECT_EXACT_FP32=1 in the environment selects instead (d <= 128).
 * Replaces torch.tensordot(X, projVecs) (reference fsw_embedding.py:909-913).  Sets
 * FSW_FLAG_X_NONFINITE in stats[FSW_STAT_FLAGS] if X holds a NaN/Inf (stats may be NULL).
 * The bf16 kernels (d % 4 == 0, d <= 256, 16-byte aligned rows of X, V and W2) need ldp >= 32 * ceil(S / 32), ldp % 4 == 0 and a
 * 16-byte aligned Xp, and store whole 32-column slabs: columns S .. 32 * ceil(S / 32) - 1 of a row receive 0.0; columns from there on, and
 * from S on in the generic kernel, are left untouched (tests/test_hip_conv_fused.py).
 * x_copy (nullable): the kernel also stores the X rows it stages to x_copy[i*ld_copy + c] -- this is
 * the right half of FSW_conv's torch.cat((emb, vertex_features)) (reference fsw_conv.py:357-358),
 * written while X is on chip anyway instead of by a separate copy kernel.
 * Non-finite and very large inputs.  A NaN or Inf in X[i, k] makes every entry of row i of Xp (and of Y2) non-finite, a NaN or Inf in
 * V[j, k] every entry of column j; all other entries are what they would be without it.  Which non-finite value comes back is not
 * specified: under bf16 x 3 an Inf becomes NaN (its second plane is Inf - Inf), and a finite magnitude above the largest bf16
 * (about 3.39e38) rounds to Inf in the first plane and then does the same.  Only FSW_FLAG_X_NONFINITE reports it, and only for X.
 * bf16 has fp32's exponent range, so scaling X by 2^a and V by 2^b scales every entry by exactly 2^(a+b) as long as no plane
 * (down to 2^-18 of its entry) and no product leaves fp32's normal range.                                                     */
int fsw_project_f32(const float* X, int64_t n, int d, int64_t ldx, const float* V, int S, int64_t ldv,
                    float* Xp, int64_t ldp, float* x_copy, int64_t ld_copy, int32_t* stats, fsw_stream_t stream);

/* ---- C[M, N] = beta * C + A^T . B for tall row-major A [K, lda >= M], B [K, ldb >= N] (K in the millions, M x N at most 16 blocks
 * of 64 x 64): the weight-gradient shape of the backward pass -- gV = gXp^T . X (reference fsw_embedding.py:909-913 differentiated by
 * torch.autograd) and the first Linear layer's gW (fsw_conv.py:361).  bf16 x 3 like the projection (six v_mfma_f32_32x32x16_bf16 per
 * 16 rows, fp32 accumulation); FSW_GEMM_TN_EXACT_FP32=1 in the environment selects exact fp32 products and sums
 * (v_mfma_f32_32x32x2_f32) instead.  The K axis is split over the grid: G = min(512, max(1, K / 512)) workgroups, workgroup g takes
 * the rows [g per, min((g + 1) per, K)) with per = ceil(K / G) rounded up to a multiple of 16 (of 2 in the exact form); the partial
 * results are summed in a fixed order (no float atomics: bitwise reproducible, whatever the workspace held).
 * K: any K >= 1 (K = 0 is refused, as are lda < M, ldb < N, ldc < N, a null pointer and more than 16 blocks).  beta = 0: C is not read.
 * workspace: G * M * N * sizeof(float) bytes are used; fsw_gemm_tn_workspace_bytes(M, N) is that for G = 512, enough for every K.
 * Non-finite and very large inputs: a NaN or Inf in A[k, m] makes every entry of row m of C non-finite, one in B[k, n] every entry
 * of column n, all other entries are unaffected; under bf16 x 3 an Inf becomes NaN, and a finite magnitude above the largest bf16
 * (about 3.39e38) rounds to Inf in the first plane and then does the same.  Scaling A by 2^a and B by 2^b scales C by exactly
 * 2^(a+b) as long as no plane and no sum leaves fp32's normal range (tests/test_hip_dense_matrix.py).                          */
size_t fsw_gemm_tn_workspace_bytes(int M, int N);
int fsw_gemm_tn_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t K, int M, int N, float* C, int64_t ldc, float beta,
                    void* workspace, size_t workspace_bytes, fsw_stream_t stream);

/* ---- unit-weight readout coefficients ------------------------------------------------------------
 * table[(D*(D-1)/2 + t) * ldt + k] = (1+xi_k) * [sin(2 pi xi_k (t+1)/D) - sin(2 pi xi_k t/D)] / (pi xi_k)
 * for 1 <= D <= max_deg, 0 <= t < D (the reference's Delta_t of fsw_embedding.py:1047-1075 times the
 * (1+xi) of :1109 for weights 1/D), evaluated in float64 and rounded once.                        */
size_t fsw_unit_table_rows(int max_deg);
int fsw_unit_coeff_table(const float* freqs, int S, int max_deg, float* table, int64_t ldt, fsw_stream_t stream);

/* ---- fused neighbourhood sort + segmented cumsum + Fourier readout --------------------------------
 * Replaces forward_helper's sparse branch (reference fsw_embedding.py:917-1112) and the epilogue
 * (:853-888) for the 'plain' total-mass method.  For every row r and slice k:
 *   out[r*ldo + has_mass + k] = out_scale * ( (1+xi_k) * sum_t Delta_t p_(t) + bias[has_mass + k] )
 *   out[r*ldo]                = out_scale * ( f(m_r) * mass_scale + bias[0] )        if has_mass     */
typedef struct {
  /* adjacency (from fsw_graph_build) */
  const int32_t* rowptr;
  const int32_t* col;
  const float* w; /* NULL = unit weights */
  const int32_t* perm;
  const int32_t* bin_start;
  int64_t num_rows;
  /* projected features and slice parameters */
  const float* Xp;
  int64_t ldp;
  const float* freqs; /* [S], any finite value of either sign: 0 and -0.0 take the linear branch, -1 yields out_scale * bias only */
  int32_t S;
  float tau;                 /* total_mass_pad_thresh */
  const float* unit_table;   /* from fsw_unit_coeff_table, required when w == NULL and tau <= 1 */
  int64_t ldt;
  /* output */
  float* out;
  int64_t ldo;
  const float* bias; /* NULL or [has_mass + S] */
  float out_scale;
  int32_t has_mass;  /* 1: column 0 of out carries the encoded total mass */
  int32_t mass_fn;   /* 0 identity, 1 sqrt: 2m/(sqrt(m+1)+1), 2 log1p      (fsw_embedding.py:857-865) */
  float mass_scale;
  /* row counts per path, host values read back from stats (num_lds_rows = stats[FSW_STAT_NUM_LDS]: every row of
   * FSW_REG_MAX_DEG < degree <= FSW_LDS_MAX_DEG, the library picks the kernel per degree bin); -1 = unknown (launch
   * every path) */
  int64_t num_reg_rows, num_lds_rows, num_global_rows, num_zero_rows;
  int64_t max_degree; /* host value of stats[FSW_STAT_MAX_DEGREE]; required when num_global_rows != 0 */
  /* scratch for rows above FSW_LDS_MAX_DEG (sorted in a scratch line per wavefront, any degree): at least
   * fsw_embed_scratch_bytes(max_degree) bytes, or NULL if num_global_rows == 0 */
  void* scratch;
  size_t scratch_bytes;
  /* edge features (reference fsw_embedding.py:934-968): the key of CSR entry e of slice k is
   * Xp[col[e], k] + sum_q efeat[e*d_edge + q] * Ve[k*ldve + q]   (Ve = projVecs[:, d_in:]).  Needs w != NULL
   * (a graph from fsw_graph_build_coalesced).  efeat == NULL / d_edge == 0: no edge features.          */
  const float* efeat;
  const float* Ve;
  int64_t ldve;
  int32_t d_edge;
  int32_t reserved;
  /* HOST copy of the FSW_NUM_BINS + 1 words bin_start points at (nullable): with it the library knows the rows of every
   * degree bin -- empty bins are not launched and every grid is sized exactly (without it the grids are sized by the class
   * totals above and surplus workgroups leave at once: 4.5 of 81 ms on a 64M-edge RMAT graph).            */
  const int32_t* bin_start_host;
} fsw_embed_args;

size_t fsw_embed_scratch_bytes(int64_t max_degree);
int fsw_embed_f32(const fsw_embed_args* args, fsw_stream_t stream);

/* ---- FSW_conv fast path: embedding fused with the first Linear layer of the MLP ---------------------
 * Y[i, :] = act( [ out_scale * E(N(i)) , x_i ] . W^T + b ),  W = [W1 | W2]  -- reference fsw_conv.py:355-362
 * (self.fsw_embed -> torch.cat((mw*emb, vertex_features)) -> mlp[0] -> activation) without writing the
 * embedding to HBM, in two calls:
 *   fsw_project_linear_f32  the projection GEMM with a second output block Y2 = X . W2^T + b2 (the
 *                           vertex-feature half of the Linear layer; W2 [H2, ldw2] row-major).  Row i of
 *                           the block is stored at Y2[row_map[i]] when row_map != NULL -- pass the graph's
 *                           invperm so that every workgroup of the fused kernel reads one contiguous run;
 *   fsw_conv_fused_f32      neighbourhood kernel + E . W1^T on the fp32 matrix cores; with Yin != NULL it
 *                           adds row invperm-position p of Yin [n, ldyin] -- or, with yin_by_node != 0, row `node` of a Yin kept
 *                           in node order (a block that a BLAS GEMM produced: no row permutation) -- else lin_bias, applies the
 *                           activation (0 none, 1 relu, 2 leaky relu with `slope`) and stores Y [n, ldy].
 * Preconditions of fsw_conv_fused_f32: unit weights (args->w == NULL), tau <= 1, fsw_conv_fused_lds_bytes() <= 64 KiB.
 * It computes the rows of in-degree 0 .. FSW_REG_MAX_DEG; rows above that are left untouched in Y -- the caller runs
 * fsw_embed_f32 for them (num_reg_rows = num_zero_rows = 0 restricts that call to the long rows) and applies the Linear
 * layer to those rows itself (fsw_gnn_amd/fsw_conv.py does: a graph with a few hubs keeps the fused kernel for the rest).
 * args->out / ldo are ignored.  Wq: W1^T packed for 16-byte operand loads, zero padded:
 *   Wq[((g*ldw + j)*8) + 4*h + i] = W1[j][8g + 2i + h],  g < ceil(K/8) + 16 (the tail groups are zero:
 *   the kernel prefetches past the end), j < ldw (Hout rounded up to 32), K = has_mass + S, h in {0,1},
 *   i in {0..3}; 16-byte aligned.                                                                      */
size_t fsw_conv_fused_lds_bytes(int S, int has_mass);
/* Packs K columns of W [Hout, ldw_in] starting at column col0 (= the W1 block that multiplies the embedding columns
 * a call of fsw_conv_fused_f32 produces: the whole embedding on one GPU, one rank's [mass |] slice block under slice
 * sharding) into Wq (fsw_packed_linear_floats(K, Hout) floats, 16-byte aligned, layout above) and, when W2out != NULL,
 * copies the d2 columns of W2 (a pointer INTO W, row stride ldw_in) to W2out [Hout, ldw2out].  One launch per
 * forward: nothing is cached on the host, so in-place edits of the weights are always seen.                        */
size_t fsw_packed_linear_floats(int K, int Hout);
int fsw_pack_linear_f32(const float* W, int64_t ldw_in, int Hout, int col0, int K, float* Wq, const float* W2, int d2,
                        float* W2out, int64_t ldw2out, fsw_stream_t stream);
int fsw_project_linear_f32(const float* X, int64_t n, int d, int64_t ldx, const float* V, int S, int64_t ldv,
                           float* Xp, int64_t ldp, const float* W2, int H2, int64_t ldw2, const float* b2, float* Y2,
                           int64_t ldy2, const int32_t* row_map, int32_t* stats, fsw_stream_t stream);
int fsw_conv_fused_f32(const fsw_embed_args* args, const float* Wq, int64_t ldw, const float* lin_bias, int Hout,
                       const float* Yin, int64_t ldyin, int yin_by_node, int act, float slope, float* Y, int64_t ldy,
                       fsw_stream_t stream);
/* R[r, c] = act(R[r, c] + Yin[r, c] + bias[c]) for rows x H floats in place, one launch (Yin, bias may be NULL; act as in
 * fsw_conv_fused_f32).  Epilogue of the slice-sharded layer forms (fsw_gnn_amd/dist.py): the rows a rank owns after the
 * reduce-scatter of the partial sums receive x . W2^T + b (reference fsw_conv.py:357-362, the vertex-feature half of mlp[0]) and
 * the activation.                                                                                                          */
int fsw_add_bias_act_f32(float* R, int64_t ldr, const float* Yin, int64_t ldyin, const float* bias, int64_t rows, int H, int act,
                         float slope, fsw_stream_t stream);

/* ---- backward of the fused neighbourhood kernels (every weight mode and degree class) -----------------
 * Replaces the reverse-mode chain of the reference's sparse autograd Functions (ag.*.backward, reference
 * fsw_embedding.py:1284-2257; reverse segcumsum :2158-2172; scatter-unsort :2055-2070).  Given the output
 * gradient g [num_rows, ldg] (column has_mass + k belongs to slice k; the same args as the forward, args->out
 * ignored) it ACCUMULATES
 *   gXp[j, k]  += out_scale * sum over edges j->i of g[i,k] * C[D_i][rank_ik(j)][k]      (gXp zeroed by the caller)
 *   gfreq[k]   += out_scale * sum_i g[i,k] * sum_t dC[D_i][t][k] * p_(t)                  (nullable)
 * with dC = dC/dxi from fsw_unit_dcoeff_table (same layout as fsw_unit_coeff_table; used on the unit-weight
 * register path, may be NULL otherwise -- weighted rows and rows above FSW_REG_MAX_DEG evaluate the
 * coefficients in float64 on the fly; args->scratch as for fsw_embed_f32 when num_global_rows != 0).  The
 * weights are constants (no gradient w.r.t. w).  The gradients of X and projVecs follow as two plain GEMMs:
 * gX = gXp . projVecs, gprojVecs = gXp^T . X.                                                              */
int fsw_unit_dcoeff_table(const float* freqs, int S, int max_deg, float* dtable, int64_t ldt, fsw_stream_t stream);
int fsw_embed_backward_f32(const fsw_embed_args* args, const float* dtable, const float* g, int64_t ldg, float* gXp,
                           int64_t ldgp, float* gfreq, fsw_stream_t stream);
/* Edge-feature graphs: the same backward, but the gradient of every KEY is stored instead of being accumulated:
 * gkey[e*ldk + k] = out_scale * g[i,k] * C(entry e, slice k) for CSR entry e of row i (gkey zeroed by the caller).
 * From it: gXp = scatter-add of gkey rows by col, g_efeat = gkey . Ve, gVe = gkey^T . efeat.               */
int fsw_embed_backward_keys_f32(const fsw_embed_args* args, const float* dtable, const float* g, int64_t ldg, float* gkey,
                                int64_t ldk, float* gfreq, fsw_stream_t stream);
/* Store-and-sum backward (no float atomics on the register rows; the reference's own backward is an index_add of the same
 * terms, ag.permute_sparse.backward fsw_embedding.py:1286): fsw_embed_backward_keys_f32 with dtable != NULL stores the key
 * gradients of a unit-weight graph, fsw_graph_transpose lists the CSR entries sender by sender (cptr [num_cols + 1], order [nnz];
 * workspace of fsw_graph_workspace_bytes(num_cols, nnz) bytes; entries whose col is out of range sort last and belong to no
 * sender), and fsw_segment_sum_rows_f32 forms out[j, 0:S] = sum over q in cptr[j] .. cptr[j+1]-1 of src[order[q], 0:S].
 * `out` must be zeroed by the caller (senders without out-edges are not written; a sender whose list crosses a 256-entry
 * segment boundary is accumulated).  Sums of up to two segments are bitwise reproducible.                    */
int fsw_graph_transpose(const int32_t* col, int64_t nnz, int64_t num_cols, int32_t* cptr, int32_t* order, void* workspace,
                        size_t workspace_bytes, fsw_stream_t stream);
int fsw_segment_sum_rows_f32(const float* src, int64_t lds, const int32_t* ptr, const int32_t* order, int64_t num_out, int64_t nnz,
                             int S, float* out, int64_t ldo, fsw_stream_t stream);

/* Backward WITH the gradient of the weights, float32, diagonal mode, no edge features (csrc/embed_w_bwd.hip).  args as for
 * fsw_embed_backward_keys_f32 with w != NULL and efeat == NULL (an error otherwise); args->tau is used as given.  For the output
 * gradient g [num_rows, ldg] (column has_mass + k belongs to slice k):
 *   gkey[e * ldk + k]  = out_scale * g[r, k] * d out[r, k] / d key_e      (stored, every entry)
 *   gfreq[k]          += out_scale * sum_r g[r, k] * d out[r, k] / d xi_k  (accumulated; nullable)
 *   gw[e]             += out_scale * sum_k g[r, k] * d out[r, k] / d w_e   (accumulated: zeroed by the caller; the total-mass
 *                        column's dependence on w is NOT included)
 * Rows of 1 .. 24 neighbours run on register kernels (float64 coefficients, the 64 slices of a chunk summed in float64, one float32
 * atomic per entry and chunk).  Rows of 25 .. fsw_embed_backward_w_tuned_max_degree() = 1024 neighbours run on the wave-sort kernels
 * of csrc/embed_w_sort_bwd.hip: one (row, slice) line of D + 1 packed (key, element index) words per wavefront, float64 cumulative
 * weights and coefficients, the slices a workgroup visits for a row summed in float64 in LDS, at most 4 float32 atomics per entry.
 * Longer rows run on the scratch-line kernels of csrc/embed_w_long_bwd.hip: one wavefront per (row, group of
 * fsw_embed_backward_w_long_slices() consecutive slices), the line sorted in chunks of 1024 packed words and merged by sweeps over a
 * line in `scratch`, the group's slices summed in float64 in that line, ceil(S / fsw_embed_backward_w_long_slices()) float32 atomics
 * per entry.  They are launched only when the host-side row counts of args (bin_start_host, else num_lds_rows / num_global_rows;
 * -1 = unknown) say such rows exist; only then is scratch required.  A wavefront's line takes 20 bytes per element of
 * pow2ceil(longest row of its degree bin + 1); the call uses min(scratch_bytes / that, 2048, tasks) wavefronts per bin and fails,
 * before anything is launched, when scratch_bytes holds no line of the largest non-empty bin.
 * fsw_embed_backward_w_scratch_bytes(max_degree, num_rows) is an UPPER BOUND of what a call needs (0 when max_degree <= 24; above,
 * fsw_embed_generic_scratch_bytes: 36 bytes per element of pow2ceil(max_degree + 1) for up to 2048 lines): a call with
 * scratch == NULL, scratch_bytes == 0 succeeds on a graph without rows above fsw_embed_backward_w_tuned_max_degree().
 * max_degree: host value, an upper bound of the longest row.                                                         */
size_t fsw_embed_backward_w_scratch_bytes(int64_t max_degree, int64_t num_rows);
int fsw_embed_backward_w_tuned_max_degree(void); /* the largest degree that needs no scratch: 1024 */
int fsw_embed_backward_w_long_slices(void);      /* slices per wavefront task of the rows above: 4 */
int fsw_embed_backward_w_f32(const fsw_embed_args* args, int64_t max_degree, const float* g, int64_t ldg, float* gkey, int64_t ldk,
                             float* gfreq, float* gw, void* scratch, size_t scratch_bytes, fsw_stream_t stream);
/* The same with weights of more than float32 precision: entry e has the weight w[e] + w_lo[e] (w_lo [nnz], NULL = 0), summed in
 * float64 by every kernel of this entry -- weights that the host computed in float64 ('gcn' normalisation, sums of parallel edges) and
 * split into a float32 value and its float32 remainder.  d out / d w at frequency xi feels a weight's rounding times 2 pi xi, so the
 * 2^-25 of a float32 weight shows in the gradient of a short row at xi ~ 100 (DESIGN.md "Per-edge weights").  The forward reads
 * w alone.                                                                                                              */
int fsw_embed_backward_w_lo_f32(const fsw_embed_args* args, const float* w_lo, int64_t max_degree, const float* g, int64_t ldg,
                                float* gkey, int64_t ldk, float* gfreq, float* gw, void* scratch, size_t scratch_bytes,
                                fsw_stream_t stream);

/* ---- generic neighbourhood kernel: any in-degree, float32 or float64 storage, float64 arithmetic -------------------------
 * (csrc/embed_generic.hip; fsw_embed_cart_generic below is the same kernel read out at every frequency)  Two uses:
 *   value_dtype 1 (float64): the float64 build of the path -- FSW_embedding / FSW_conv(dtype=torch.float64), which the
 *       reference's own test_conv.py runs (test_conv.py:24); forward (g == NULL) and backward (g != NULL);
 *   value_dtype 0 (float32): gradients with respect to the weights for the float32 path (gw), which the tuned backward
 *       kernels above treat as constants (reference ag.div_sparse_dense.backward fsw_embedding.py:1656,
 *       ag.cumsum_sparse.backward :2160, ag.permute_sparse.backward :1286).
 * The graph is a plain CSR (rowptr / col / w in CSR order, no degree bins).  All value pointers have the type selected by
 * value_dtype.  Ke (nullable): the edge-feature term of every key, Ke[e * ldke + k] = <efeat_e, projVecs[k, d_in:]>
 * (reference fsw_embedding.py:934-968), added to Xp[col[e], k].
 * Forward:  out[r * ldo + has_mass + k] = out_scale * ((1 + xi_k) sum_t Delta_t p_(t) + bias[has_mass + k]), and with has_mass
 *           out[r * ldo] = out_scale * (f(m_r) * mass_scale + bias[0]).
 * Backward: for the output gradient g [num_rows, ldg] (column has_mass + k belongs to slice k)
 *           gkey[e * ldk + k]  = out_scale * g[r, k] * d out[r, k] / d key_e              (stored; nullable)
 *           gfreq[k]          += out_scale * sum_r g[r, k] * d out[r, k] / d xi_k          (accumulated; nullable)
 *           gw[e]             += out_scale * sum_k g[r, k] * d out[r, k] / d w_e           (accumulated; nullable; the
 *                                total-mass column's dependence on w is NOT included).
 * scratch: fsw_embed_generic_scratch_bytes(max_degree, num_rows) bytes: 36 bytes per element of a line of the next power of two
 *          >= max_degree + 1 elements, one line for each of up to 2048 workgroups, at most 1 GiB.  The diagonal and the Cartesian
 *          entry share the layout, so both *_scratch_bytes functions return the same value (the diagonal one returned 28 bytes
 *          per element, 7/9 of this, while it had a kernel of its own); always ask the library for the size.          */
typedef struct {
  int32_t value_dtype;   /* 0 float32, 1 float64 */
  int32_t S;
  const int32_t* rowptr;
  const int32_t* col;
  const void* w;         /* [nnz] raw weights, NULL = unit */
  int64_t num_rows;
  int64_t max_degree;    /* host value: an upper bound of the longest row */
  const void* Xp;
  int64_t ldp;
  const void* Ke;
  int64_t ldke;
  const void* freqs;
  double tau;
  void* out;
  int64_t ldo;
  const void* bias;
  double out_scale;
  int32_t has_mass;
  int32_t mass_fn;
  double mass_scale;
  const void* g;
  int64_t ldg;
  void* gkey;
  int64_t ldk;
  void* gfreq;
  void* gw;
  void* scratch;
  size_t scratch_bytes;
} fsw_generic_args;

size_t fsw_embed_generic_scratch_bytes(int64_t max_degree, int64_t num_rows);
int fsw_embed_generic(const fsw_generic_args* args, fsw_stream_t stream);
/* Xp [n, ldp] = X [n, ldx] . V [S, ldv]^T in float64 on the matrix cores (v_mfma_f64_16x16x4_f64); sets
 * FSW_FLAG_X_NONFINITE in stats[FSW_STAT_FLAGS] (stats nullable) */
int fsw_project_f64(const double* X, int64_t n, int d, int64_t ldx, const double* V, int S, int64_t ldv, double* Xp,
                    int64_t ldp, int32_t* stats, fsw_stream_t stream);

/* ---- Cartesian slice x frequency mode (csrc/embed_cart.hip; the generic kernel: csrc/embed_generic.hip) ------------------------
 * FSW_embedding(d_in, nSlices=S, nFreqs=F) (reference fsw_embedding.py:241-259, 1037-1045): every slice s is sorted once and read
 * out at every frequency f.  Column has_mass + s * F + f of out belongs to (slice s, frequency f) (torch.flatten order, :853-854):
 *   out[r * ldo + has_mass + s F + f] = out_scale * ((1 + xi_f) sum_t Delta_t(xi_f) p_(t) + bias[has_mass + s F + f])
 *   out[r * ldo]                      = out_scale * (f(m_r) * mass_scale + bias[0])                     if has_mass
 * where p_(t) sorts Xp[col[e], s] over the row's entries (+ the pad element) and Delta_t is the readout of fsw_embed_generic.
 * fsw_embed_cart_backward_keys_f32 (below) is the tuned float32 backward of fsw_embed_cart_f32 for keys and frequencies.
 * fsw_embed_cart_f32      tuned float32 forward on a graph of fsw_graph_build: needs perm, bin_start and bin_start_host and
 *                         unit_table = fsw_unit_coeff_table(freqs, F, FSW_REG_MAX_DEG) when w == NULL and tau <= 1.
 *                         Scratch: fsw_embed_cart_forward_scratch_bytes(args) bytes (0: scratch may be NULL).  Only the rows of
 *                         the longest class (csrc/embed_cart.h: kCartLong -- w == NULL and tau <= 1: above FSW_HUB_MAX_DEG neighbours;
 *                         general weights: FSW_CART_W_MAX_LINE neighbours and more) need it: their lines are sorted in blocks in a
 *                         scratch line per workgroup.  The minimum is ONE line (the query for one such row and S = 1), 16-byte
 *                         aligned; a buffer of fsw_embed_cart_scratch_bytes(args, 0) bytes, the size before that query existed,
 *                         still works.  The output does not depend on the size of the buffer.
 *                         max_degree (host value) is required: with max_degree == 0 and a row in the first degree bin of
 *                         the longest class the call is refused.
 *                         Rows of 1 .. FSW_REG_MAX_DEG unit-weight neighbours are stored 16 bytes at a time when F % 4 == 0,
 *                         ldo % 4 == 0, ldt % 4 == 0 and out + has_mass, bias + has_mass and unit_table are 16-byte aligned (a
 *                         caller with a mass column gets there by starting its rows 3 floats into an aligned buffer).
 * fsw_embed_cart_generic  the kernel of fsw_embed_generic with every sorted slice read out at all F frequencies: any degree, float32 or
 *                         float64 storage (value_dtype), float64 arithmetic, on a plain CSR (perm, bin_start ignored; no edge term);
 *                         forward (g == NULL) or backward (g != NULL): for the output gradient g [num_rows, ldg]
 *                           gkey[e * ldk + s]  = sum_f out_scale g[r, has_mass + s F + f] d out / d key_e     (stored; nullable)
 *                           gfreq[f]          += out_scale sum_{r,s} g[r, has_mass + s F + f] d out / d xi_f  (nullable)
 *                           gw[e]             += out_scale sum_{s,f} g[r, has_mass + s F + f] d out / d w_e   (nullable; the
 *                                                total-mass column's dependence on w is NOT included).
 *                         scratch: fsw_embed_cart_generic_scratch_bytes(max_degree, num_rows) bytes.                         */
typedef struct {
  int32_t value_dtype;   /* 0 float32, 1 float64 (fsw_embed_cart_f32: 0) */
  int32_t S;             /* slices (columns of Xp used) */
  int32_t F;             /* frequencies */
  int32_t has_mass;
  const int32_t* rowptr;
  const int32_t* col;
  const void* w;         /* [nnz] raw weights, NULL = unit */
  const int32_t* perm;
  const int32_t* bin_start;
  const int32_t* bin_start_host;   /* HOST copy of the FSW_NUM_BINS + 1 words of bin_start */
  int64_t num_rows;
  int64_t max_degree;    /* host value: an upper bound of the longest row */
  const void* Xp;
  int64_t ldp;
  const void* freqs;     /* [F], any finite value of either sign: 0 and -0.0 take the linear branch, -1 yields out_scale * bias only */
  double tau;
  const float* unit_table;
  int64_t ldt;
  void* out;
  int64_t ldo;
  const void* bias;      /* NULL or [has_mass + S F] */
  double out_scale;
  int32_t mass_fn;
  int32_t flags;         /* 0, or bits: FSW_CART_SPLIT_LINES, FSW_CART_SPLIT_W_LINES (fsw_embed_cart_f32 only), FSW_CART_SPLIT_BWD_LINES, FSW_CART_SPLIT_W_BWD_LINES (fsw_embed_cart_backward_keys_f32 only) */
  double mass_scale;
  const void* g;
  int64_t ldg;
  void* gkey;
  int64_t ldk;
  void* gfreq;
  void* gw;
  void* scratch;
  size_t scratch_bytes;
} fsw_cart_args;

size_t fsw_embed_cart_generic_scratch_bytes(int64_t max_degree, int64_t num_rows);
int fsw_embed_cart_generic(const fsw_cart_args* args, fsw_stream_t stream);
int fsw_embed_cart_f32(const fsw_cart_args* args, fsw_stream_t stream);
/* Backward of fsw_embed_cart_f32 on the same graph (perm, bin_start, bin_start_host), float32 (csrc/embed_cart_bwd.hip).
 * Reads   args->g [num_rows, ldg]  (column has_mass + s F + f; column 0 of a mass module is ignored here)
 * Stores  args->gkey[e * ldk + s] = out_scale * sum_f g[r, has_mass + s F + f] * d out[r,s,f] / d key_e   for EVERY entry e, s < S
 * Adds    args->gfreq[f]         += out_scale * sum_{r,s} g[r, has_mass + s F + f] * d out[r,s,f] / d xi_f  (nullable; caller zeroes)
 * args->gw must be NULL (gradients w.r.t. the weights stay on fsw_embed_cart_generic).
 * unit_dtable: fsw_unit_dcoeff_table(freqs, F, FSW_REG_MAX_DEG) when w == NULL and tau <= 1 (with args->unit_table as in the forward).
 * Scratch: fsw_embed_cart_backward_keys_scratch_bytes(args) bytes (0: scratch may be NULL).
 *   A buffer of fsw_embed_cart_scratch_bytes(args, 1) bytes, the size before that query existed, or of
 *   fsw_embed_cart_generic_scratch_bytes(max_degree, rows >= 1) bytes also suffices and gives bit-identical gkey.
 * The buffer must be 16-byte aligned.  No float32 row runs on the generic kernel: the rows of the longest class (csrc/embed_cart.h:
 * kCartLong; csrc/embed_giant_cart_bwd.hip) are sorted in runs in a scratch line per workgroup, as in the forward. */
int fsw_embed_cart_backward_keys_f32(const fsw_cart_args* args, const float* unit_dtable, int64_t lddt, fsw_stream_t stream);
/* Scratch of fsw_embed_cart_f32 (backward == 0) or fsw_embed_cart_backward_keys_f32 (backward != 0) for the graph and weight mode of
 * args, of which it reads bin_start_host, max_degree, w (NULL or not), tau and S: host values only, no device is needed. */
size_t fsw_embed_cart_scratch_bytes(const fsw_cart_args* args, int backward);
/* Scratch of fsw_embed_cart_f32 for the graph and weight mode of args, of which it reads bin_start_host, max_degree, w (NULL or not),
 * tau and S: host values only.  0 when no row belongs to the longest class of its mode.  Otherwise lines x line_bytes: line_bytes is
 * what ONE workgroup needs for the longest row -- 4 bytes per key of the line rounded up to whole blocks (w == NULL and tau <= 1),
 * four float lines of max_degree + 1 elements rounded up to whole blocks (general weights: keys and weights, twice) --, and
 * lines = min(rows from the class's first degree bin on x S, the workgroups the launch would use), the whole at most 2 GiB and never below one line.
 *   (general weights: that bin also holds shorter rows of the class below, which are counted but skipped by the kernel.)
 *   Any 16-byte aligned buffer that holds at least one line works: fewer workgroups then share the rows, with bit-identical output.
 *   A buffer of fsw_embed_cart_generic_scratch_bytes(max_degree, 1) bytes still suffices: its 36 * pow2ceil(max_degree + 1) bytes
 *   exceed one line in both modes. */
size_t fsw_embed_cart_forward_scratch_bytes(const fsw_cart_args* args);
/* Split form of the longest unit-weight rows (csrc/embed_split_cart.hip): args->flags & FSW_CART_SPLIT_LINES asks fsw_embed_cart_f32 to
 * run the rows above FSW_HUB_MAX_DEG neighbours (w == NULL and tau <= 1) with every phase -- sorting blocks of 32768 keys, the
 * exchanges between blocks, the tail of every merge level, the readout -- as a launch of its own over (line, block), so that ONE long line
 * keeps the whole chip busy instead of one workgroup.  Consecutive launches in the caller's stream are the only synchronisation.
 * All other rows run as without the flag; a line's output depends on the line only (not on S, the other rows or the scratch's content).
 *   fsw_embed_cart_split_scratch_bytes  host values only (bin_start_host, max_degree, w, tau, S, F).  With the flag set, args->scratch
 *       must be 16-byte aligned and hold at least this many bytes, else the call is refused before any launch:
 *         lines = (rows from the first degree bin of that class on) x S,   nbmax = ceil(max_degree / 32768),
 *         bytes = lines * nbmax * 32768 * 4   (every line owns a region of block-rounded max_degree keys, 4 bytes each)
 *               + lines * nbmax * F * 4       (one partial sum per line, block and frequency; the part starts 16-byte aligned).
 *       0 when there is nothing to split -- w != NULL, tau > 1, no row in that bin, max_degree < 32769 -- or when bytes would exceed
 *       2 GiB.  Where it is 0 the flag is ignored: the call is then bit-identical to flags == 0 (scratch rules above).
 *   fsw_embed_cart_split_lines          the lines the split form takes for args (rows x S), 0 where the size query is 0.
 *   fsw_embed_cart_split_max_lines      the largest line count for which the host layer (fsw_gnn_amd/fsw_embedding.py) sets the flag: with
 *       more lines the one-workgroup-per-line kernel fills the chip by itself.  At least 16.  The library does what the flag says.
 * fsw_embed_cart_backward_keys_f32, fsw_embed_cart_generic and fsw_conv_fused_cart_f32 ignore the flag, and so does
 * fsw_embed_cart_forward_scratch_bytes. */
#define FSW_CART_SPLIT_LINES 1
size_t fsw_embed_cart_split_scratch_bytes(const fsw_cart_args* args);
int64_t fsw_embed_cart_split_lines(const fsw_cart_args* args);
int64_t fsw_embed_cart_split_max_lines(void);
/* Split form of the longest unit-weight rows' BACKWARD (csrc/embed_split_cart_bwd.hip): args->flags & FSW_CART_SPLIT_BWD_LINES asks
 * fsw_embed_cart_backward_keys_f32 to run the rows above FSW_HUB_MAX_DEG neighbours (w == NULL and tau <= 1) with every phase -- sorting
 * runs of FSW_LDS_MAX_DEG packed (key, entry index) words, every merge level, the walk over the sorted line in tiles of 4096 ranks, the
 * sum of the frequency gradients -- as a launch of its own over (line, piece).  Consecutive launches in the caller's stream are the only
 * synchronisation.  All other rows run as without the flag.  gkey of these rows is bit-identical to the call without the flag and depends
 * on the line only (not on S, the other rows or the scratch's content); gfreq differs by the order of summation.
 *   fsw_embed_cart_split_backward_scratch_bytes  host values only (bin_start_host, max_degree, w, tau, S, F).  With the flag set,
 *       args->scratch must be 16-byte aligned and hold at least this many bytes, else the call is refused before any launch:
 *         lines = (rows from the first degree bin of that class on) x S,
 *         words = max_degree rounded up to whole runs of 2048,   tiles = ceil(max_degree / 4096),
 *         bytes = lines * words * 16        (every line owns two regions, ping and pong, of 8-byte words)
 *               + lines * tiles * F * 4     (one partial sum per line, walk tile and frequency), rounded up to a multiple of 16,
 *       or, where that is larger, what part 1 of fsw_embed_cart_backward_keys_scratch_bytes says for the rows of 2049 .. FSW_HUB_MAX_DEG
 *       neighbours, which run their kernels out of the same buffer.
 *       0 when there is nothing to split -- w != NULL, tau > 1, no row in that bin, max_degree < 32769 -- or when the two terms would
 *       exceed 2 GiB.  Where it is 0 the flag is ignored: the call is then bit-identical to flags without it (scratch rules above).
 *   fsw_embed_cart_split_backward_lines          the lines the split form takes for args (rows x S), 0 where the size query is 0.
 *   fsw_embed_cart_split_backward_max_lines      the largest line count for which the host layer (fsw_gnn_amd/fsw_embedding.py) sets
 *       the flag: the largest measured count at which the split form won.  The library does what the flag says.
 * fsw_embed_cart_f32, fsw_embed_cart_generic, fsw_conv_fused_cart_f32 and every scratch query above ignore this flag;
 * fsw_embed_cart_backward_keys_f32 keeps ignoring FSW_CART_SPLIT_LINES. */
#define FSW_CART_SPLIT_BWD_LINES 2
size_t fsw_embed_cart_split_backward_scratch_bytes(const fsw_cart_args* args);
int64_t fsw_embed_cart_split_backward_lines(const fsw_cart_args* args);
int64_t fsw_embed_cart_split_backward_max_lines(void);
/* Split form of the longest GENERAL-WEIGHT rows (csrc/embed_split_cart_w.hip): args->flags & FSW_CART_SPLIT_W_LINES asks fsw_embed_cart_f32
 * to run the rows of FSW_CART_W_MAX_LINE neighbours and more (w != NULL or tau > 1: lines of max_degree + 1 elements with the pad element)
 * with every phase -- the rows' masses, sorting blocks of 8192 (key, weight) elements, every merge-path level, the readout of tiles of 4096
 * ranks, the sum of the tiles -- as a launch of its own over (line, piece).  Consecutive launches in the caller's stream are the only
 * synchronisation.  All other rows run as without the flag (the shorter rows that share the class's first degree bin included); a line's
 * output depends on the line only (not on S, the other rows or the scratch's content).  It is NOT bit-identical to the call without the
 * flag: the float32 sums of a line are formed per tile and added in tile order; both are within the library's bound of the float64 value.
 *   fsw_embed_cart_split_w_scratch_bytes  host values only (bin_start_host, max_degree, w, tau, S, F).  With the flag set, args->scratch
 *       must be 16-byte aligned and hold at least this many bytes, else the call is refused before any launch:
 *         rows = rows from the first degree bin of that class on,   lines = rows x S,
 *         cap = max_degree + 1 rounded up to whole blocks of 8192,   nbmax = cap / 8192,   tiles = cap / 4096,
 *         bytes = lines * cap * 16          (every line owns four float lines: keys and weights, ping and pong)
 *               + lines * tiles * 8         (the float64 sum of the weights of every tile)
 *               + lines * tiles * F * 4     (one partial sum per line, tile and frequency)
 *               + rows * nbmax * 8          (the float64 partial sums of the rows' masses, one per block),
 *       every part rounded up to a multiple of 16, so that each starts 16-byte aligned.
 *       0 when there is nothing to split -- w == NULL and tau <= 1, no row in that bin, max_degree < FSW_CART_W_MAX_LINE, args == NULL --
 *       or when bytes would exceed 2 GiB.  Where it is 0 the flag is ignored: the call is then bit-identical to the same flags without it.
 *   fsw_embed_cart_split_w_lines          the lines the split form takes for args (rows x S), 0 where the size query is 0.
 *   fsw_embed_cart_split_w_max_lines      the largest line count for which the host layer (fsw_gnn_amd/fsw_embedding.py) sets the flag:
 *       the largest measured count at which the split form won.  The library does what the flag says.
 * fsw_embed_cart_backward_keys_f32, fsw_embed_cart_generic, fsw_conv_fused_cart_f32 and every scratch query above ignore this flag;
 * FSW_CART_SPLIT_LINES and FSW_CART_SPLIT_BWD_LINES keep being ignored for general weights. */
#define FSW_CART_SPLIT_W_LINES 4
size_t fsw_embed_cart_split_w_scratch_bytes(const fsw_cart_args* args);
int64_t fsw_embed_cart_split_w_lines(const fsw_cart_args* args);
int64_t fsw_embed_cart_split_w_max_lines(void);
/* Split form of the longest GENERAL-WEIGHT rows' BACKWARD (csrc/embed_split_cart_w_bwd.hip): args->flags & FSW_CART_SPLIT_W_BWD_LINES asks
 * fsw_embed_cart_backward_keys_f32 to run the rows of FSW_CART_W_MAX_LINE neighbours and more (w != NULL or tau > 1: lines of max_degree + 1
 * elements with the pad element) with every phase -- the rows' masses, sorting runs of FSW_LDS_MAX_DEG packed (key, entry index) words, every
 * merge level, the sums of the weights of the tiles of 2048 ranks, the walk over the sorted line tile by tile, the sum of the frequency
 * gradients -- as a launch of its own over (line, piece).  Consecutive launches in the caller's stream are the only synchronisation.  All
 * other rows run as without the flag (the shorter rows that share the class's first degree bin included).  gkey of these rows depends on
 * the line only (not on S, the other rows or the scratch's content).  It is NOT bit-identical to the call without the flag: the row mass
 * and the cumulative weights are added in another float64 order; both are within the library's bound of the float64 value.  gfreq differs
 * by the order of summation.
 *   fsw_embed_cart_split_w_backward_scratch_bytes  host values only (bin_start_host, max_degree, w, tau, S, F).  With the flag set,
 *       args->scratch must be 16-byte aligned and hold at least this many bytes, else the call is refused before any launch:
 *         rows = rows from the first degree bin of that class on,   lines = rows x S,
 *         words = max_degree + 1 rounded up to whole runs of 2048,   tiles = words / 2048,
 *         bytes = lines * words * 16        (every line owns two regions, ping and pong, of 8-byte words)
 *               + rows * tiles * 8          (the float64 partial sums of the rows' masses, one per run)
 *               + lines * tiles * 8         (the float64 sum of the weights of every walk tile)
 *               + lines * tiles * F * 4     (one partial sum per line, walk tile and frequency),
 *       every part rounded up to a multiple of 16, so that each starts 16-byte aligned,
 *       or, where that is larger, what part 1 of fsw_embed_cart_backward_keys_scratch_bytes says for the lines of FSW_LDS_MAX_DEG + 1 ..
 *       FSW_CART_W_MAX_LINE elements, which run their kernels out of the same buffer.
 *       0 when there is nothing to split -- w == NULL and tau <= 1, no row in that bin, max_degree < FSW_CART_W_MAX_LINE, args == NULL --
 *       or when the four parts would exceed 2 GiB.  Where it is 0 the flag is ignored: the call is then bit-identical to the same flags
 *       without it (scratch rules above).
 *   fsw_embed_cart_split_w_backward_lines          the lines the split form takes for args (rows x S), 0 where the size query is 0.
 *   fsw_embed_cart_split_w_backward_max_lines      the largest line count for which the host layer (fsw_gnn_amd/fsw_embedding.py) sets
 *       the flag: the largest measured count at which the split form won.  At least 16.  The library does what the flag says.
 * fsw_embed_cart_f32, fsw_embed_cart_generic, fsw_conv_fused_cart_f32 and every scratch query above ignore this flag;
 * FSW_CART_SPLIT_BWD_LINES keeps meaning unit weights only: fsw_embed_cart_split_backward_* return 0 for general weights. */
#define FSW_CART_SPLIT_W_BWD_LINES 8
size_t fsw_embed_cart_split_w_backward_scratch_bytes(const fsw_cart_args* args);
int64_t fsw_embed_cart_split_w_backward_lines(const fsw_cart_args* args);
int64_t fsw_embed_cart_split_w_backward_max_lines(void);
/* Scratch of fsw_embed_cart_backward_keys_f32 for the graph and weight mode of args, of which it reads bin_start_host, max_degree, w
 * (NULL or not), tau and S: host values only.  The maximum of two parts, 0 when neither applies:
 *   1. the rows of FSW_LDS_MAX_DEG + 1 .. FSW_HUB_MAX_DEG neighbours (general weights: lines of FSW_LDS_MAX_DEG + 1 ..
 *      FSW_CART_W_MAX_LINE elements), one scratch line per wavefront: fsw_embed_cart_backward_scratch_bytes /
 *      fsw_embed_cart_weighted_backward_scratch_bytes for min(max_degree, the longest such row) and the rows from the first
 *      degree bin of these classes on -- the rule of fsw_embed_cart_scratch_bytes(args, 1) without the generic kernel's term;
 *      nothing when w == NULL, tau <= 1 and the degree bins of these classes are empty;
 *   2. the rows of the longest class (w == NULL and tau <= 1: above FSW_HUB_MAX_DEG neighbours; general weights: FSW_CART_W_MAX_LINE
 *      neighbours and more), one scratch line per workgroup: lines x line_bytes, line_bytes = 16 bytes per element of the longest line
 *      (max_degree elements; general weights: max_degree + 1) rounded up to whole runs of FSW_LDS_MAX_DEG elements -- two lines of
 *      packed (key, entry index) words, of which the one that the last merge level leaves free carries the key gradients in entry
 *      order --, lines = min(rows from the class's first degree bin on x S, the workgroups the launch would use: at most 512, a
 *      multiple of 8 from 8 on), the whole at most 2 GiB and never below one line.
 *      (general weights: that bin also holds shorter rows of the class below, which are counted but skipped by the kernel.)
 *   Any 16-byte aligned buffer that holds what part 1 needs and at least one line of part 2 works: fewer workgroups then share the
 *   rows, with bit-identical gkey.  A buffer of fsw_embed_cart_generic_scratch_bytes(max_degree, 1) bytes still suffices: its
 *   36 * pow2ceil(max_degree + 1) bytes exceed the 16 * (max_degree + 1 + FSW_LDS_MAX_DEG) bytes of a line for every row of the class. */
size_t fsw_embed_cart_backward_keys_scratch_bytes(const fsw_cart_args* args);
/* The parts of the answer of fsw_embed_cart_scratch_bytes for a caller without the bins: the backward's scratch for w == NULL and tau <= 1 given the rows above
 * FSW_LDS_MAX_DEG neighbours, and for general weights given the rows of FSW_LDS_MAX_DEG neighbours and more (lines of 12 bytes per
 * element of the padded longest line, min(2048, long_rows * S) of them, at most 2 GiB; 0 when no row is that long). */
size_t fsw_embed_cart_backward_scratch_bytes(int64_t max_degree, int64_t long_rows, int32_t S);
size_t fsw_embed_cart_weighted_backward_scratch_bytes(int64_t max_degree, int64_t long_rows, int32_t S);
/* FSW_conv with a Cartesian embedding, fast path (csrc/conv_fused.hip: k_conv_fused_cart): fsw_conv_fused_f32 for an embedding row
 * [mass | S runs of F outputs], K = has_mass + S F.  One workgroup per 32 rows of one in-degree: every (row, slice) line is gathered
 * from Xp and sorted once, its F outputs go to the LDS tile (never to HBM), then the tile is multiplied by W1^T and finished exactly
 * as in fsw_conv_fused_f32 (same Wq layout with K = has_mass + S F, same Yin / yin_by_node / lin_bias / act / slope / Y arguments).
 * args: as for fsw_embed_cart_f32 (Xp of fsw_project_f32 at ldp >= S, unit_table = fsw_unit_coeff_table(freqs, F, FSW_REG_MAX_DEG)
 * with ldt >= F, bias NULL or [has_mass + S F], out_scale, mass_fn, mass_scale, perm, bin_start, bin_start_host); out / ldo / g /
 * scratch are ignored.  Preconditions: w == NULL, tau <= 1, fsw_conv_fused_cart_lds_bytes(S, F, has_mass) <= 64 KiB and NO row above
 * FSW_REG_MAX_DEG neighbours (checked against bin_start_host: the call fails instead of leaving rows of Y unwritten; the caller
 * runs fsw_embed_cart_f32 + its own GEMM on such graphs).                                                                      */
size_t fsw_conv_fused_cart_lds_bytes(int S, int F, int has_mass);
int fsw_conv_fused_cart_f32(const fsw_cart_args* args, const float* Wq, int64_t ldw, const float* lin_bias, int Hout,
                            const float* Yin, int64_t ldyin, int yin_by_node, int act, float slope, float* Y, int64_t ldy,
                            fsw_stream_t stream);
/* Cartesian mode with edge features (csrc/edge_keys.hip): the key of every CSR entry, stored once,
 *   K[e*ldk + s] = Xp[col[e]*ldp + s] followed by key = fmaf(efeat[e*d_edge + q], Ve[s*ldve + q], key) for q = 0 .. d_edge - 1 in
 *   that order, in float32 -- the rounding rule of the diagonal edge-feature kernels (fsw_embed_args.efeat above).
 * The Cartesian entry points then run unchanged on (Xp := K, ldp := ldk, col := the identity 0 .. nnz - 1), and the gkey [nnz, S] their
 * backward stores is dL/dK: no field of fsw_cart_args and no kernel of theirs knows about edge features.  Ve = projVecs[:, d_in:] read
 * in place (ldve = d_in + d_edge).  Columns S .. ldk - 1 of K are not written.  Any S >= 1, d_edge >= 1, 0 <= nnz < 2^31 (nnz == 0:
 * no launch); needs ldp >= S, ldk >= S, ldve >= d_edge.  The entries of col are trusted (fsw_graph_build_coalesced validated them).
 * A streaming kernel: nnz * (4 + 4 d_edge + 8 S) bytes. */
int fsw_edge_keys_f32(const int32_t* col, int64_t nnz, const float* Xp, int64_t ldp, const float* efeat, int d_edge, const float* Ve,
                      int64_t ldve, int S, float* K, int64_t ldk, fsw_stream_t stream);

/* ---- stand-alone segmented cumulative sum --------------------------------------------------------
 * Replaces segcumsum / segcumsum_cuda (reference fsw_embedding.py:2795-3012): inclusive scan of
 * values restarted wherever consecutive segment ids differ, ONE streaming pass (chained scan with decoupled
 * look-back: every element read once and written once), in place allowed (out == values).  value_dtype: 0 float32, 1 float64 (the reference's torch_dtype
 * enum, fsw_embedding.cu:14-17).  id_bytes: 4 or 8.  reverse != 0 scans from the end (the backward
 * pass of cumsum_sparse, fsw_embedding.py:2158-2172).  workspace: fsw_segcumsum_workspace_bytes(n). */
size_t fsw_segcumsum_workspace_bytes(int64_t n);
int fsw_segcumsum(int value_dtype, const void* values, void* out, const void* segment_ids, int id_bytes,
                  int64_t n, int reverse, void* workspace, size_t workspace_bytes, fsw_stream_t stream);
/* Shape of the scan for one (value_dtype, id_bytes, reverse), for tests that place segment boundaries where the kernel
 * branches: out = { elements per lane and load, elements per group of 64 lanes (the halo), elements per tile,
 * workgroups of the persistent grid on the current device for a large n }.  A wavefront's chunk is a quarter of a tile.
 * No launch; the last value comes from the occupancy computation that fsw_segcumsum itself uses. */
int fsw_segcumsum_geometry(int value_dtype, int id_bytes, int reverse, int32_t out[4]);

/* ---- legacy entry points: exact signatures of reference fsw_embedding.cu:194, 212, 231 ------------
 * Same semantics as the reference kernels (block-local segmented scan + carry add), launched on the
 * default stream with a stream synchronise after the launch, void return.                           */
void segcumsum_wrapper(int dtype, void* values, const int64_t* segment_ids, int64_t size, int64_t max_seg_size,
                       void* block_sums_out, int64_t* block_last_ids_out, bool return_next_level, int64_t num_blocks,
                       int64_t threads_per_block, size_t shared_memory_size);
void add_block_sums_wrapper(int dtype, void* output, const void* block_sums, const int64_t* segment_ids,
                            const int64_t* block_last_id, int64_t size, int64_t num_blocks, int64_t threads_per_block);
int get_max_threads_per_block(int device_index);
/* the launch helpers the reference library exports next to its wrappers (fsw_embedding.cu:125-183): default stream, no
 * synchronisation, void return */
void launch_segcumsum_kernel_float(float* values, const int64_t* segment_ids, int64_t size, int64_t max_seg_size,
                                   float* block_sums_out, int64_t* block_last_ids_out, bool return_next_level,
                                   int64_t num_blocks, int64_t threads_per_block, int64_t shared_memory_size);
void launch_segcumsum_kernel_double(double* values, const int64_t* segment_ids, int64_t size, int64_t max_seg_size,
                                    double* block_sums_out, int64_t* block_last_ids_out, bool return_next_level,
                                    int64_t num_blocks, int64_t threads_per_block, int64_t shared_memory_size);
void launch_add_block_sums_kernel_float(float* output, const float* block_sums, const int64_t* segment_ids,
                                        const int64_t* block_last_id, int64_t size, int64_t num_blocks, int64_t threads_per_block);
void launch_add_block_sums_kernel_double(double* output, const double* block_sums, const int64_t* segment_ids,
                                         const int64_t* block_last_id, int64_t size, int64_t num_blocks, int64_t threads_per_block);

#ifdef __cplusplus
}
#endif
#endif /* FSW_HIP_H */
