"""Cases, float64 references, bounds and check functions of the dense matrix kernel tests (tests/test_hip_dense_matrix.py):
fsw_gemm_tn_f32 (csrc/gemm_tn.hip), the generic fp32 projection kernel k_project and the exact-fp32 kernel k_project_bs
(csrc/project.hip), fsw_project_f64 (csrc/embed_generic.hip).  Every call goes through the C ABI on device buffers whose outputs and
workspace are pre-filled with NaN and whose input rows are padded with NaN: the kernels guard their reads with m < M, so a read of
the padding shows up as a NaN in the result, and a store outside the result shows up as a padding entry that is no longer NaN.

`python -m tests.dense_matrix_cases OUT.npz` is the child process of test_exact_fp32_kernels_in_a_child_process: both EXACT_FP32
switches are read once per process, so the kernels they select need an interpreter of their own.

The k split of fsw_gemm_tn_f32 (include/fsw_hip.h; checked by hand against csrc/gemm_tn.hip, k_gemm_tn_partial_bf3 and the host
function): G = min(512, max(1, K / 512)) workgroups; workgroup g takes the rows [g per, min((g + 1) per, K)) with per =
ceil(K / G) rounded up to a multiple of 16 (bf16 x 3) or of 2 (exact fp32); a workgroup whose range starts at or after K writes
zeros.  64 x 64 blocks of C are numbered row-major, block w and block w + 8 belong to wavefront w.

The bound of fsw_gemm_tn_f32, derived like conv_fused_ref.project_bound.  u = 2^-24, T[m, n] = sum_k |A[k, m]| |B[k, n]|.
  * One workgroup adds `planes` bf16 plane products (x = x1 + x2 + x3, the six products x_i y_j with i + j <= 4; each product of
    two bf16 values is exact in float32) of each of its `per` rows into one float32 accumulator: planes . per terms, whose
    absolute values sum to at most (1 + 2^-7) T_g, in some order: at most planes . per roundings of at most u T_g (1 + 2^-7) each.
  * The G partial sums are added in a fixed order: G - 1 roundings of at most u T each.
  * The dropped products x2 y3, x3 y2, x3 y3 and what is left of x and y after three planes: |x2| <= 2^-9 |x|, |x3| <= 2^-18 |x|,
    remainder <= 2^-27 |x|, together below 4 . 2^-27 |x| |y| = u / 2 per term.  project_bound keeps 8 units for this and for
    the second-order terms; the same 8 are kept here.
  bound = (planes . per + G + 8) u T for the six bf16 planes, and (per + G + 2) u T for the one exact fp32 chain (no dropped
  terms; 2 units for the second-order terms), plus 2 u |beta C0| when beta != 0 (the product beta C0 and the sum are rounded once
  each)."""
import math
import sys

import numpy as np
import torch

from tests import conv_fused_ref as R
from tests.conftest import relerr
from tests.test_hip_conv_fused import TOL, full_significands, last_error, run_project_linear, stream_of, t
from tests.test_hip_conv_fused import test_project_linear_exact_cases as project_linear_exact_cases
from tests.test_hip_project_direct_store import run_project

U = R.U
NAN = float("nan")
TN_MAX_GRID = 512
FLAG_X_NONFINITE = 8              # include/fsw_hip.h (fsw_gnn_amd._lib.FLAG_X_NONFINITE)


# ---- fsw_gemm_tn_f32: the k split, the bound ------------------------------------------------------------------------------------------
def tn_grid(K):
    return min(TN_MAX_GRID, max(1, K // 512))


def tn_piece(K, planes=6):
    """Rows per workgroup."""
    q = -(-K // tn_grid(K))
    return (q + 15) // 16 * 16 if planes == 6 else (q + 1) // 2 * 2


def tn_ranges(K, planes=6):
    """[k0, k1) of every workgroup; k1 == k0 where a workgroup has nothing to do."""
    per = tn_piece(K, planes)
    return [(min(g * per, K), min((g + 1) * per, K)) for g in range(tn_grid(K))]


def tn_blocks(M, N):
    return -(-M // 64) * -(-N // 64)


def tn_needed_bytes(K, M, N):
    return tn_grid(K) * M * N * 4


def tn_bound(A, B, planes=6, beta=0.0, C0=None):
    """The per-entry bound of the module docstring."""
    K = A.shape[0]
    T = np.abs(A.astype(np.float64)).T @ np.abs(B.astype(np.float64))
    bound = (planes * tn_piece(K, planes) + tn_grid(K) + (8.0 if planes == 6 else 2.0)) * U * T
    if beta != 0.0:
        bound = bound + 2.0 * U * np.abs(beta * C0.astype(np.float64))
    return bound


def project_bound(X, V, b=None, planes=6):
    """conv_fused_ref.project_bound ((6 d + 8) units) for six bf16 planes; (d + 2) units for the one exact fp32 chain."""
    d = X.shape[1]
    return R.project_bound(X, V, b) * (1.0 if planes == 6 else (d + 2.0) / (6.0 * d + 8.0))


def worst_ratio(err, bound):
    """Largest |err| / bound and its index; an error where the bound is 0 counts as infinite."""
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = np.unravel_index(ratio.argmax(), ratio.shape)
    return float(ratio[i]), tuple(int(x) for x in i)


def padded(a, pad, dtype=np.float32):
    """a with `pad` more columns of NaN."""
    out = np.full((a.shape[0], a.shape[1] + pad), np.nan, dtype=dtype)
    out[:, :a.shape[1]] = a
    return out


def run_gemm_tn(dev, A, B, beta=0.0, C0=None, pads=(3, 2, 3), ws_fill=NAN, ws_bytes=None, edit=None):
    """fsw_gemm_tn_f32 on host arrays A [K, M], B [K, N]: (status, C [M, N + pads[2]]).  C starts as NaN (or C0 with NaN padding),
    the workspace (fsw_gemm_tn_workspace_bytes unless ws_bytes is given) as ws_fill.  edit(call) changes the arguments."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    (K, M), N = A.shape, B.shape[1]
    Ad, Bd = t(padded(A, pads[0]), dev), t(padded(B, pads[1]), dev)
    Ch = np.full((M, N + pads[2]), np.nan, dtype=np.float32)
    if C0 is not None:
        Ch[:, :N] = C0
    Cd = t(Ch, dev)
    nbytes = int(L.fsw_gemm_tn_workspace_bytes(M, N)) if ws_bytes is None else ws_bytes
    ws = torch.full(((nbytes + 3) // 4 + 1,), ws_fill, device=dev)
    call = dict(A=_lib.ptr(Ad), lda=Ad.stride(0), B=_lib.ptr(Bd), ldb=Bd.stride(0), K=K, M=M, N=N, C=_lib.ptr(Cd), ldc=Cd.stride(0),
                beta=beta, ws=_lib.ptr(ws), ws_bytes=nbytes)
    if edit is not None:
        edit(call)
    rc = L.fsw_gemm_tn_f32(call["A"], call["lda"], call["B"], call["ldb"], call["K"], call["M"], call["N"], call["C"], call["ldc"],
                           call["beta"], call["ws"], call["ws_bytes"], stream_of(dev))
    torch.cuda.synchronize()
    return rc, Cd.cpu().numpy()


def gemm_ok(dev, A, B, **kw):
    """An accepted call: C [M, N], the padding of C still NaN."""
    rc, C = run_gemm_tn(dev, A, B, **kw)
    assert rc == 0, last_error()
    N = B.shape[1]
    assert np.isnan(C[:, N:]).all(), "padding of C was written"
    return np.ascontiguousarray(C[:, :N])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1 (a), (d): integer inputs -------------------------------------------------------------------------------------------------------
TN_INT_K = [1, 2, 7, 8, 9, 15, 16, 17, 511, 512, 1023, 1024, 1025, 4097]      # at (33, 17)
TN_INT_K_LARGE = [65_537, 262_144, 262_145]                                   # at (33, 17); the first one at (65, 64) too
TN_INT_MN = [(1, 1), (31, 33), (32, 32), (64, 64), (65, 64), (512, 64), (513, 64), (64, 1024), (1024, 64), (256, 256), (128, 385)]   # K = 1025
TN_INT_CASES = ([(K, 33, 17) for K in TN_INT_K + TN_INT_K_LARGE] + [(65_537, 65, 64)] + [(1025, M, N) for M, N in TN_INT_MN])
TN_BETAS = [0.0, 1.0, -0.5]
TN_BETA_INT_CASE, TN_BETA_RANDOM_CASE = (4097, 33, 17), (1025, 65, 64)


def check_tn_integer(dev, K, M, N, beta=0.0):
    """Integer A and B, integer even C0: every product and every partial sum is an integer below 2^24, so C equals the int64
    product (+ beta C0) entry for entry whatever the order of the sums."""
    rng = np.random.default_rng(K + 1000 * M + N)
    amax = 4 if K >= 262_144 else 8
    c0max = 64
    assert K * amax * amax + c0max < 2 ** 24
    A = rng.integers(-amax, amax + 1, (K, M)).astype(np.float32)
    B = rng.integers(-amax, amax + 1, (K, N)).astype(np.float32)
    C0 = (2 * rng.integers(-c0max // 2, c0max // 2 + 1, (M, N))).astype(np.float32) if beta != 0.0 else None
    want = np.rint(A.astype(np.float64).T @ B.astype(np.float64)).astype(np.int64)      # float64: exact below 2^53
    if beta != 0.0:
        want = want + np.rint(beta * C0.astype(np.float64)).astype(np.int64)
    C = gemm_ok(dev, A, B, beta=beta, C0=C0)
    assert np.isfinite(C).all(), "entries never written, or C read with beta = 0"
    wrong = np.argwhere(C.astype(np.float64) != want).tolist()
    assert not wrong, ("K %d M %d N %d beta %g: %d wrong entries, first (m, n) = %s: %r, want %d"
                       % (K, M, N, beta, len(wrong), tuple(wrong[0]), float(C[tuple(wrong[0])]), want[tuple(wrong[0])]))


# ---- 1 (b): probe rows ----------------------------------------------------------------------------------------------------------------
TN_PROBE_CASES = [(4097, 1024, 64), (262_145, 33, 17)]


def tn_probe_rows(K, limit, rng, planes=6):
    """Up to `limit` distinct rows: the first and the last row of four workgroups' ranges (the first two, a middle one, the last
    that has rows), K - 1, a row inside the last range, the first 16 of the second range (every residue mod 16, so both halves k
    mod 16 < 8 and >= 8 of a bf16 matrix instruction's k step, and every place in the fp32 kernel's step of four k pairs), the rest
    drawn from all rows."""
    ranges = [r for r in tn_ranges(K, planes) if r[1] > r[0]]
    assert len(ranges) >= 3
    edge = [ranges[g] for g in sorted({0, 1, len(ranges) // 2, len(ranges) - 1})]
    rows = {k for k0, k1 in edge for k in (k0, k1 - 1)} | {K - 1, (ranges[-1][0] + ranges[-1][1]) // 2}
    rows |= {ranges[1][0] + r for r in range(1, 16)}
    assert len(rows) <= limit and len({k % 16 for k in rows}) == 16
    rest = np.setdiff1d(np.arange(K), np.fromiter(rows, dtype=np.int64))
    more = rng.choice(rest, size=min(limit - len(rows), rest.size), replace=False)
    return np.sort(np.concatenate([np.fromiter(rows, dtype=np.int64), more])), edge


def check_tn_probes(dev, K, M, N, exchanged, planes=6):
    """A zero but for one-hot probe rows k (column m(k), value 2^(k mod 5 - 2)), B with full 24-bit significands:
    C[m(k), :] == 2^e B[k, :] bit for bit, every other row of C is 0 (exact in either format: 2^e b is one product, all other
    terms are 0).  exchanged: the roles of A and B (and of M and N) swapped.  planes: the format whose k ranges the probes follow."""
    rng = np.random.default_rng(K + M)
    rows, edge = tn_probe_rows(K, M, rng, planes)
    if K == 262_145:
        ranges = tn_ranges(K, planes)
        if planes == 6:         # the piece rounds up to 528 rows: 497 ranges have rows, the last of them is partly filled
            assert tn_piece(K) == 528 and sum(k1 > k0 for k0, k1 in ranges) == 497 and ranges[496] == (261_888, 262_145)
            assert ranges[-1][0] == ranges[-1][1] and 262_016 in rows
        else:                   # pieces of 514 rows: 511 ranges have rows, the last of them has five, one workgroup has none
            assert tn_piece(K, planes) == 514 and sum(k1 > k0 for k0, k1 in ranges) == 511 and ranges[510] == (262_140, 262_145)
            assert ranges[511][0] == ranges[511][1] and {262_140, 262_142, 262_144} <= set(rows.tolist())
    where = rng.permutation(M)[:rows.size]
    scale = (2.0 ** (rows % 5 - 2)).astype(np.float32)
    hot = np.zeros((K, M), dtype=np.float32)
    hot[rows, where] = scale
    full = full_significands(rng, (K, N))
    want = np.zeros((M, N), dtype=np.float32)
    want[where] = full[rows] * scale[:, None]
    C = gemm_ok(dev, full, hot) if exchanged else gemm_ok(dev, hot, full)
    if exchanged:
        want = np.ascontiguousarray(want.T)
    wrong = np.argwhere(bits(C) != bits(want)).tolist()
    assert not wrong, "K %d: %d wrong entries, first (m, n) = %s; ranges with probes at their edges: %s" % (K, len(wrong), tuple(wrong[0]), edge)
    return rows.size


def check_tn_plane_product(dev):
    """(1 + 2^-9) (1 + 2^-9) = 1 + 2^-8 + 2^-18: both operands are 1 + 2^-9 in their first two bf16 planes, the last term is x2 y2.
    19 significand bits: exact in the fp32 form too."""
    K = M = N = 33
    one = np.float32(1.0 + 2.0 ** -9)
    pi = np.random.default_rng(3).permutation(N)
    A, B = np.zeros((K, M), dtype=np.float32), np.zeros((K, N), dtype=np.float32)
    A[np.arange(K), np.arange(M)] = one
    B[np.arange(K), pi] = one
    want = np.zeros((M, N), dtype=np.float32)
    want[np.arange(M), pi] = np.float32(1.0 + 2.0 ** -8 + 2.0 ** -18)
    assert float(want.max()) == 1.0 + 2.0 ** -8 + 2.0 ** -18
    assert np.array_equal(gemm_ok(dev, A, B), want)


# ---- 1 (c), (d): random inputs --------------------------------------------------------------------------------------------------------
TN_RANDOM_CASES = [(1025, 65, 64), (4097, 128, 385), (70_001, 40, 17)]


def tn_random_inputs(K, M, N):
    rng = np.random.default_rng(K + 1000 * M + N + 1)
    return (rng.standard_normal((K, M)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32),
            rng.standard_normal((M, N)).astype(np.float32))


def check_tn_entries(C, A, B, planes, beta=0.0, C0=None, what="", rows=None, cols=None, normwise=True):
    """|C - ref| <= tn_bound entry for entry (on rows / cols only, if given), and max |C - ref| / max |ref| < 2e-6, the figure of
    test_gemm_tn_weight_gradient_shape (normwise = False: not for the BLAS product, which measures 3.8e-6 at 65 535 x 40 x 17 and
    4.5e-6 at 65 536 x 257 x 256, where the kernel measures 4.5e-7 at 65 536 x 40 x 17).  Returns the largest |err| / bound."""
    ref = A.astype(np.float64).T @ B.astype(np.float64)
    if beta != 0.0:
        ref = ref + beta * C0.astype(np.float64)
    bound = tn_bound(A, B, planes, beta, C0)
    sel = np.ix_(np.arange(C.shape[0]) if rows is None else rows, np.arange(C.shape[1]) if cols is None else cols)
    got, ref, bound = C[sel].astype(np.float64), ref[sel], bound[sel]
    assert np.isfinite(got).all(), what + ": entries never written, or C read with beta = 0"
    err = np.abs(got - ref)
    ratio, at = worst_ratio(err, bound)
    print("gemm_tn %s planes %d beta %g: largest |err| / bound %.4f at %s, max |err| / max |ref| %.2e"
          % (what, planes, beta, ratio, at, err.max() / np.abs(ref).max()))
    assert ratio <= 1.0, (what, at, float(got[at]), float(ref[at]))
    assert not normwise or err.max() / np.abs(ref).max() < 2e-6
    return ratio


def check_tn_random(dev, K, M, N, planes, beta=0.0):
    A, B, C0 = tn_random_inputs(K, M, N)
    C = gemm_ok(dev, A, B, beta=beta, C0=C0 if beta != 0.0 else None)
    check_tn_entries(C, A, B, planes, beta, C0, "K %d M %d N %d" % (K, M, N))
    return C


# ---- 1 (e): workspace -----------------------------------------------------------------------------------------------------------------
TN_WORKSPACE_CASES = [(1025, 65, 64), (4097, 33, 17)]


def check_tn_workspace(dev, K, M, N, planes):
    """G M N 4 bytes are enough and give the same bits as the full size; one byte less is refused and C stays NaN; the bits do not
    depend on what the workspace held, and not on the call."""
    A, B, _ = tn_random_inputs(K, M, N)
    need = tn_needed_bytes(K, M, N)
    C = gemm_ok(dev, A, B)
    check_tn_entries(C, A, B, planes, what="workspace K %d" % K)
    assert np.array_equal(bits(C), bits(gemm_ok(dev, A, B, ws_bytes=need))), "exact-size workspace"
    assert np.array_equal(bits(C), bits(gemm_ok(dev, A, B, ws_bytes=need, ws_fill=0.0))), "workspace of zeros"
    assert np.array_equal(bits(C), bits(gemm_ok(dev, A, B))), "second call"
    rc, Cr = run_gemm_tn(dev, A, B, ws_bytes=need - 1)
    assert rc != 0 and last_error(), "a workspace one byte short was accepted"
    assert np.isnan(Cr).all()


# ---- 1 (f): refusals ------------------------------------------------------------------------------------------------------------------
def _set(**kw):
    return lambda call: call.update(kw)


TN_REFUSALS = {
    "17 blocks": ((16, 1025, 64), None),
    "20 blocks": ((16, 257, 256), None),
    "32 blocks": ((16, 65, 1024), None),
    "K = 0": ((16, 33, 17), _set(K=0)),
    "lda < M": ((16, 33, 17), _set(lda=32)),
    "ldb < N": ((16, 33, 17), _set(ldb=16)),
    "ldc < N": ((16, 33, 17), _set(ldc=16)),
    "A null": ((16, 33, 17), _set(A=None)),
    "B null": ((16, 33, 17), _set(B=None)),
    "C null": ((16, 33, 17), _set(C=None)),
    "workspace null": ((16, 33, 17), _set(ws=None)),
}


def check_tn_refusal(dev, name):
    (K, M, N), edit = TN_REFUSALS[name]
    rng = np.random.default_rng(1)
    A, B = rng.standard_normal((K, M)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    rc, C = run_gemm_tn(dev, A, B, edit=edit)
    assert rc != 0 and last_error(), name
    assert np.isnan(C).all(), name + ": C was written"
    if edit is not None:                                   # the same call without the edit is accepted
        assert np.isfinite(gemm_ok(dev, A, B)).all()


# ---- 1 (g): power-of-two scaling ------------------------------------------------------------------------------------------------------
def check_tn_scaling(dev):
    """Magnitudes in [1/16, 16]: (A 2^40, B 2^-40) gives the same bits, (A 2^100, B 2^-60) exactly 2^40 C -- every split, product
    and sum scales exactly as long as the intermediate format has float32's exponent range."""
    K, M, N = 1025, 65, 64
    rng = np.random.default_rng(7)

    def draw(shape):
        return (rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(-4.0, 4.0, shape)).astype(np.float32)

    A, B = draw((K, M)), draw((K, N))
    C = gemm_ok(dev, A, B)
    assert np.isfinite(C).all()
    up, down, big, small = np.float32(2.0 ** 40), np.float32(2.0 ** -40), np.float32(2.0 ** 100), np.float32(2.0 ** -60)
    assert np.array_equal(bits(gemm_ok(dev, A * up, B * down)), bits(C)), "2^40, 2^-40"
    assert np.array_equal(bits(gemm_ok(dev, A * big, B * small)), bits(C * up)), "2^100, 2^-60"


# ---- 1 (h): non-finite input ----------------------------------------------------------------------------------------------------------
def check_tn_nonfinite(dev, planes):
    """A NaN / Inf in A[k, m]: row m of C is non-finite throughout, every other row within the bound; the same for B and column n.
    k = 1024 is the last row (second workgroup), m = n = 40 lies in the second 32-wide tile."""
    K, M, N = 1025, 65, 64
    A, B, _ = tn_random_inputs(K, M, N)
    k, m, n = K - 1, 40, 40
    for bad in (np.nan, np.inf, -np.inf):
        A2, A0 = A.copy(), A.copy()
        A2[k, m], A0[k, m] = bad, 0.0
        C = gemm_ok(dev, A2, B)
        assert not np.isfinite(C[m]).any(), ("A", bad)
        check_tn_entries(C, A0, B, planes, what="non-finite A[%d, %d]" % (k, m), rows=np.delete(np.arange(M), m))
        B2, B0 = B.copy(), B.copy()
        B2[k, n], B0[k, n] = bad, 0.0
        C = gemm_ok(dev, A, B2)
        assert not np.isfinite(C[:, n]).any(), ("B", bad)
        check_tn_entries(C, A, B0, planes, what="non-finite B[%d, %d]" % (k, n), cols=np.delete(np.arange(N), n))


# ---- 2, 3: the projection entry points ------------------------------------------------------------------------------------------------
def run_project_call(dev, X, V, W2, b2, row_map, ldp, ldy2, pads, x_offset=0, with_copy=False):
    """fsw_project_linear_f32 (W2 given) or fsw_project_f32 on host arrays X [n, d], V [S, d], W2 [H2, d] whose device rows carry
    pads = (X, V, W2) columns of NaN; x_offset: X starts that many floats into its buffer.  Outputs pre-filled with NaN.
    Returns (Xp [n, ldp], Y2 [n, ldy2] or None, x_copy [n, d + 3] or None, flags)."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    n, d = X.shape
    S = V.shape[0]
    ldx = d + pads[0]
    buf = torch.full((n * ldx + x_offset,), NAN, device=dev)
    Xd = buf[x_offset:].view(n, ldx)
    Xd.copy_(t(padded(X, pads[0]), dev))
    Vd = t(padded(V, pads[1]), dev)
    Xp = torch.full((n, ldp), NAN, device=dev)
    stats = torch.zeros(_lib.NUM_STATS, dtype=torch.int32, device=dev)
    Y2 = xc = None
    if W2 is not None:
        assert not with_copy
        H2 = W2.shape[0]
        Wd = t(padded(W2, pads[2]), dev)
        bd = t(b2, dev) if b2 is not None else None
        md = t(row_map, dev, torch.int32) if row_map is not None else None
        Y2 = torch.full((n, ldy2), NAN, device=dev)
        rc = L.fsw_project_linear_f32(_lib.ptr(Xd), n, d, ldx, _lib.ptr(Vd), S, Vd.stride(0), _lib.ptr(Xp), ldp, _lib.ptr(Wd), H2,
                                      Wd.stride(0), _lib.ptr(bd), _lib.ptr(Y2), ldy2, _lib.ptr(md), _lib.ptr(stats), stream_of(dev))
    else:
        xc = torch.full((n, d + 3), NAN, device=dev) if with_copy else None
        rc = L.fsw_project_f32(_lib.ptr(Xd), n, d, ldx, _lib.ptr(Vd), S, Vd.stride(0), _lib.ptr(Xp), ldp, _lib.ptr(xc),
                               d + 3 if with_copy else 0, _lib.ptr(stats), stream_of(dev))
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return (Xp.cpu().numpy(), None if Y2 is None else Y2.cpu().numpy(), None if xc is None else xc.cpu().numpy(),
            int(stats.cpu()[_lib.STAT_FLAGS]))


def project_inputs(n, d, S, H2, mapped, with_b2, seed=0):
    rng = np.random.default_rng(seed + n + 7 * d + 11 * S + 13 * H2)
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = (rng.standard_normal((S, d)) / np.sqrt(d)).astype(np.float32)
    W2 = (rng.standard_normal((H2, d)) / np.sqrt(d)).astype(np.float32) if H2 else None
    b2 = rng.standard_normal(H2).astype(np.float32) if H2 and with_b2 else None
    row_map = rng.permutation(n).astype(np.int32) if H2 and mapped else None
    return X, V, W2, b2, row_map


def check_project_outputs(Xp, Y2, xc, X, V, W2, b2, row_map, slab_end, planes, what):
    """The rules of test_project_linear_random_cases: every entry within project_bound of the float64 product, the columns
    S .. slab_end of Xp hold 0.0 or NaN only, everything from slab_end on and the padding of Y2 and of x_copy keep their NaN, every
    Y2 row is written once, where row_map says; x_copy is X bit for bit.  Returns the largest |err| / bound."""
    S = V.shape[0]
    X64 = X.astype(np.float64)
    assert np.isfinite(Xp[:, :S]).all(), what + ": Xp entries never written"
    pad = Xp[:, S:slab_end]
    assert (np.isnan(pad) | (pad == 0.0)).all() and np.isnan(Xp[:, slab_end:]).all(), what + ": padding of Xp"
    ratio, at = worst_ratio(np.abs(Xp[:, :S] - X64 @ V.astype(np.float64).T), project_bound(X, V, None, planes))
    assert ratio <= 1.0, (what, "Xp", at)
    assert relerr(Xp[:, :S], X64 @ V.astype(np.float64).T) < TOL
    if W2 is not None:
        H2 = W2.shape[0]
        assert np.isfinite(Y2[:, :H2]).all(), what + ": Y2 rows never written"
        assert np.isnan(Y2[:, H2:]).all(), what + ": padding of Y2"
        got = Y2[row_map, :H2] if row_map is not None else Y2[:, :H2]
        ref = X64 @ W2.astype(np.float64).T + (b2.astype(np.float64) if b2 is not None else 0.0)
        r2, at = worst_ratio(np.abs(got - ref), project_bound(X, W2, b2, planes))
        assert r2 <= 1.0, (what, "Y2", at)
        assert relerr(got, ref) < TOL
        ratio = max(ratio, r2)
    if xc is not None:
        d = X.shape[1]
        assert np.array_equal(bits(xc[:, :d]), bits(X)), what + ": x_copy"
        assert np.isnan(xc[:, d:]).all(), what + ": padding of x_copy"
    print("project %s planes %d: largest |err| / bound %.4f" % (what, planes, ratio))
    return ratio


# n, d, S, H2, row_map, b2, x_copy (H2 = 0 only), form.  Forms: "vec" 16-byte aligned rows (k_project<true>: d % 4 != 0 or d > 256),
# "ldx" a row stride of X that is no multiple of 4, "offset" X four bytes into its buffer (both k_project<false>).
# n 1 | 127 | 128 | 129 around the 128-row tile; S + H2 = 127 | 128 | 129 around the 128-column tile; S = 100, H2 = 28 | 29 and
# S = 130, H2 = 20: a column tile that holds columns of Xp and of Y2.
GENERIC_CASES = [
    (1, 1, 1, 0, False, False, True, "vec"),
    (127, 3, 127, 0, False, False, True, "ldx"),
    (128, 13, 100, 28, True, True, False, "vec"),
    (129, 31, 100, 29, True, False, False, "offset"),
    (129, 33, 130, 20, False, True, False, "ldx"),
    (128, 257, 129, 0, False, False, True, "vec"),
    (129, 260, 100, 29, True, True, False, "vec"),
    (127, 260, 19, 33, False, True, False, "ldx"),
    (1, 260, 129, 0, False, False, True, "offset"),
    (129, 13, 19, 160, True, True, False, "ldx"),
    (128, 3, 127, 0, False, False, False, "offset"),
]


def generic_pads(d, form):
    """(pads, x_offset): rows of X, V and W2 padded to a multiple of 4 floats (at least one float of NaN), or X to 1 mod 4."""
    to4 = 4 - d % 4
    if form == "ldx":
        return (to4 + 1, to4, to4), 0
    return (to4, to4, to4), (1 if form == "offset" else 0)


def check_project_generic(dev, n, d, S, H2, mapped, with_b2, with_copy, form, bad=None):
    """One call that k_project serves.  bad = (row, column): X holds an Inf there, and only the flag is checked."""
    X, V, W2, b2, row_map = project_inputs(n, d, S, H2, mapped, with_b2)
    pads, x_offset = generic_pads(d, form)
    if bad is not None:
        X[bad] = np.inf
    Xp, Y2, xc, flags = run_project_call(dev, X, V, W2, b2, row_map, S + 3, H2 + 3, pads, x_offset, with_copy)
    if bad is not None:
        return flags
    assert flags == 0
    return check_project_outputs(Xp, Y2, xc, X, V, W2, b2, row_map, S, 6, "generic n %d d %d S %d H2 %d %s" % (n, d, S, H2, form))


# ---- fsw_project_f64 ------------------------------------------------------------------------------------------------------------------
F64_N, F64_S, F64_D = [1, 15, 16, 17, 65], [1, 15, 16, 17, 33], [1, 3, 4, 5, 13]


def exact_product(X, V):
    """X V^T for the float64 kernel: in np.longdouble where it carries 64 significand bits; otherwise rounded once per entry, by
    math.fsum over the products split exactly in two (Veltkamp / Dekker; no overflow at these magnitudes)."""
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        return X.astype(np.longdouble) @ V.astype(np.longdouble).T

    def halves(a):
        c = 134217729.0 * a                              # 2^27 + 1
        hi = c - (c - a)
        return hi, a - hi

    out = np.empty((X.shape[0], V.shape[0]))
    for i in range(X.shape[0]):
        for j in range(V.shape[0]):
            terms = []
            for x, v in zip(X[i].tolist(), V[j].tolist()):
                (xh, xl), (vh, vl) = halves(x), halves(v)
                terms += [xh * vh, xh * vl, xl * vh, xl * vl]
            out[i, j] = math.fsum(terms)
    return out


def run_project_f64(dev, X, V):
    """fsw_project_f64 with ldx = d + 3, ldv = d + 1 (NaN padding), ldp = S + 5: (Xp [n, S], flags)."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    (n, d), S = X.shape, V.shape[0]
    Xd, Vd = t(padded(X, 3, np.float64), dev, torch.float64), t(padded(V, 1, np.float64), dev, torch.float64)
    Xp = torch.full((n, S + 5), NAN, device=dev, dtype=torch.float64)
    stats = torch.zeros(_lib.NUM_STATS, dtype=torch.int32, device=dev)
    rc = L.fsw_project_f64(_lib.ptr(Xd), n, d, d + 3, _lib.ptr(Vd), S, d + 1, _lib.ptr(Xp), S + 5, _lib.ptr(stats), stream_of(dev))
    assert rc == 0, last_error()
    out = Xp.cpu().numpy()
    assert np.isnan(out[:, S:]).all(), "padding of Xp was written"
    return out[:, :S], int(stats.cpu()[_lib.STAT_FLAGS])


def check_project_f64(dev, n, d, S):
    """Per entry within (d + 2) 2^-53 sum |x| |v| of the exactly rounded product: a chain of d fused multiply-adds."""
    rng = np.random.default_rng(n + 100 * d + 10_000 * S)
    X, V = rng.standard_normal((n, d)), rng.standard_normal((S, d))
    Xp, flags = run_project_f64(dev, X, V)
    assert flags == 0 and np.isfinite(Xp).all()
    err = np.abs(Xp.astype(np.longdouble) - exact_product(X, V)).astype(np.float64)
    ratio, at = worst_ratio(err, (d + 2.0) * 2.0 ** -53 * (np.abs(X) @ np.abs(V).T))
    assert ratio <= 1.0, (n, d, S, at)
    return ratio


# ---- 3: the exact-fp32 projection kernel k_project_bs (d <= 128, d % 4 == 0, 16-byte aligned rows) ---------------------------------------
# n, d, S, H2, row_map, b2, x_copy (H2 = 0 only), ldy2 a multiple of 4.  KQ = 16 | 32 | 64 at d <= 32 | 64 | 128.  (19, 33) and
# (33, 31): a 32-column slab that holds columns of Xp and of Y2; (256, 128): 12 slab wavefronts; (257, 160): 14 slabs, two column
# groups of seven and a helper wavefront.  8192 + 45 rows: a second tile on some workgroups; 3 . 8192 + 167: three or four tiles.
BS_CASES = [
    (1, 4, 19, 33, False, True, False, False),
    (31, 36, 33, 31, True, False, False, True),
    (33, 68, 256, 128, True, True, False, True),
    (33, 128, 257, 160, False, True, False, False),
    (8192 + 45, 128, 256, 128, True, True, False, True),
    (3 * 8192 + 167, 128, 257, 160, True, True, False, False),
    (3 * 8192 + 167, 36, 19, 33, True, False, False, True),
    (8192 + 45, 68, 64, 0, False, False, True, False),
    (33, 4, 33, 0, False, False, True, False),
    (31, 128, 256, 0, False, False, False, False),
    (33, 32, 64, 32, False, False, False, True),
]
BS_MARKER_CASE = (33, 128, 257, 160, False, True, False, False)
WIDE_CASE = (65, 192, 64, 160, True, True, False, True)          # d > 128: the switch changes nothing


def run_project_slabs(dev, n, d, S, H2, mapped, with_b2, with_copy, aligned, bad=None):
    """One call of the matrix-core kernels' shape (ldp = 32 ceil(S / 32) + 4, rows padded with 4 floats of NaN)."""
    X, V, W2, b2, row_map = project_inputs(n, d, S, H2, mapped, with_b2)
    if bad is not None:
        X[bad] = np.inf
    slab_end = 32 * ((S + 31) // 32)
    ldy2 = 4 * ((H2 + 3) // 4) if aligned else H2 + 3
    out = run_project_call(dev, X, V, W2, b2, row_map, slab_end + 4, ldy2, (4, 4, 4), 0, with_copy)
    return out, (X, V, W2, b2, row_map, slab_end)


def check_project_slabs(dev, case, planes):
    (Xp, Y2, xc, flags), (X, V, W2, b2, row_map, slab_end) = run_project_slabs(dev, *case)
    assert flags == 0
    check_project_outputs(Xp, Y2, xc, X, V, W2, b2, row_map, slab_end, planes, "slabs n %d d %d S %d H2 %d" % case[:4])
    S, H2 = case[2:4]
    return np.ascontiguousarray(Xp[:, :S]), None if Y2 is None else np.ascontiguousarray(Y2[:, :H2])


def wide_outputs(dev):
    """WIDE_CASE through run_project_linear: d = 192 is above the exact-fp32 kernel's 128, bf16 x 3 with or without the switch."""
    n, d, S, H2, mapped, with_b2, _, aligned = WIDE_CASE
    X, V, W2, b2, row_map = project_inputs(n, d, S, H2, mapped, with_b2)
    Xp, Y2, flags = run_project_linear(dev, X, V, S, W2, b2, row_map, S + 4, H2)
    assert flags == 0
    check_project_outputs(Xp, Y2, None, X, V, W2, b2, row_map, S, 6, "wide d %d" % d)
    return Xp, Y2


def check_copy_slabs(dev, planes):
    """test_x_copy_is_bit_exact's shape through run_project: 8192 + 45 rows, d = 128, S = 256 and a copy of X."""
    n, d, S = 8192 + 45, 128, 256
    X, V, _, _, _ = project_inputs(n, d, S, 0, False, False, seed=5)
    X[3, 5], X[n - 1, d - 1] = -0.0, np.float32(1e-42)
    Xp, xc, flags = run_project(dev, X, V, S + 4, with_copy=True)
    assert flags == 0
    check_project_outputs(Xp, None, xc, X, V, None, None, None, S, planes, "x_copy n %d d %d S %d" % (n, d, S))


def marker_outputs(dev, planes):
    """The outputs that the child process hands to its parent: one gemm case of 1 (c), one projection case with d = 128, the
    d = 192 case."""
    out = dict(gemm=check_tn_random(dev, *TN_RANDOM_CASES[0], planes))
    out["project_xp"], out["project_y2"] = check_project_slabs(dev, BS_MARKER_CASE, planes)
    out["wide_xp"], out["wide_y2"] = wide_outputs(dev)
    return out


def main(path):
    """The child process: FSW_GEMM_TN_EXACT_FP32=1 and FSW_PROJECT_EXACT_FP32=1 are set, one fp32 chain instead of six planes."""
    import os
    assert os.environ.get("FSW_GEMM_TN_EXACT_FP32") == "1" and os.environ.get("FSW_PROJECT_EXACT_FP32") == "1"
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    planes = 1
    for K, M, N in TN_INT_CASES:
        check_tn_integer(dev, K, M, N)
    for beta in TN_BETAS:
        check_tn_integer(dev, *TN_BETA_INT_CASE, beta=beta)
        check_tn_random(dev, *TN_BETA_RANDOM_CASE, planes, beta=beta)
    for case in TN_RANDOM_CASES:
        check_tn_random(dev, *case, planes)
    for case in TN_WORKSPACE_CASES:
        check_tn_workspace(dev, *case, planes)
    for K, M, N in TN_PROBE_CASES:
        for exchanged in (False, True):
            assert check_tn_probes(dev, K, M, N, exchanged, planes) == M
    check_tn_plane_product(dev)
    check_tn_scaling(dev)
    check_tn_nonfinite(dev, planes)
    print("gemm_tn checks done")
    for d in (4, 32, 64, 128):
        project_linear_exact_cases(dev, d)
    for case in BS_CASES:
        check_project_slabs(dev, case, planes)
    check_copy_slabs(dev, planes)
    n = 8192 + 45
    for bad in ((n - 3, 77), (n - 1, 127)):                     # in a workgroup's second tile
        (_, _, _, flags), _ = run_project_slabs(dev, n, 128, 256, 128, True, True, False, True, bad=bad)
        assert flags & FLAG_X_NONFINITE, "non-finite flag"
    np.savez(path, **marker_outputs(dev, planes))
    print("exact-fp32 checks done")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
