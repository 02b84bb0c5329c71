"""Plain float64 numpy references for csrc/conv_fused.hip and the second output block of csrc/project.hip: the unit-weight
coefficient table, the embedding rows of a unit-weight CSR with their magnitudes, the first Linear layer with a per-entry error
bound, the packed weight operand, and the inputs the kernel-level tests share (degree ladder, keys, frequencies).  Nothing here
calls the library.  tests/test_conv_fused_ref_cpu.py pins these formulae to the oracle and the goldens; tests/test_hip_conv_fused.py
holds the C entry points against them.

The bound.  For an output Y[i, j] = act(sum_k E[i, k] W1[j, k] + yin[i, j]) of a row of in-degree D and an embedding K wide,
    bound[i, j] = (D + K + 8) 2^-24 max(1, |slope|) M[i, j],     M = A |W1|^T + |yin|,
where A is E with every term replaced by its absolute value.  It counts roundings of relative size 2^-24 of a term of M: one for the
coefficient (evaluated in float64, stored as float32), one for out_scale * coefficient, D fused multiply-adds along the sorted line,
at most 4 ulp for sqrtf / log1pf in the mass column, K + 1 accumulations of the product and the yin term, and a margin of 2 for the
second-order terms; ReLU and LeakyReLU are Lipschitz with constant max(1, |slope|).  It is derived, not measured."""
import numpy as np

U = 2.0 ** -24                     # unit roundoff of float32
REG_MAX_DEG = 32                   # include/fsw_hip.h: FSW_REG_MAX_DEG
NUM_COLS = 701                     # senders of the ladder graphs
LONG_DEGREES = (33, 40, 257, 2049)
DEFAULT_COUNTS = (1, 31, 32, 33, 127, 128, 129, 257)
PLANTED_FREQS = (0.0, -0.0, -1.0, 1.0, 2.0, 0.5)


# ---- coefficients ---------------------------------------------------------------------------------------------------------------
def unit_coeffs(freqs, max_deg=REG_MAX_DEG):
    """T[D][t][k] for D = 1 .. max_deg, t < D (T[0] is empty): with w = 1 / D and c = (t + 1) / D,
    (1 + xi) 2 w sinc(xi w) cos(pi xi (2 c - w)), which is 2 w at xi = 0 (oracle/fsw_oracle.py: fsw_embed_csr).  xi: the float32
    frequencies widened to float64."""
    return [unit_coeffs_deg(freqs, D) for D in range(max_deg + 1)]


def unit_coeffs_deg(freqs, D):
    """The rows of one degree: [D, K] (empty for D = 0)."""
    xi = np.asarray(freqs, dtype=np.float32).astype(np.float64)
    if D == 0:
        return np.zeros((0, xi.size))
    w = 1.0 / D
    c = (np.arange(D, dtype=np.float64)[:, None] + 1.0) / D
    return (1.0 + xi)[None, :] * 2.0 * w * np.sinc(xi * w)[None, :] * np.cos(np.pi * xi[None, :] * (2.0 * c - w))


def unit_coeffs_flat(freqs, max_deg=REG_MAX_DEG):
    """The same table in the library's row order D (D - 1) / 2 + t: [max_deg (max_deg + 1) / 2, K]."""
    return np.concatenate(unit_coeffs(freqs, max_deg)[1:], axis=0)


def mass_value(m, mass_fn):
    """f of oracle.total_mass_encode: 0 identity, 1 sqrt, 2 log."""
    m = np.asarray(m, dtype=np.float64)
    if mass_fn == 0:
        return m.copy()
    if mass_fn == 1:
        return 2.0 * (m / (np.sqrt(m + 1.0) + 1.0))
    if mass_fn == 2:
        return np.log1p(m)
    raise ValueError("mass_fn")


MASS_FN_NAMES = ("identity", "sqrt", "log")


# ---- embedding rows -------------------------------------------------------------------------------------------------------------
def embed_rows(rowptr, col, Xp, T, bias=None, out_scale=1.0, has_mass=0, mass_fn=0, mass_scale=1.0):
    """E, A [rows, has_mass + S] in float64 for a unit-weight CSR (parallel edges are separate entries):
        E[i, hm + k] = s (sum_t T[D_i][t][k] sort(Xp[col[row i], k])[t] + b[hm + k]),    E[i, 0] = s (f(D_i) mass_scale + b[0]);
    rows of degree 0 give s b.  A: the same expression with the absolute value of every term.  Xp: the float32 keys the kernel
    reads (any float dtype; widened here).  T: unit_coeffs(...), or a dict {D: unit_coeffs_deg(freqs, D)}; rows of a degree it does not hold are
    NaN in both."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    Xp = np.asarray(Xp, dtype=np.float64)
    T = dict(enumerate(T)) if isinstance(T, (list, tuple)) else T
    S = next(iter(T.values())).shape[1]
    assert Xp.shape[1] >= S
    hm = int(has_mass)
    K = hm + S
    s = float(out_scale)
    b = np.zeros(K) if bias is None else np.asarray(bias, dtype=np.float64).reshape(K)
    deg = np.diff(rowptr)
    E = np.full((deg.size, K), np.nan)
    A = np.full((deg.size, K), np.nan)
    for D in np.unique(deg):
        D = int(D)
        if D not in T:
            continue
        rows = np.nonzero(deg == D)[0]
        e = np.zeros((rows.size, S))
        a = np.zeros((rows.size, S))
        if D > 0:
            idx = rowptr[rows][:, None] + np.arange(D)[None, :]
            keys = np.sort(Xp[col[idx], :S], axis=1)                       # [R, D, S]
            e = np.einsum("tk,rtk->rk", T[D], keys)
            a = np.einsum("tk,rtk->rk", np.abs(T[D]), np.abs(keys))
        E[rows, hm:] = s * (e + b[hm:])
        A[rows, hm:] = abs(s) * (a + np.abs(b[hm:]))
        if hm:
            f = float(mass_value(float(D), mass_fn))
            E[rows, 0] = s * (f * float(mass_scale) + b[0])
            A[rows, 0] = abs(s) * (abs(f * float(mass_scale)) + abs(b[0]))
    return E, A


def cartesian_expand(Xp, freqs, S):
    """Cartesian mode as a diagonal embedding (tests/test_hip_ties.py: cartesian_reference): key column s repeated F times,
    the F frequencies tiled S times; column s F + f belongs to (slice s, frequency f).  Returns (keys [n, S F], freqs [S F])."""
    fr = np.asarray(freqs, dtype=np.float32)
    return np.repeat(np.asarray(Xp)[:, :S], fr.size, axis=1), np.tile(fr, S)


# ---- the first Linear layer -----------------------------------------------------------------------------------------------------
def activation(y, act, slope):
    if act == 0:
        return y
    if act == 1:
        return np.maximum(y, 0.0)
    if act == 2:
        return np.where(y >= 0, y, float(slope) * y)
    raise ValueError("act")


def layer_reference(E, A, W1, deg, yin=None, act=0, slope=0.0):
    """Y_ref = act(E W1^T + yin) and the per-entry bound (module docstring).  yin: [rows, Hout] (a Yin block by node), [Hout]
    (lin_bias) or None.  deg: in-degree per row."""
    W1 = np.asarray(W1, dtype=np.float64)
    K = W1.shape[1]
    y0 = 0.0 if yin is None else np.asarray(yin, dtype=np.float64)
    Y = activation(E @ W1.T + y0, act, slope)
    M = A @ np.abs(W1).T + np.abs(y0)
    lip = max(1.0, abs(float(slope))) if act == 2 else 1.0
    bound = (np.asarray(deg, dtype=np.float64)[:, None] + K + 8.0) * U * lip * M
    return Y, bound


def project_bound(X, V, b=None):
    """Worst-case bound of the bf16x3 projection (csrc/project.hip): (6 d + 8) 2^-24 sum_k |x_k| |v_k| (+ |b|) -- six bf16 planes,
    each accumulated over d terms, and the dropped terms below 2^-24."""
    X = np.abs(np.asarray(X, dtype=np.float64))
    V = np.abs(np.asarray(V, dtype=np.float64))
    M = X @ V.T
    if b is not None:
        M = M + np.abs(np.asarray(b, dtype=np.float64))[None, :]
    return (6.0 * X.shape[1] + 8.0) * U * M


# ---- packed weights -------------------------------------------------------------------------------------------------------------
def packed_floats(K, Hout):
    return ((K + 7) // 8 + 16) * (32 * ((Hout + 31) // 32)) * 8


def pack_reference(W, ldw_in, Hout, col0, K):
    """include/fsw_hip.h verbatim: Wq[((g ldw + j) 8) + 4 h + i] = W1[j][8 g + 2 i + h] with W1 = W[:, col0 : col0 + K], g <
    ceil(K / 8) + 16, ldw = 32 ceil(Hout / 32); zero wherever j >= Hout or k >= K.  W: float32 [Hout, ldw_in]."""
    W = np.asarray(W, dtype=np.float32)
    assert W.shape == (Hout, ldw_in) and col0 + K <= ldw_in
    G, ldw = (K + 7) // 8 + 16, 32 * ((Hout + 31) // 32)
    Wq = np.zeros((G, ldw, 8), dtype=np.float32)
    for g in range((K + 7) // 8):
        for h in range(2):
            for i in range(4):
                k = 8 * g + 2 * i + h
                if k < K:
                    Wq[g, :Hout, 4 * h + i] = W[:, col0 + k]
    return Wq.reshape(-1)


def unpack_reference(Wq, Hout, K):
    """W1 [Hout, K] read back out of a packed operand by the same formula."""
    ldw = 32 * ((Hout + 31) // 32)
    q = np.asarray(Wq).reshape(-1, ldw, 8)
    W1 = np.empty((Hout, K), dtype=q.dtype)
    for k in range(K):
        g, r = divmod(k, 8)
        i, h = divmod(r, 2)
        W1[:, k] = q[g, :Hout, 4 * h + i]
    return W1


# ---- shared inputs --------------------------------------------------------------------------------------------------------------
def ladder(offset=0, counts=DEFAULT_COUNTS, long_rows=False, num_cols=NUM_COLS, square=False, seed=7):
    """Seeded edge list (recipients, senders, num_rows, num_cols): counts[(D + offset) % len(counts)] recipients of every in-degree
    D = 0 .. 32, recipient ids shuffled (perm is then not the identity), senders drawn with replacement from num_cols columns
    (duplicates inside a row: tied keys), edges shuffled; long_rows adds one recipient each of LONG_DEGREES.  square: senders are
    drawn from all nodes (num_cols = num_rows), the graph of a layer."""
    rng = np.random.default_rng(seed + 1000 * offset + len(counts))
    degs = np.concatenate([np.full(counts[(D + offset) % len(counts)], D, dtype=np.int64) for D in range(REG_MAX_DEG + 1)])
    if long_rows:
        degs = np.concatenate([degs, np.array(LONG_DEGREES, dtype=np.int64)])
    num_rows = degs.size
    if square:
        num_cols = num_rows
    assert num_rows != num_cols or square
    degs = degs[rng.permutation(num_rows)]
    rec = np.repeat(np.arange(num_rows, dtype=np.int64), degs)
    snd = rng.integers(0, num_cols, size=rec.size).astype(np.int64)
    order = rng.permutation(rec.size)
    return rec[order], snd[order], num_rows, num_cols


def csr_of(rec, snd, num_rows):
    """(rowptr, col) by recipient, entries of a row in edge-list order."""
    order = np.argsort(rec, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rec, minlength=num_rows))]).astype(np.int64)
    return rowptr, snd[order]


def keys(ncols, ldp, seed=11):
    """float32 standard normal [ncols, ldp]; three sender rows scaled by 1e3 and three by 1e-3, two pairs of identical rows, one row
    of +0.0 and one of -0.0."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((ncols, ldp)).astype(np.float32)
    pick = rng.permutation(ncols)[:12]
    X[pick[0:3]] *= np.float32(1e3)
    X[pick[3:6]] *= np.float32(1e-3)
    X[pick[6]] = X[pick[7]]
    X[pick[8]] = X[pick[9]]
    X[pick[10]] = np.float32(0.0)
    X[pick[11]] = np.float32(-0.0)
    return X


def freqs(S, seed=13):
    """float32 uniform in [-3, 3] with PLANTED_FREQS in the first columns, as many as S allows."""
    fr = np.random.default_rng(seed).uniform(-3.0, 3.0, size=S).astype(np.float32)
    m = min(S, len(PLANTED_FREQS))
    fr[:m] = np.array(PLANTED_FREQS[:m], dtype=np.float32)
    return fr
