"""Inputs and the numpy restatement shared by tests/test_edge_weight_long_cpu.py and tests/test_hip_edge_weight_long.py: the weight
gradient of rows above 24 neighbours (csrc/embed_w_sort_bwd.hip).

lane_blocked_weight_grad: the sorted, lane-blocked form that kernel evaluates.  A (row, slice) line of D + 1 elements -- the pad
element (key 0, weight max(tau - m, 0)) is element D -- is sorted by key with ties by element index and laid out over 64 lanes of M
ranks each (fillers of weight 0 whose key counts as 0 behind the line).  With h(c) = 2 (1 + xi) cos(2 pi xi c), c1_t = cum_t / M_row,
c0_t = c1_{t-1} (cum: the lane's running sum on top of the exclusive scan of the lanes' weights),
    q_t     = (h(c1_t) - h(c0_t)) key_t
    R(t)    = h(c1_t) key_t + (sum of q over the lanes above) + (sum of q over the later ranks of the same lane)
    HC      = sum_t (h(c1_t) c1_t - h(c0_t) c0_t) key_t
    gw_j(s) = G[row, s] (R(rank_j) - [m <= tau] R(rank_pad) - [m >= tau] HC) / M_row,        M_row = max(m, tau)
The yardstick it is measured against is tests/weight_grad_ref.py (autograd of the forward; none of these formulas).

The rows: one recipient per degree of DEGREES -- both sides of the register class (24 | 25), of every instance's first and last bin
(32 | 33, 192 | 193, 256 | 257, 512 | 513, 1024 | 1025), of D + 1 crossing 64 M (63, 127, 255, 511, 1023, 2047), of the class limit
and of FSW_LDS_MAX_DEG (2048 | 2049) -- with weights of edge_weight_cases.row_weights, the kind (mass below tau / tau exactly /
above tau) cycling over the rows: long rows below tau carry many exact zero weights.  Keys and slices as in edge_weight_cases: BASE
key columns exact in float32, distinct of both signs or tied on the grid of 1/8 with the pad key, expanded to S slices by signed
powers of two (exact, so the reference is computed for BASE slices once per (tau, keys)).
"""
import functools

import numpy as np

from tests import edge_weight_cases as C
from tests import weight_grad_ref as R

DEGREES = (0, 24, 25, 32, 33, 40, 41, 48, 49, 63, 64, 65, 96, 97, 127, 128, 129, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024,
           1025, 2047, 2048, 2049)
ZERO_ROW = DEGREES.index(257)                                 # the long recipient whose output gradient is zero
REG_MAX, TUNED_MAX = 24, 1024                                 # csrc/embed_launch.h: kWRegMaxDeg, kWSortMaxDeg
NO_SCRATCH_MAX = 300                                          # the rows of the test without scratch
BASE = 9                                                      # odd, and small: the reference costs a Python loop per row and slice
S_VALUES = (3, 8, 70)


def ranks_per_lane(D):
    """M of the instance that takes a row of D neighbours (launch_embed_wsort_w_bwd); above the class limit the M the form would
    need (D + 1 <= 64 M), for the restatement only."""
    for M, top in ((4, 192), (8, 256), (16, 512), (32, 1024), (64, 4095)):
        if D <= top:
            return M
    raise ValueError(D)


def slices_per_group(M):
    """SC of the instance (ws_slices in csrc/embed_w_sort_bwd.hip): the float tile next to two float64 lines in 69 KB of LDS."""
    line = 64 * M + 65
    lines = (69 * 1024 // 4 - 4 * line) // line
    return 64 if lines >= 64 else (lines & ~3 if lines >= 4 else lines)


def float32_adds(D, S):
    """Float32 atomic adds an entry of a row of D neighbours receives: one per chunk of 64 slices on the register kernels, one per
    workgroup that visits the row on the wave-sort kernels (gridDim.y = min(4, ceil(S / SC)) of them), one per slice on the generic
    kernel."""
    if D <= REG_MAX:
        return -(-S // 64)
    if D <= TUNED_MAX:
        return min(4, -(-S // slices_per_group(ranks_per_lane(D))))
    return S


def lane_blocked_weight_grad(rowptr, w, K, freqs, tau, G):
    """gW_s [nnz, S] in float64 by the form of the module docstring: rowptr [rows + 1], w [nnz] float64, per-entry keys K [nnz, S],
    freqs [S], G [rows, S] (out_scale included).  Rows of at most REG_MAX neighbours are left at zero."""
    w, K, fr, G = (np.asarray(a, dtype=np.float64) for a in (w, K, freqs, G))
    S = K.shape[1]
    out = np.zeros((w.size, S))
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        D = int(b - a)
        if D <= REG_MAX:
            continue
        M = ranks_per_lane(D)
        m = w[a:b].sum()
        inv = 1.0 / max(m, tau)
        wgt = np.concatenate([w[a:b], [max(tau - m, 0.0)], np.zeros(64 * M - D - 1)])
        idx = np.arange(D + 1)
        for s in range(S):
            xi = fr[s]
            key = np.concatenate([K[a:b, s], [0.0]])
            order = np.lexsort((idx, key))                                       # by key, ties by element index
            ks = np.concatenate([key[order], np.zeros(64 * M - D - 1)]).reshape(64, M)
            ws = np.concatenate([wgt[order], np.zeros(64 * M - D - 1)]).reshape(64, M)
            lanew = np.zeros(64)
            for j in range(M):
                lanew = lanew + ws[:, j]
            cstart = np.concatenate([[0.0], np.cumsum(lanew)[:-1]])              # exclusive scan over the lanes
            c = cstart[:, None] + np.cumsum(ws, axis=1)                          # the lane's running sum
            c1 = c * inv
            c0 = np.concatenate([cstart[:, None] * inv, c1[:, :-1]], axis=1)
            h1, h0 = 2 * (1 + xi) * np.cos(2 * np.pi * xi * c1), 2 * (1 + xi) * np.cos(2 * np.pi * xi * c0)
            q = (h1 - h0) * ks
            Q = q.sum(axis=1)
            above = np.concatenate([np.cumsum(Q[::-1])[::-1][1:], [0.0]])        # reverse exclusive scan over the lanes
            suffix = np.cumsum(q[:, ::-1], axis=1)[:, ::-1] - q                  # the later ranks of the same lane
            Rr = (h1 * ks + above[:, None] + suffix).reshape(-1)[:D + 1]
            HC = ((h1 * c1 - h0 * c0) * ks).sum()
            Rel = np.empty(D + 1)
            Rel[order] = Rr                                                      # back to element order; the pad element is element D
            corr = (Rel[D] if m <= tau else 0.0) + (HC if m >= tau else 0.0)
            out[a:b, s] = G[r, s] * (Rel[:D] - corr) * inv
    return out


def sigma(S):
    s = np.arange(S)
    return np.where(s < BASE, 1.0, (-1.0) ** (s // BASE) * 2.0 ** ((s * 7) % 3 - 1))


def base_freqs():
    """The eight frequencies of weight_grad_ref.DIAG_FREQS (0, a negative one, small and large), then the spread of edge_weight_cases."""
    return np.concatenate([C.FREQS8, (np.arange(8, BASE) * 0.37) % 5.0 - 0.5]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def kernel_inputs(tau, tied):
    """A plain CSR with one recipient per entry of DEGREES and one sender per entry (col a permutation); BASE key columns as
    edge_weight_cases.kernel_inputs; weights of row_weights with the kind cycling over the rows; w_lo: a multiple of 2^-12 with
    |w_lo| <= 2^-6 on a few entries per row, w + w_lo >= 0 and exact in float64 -- on the rows of mass tau exactly in cancelling pairs
    (m stays tau), elsewhere nonnegative (at most 8 per row: the row stays on its side of tau); a float32 output gradient
    G [rows, 1 + BASE] (column 0: the mass column) with scattered zero readouts and one zero row."""
    rng = np.random.default_rng(5200 + int(tau) + 10 * tied)
    deg = np.array(DEGREES, dtype=np.int64)
    nnz = int(deg.sum())
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.permutation(nnz).astype(np.int64)
    if tied:
        K = C.grid_keys(rng, nnz, BASE)
    else:
        K = np.stack([(rng.permutation(nnz) - nnz // 2 + 0.5) / 1024.0 for _ in range(BASE)], axis=1).astype(np.float32)
        assert all(np.unique(K[:, s]).size == nnz for s in range(BASE)) and (K != 0).all()
    assert tuple(sorted(DEGREES)) == DEGREES
    ws, los, kinds = [], [], []
    for r, D in enumerate(deg):
        w, kind = np.zeros(0, dtype=np.float32), "lt"
        for kind in (("lt", "eq", "gt") * 2)[r % 3:r % 3 + 3] if D else ():
            w = C.row_weights(int(D), kind, tau, rng)
            if w is not None:
                break
        lo = np.zeros(w.size, dtype=np.float32)
        if D:
            step = (rng.integers(1, 65, size=8) * 2.0 ** -12).astype(np.float32)
            if kind == "eq":
                pos = np.nonzero(w > 0)[0]
                minus = pos[rng.permutation(pos.size)[:4]]
                plus = np.setdiff1d(np.arange(D), minus)
                plus = plus[rng.permutation(plus.size)[:minus.size]]
                lo[minus], lo[plus] = -step[:minus.size], step[:minus.size]
            else:
                lo[rng.permutation(int(D))[:8]] = step[:min(8, int(D))]
        ws.append(w)
        los.append(lo)
        kinds.append(kind)
    w, w_lo = np.concatenate(ws), np.concatenate(los)
    w64 = w.astype(np.float64) + w_lo.astype(np.float64)
    assert (w64 >= 0).all() and (np.abs(w_lo) <= 2.0 ** -6).all() and np.array_equal(w_lo * 4096, np.round(w_lo * 4096))
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        m, m64 = w[a:b].sum(dtype=np.float64), w64[a:b].sum()
        assert b == a or {"lt": m < tau and m64 < tau, "eq": m == tau and m64 == tau, "gt": m > tau and m64 > tau}[kinds[r]], (r, m, m64)
    G = rng.standard_normal((deg.size, 1 + BASE)).astype(np.float32)
    G[ZERO_ROW] = 0.0
    G[rng.integers(0, deg.size, size=12), 1 + rng.integers(0, BASE, size=12)] = 0.0
    res = {"degrees": deg, "rowptr": rowptr, "col": col, "K": K, "w": w, "w_lo": w_lo, "w64": w64, "G": G, "kinds": tuple(kinds)}
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def expand(k, S):
    """The S-slice problem of kernel_inputs k: (Xp [nnz, ldp] float32 with Xp[col, s] = K[:, s % BASE], freqs [S] float32,
    G [rows, 1 + S] float32)."""
    sel, sg = np.arange(S) % BASE, sigma(S)
    nnz = k["w"].size
    Xp = np.zeros((nnz, (S + 63) // 64 * 64), dtype=np.float32)
    Xp[k["col"], :S] = k["K"][:, sel]
    G = np.concatenate([k["G"][:, :1], (k["G"][:, 1 + sel] * sg[None, :]).astype(np.float32)], axis=1)
    return Xp, base_freqs()[sel], G


def rows_up_to(top):
    """(rows, entries) of the leading recipients of at most `top` neighbours (DEGREES ascends); None: all."""
    rows = len(DEGREES) if top is None else sum(d <= top for d in DEGREES)
    return rows, sum(DEGREES[:rows])


@functools.lru_cache(maxsize=None)
def base_reference(tau, tied, out_scale, lo=False, top=None):
    """weight_grad_ref.weight_grad_reference on the BASE slices of kernel_inputs(tau, tied), one call per slice, output gradient
    out_scale G, weights w or (lo) w + w_lo in float64, the recipients of at most `top` neighbours (None: all):
    gW_s [nnz, BASE], gkey [nnz, BASE], gfreq [BASE]."""
    k = kernel_inputs(tau, tied)
    rows, nnz = rows_up_to(top)
    rowptr = k["rowptr"][:rows + 1]
    K, fr = k["K"][:nnz].astype(np.float64), base_freqs().astype(np.float64)
    G = out_scale * k["G"][:rows, 1:].astype(np.float64)
    w = (k["w64"] if lo else k["w"].astype(np.float64))[:nnz]
    gws, gkey, gfreq = np.zeros(K.shape), np.zeros(K.shape), np.zeros(BASE)
    for s in range(BASE):
        res = R.weight_grad_reference(rowptr, None, w, K[:, s:s + 1], fr[s:s + 1], tau, G[:, s:s + 1], per_slice=False)
        gws[:, s], gkey[:, s], gfreq[s] = res["gW"], res["gkey"][:, 0], res["gfreq"][0]
    for a in (gws, gkey, gfreq):
        a.setflags(write=False)
    return {"gW_s": gws, "gkey": gkey, "gfreq": gfreq}


def reference(tau, tied, out_scale, S, lo=False, top=None):
    """The reference of the S-slice problem from base_reference (exact scaling by sigma): gW_s, gW, gkey, gfreq, and the
    coefficient scale of every (row, slice) line for the per-entry check of gkey."""
    from tests.test_hip_ties import coefficient_scale
    b = base_reference(tau, tied, out_scale, lo, top)
    k = kernel_inputs(tau, tied)
    sel, sg = np.arange(S) % BASE, sigma(S)
    gws = b["gW_s"][:, sel] * sg[None, :]
    G = out_scale * k["G"][:rows_up_to(top)[0], 1 + sel].astype(np.float64) * sg[None, :]
    return {"gW_s": gws, "gW": gws.sum(axis=1), "gkey": b["gkey"][:, sel] * sg[None, :], "gfreq": b["gfreq"][sel] * sg,
            "scale": coefficient_scale(G, base_freqs()[sel].astype(np.float64))}


def gw_bound(ref, rowptr, S, adds, fill=0.0):
    """Per entry: twice [G64_ROW of the row maximum + (adds + 2) 2^-24 sum_s |gW_s| + (S + 1) 2^-24 |fill|]; adds [nnz] or a number."""
    from tests.test_hip_ties import G64_ROW
    eps = 2.0 ** -24
    return 2.0 * (G64_ROW * R.row_maxima(ref["gW"], rowptr) + (S + 1) * eps * abs(fill) + (adds + 2) * eps * np.abs(ref["gW_s"]).sum(axis=1))
