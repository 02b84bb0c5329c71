"""Inputs and the numpy restatement shared by tests/test_edge_weight_cpu.py and tests/test_hip_edge_weight.py.

rank_free_weight_grad: the form of d out / d w that csrc/embed_w_bwd.hip evaluates -- no sort, no successor key --
    h(c) = 2 (1 + xi) cos(2 pi xi c),  c1_u = cum_u / M,  c0_u = (cum_u - w_u) / M,  q_u = (h(c1_u) - h(c0_u)) key_u
    R(rank_u) = h(c1_u) key_u + sum_{v sorted after u} q_v,     sum_t H_t c_t = sum_u (h(c1_u) c1_u - h(c0_u) c0_u) key_u
    gw_j (slice s) = G[row, s] (R(rank_j) - [m <= tau] R(rank_pad) - [m >= tau] sum_t H_t c_t) / M
with the pad element (key 0, weight max(tau - m, 0)) as the row's last element and ties by element index.  The yardstick it is
measured against is tests/weight_grad_ref.py (autograd of the forward; none of these formulas).

The rows: weights from {0, 1/4, 1/2, 1}, one of three kinds of total mass per row -- below tau, tau exactly, above tau -- where the
row's length allows it (a row of D neighbours has m <= D).
"""
import functools

import numpy as np

from tests import weight_grad_ref as R

WEIGHT_SET = np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32)
FREQS8 = np.array(R.DIAG_FREQS, dtype=np.float32)


def rank_free_weight_grad(rowptr, w, K, freqs, tau, G):
    """gW_s [nnz, S] in float64: rowptr [rows + 1], w [nnz], per-entry keys K [nnz, S], freqs [S], G [rows, S] (module docstring)."""
    w, K, fr, G = (np.asarray(a, dtype=np.float64) for a in (w, K, freqs, G))
    S = K.shape[1]
    out = np.zeros((w.size, S))
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        D = b - a
        if D == 0:
            continue
        m = w[a:b].sum()
        M = max(m, tau)
        wgt = np.concatenate([w[a:b], [max(tau - m, 0.0)]])
        idx = np.arange(D + 1)
        for s in range(S):
            xi = fr[s]
            key = np.concatenate([K[a:b, s], [0.0]])
            before = (key[:, None] < key[None, :]) | ((key[:, None] == key[None, :]) & (idx[:, None] < idx[None, :]))   # [v, u]: v sorts ahead of u
            cum = wgt + wgt @ before
            c1, c0 = cum / M, (cum - wgt) / M
            h1, h0 = 2 * (1 + xi) * np.cos(2 * np.pi * xi * c1), 2 * (1 + xi) * np.cos(2 * np.pi * xi * c0)
            q = (h1 - h0) * key
            Rr = h1 * key + before @ q
            HC = ((h1 * c1 - h0 * c0) * key).sum()
            corr = (Rr[D] if m <= tau else 0.0) + (HC if m >= tau else 0.0)
            out[a:b, s] = G[r, s] * (Rr[:D] - corr) / M
    return out


def row_weights(D, kind, tau, rng):
    """float32 weights of a row of D neighbours from WEIGHT_SET with total mass below tau ('lt'), tau exactly ('eq') or above ('gt');
    None when no such row exists (m <= D)."""
    tau = int(tau)
    if kind == "eq":
        if D < tau:
            return None
        w = np.zeros(D, dtype=np.float32)
        if D >= tau + 1:
            w[:tau - 1], w[tau - 1:tau + 1] = 1.0, 0.5
            if D >= tau + 3:                         # ... 1/2 = 1/4 + 1/4 and an exact zero
                w[tau], w[tau + 1:tau + 3] = 0.0, 0.25
        else:
            w[:] = 1.0
        assert float(w.sum(dtype=np.float64)) == tau
        return w[rng.permutation(D)]
    for _ in range(64):
        w = WEIGHT_SET[rng.integers(0, 4, size=D)] if kind == "lt" else WEIGHT_SET[rng.integers(1, 4, size=D)]
        if kind == "lt" and D > 2 * tau:
            w[rng.permutation(D)[2 * tau:]] = 0.0           # long rows: at most 2 tau nonzero weights
            w[rng.integers(0, D)] = 0.25
        m = float(w.sum(dtype=np.float64))
        if (kind == "lt" and 0 < m < tau) or (kind == "gt" and m > tau):
            return w
    return None


def grid_keys(rng, nnz, S):
    """Keys on the grid of 1/8 in [-1, 1], the pad key 0 included: many ties inside every row and with the pad element."""
    return (rng.integers(-8, 9, size=(nnz, S)) / 8.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cpu_rows(tau, nopad=False):
    """Rows of every degree 1 .. 32, the three kinds each where they exist (nopad: only 'eq' and 'gt', no row below tau), S = 8,
    grid keys, G standard normal: dict(rowptr, w, K, G, kinds)."""
    rng = np.random.default_rng(4100 + int(tau) + 10 * nopad)
    ws, kinds = [], []
    for D in range(1, 33):
        for kind in ("eq", "gt") if nopad else ("lt", "eq", "gt"):
            w = row_weights(D, kind, tau, rng)
            if w is not None:
                ws.append(w)
                kinds.append(kind)
    deg = np.array([w.size for w in ws], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    w = np.concatenate(ws)
    res = {"rowptr": rowptr, "w": w, "K": grid_keys(rng, w.size, 8), "G": rng.standard_normal((deg.size, 8)), "kinds": tuple(kinds)}
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


# ---- kernel-level inputs of tests/test_hip_edge_weight.py ------------------------------------------------------------------------------
KERNEL_DEGREES = tuple(range(0, 41)) + (300,) + (5,) * 70     # both sides of the register class and of the degree bins; the generic
                                                              # hand-over (LDS line); three 32-row tiles of one bin, the last partial
ZERO_ROW = 12                                                 # the recipient (12 neighbours) whose output gradient is zero
# The slices repeat with period BASE: slice s has the keys and the frequency of slice s % BASE and sigma(s) times its output
# gradient, sigma a signed power of two.  Scaling by a power of two is exact, so every reference quantity of slice s is sigma(s)
# times that of slice s % BASE, bit for bit, and the reference (a Python loop over rows and slices: 70 ms per slice) is computed
# for BASE slices once per (tau, keys) and serves S = 8, 70 and 260.  BASE is odd: slices k and k +- 64 (the same lane of another
# chunk) differ in keys, frequency and gradient.
BASE = 33


def sigma(S):
    s = np.arange(S)
    return np.where(s < BASE, 1.0, (-1.0) ** (s // BASE) * 2.0 ** ((s * 7) % 3 - 1))


def base_freqs():
    """The eight frequencies of weight_grad_ref.DIAG_FREQS (0, a negative one, small and large), then a spread over [-0.5, 4.5)."""
    return np.concatenate([FREQS8, (np.arange(8, BASE) * 0.37) % 5.0 - 0.5]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def kernel_inputs(tau, tied):
    """A plain CSR with one recipient per entry of KERNEL_DEGREES and one sender per entry (col a permutation); BASE key columns,
    exact in float32, distinct over the whole array and of both signs, K[:, s] = (permutation - nnz // 2 + 1/2) / 1024
    (weight_grad_ref.kernel_inputs), or `tied` on the grid of 1/8 with the pad key; weights of row_weights with the kind cycling
    over the rows; a float32 output gradient G [rows, 1 + BASE] (column 0: the mass column) with zero readouts and one zero row."""
    rng = np.random.default_rng(4200 + int(tau) + 10 * tied)
    deg = np.array(KERNEL_DEGREES, dtype=np.int64)
    nnz = int(deg.sum())
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.permutation(nnz).astype(np.int64)
    if tied:
        K = grid_keys(rng, nnz, BASE)
    else:
        K = np.stack([(rng.permutation(nnz) - nnz // 2 + 0.5) / 1024.0 for _ in range(BASE)], axis=1).astype(np.float32)
        assert all(np.unique(K[:, s]).size == nnz for s in range(BASE)) and (K != 0).all()
    ws, kinds = [], []
    for r, D in enumerate(deg):
        w = None
        for kind in (("lt", "eq", "gt") * 2)[r % 3:r % 3 + 3]:
            w = row_weights(int(D), kind, tau, rng) if D else np.zeros(0, dtype=np.float32)
            if w is not None:
                break
        ws.append(w)
        kinds.append(kind if D else "lt")
    G = rng.standard_normal((deg.size, 1 + BASE)).astype(np.float32)
    G[ZERO_ROW] = 0.0
    G[rng.integers(0, deg.size, size=40), 1 + rng.integers(0, BASE, size=40)] = 0.0
    G[5, 1:9] = 0.0                                               # all of S = 8 but the mass column
    res = {"degrees": deg, "rowptr": rowptr, "col": col, "K": K, "w": np.concatenate(ws), "G": G, "kinds": tuple(kinds)}
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


@functools.lru_cache(maxsize=None)
def base_reference(tau, tied, out_scale):
    """weight_grad_ref.weight_grad_reference on the BASE slices of kernel_inputs(tau, tied), one call per slice (the slices are
    independent; this keeps autograd's graph small), output gradient out_scale G: gW_s [nnz, BASE], gkey [nnz, BASE], gfreq [BASE]."""
    k = kernel_inputs(tau, tied)
    K, fr = k["K"].astype(np.float64), base_freqs().astype(np.float64)
    G = out_scale * k["G"][:, 1:].astype(np.float64)
    gws, gkey, gfreq = np.zeros(K.shape), np.zeros(K.shape), np.zeros(BASE)
    for s in range(BASE):
        res = R.weight_grad_reference(k["rowptr"], None, k["w"], K[:, s:s + 1], fr[s:s + 1], tau, G[:, s:s + 1], per_slice=False)
        gws[:, s], gkey[:, s], gfreq[s] = res["gW"], res["gkey"][:, 0], res["gfreq"][0]
    for a in (gws, gkey, gfreq):
        a.setflags(write=False)
    return {"gW_s": gws, "gkey": gkey, "gfreq": gfreq}


def reference(tau, tied, out_scale, S):
    """The reference of the S-slice problem from base_reference (exact scaling by sigma): gW_s, gW, gkey, gfreq, and the
    coefficient scale of every (row, slice) line for the per-entry check of gkey."""
    from tests.test_hip_ties import coefficient_scale
    b = base_reference(tau, tied, out_scale)
    k = kernel_inputs(tau, tied)
    sel, sg = np.arange(S) % BASE, sigma(S)
    gws = b["gW_s"][:, sel] * sg[None, :]
    G = out_scale * k["G"][:, 1 + sel].astype(np.float64) * sg[None, :]
    return {"gW_s": gws, "gW": gws.sum(axis=1), "gkey": b["gkey"][:, sel] * sg[None, :], "gfreq": b["gfreq"][sel] * sg,
            "scale": coefficient_scale(G, base_freqs()[sel].astype(np.float64))}
