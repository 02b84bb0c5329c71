"""Inputs and the numpy restatement shared by tests/test_edge_weight_hub_cpu.py and tests/test_hip_edge_weight_hub.py: the weight
gradient of rows above 1024 neighbours (csrc/embed_w_long_bwd.hip).

chunked_weight_grad: the chunked total-minus-prefix form that kernel evaluates.  A (row, slice) line of D + 1 elements -- the pad
element (key 0, weight max(tau - m, 0)) is element D -- is sorted by key with ties by element index and walked in chunks of 64 M
ranks, lane l of a chunk owning M consecutive ranks (fillers of weight 0 whose key counts as 0 behind the line).  With
h(c) = 2 (1 + xi) cos(2 pi xi c), c1_t = cum_t / M_row, c0_t = c1_{t-1} (cum: the lane's running sum on top of the exclusive scan of
the chunk's lanes on top of the carry of the chunks before),
    q_t     = (h(c1_t) - h(c0_t)) key_t                       h(c0) of a lane's first rank: h of the lane's starting cumulative weight
    P_t     = (sum of q over the chunks before) + (exclusive scan of the lanes' sums of q) + (in-lane prefix up to and including t)
    e_t     = h(c1_t) key_t - P_t,     Qtot = P of the last rank,     HC = sum_t (h(c1_t) c1_t - h(c0_t) c0_t) key_t
    K'      = -e_pad  (m < tau)   |   -e_pad - HC  (m == tau)   |   Qtot - HC  (m > tau)
    gw_j(s) = gd_s (e_rank(j) + K'_s),    gd_s = G[row, s] / M_row,    M_row = max(m, tau)
and over a group of G consecutive slices acc[j] = sum_s gd_s e_rank(j), Ksum = sum_s gd_s K'_s in float64; the group's value
acc[j] + Ksum is what the kernel adds to gw in float32 (grouped=True returns these [nnz, ceil(S / G)] values).
The yardstick it is measured against is tests/weight_grad_ref.py (autograd of the forward; none of these formulas).

The rows: one recipient per degree of DEGREES -- both sides of the hand-over from the wave-sort class (1024 | 1025), D + 1 crossing
one chunk of 1024 or 2048 words, two chunks and every power of two up to 32768 (every merge level), both sides of every bin edge
(2048, 4096, 8192, 16384, 32768: the row of 32769 is the first of FSW_BIN_GLOBAL), and 6001, whose last chunk is partly filled.
Everything else as in tests/edge_weight_long_cases.py: weights of edge_weight_cases.row_weights with the kind (mass below tau / tau
exactly / above tau) cycling over the rows, keys exact in float32, distinct or tied on the grid of 1/8 with the pad key, BASE = 9
slices expanded to S by signed powers of two, w_lo multiples of 2^-12.
"""
import functools

import numpy as np

from tests import edge_weight_cases as C
from tests import edge_weight_long_cases as LC
from tests import weight_grad_ref as R

DEGREES = (0, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6001, 8192, 8193, 16384, 16385, 32768, 32769)
ZERO_ROW = DEGREES.index(4096)                                # the long recipient whose output gradient is zero
TUNED_MAX = LC.TUNED_MAX                                      # csrc/embed_launch.h: kWSortMaxDeg
RANKS = 16                                                    # csrc/embed_launch.h: kWLongRanks (chunks of 64 * 16 words)
BYTES_PER_ELEM = 20                                           # csrc/embed_w_long_bwd.hip: packed word, accumulator, key gradient
BASE = LC.BASE
S_VALUES = (3, 8, 70)
sigma, base_freqs, expand, gw_bound = LC.sigma, LC.base_freqs, LC.expand, LC.gw_bound


def pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def slices_per_task():
    """G of the library (fsw_embed_backward_w_long_slices)."""
    from fsw_gnn_amd import _lib
    return int(_lib.lib().fsw_embed_backward_w_long_slices())


def float32_adds(D, S, G=None):
    """Float32 atomic adds an entry of a row of D neighbours receives: above the wave-sort class one per task, ceil(S / G)."""
    if D <= TUNED_MAX:
        return LC.float32_adds(D, S)
    return -(-S // (slices_per_task() if G is None else G))


def chunked_weight_grad(rowptr, w, K, freqs, tau, Gout, M=RANKS, group=None):
    """gW_s [nnz, S] in float64 by the form of the module docstring: rowptr [rows + 1], w [nnz] float64, per-entry keys K [nnz, S],
    freqs [S], Gout [rows, S] (out_scale included).  Rows of at most TUNED_MAX neighbours are left at zero.  group = G: the
    float64 values acc[j] + Ksum of every task instead, [nnz, ceil(S / G)]."""
    w, K, fr, Gout = (np.asarray(a, dtype=np.float64) for a in (w, K, freqs, Gout))
    S = K.shape[1]
    CAP = 64 * M
    ntask = -(-S // group) if group else 0
    out = np.zeros((w.size, ntask if group else S))
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        D = int(b - a)
        if D <= TUNED_MAX:
            continue
        m = w[a:b].sum()
        inv = 1.0 / max(m, tau)
        nchunk = -(-(D + 1) // CAP)
        fill = np.zeros(nchunk * CAP - D - 1)
        wgt = np.concatenate([w[a:b], [max(tau - m, 0.0)]])
        idx = np.arange(D + 1)
        acc, Ksum = np.zeros(D), 0.0
        for s in range(S):
            xi = fr[s]
            h = lambda c: 2 * (1 + xi) * np.cos(2 * np.pi * xi * c)      # noqa: E731
            gd = Gout[r, s] * inv
            key = np.concatenate([K[a:b, s], [0.0]])
            order = np.lexsort((idx, key))                               # by key, ties by element index
            ks = np.concatenate([key[order], fill]).reshape(nchunk, 64, M)
            ws = np.concatenate([wgt[order], fill]).reshape(nchunk, 64, M)
            e = np.zeros((nchunk, 64, M))
            carry = Pcarry = HC = 0.0
            for ch in range(nchunk):                                     # the walk of the last merge level
                lanew = ws[ch].sum(axis=1)
                cstart = carry + np.concatenate([[0.0], np.cumsum(lanew)[:-1]])
                carry = carry + lanew.sum()
                c1 = (cstart[:, None] + np.cumsum(ws[ch], axis=1)) * inv
                c0 = np.concatenate([cstart[:, None] * inv, c1[:, :-1]], axis=1)
                h1, h0 = h(c1), h(c0)
                q = (h1 - h0) * ks[ch]
                Q = q.sum(axis=1)
                Pbase = Pcarry + np.concatenate([[0.0], np.cumsum(Q)[:-1]])
                Pcarry = Pcarry + Q.sum()
                e[ch] = (h1 * ks[ch] - np.cumsum(q, axis=1)) - Pbase[:, None]
                HC = HC + ((h1 * c1 - h0 * c0) * ks[ch]).sum()
            eel = np.empty(D + 1)
            eel[order] = e.reshape(-1)[:D + 1]                           # back to element order; the pad element is element D
            Kc = -eel[D] if m < tau else (-eel[D] - HC if m == tau else Pcarry - HC)
            if not group:
                out[a:b, s] = gd * (eel[:D] + Kc)
                continue
            if Gout[r, s] != 0:                                          # a zero line adds nothing
                acc, Ksum = acc + gd * eel[:D], Ksum + gd * Kc
            if s % group == group - 1 or s == S - 1:
                out[a:b, s // group] = acc + Ksum
                acc, Ksum = np.zeros(D), 0.0
    return out


@functools.lru_cache(maxsize=None)
def kernel_inputs(tau, tied):
    """edge_weight_long_cases.kernel_inputs on DEGREES: a plain CSR with one recipient per degree and one sender per entry (col a
    permutation); BASE key columns exact in float32, distinct over the whole array and of both signs, or `tied` on the grid of 1/8
    with the pad key; weights of row_weights with the kind cycling over the rows; w_lo: a multiple of 2^-12 with |w_lo| <= 2^-6,
    w + w_lo >= 0 and exact in float64 -- on the rows of mass tau exactly in cancelling pairs (m stays tau), on the rows below tau on
    8 entries (the row stays below), on the rows above tau on D / 8 entries; a float32 output gradient G [rows, 1 + BASE] (column 0:
    the mass column) with scattered zero readouts and one zero row."""
    rng = np.random.default_rng(6200 + int(tau) + 10 * tied)
    deg = np.array(DEGREES, dtype=np.int64)
    nnz = int(deg.sum())
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.permutation(nnz).astype(np.int64)
    if tied:
        K = C.grid_keys(rng, nnz, BASE)
    else:
        K = np.stack([(rng.permutation(nnz) - nnz // 2 + 0.5) / 1024.0 for _ in range(BASE)], axis=1).astype(np.float32)
        assert all(np.unique(K[:, s]).size == nnz for s in range(BASE)) and (K != 0).all()
    ws, los, kinds = [], [], []
    for r, D in enumerate(deg):
        D = int(D)
        w, kind = np.zeros(0, dtype=np.float32), "lt"
        for kind in (("lt", "eq", "gt") * 2)[r % 3:r % 3 + 3] if D else ():
            w = C.row_weights(D, kind, tau, rng)
            if w is not None:
                break
        lo = np.zeros(w.size, dtype=np.float32)
        if D:
            if kind == "eq":
                pos = np.nonzero(w > 0)[0]
                minus = pos[rng.permutation(pos.size)[:4]]
                plus = np.setdiff1d(np.arange(D), minus)
                plus = plus[rng.permutation(plus.size)[:minus.size]]
                step = (rng.integers(1, 65, size=minus.size) * 2.0 ** -12).astype(np.float32)
                lo[minus], lo[plus] = -step, step
            else:
                n = 8 if kind == "lt" else max(8, D // 8)
                lo[rng.permutation(D)[:n]] = (rng.integers(1, 65, size=n) * 2.0 ** -12).astype(np.float32)
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


@functools.lru_cache(maxsize=None)
def base_reference(tau, tied, out_scale, lo=False):
    """weight_grad_ref.weight_grad_reference on the BASE slices of kernel_inputs(tau, tied), one call per slice, output gradient
    out_scale G, weights w or (lo) w + w_lo in float64: gW_s [nnz, BASE], gkey [nnz, BASE], gfreq [BASE]."""
    k = kernel_inputs(tau, tied)
    K, fr = k["K"].astype(np.float64), base_freqs().astype(np.float64)
    G = out_scale * k["G"][:, 1:].astype(np.float64)
    w = k["w64"] if lo else k["w"].astype(np.float64)
    gws, gkey, gfreq = np.zeros(K.shape), np.zeros(K.shape), np.zeros(BASE)
    for s in range(BASE):
        res = R.weight_grad_reference(k["rowptr"], None, w, K[:, s:s + 1], fr[s:s + 1], tau, G[:, s:s + 1], per_slice=False)
        gws[:, s], gkey[:, s], gfreq[s] = res["gW"], res["gkey"][:, 0], res["gfreq"][0]
    for a in (gws, gkey, gfreq):
        a.setflags(write=False)
    return {"gW_s": gws, "gkey": gkey, "gfreq": gfreq}


def reference(tau, tied, out_scale, S, lo=False):
    """The reference of the S-slice problem from base_reference (exact scaling by sigma): gW_s, gW, gkey, gfreq, and the
    coefficient scale of every (row, slice) line for the per-entry check of gkey."""
    from tests.test_hip_ties import coefficient_scale
    b = base_reference(tau, tied, out_scale, lo)
    k = kernel_inputs(tau, tied)
    sel, sg = np.arange(S) % BASE, sigma(S)
    gws = b["gW_s"][:, sel] * sg[None, :]
    G = out_scale * k["G"][:, 1 + sel].astype(np.float64) * sg[None, :]
    return {"gW_s": gws, "gW": gws.sum(axis=1), "gkey": b["gkey"][:, sel] * sg[None, :], "gfreq": b["gfreq"][sel] * sg,
            "scale": coefficient_scale(G, base_freqs()[sel].astype(np.float64))}
