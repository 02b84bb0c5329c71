"""Inputs of the edge-feature kernel tests (tests/test_hip_edge_features.py, tests/test_edge_features_cpu.py).  numpy only.

Exact keys.  The kernels form the key of CSR entry e in slice k as Xp[col[e], k] followed by fmaf(ef[e, q], Ve[k, q], key) for
q = 0 .. d_edge - 1, in float32.  Every operand here lies on a dyadic grid:
    Xp   multiples of 2^-6, |Xp| <= 512         (17 bits)
    ef   multiples of 1/4 in [-2, 2]            (products with Ve: multiples of 2^-5, |.| <= 2)
    Ve   multiples of 1/8 in [-1, 1]
    d_edge <= 5                                 (edge term: a multiple of 2^-5, |.| <= 10)
so every product and every partial sum is a multiple of 2^-6 below 2^10 -- 16 significant bits, exact in float32 in any order of
evaluation, with or without fma -- and the float64 oracle forms the same keys bit for bit.
"""
import os
import re

import numpy as np

LOW_MASS_ROWS = (31, 193, 2049)     # degrees of the rows scaled to total mass 0.4 (tests/test_hip_ties.py, 'random' weights)
XP_STEP = 2.0 ** -6
# key columns: e distinct keys (control), a one constant, b +0.0 / -0.0, c four values, d_up / d_down runs of three, cancel: the edge
# term cancels the difference between the two Xp of a pair (ties exist only on the sum), zero_ve: the slice's Ve row is all zero
KIND_CYCLE = ("e", "a", "b", "c", "d_up", "d_down", "cancel", "zero_ve", "e", "c", "cancel", "b")
# FREQS of tests/test_hip_ties.py + both zeros, -1 (the factor 1 + xi vanishes) and two more negative values
FREQ_CYCLE = (0.0, 0.37, 1.0, 1.5, 2.5, 4.0, 7.25, 13.0, -0.0, -1.0, -0.37, -2.5, 3.0)


def kinds(S):
    return tuple(KIND_CYCLE[c % len(KIND_CYCLE)] for c in range(S))


def freqs(S):
    return np.array([FREQ_CYCLE[c % len(FREQ_CYCLE)] for c in range(S)], dtype=np.float32)


def edge_list(degrees, d_edge, seed=41):
    """One recipient per entry of `degrees`, every sender exactly once, shuffled: (rec, snd, w, ef [E, d_edge]) in edge-list order.
    w: values {0.25, 0.5, 1}, 40 exact zeros (fewer on tiny graphs), the rows of LOW_MASS_ROWS neighbours scaled to total mass 0.4."""
    rng = np.random.default_rng(seed)
    nnz = int(sum(degrees))
    rec = np.repeat(np.arange(len(degrees)), degrees).astype(np.int64)
    snd = rng.permutation(nnz).astype(np.int64)
    w = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), size=nnz)
    w[rng.choice(nnz, size=min(40, nnz // 8), replace=False)] = 0.0
    for deg in LOW_MASS_ROWS:
        if deg in degrees:
            low = rec == degrees.index(deg)
            w[low] *= np.float32(0.4) / w[low].sum(dtype=np.float32)
    ef = (rng.integers(-8, 9, size=(nnz, d_edge)) / 4.0).astype(np.float32)
    order = rng.permutation(nnz)
    return rec[order], snd[order], w[order], ef[order]


def csr_order(rec, snd):
    """Edge-list positions in the order of the coalescing build: by (recipient, sender)."""
    return np.lexsort((snd, rec))


def slice_vectors(S, d_edge, seed=45):
    """Ve [S, d_edge]: multiples of 1/8 in [-1, 1], no all-zero row except in the 'zero_ve' columns."""
    rng = np.random.default_rng(seed)
    Ve = rng.integers(-8, 9, size=(S, d_edge)) / 8.0
    for k, kind in enumerate(kinds(S)):
        if kind == "zero_ve":
            Ve[k] = 0.0
        elif not Ve[k].any():
            Ve[k, k % d_edge] = 0.625
    return Ve.astype(np.float32)


def edge_term(ef, Ve):
    """[nnz, S] float64 <ef_e, Ve_k>: exact on the grids."""
    return ef.astype(np.float64) @ Ve.astype(np.float64).T


def xp_columns(rowptr, term, seed=42):
    """float32 Xp value of every CSR entry [nnz, S], column c of kind kinds(S)[c], on the 2^-6 grid with |Xp| <= 512."""
    rng = np.random.default_rng(seed)
    nnz, S = term.shape
    deg = np.diff(rowptr)
    pos = np.arange(nnz) - np.repeat(rowptr[:-1], deg)              # position of the entry in its row
    last = np.repeat(deg, deg) - 1 - pos
    K = np.empty((nnz, S), dtype=np.float64)
    for c, kind in enumerate(kinds(S)):
        if kind == "a":
            K[:, c] = 0.75
        elif kind == "b":
            K[:, c] = np.where(rng.random(nnz) < 0.5, 0.0, -0.0)
        elif kind == "c":
            K[:, c] = rng.choice(np.array([-1.0, -0.0, 0.0, 0.5]), size=nnz)
        elif kind == "d_up":
            K[:, c] = (pos // 3) * 2.0 ** -5 - 100.0
        elif kind == "d_down":
            K[:, c] = (last // 3) * 2.0 ** -5 - 100.0
        elif kind == "cancel":                                      # key = the pair's value; the two Xp differ by their edge terms
            K[:, c] = (pos // 2) * 2.0 ** -5 - 200.0 - term[:, c]
        else:                                                       # e, zero_ve: the KEY (Xp + edge term) is distinct inside every row
            key = np.empty(nnz)
            for a, b in zip(rowptr[:-1], rowptr[1:]):
                key[a:b] = (rng.choice(2 * 500 * 64 + 1, size=b - a, replace=False) - 500 * 64) * XP_STEP
            K[:, c] = key - term[:, c]
    assert np.abs(K).max() <= 512.0 and np.array_equal(K, np.round(K / XP_STEP) * XP_STEP)
    return K.astype(np.float32)


def keys_float32(xp, ef, Ve, reverse=False):
    """The kernels' evaluation in float32: key = Xp, then key += ef[q] * Ve[k, q] for q in forward (or reverse) order, every product
    and every sum rounded to float32 (a fused multiply-add rounds once instead of twice: no difference where nothing rounds)."""
    key = xp.astype(np.float32).copy()
    qs = range(ef.shape[1])
    for q in (reversed(qs) if reverse else qs):
        prod = (ef[:, q].astype(np.float32)[:, None] * Ve[:, q].astype(np.float32)[None, :]).astype(np.float32)
        key = (key + prod).astype(np.float32)
    return key


def header_constants():
    """The degree-bin constants of include/fsw_hip.h."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fsw_hip.h")
    text = open(path).read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    mid = tuple(int(x) for x in re.search(r"#define FSW_MID_SIZES \{([^}]*)\}", text).group(1).split(","))
    return {"reg": val("FSW_REG_MAX_DEG"), "mid": mid, "lds": val("FSW_NUM_LDS_BINS"), "hub": val("FSW_NUM_HUB_BINS"),
            "mid_max": val("FSW_MID_MAX_DEG"), "lds_max": val("FSW_LDS_MAX_DEG"), "hub_max": val("FSW_HUB_MAX_DEG")}


def bin_names():
    """Name of every degree bin, in the order of include/fsw_hip.h."""
    h = header_constants()
    return (["reg%d" % d for d in range(h["reg"] + 1)] + ["mid%d" % m for m in h["mid"]] + ["lds%d" % i for i in range(h["lds"])] +
            ["hub%d" % i for i in range(h["hub"])] + ["global"])


def bin_of(degree):
    """Index of the degree bin of a row of `degree` neighbours (include/fsw_hip.h)."""
    h = header_constants()
    uppers = (list(range(h["reg"] + 1)) + list(h["mid"]) + [(h["mid_max"] * 2) << i for i in range(h["lds"])] +
              [(h["lds_max"] * 2) << i for i in range(h["hub"])] + [1 << 62])
    assert uppers[h["reg"] + len(h["mid"])] == h["mid_max"] and uppers[-2] == h["hub_max"]
    return next(i for i, u in enumerate(uppers) if degree <= u)


def bin_rows(degrees):
    rows = [0] * len(bin_names())
    for d in degrees:
        rows[bin_of(d)] += 1
    return rows
