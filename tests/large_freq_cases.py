"""Inputs and long-double references of the large-frequency tests (tests/test_hip_large_freqs.py, tests/test_large_freq_cases_cpu.py).
numpy only.

Frequencies.  'spread' gives xi up to 2 nFreqs - 1, 'random' draws u / (1 - u): the shipped layers carry frequencies far above the
|xi| <= 13 of the tie and edge-feature suites.  One column per frequency, every value a float32 (0.37 is rounded to float32 once,
here, and both sides get that number):
    0.37, 13             controls: the regime of the older suites
    127, 511, 2047       the tops of 'spread' at S = 64, 256, 1024
    -1500                a negative frequency of that size
    1e4                  the tail of 'random'
    1024, 2048, 4096     with the unit-weight rows of 2048 and 4096 neighbours: xi / D in {1/2, 1, 2} and 1/4 -- the per-rank rotation
                         of the unit kernels' recurrence has 2 cos = +-2, every coefficient vanishes analytically (sin(pi xi / D) = 0),
                         and xi / D >= 1/2 lies at and above the per-rank Nyquist rate
Keys.  Distinct inside every row, multiples of 2^-7 in [-512, -256] and [128, 512] (17 bits: exact in float32, and never equal to the
pad element's key 0, so no order among equal keys enters); Ladder.key_columns says how they are placed.
Degree ladders.  One recipient per degree, every sender exactly once (tests/test_hip_ties.py).  LADDERS splits the degrees of
tests/test_hip_ties.py plus the hub and giant edges 16384, 16385, 32768, 32769 over three graphs so that one case stays at a few
seconds; each starts with an empty row.
Weight modes (name, tau):
    unit      tau = 1            unit weights, no pad element: the coefficient-table and recurrence kernels
    unit      tau = 3.3          unit weights through the general kernels; rows of 1 .. 3 neighbours have a non-integer pad weight
    deficient tau = 1            arbitrary float32 weights, every row scaled 'gcn'-like to a total mass in (0.3, 0.9): every row is padded
    full      tau = 1            arbitrary float32 weights with mass >= tau and a few exact zeros: no pad weight, the control that
                                 separates the pad element from everything else
tau is a double in the argument blocks of the Cartesian and generic entry points and a float32 in fsw_embed_args: there the kernels
see TAU_B_F32 = float32(3.3), and so does their reference.  (float32(3.3) - D is exact in float32 for D = 1, 2, 3, so that entry's
unit rows never had a pad weight to round; 3.3 - D in double has.)
"""
import functools

import numpy as np

FREQS = tuple(float(np.float32(x)) for x in (0.37, 13.0, 127.0, 511.0, 2047.0, -1500.0, 1e4, 1024.0, 2048.0, 4096.0))
CONTROL_FREQS = FREQS[:2]
TIES_DEGREES = (0, 1, 2, 3, 16, 17, 31, 32, 33, 40, 41, 64, 65, 128, 129, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025,
                2047, 2048, 2049, 4096, 4097, 9000)          # DEGREES of tests/test_hip_ties.py
TAU_B = 3.3
TAU_B_F32 = float(np.float32(3.3))
MODES = (("unit", 1.0), ("unit", TAU_B), ("deficient", 1.0), ("full", 1.0))
KEY_STEP = 2.0 ** -7


class Ladder:
    """One graph: a recipient per entry of `degrees`, every sender exactly once, in shuffled edge-list order."""

    def __init__(self, name, degrees, seed):
        self.name, self.degrees, self.seed = name, tuple(degrees), seed
        self.nnz = int(sum(degrees))

    def __repr__(self):
        return "ladder_%s" % self.name

    def edge_list(self, weights):
        """(recipients, senders, float32 weights or None)."""
        rng = np.random.default_rng(self.seed)
        deg, nnz = self.degrees, self.nnz
        rec = np.repeat(np.arange(len(deg)), deg).astype(np.int64)
        snd = rng.permutation(nnz).astype(np.int64)
        order = rng.permutation(nnz)
        w = None
        if weights != "unit":
            w = rng.uniform(0.05, 1.0, size=nnz).astype(np.float32)
            start = np.concatenate([[0], np.cumsum(deg)])
            for r, (a, b) in enumerate(zip(start[:-1], start[1:])):
                if b == a:
                    continue
                if weights == "deficient":                     # 'gcn'-like: the whole row times one factor, total mass in (0.3, 0.9)
                    target = rng.uniform(0.3, 0.9)
                    w[a:b] = (w[a:b].astype(np.float64) * (target / w[a:b].sum(dtype=np.float64))).astype(np.float32)
                elif weights == "full":                        # mass >= tau = 1 with room for float32 rounding; exact zeros in the longer rows
                    if b - a >= 16:
                        w[a + rng.choice(b - a, size=3, replace=False)] = 0.0
                    m = w[a:b].sum(dtype=np.float64)
                    if m < 1.25:
                        w[a:b] = (w[a:b].astype(np.float64) * (rng.uniform(1.25, 2.5) / m)).astype(np.float32)
                else:
                    raise ValueError(weights)
        return rec[order], snd[order], None if w is None else w[order]

    def key_columns(self, weights, tau, ncols=None, freqs=None):
        """float32 keys [nnz, ncols] per CSR entry of the ladder under (weights, tau): distinct inside every (row, column) line,
        non-zero, on the 2^-7 grid, and fit for every frequency of `freqs` in every column (Cartesian mode pairs each column with all).
        A line's output is sum_t F(c_t) (k_(t) - k_(t+1)), F(c) = (1 + xi) sin(2 pi xi c) / (pi xi): under keys spread evenly it is
        the Fourier coefficient of a smooth quantile function and cancels to 1e-3 of the line's scale and less, so that a relative
        error per (row, column) would measure the cancellation, not the kernel.  Here the first n entries of a row lie in
        [-512, -256], the others in [128, 512] and the pad element (key 0) between them: the quantile function jumps at the cumulative
        weight c_n of those n entries by at least 256 and 128, and n (one per row, between 0.2 D and 0.55 D; any n in rows of up to
        64, with a key on either side of the pad element from 2 neighbours on) is the value whose smallest jump term |256 sin(2 pi xi c_n) + 128 sin(2 pi xi (c_n + pad))| over the frequencies is
        largest.  Frequencies whose term vanishes for every n (unit weights with xi / D a multiple of 1/2: the line's coefficients
        all vanish) do not take part."""
        rowptr, _col, w, _w32 = csr(self, weights)
        return place_keys(rowptr, w, tau, len(FREQS if freqs is None else freqs) if ncols is None else ncols,
                          FREQS if freqs is None else freqs, np.random.default_rng(self.seed + 1))


def place_keys(rowptr, w, tau, ncols, freqs, rng):
    """The keys of Ladder.key_columns for any CSR: w [nnz] float64 weights in CSR order."""
    freqs = np.array(freqs)
    K = np.empty((int(rowptr[-1]), ncols), dtype=np.float32)
    for a, b in zip(rowptr[:-1], rowptr[1:]):
        D = int(b - a)
        if D == 0:
            continue
        m = w[a:b].sum()
        denom, pad = max(m, tau), max(tau - m, 0.0) / max(m, tau)
        cw = np.concatenate([[0.0], np.cumsum(w[a:b])]) / denom           # cw[n]: cumulative weight of the first n entries
        cand = np.arange(min(1, D - 1), D) if D <= 64 else np.arange(int(0.2 * D), int(0.55 * D) + 1)
        ph = 2 * np.pi * freqs[None, :] * cw[cand][:, None]
        jump = np.abs(256 * np.sin(ph) + 128 * np.sin(ph + 2 * np.pi * freqs[None, :] * pad))     # [candidates, frequencies]
        live = jump.max(axis=0) > 1e-6
        n = int(cand[jump[:, live].min(axis=1).argmax()]) if live.any() else D // 2
        for c in range(ncols):
            lo = -512 + rng.choice(256 * 128 + 1, size=D, replace=False) * KEY_STEP
            hi = 128 + rng.choice(384 * 128 + 1, size=D, replace=False) * KEY_STEP
            K[a:b, c] = np.where(np.arange(D) < n, lo, hi)
    return K


LADDERS = (Ladder("ties", TIES_DEGREES, 141), Ladder("hub", (0, 16384, 16385), 151), Ladder("giant", (0, 32768, 32769), 161))


@functools.lru_cache(maxsize=None)
def csr(ladder, weights):
    """(rowptr, col, float64 w in CSR order, float32 w or None): rows keep the order of the shuffled edge list (a stable sort by
    recipient -- the order of fsw_gnn_amd.build_csr)."""
    rec, snd, w = ladder.edge_list(weights)
    order = np.argsort(rec, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rec, minlength=len(ladder.degrees)))]).astype(np.int64)
    w32 = None if w is None else w[order]
    return rowptr, snd[order], (np.ones(ladder.nnz) if w is None else w32.astype(np.float64)), w32


@functools.lru_cache(maxsize=None)
def cached_keys(ladder, weights, tau):
    K = ladder.key_columns(weights, tau)
    K.setflags(write=False)
    return K


# ---- long-double restatement ----------------------------------------------------------------------------------------------------------
LD = np.longdouble
PI_LD = LD(4) * np.arctan(LD(1))


def _cospi_ld(u):
    """cos(pi u) for long-double u of any size: u is reduced modulo 2 exactly first."""
    return np.cos(PI_LD * (u - LD(2) * np.rint(u / LD(2))))


def _sinc_ld(z):
    """sin(pi z) / (pi z), z reduced modulo 2 exactly for the sine."""
    zr = z - LD(2) * np.rint(z / LD(2))
    safe = np.where(z == 0, LD(1), z)
    return np.where(z == 0, LD(1), np.sin(PI_LD * zr) / (PI_LD * safe))


def coefficients(keys, w, tau, xi, pad_weight=None, dtype=LD):
    """One row: the coefficients (1 + xi) Delta_t of every neighbour [D, S] in entry order (so out[k] = sum_t coef[t, k] key[t, k],
    gkey[t, k] = g[k] coef[t, k]) in `dtype` arithmetic.  keys [D, S], w [D], xi [S]; the pad element (key 0, weight max(tau - m, 0))
    is the row's last entry, as in oracle/fsw_oracle.py.  pad_weight: a function applied to the pad weight before it enters the
    cumulative sum (the float32 rounding of the kernels, for the demonstration in tests/test_large_freq_cases_cpu.py); the
    denominator max(m, tau) is not affected."""
    D, S = keys.shape
    w = np.asarray(w, dtype=dtype)
    m = w.sum()
    tau = dtype(tau)
    pad = max(tau - m, dtype(0))
    denom = max(m, tau)
    if pad_weight is not None:
        pad = dtype(pad_weight(pad))
    wts = np.concatenate([w, [pad]]) / denom
    kp = np.concatenate([np.asarray(keys, dtype=np.float64), np.zeros((1, S))], axis=0)
    order = np.argsort(kp, axis=0, kind="stable")
    ws = wts[order]                                               # [D + 1, S]
    c = np.cumsum(ws, axis=0)
    x = np.asarray(xi, dtype=dtype)[None, :]
    if dtype is LD:
        delta = 2 * ws * _sinc_ld(x * ws) * _cospi_ld(x * (2 * c - ws))
    else:
        delta = 2 * ws * np.sinc(x * ws) * np.cos(np.pi * x * (2 * c - ws))
    coef = np.empty_like(delta)
    np.put_along_axis(coef, order, (1 + x) * delta, axis=0)
    return coef[:D]


def reference(ladder, weights, tau, freqs=FREQS, pad_weight=None, dtype=LD, cols=None):
    """(out [rows, S], coef [nnz, S]) of the ladder in `dtype` arithmetic; key column cols[k] (default k) at frequency freqs[k]."""
    rowptr, _col, w, _w32 = csr(ladder, weights)
    K = cached_keys(ladder, weights, tau)[:, list(range(len(freqs)) if cols is None else cols)]
    out = np.zeros((len(ladder.degrees), len(freqs)), dtype=dtype)
    coef = np.zeros((ladder.nnz, len(freqs)), dtype=dtype)
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        if b > a:
            coef[a:b] = coefficients(K[a:b], w[a:b], tau, freqs, pad_weight, dtype)
            out[r] = (coef[a:b] * K[a:b].astype(dtype)).sum(axis=0)
    return out, coef


def forward_scale(keys, rowptr, freqs):
    """[rows, S]: the size a line's output has when its coefficients do not cancel, max|key| times the size of the two values
    F(xi; c) = (1 + xi) sin(2 pi xi c) / (pi xi) whose difference a coefficient is (tests/test_hip_ties.py: coefficient_scale)."""
    xi = np.asarray(freqs, dtype=np.float64)
    f = np.abs(1 + xi) * np.minimum(2.0, 1.0 / (np.pi * np.maximum(np.abs(xi), 1e-300)))
    kmax = np.array([np.abs(keys[a:b]).max(axis=0) if b > a else np.zeros(keys.shape[1]) for a, b in zip(rowptr[:-1], rowptr[1:])])
    return kmax * f[None, :]
