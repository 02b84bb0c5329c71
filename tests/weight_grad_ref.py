"""A plain float64 restatement of the embedding's forward, differentiated by torch.autograd: the yardstick for d loss / d W.

No GPU, no kernel formula: the closed form of csrc/embed_generic.hip (H_t, the reverse cumulative sums R, the two clamp indicators)
appears nowhere here.  The forward is written as the reference states it and autograd does the rest:

  per row:   a = the row's weights, m = sum a; with padding on, the pad element (key 0, the row's last element) gets
             clamp(tau - m, min=0) and every weight is divided by clamp(m, min=tau); with padding off, a / m
  per slice: order = np.lexsort((element index, key)), w = weights in that order, c = cumsum(w), p = keys in that order
             Delta = 2 w sinc(xi w) cos(pi xi (2 c - w)),   out = (1 + xi) sum Delta p
  diagonal:  slice s at freqs[s] -> column s;   Cartesian: slice s at every freqs[f] -> column s F + f
  mass:      f(m) scale with f = identity / sqrt / log, methods plain / homog / homog_alt as oracle.fsw_oracle.total_mass_encode

The pad rule is the reference's global one (`if (W_pad > 0).any()`): rows are padded only if SOME row, empty recipients included,
has m < tau.  torch.clamp passes the gradient at the bound itself, like the reference's custom_lowclamp, so a row with m == tau
among deficient rows gets both clamp terms, and without a deficient row it gets plain division by m.

tests/test_weight_grad_ref_cpu.py pins this file to the reference's own float64 autograd (four fixtures, and the reference
itself where it is present) per entry; tests/test_hip_weight_grad.py measures the kernels with it.
"""
import functools

import numpy as np
import torch

MASS_FUNCTIONS = ("identity", "sqrt", "log")
METHODS = ("plain", "homog", "homog_alt")


def mass_encode(emb, m, fn, scale, method):
    """[f(m) scale | emb] and the two homogeneous variants, torch float64 (differentiable in emb and m)."""
    if fn == "identity":
        f = m
    elif fn == "sqrt":
        f = 2 * (m / (torch.sqrt(m + 1) + 1))
    elif fn == "log":
        f = torch.log1p(m)
    else:
        raise ValueError(fn)
    tm = (f * scale)[:, None]
    if method == "plain":
        return torch.cat([tm, emb], dim=1)
    norm = emb.abs().mean(dim=1, keepdim=True)
    if method == "homog":
        return torch.cat([tm * norm, emb], dim=1)
    if method == "homog_alt":
        one = torch.ones_like(tm)
        return torch.cat([torch.where(tm <= 1, tm * (2 - tm), one) * norm, torch.where(tm <= 1, tm * tm, 2 * tm - 1) * emb], dim=1)
    raise ValueError(method)


def embed(rowptr, w, K, freqs, tau, cartesian):
    """emb [rows, S] (diagonal) or [rows, S F] (Cartesian) from torch float64 weights w [nnz], per-entry keys K [nnz, S] and freqs;
    also the row masses m [rows]."""
    S = K.shape[1]
    Kn = K.detach().numpy()
    nrows = len(rowptr) - 1
    zero = torch.zeros((), dtype=torch.float64)
    m = torch.stack([w[a:b].sum() if b > a else zero for a, b in zip(rowptr[:-1], rowptr[1:])])
    pad = bool((m.detach() < tau).any())                     # the global switch
    rows = []
    for r in range(nrows):
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        if pad:
            wr = torch.cat([w[a:b], torch.clamp(tau - m[r], min=0.0)[None]]) / torch.clamp(m[r], min=tau)
            Kr = torch.cat([K[a:b], torch.zeros((1, S), dtype=torch.float64)], dim=0)
            Krn = np.concatenate([Kn[a:b], np.zeros((1, S))], axis=0)
        else:
            assert b > a
            wr, Kr, Krn = w[a:b] / m[r], K[a:b], Kn[a:b]
        index = np.arange(Krn.shape[0])
        cols = []
        for s in range(S):
            order = torch.from_numpy(np.lexsort((index, Krn[:, s])))
            ws, p = wr[order], Kr[order, s]
            c = torch.cumsum(ws, dim=0)
            xi = freqs if cartesian else freqs[s:s + 1]
            phase = torch.remainder(xi[None, :] * (2 * c - ws)[:, None], 2.0)        # exact reduction: cos(pi x) has period 2
            delta = 2 * ws[:, None] * torch.sinc(xi[None, :] * ws[:, None]) * torch.cos(np.pi * phase)
            cols.append((1 + xi) * (delta * p[:, None]).sum(dim=0))
        rows.append(torch.cat(cols))
    return torch.stack(rows), m


def forward_longdouble(rowptr, col, w, keys, freqs, tau, cartesian=False):
    """The embedding's forward (no mass column, every row padded: a pad of weight 0 changes nothing) in numpy long double, rounded
    to float64: tells whose rounding a difference between two float64 forwards is.  keys [n, S] long double or float64."""
    LD = np.longdouble
    pi = LD("3.14159265358979323846264338327950288")
    K_all, fr, tau = np.asarray(keys, dtype=LD), np.asarray(freqs, dtype=LD), LD(tau)
    S = K_all.shape[1]
    F = fr.size if cartesian else 1
    out = np.zeros((len(rowptr) - 1, S * F), dtype=LD)
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        wr = np.asarray(w[a:b], dtype=LD)
        m = wr.sum()
        wr = np.concatenate([wr, [max(tau - m, LD(0))]]) / max(m, tau)
        K = np.concatenate([K_all[col[a:b]], np.zeros((1, S), dtype=LD)])
        for s in range(S):
            order = np.lexsort((np.arange(K.shape[0]), K[:, s]))
            ws, p = wr[order], K[order, s]
            c = np.cumsum(ws)
            for f, xi in enumerate(fr if cartesian else fr[s:s + 1]):
                z = xi * ws
                sinc = np.where(z == 0, LD(1), np.sin(pi * z) / np.where(z == 0, LD(1), pi * z))
                out[r, s * F + f] = (1 + xi) * (2 * ws * sinc * np.cos(pi * xi * (2 * c - ws)) * p).sum()
    return out.astype(np.float64)


def weight_grad_reference(rowptr, col, w, keys, freqs, tau, G, Ke=None, cartesian=False, mass_fn=None, mass_scale=1.0, method="plain",
                          per_slice=True):
    """rowptr [rows + 1]; col [nnz] into keys [n, S], or None for per-entry keys [nnz, S]; w [nnz]; Ke [nnz, S] added to every entry's
    key; freqs [S] (diagonal) or [F]; G: the output gradient, [rows, (1 if mass_fn) + S or S F].
    Returns float64 numpy arrays: out; gW [nnz] = d sum(G out) / d w; gkey [nnz, S] (per entry) and gfreq; and with per_slice
    gW_s [nnz, S], the part of gW that flows through slice s of the embedding (gW - gW_s.sum(1) is what flows through the mass
    column's f(m))."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    keys = np.asarray(keys, dtype=np.float64)
    Kn = keys if col is None else keys[np.asarray(col, dtype=np.int64)]
    if Ke is not None:
        Kn = Kn + np.asarray(Ke, dtype=np.float64)
    S = Kn.shape[1]
    wt = torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True)
    Kt = torch.tensor(Kn, requires_grad=True)
    ft = torch.tensor(np.asarray(freqs, dtype=np.float64), requires_grad=True)
    Gt = torch.tensor(np.asarray(G, dtype=np.float64))
    emb, m = embed(rowptr, wt, Kt, ft, float(tau), cartesian)
    out = emb if mass_fn is None else mass_encode(emb, m, mass_fn, float(mass_scale), method)
    assert out.shape == Gt.shape, (out.shape, Gt.shape)
    loss = (out * Gt).sum()
    gW, gkey, gfreq = torch.autograd.grad(loss, (wt, Kt, ft), retain_graph=per_slice, allow_unused=True)
    res = {"out": out.detach().numpy(), "gW": gW.numpy() if gW is not None else np.zeros(wt.shape[0]),
           "gkey": gkey.numpy() if gkey is not None else np.zeros(Kn.shape), "gfreq": gfreq.numpy(), "mass": m.detach().numpy()}
    if per_slice:
        (gemb,) = torch.autograd.grad(loss, emb, retain_graph=True)
        width = emb.shape[1] // S
        gws = np.zeros((wt.shape[0], S))
        for s in range(S):
            sl = slice(s * width, (s + 1) * width)
            (g,) = torch.autograd.grad((gemb[:, sl] * emb[:, sl]).sum(), wt, retain_graph=True, allow_unused=True)
            if g is not None:
                gws[:, s] = g.numpy()
        res["gW_s"] = gws
    return res


# ---- inputs shared by the fixture's generator and the GPU tests -----------------------------------------------------------------
FIXTURE_DEGREES = (0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4500)
FIXTURE_SENDERS, FIXTURE_D = 4600, 3
# rows scaled to these total masses; the row of 256 has m == 1 exactly.  The row of one neighbour is kept off the weights 1/2 and 1:
# there (with its pad element at tau = 1) every phase xi (2 c - w) at xi = 1 is a half-integer and the readout vanishes identically,
# a kink of the |emb| of the 'homog' methods, where the kernel (cospi: an exact 0, sign 0) and the reference (cos(pi / 2) = 6e-17,
# sign +-1) pick different subgradients
PAD_MASSES = {1: 0.3, 2: 0.4, 257: 2.0, 2049: 0.9}
NOPAD_MASSES = {1: 1.0, 2: 1.5, 257: 2.0, 2049: 1.25}     # no row below tau = 1: the row of one has m == 1 exactly as well
DIAG_FREQS = (0.0, -0.75, 0.37, 1.0, 1.5, 2.5, 4.5, 0.125)
CART_FREQS = (0.0, -0.75, 4.5)


def long_row_weights(degrees, masses, seed, zeros=24, dyadic_mass=False):
    """float32 weights [nnz] from {0.25, 0.5, 1}: `zeros` exact zeros inside the rows of 255 and more neighbours, the rows in
    `masses` scaled to that total mass (in float32), the row of 256 set to 1/256 each (m == 1 exactly in any summation order).
    dyadic_mass: in every other row of 255 and more neighbours, weights picked in a hashed order are lowered (1 -> 0.5 or 0.25,
    0.5 -> 0.25) until the row's mass is the power of two below it.  Then a / m and every partial sum of it are exact in float64, in
    any order of summation: the reference's dense-W path, which divides first and then runs one sequential torch.cumsum over all
    senders of a row, is otherwise off by 1e-12 on such rows (test_weight_grad_ref_cpu.py::test_the_fixture_forward_against_long_double)."""
    from fsw_gnn_amd import synth
    deg = np.asarray(degrees, dtype=np.int64)
    nnz = int(deg.sum())
    rowdeg = np.repeat(deg, deg)
    w = np.array([0.25, 0.5, 1.0], dtype=np.float32)[synth.randint(seed, 1, 3, nnz)]
    cand = np.nonzero((rowdeg >= 255) & (rowdeg != 256))[0]
    w[cand[synth.randint(seed + 1, 1, cand.size, zeros)]] = 0.0
    if dyadic_mass:
        for d in sorted(set(int(x) for x in deg if x >= 255 and x != 256 and x not in masses)):
            pos = np.nonzero(rowdeg == d)[0]
            excess = float(w[pos].sum(dtype=np.float64))
            excess -= 2.0 ** np.floor(np.log2(excess))              # a multiple of 1/4
            for j in pos[np.argsort(synth.uniform01(seed + 2, d, 0, pos.size), kind="stable")]:
                steps = {1.0: (0.75, 0.5), 0.5: (0.25,)}.get(float(w[j]), ())
                step = next((s for s in steps if s <= excess), 0.0)
                w[j] -= np.float32(step)
                excess -= step
            assert excess == 0.0, (d, excess)
    for d, mass in masses.items():
        sel = rowdeg == d
        w[sel] *= np.float32(mass) / w[sel].sum(dtype=np.float32)
    w[rowdeg == 256] = np.float32(1.0 / 256.0)
    return w


def long_row_cols(degrees, n, seed):
    """Per row `degree` distinct senders out of n, ascending (the coalesced order): [nnz] int64."""
    from fsw_gnn_amd import synth
    return np.concatenate([np.sort(np.argsort(synth.uniform01(seed, r, 0, n), kind="stable")[:d]) for r, d in enumerate(degrees)]
                          + [np.zeros(0, dtype=np.int64)]).astype(np.int64)


KERNEL_DEGREES = (0, 1, 2, 3, 254, 255, 256, 257, 511, 512, 1023, 2046, 2047, 2048, 2049, 4095, 4096, 4500)
S_DIAG, S_CART = 8, 4
# (row degree, output columns after the mass column) whose output gradient is zero: single readouts, whole Cartesian slices
# (columns 3 f .. 3 f + 2), and one whole row
ZERO_G = ((254, (1, 5)), (257, (3, 4, 5)), (512, tuple(range(12))), (2049, (0, 1, 2)), (4500, (7,)))


@functools.lru_cache(maxsize=None)
def kernel_inputs():
    """Inputs of the kernel-level tests, numpy only: a plain CSR with one recipient per degree of KERNEL_DEGREES and one sender per
    entry (col a permutation), hand-made keys that are exact in float32 and distinct over the whole array,
    K[:, s] = (permutation - nnz // 2 + 1/2) / 1024 (both signs: the pad element's key 0 falls inside every row), an edge term
    Ke in {0, 2^-11} (K + Ke stays exact and distinct), Xp [nnz, 64] with Xp[col] = K, the weights of long_row_weights, and a
    float32 output gradient G [rows, 1 + 12] with the zeros of ZERO_G."""
    rng = np.random.default_rng(81)
    deg = np.array(KERNEL_DEGREES, dtype=np.int64)
    nnz = int(deg.sum())
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.permutation(nnz).astype(np.int64)
    K = np.stack([(rng.permutation(nnz) - nnz // 2 + 0.5) / 1024.0 for _ in range(S_DIAG)], axis=1).astype(np.float32)
    Ke = (rng.integers(0, 2, size=(nnz, S_DIAG)) * 2.0 ** -11).astype(np.float32)
    assert all(np.unique(K[:, s]).size == nnz and np.unique(K[:, s] + Ke[:, s]).size == nnz for s in range(S_DIAG)) and (K != 0).all()
    assert np.array_equal((K.astype(np.float64) + Ke).astype(np.float32).astype(np.float64), K.astype(np.float64) + Ke)
    Xp = np.zeros((nnz, 64), dtype=np.float32)
    Xp[col, :S_DIAG] = K
    w = long_row_weights(KERNEL_DEGREES, PAD_MASSES, seed=82)
    G = rng.standard_normal((deg.size, 1 + 12)).astype(np.float32)
    for d, cols in ZERO_G:
        G[KERNEL_DEGREES.index(d), 1 + np.array(cols)] = 0.0
    res = {"degrees": deg, "rowptr": rowptr, "col": col, "K": K, "Ke": Ke, "Xp": Xp, "w": w, "G": G}
    for a in res.values():
        a.setflags(write=False)
    return res


def reference_run(emb, X, degrees, cols, w, V, fr, tau, cartesian, fn, method, mass_scale=1.0, G=None, seed=0):
    """The unmodified reference module `emb.FSW_embedding` (oracle/ref_harness.py) in float64 on X [n, d] and the graph (degrees, cols, w),
    sparse COO W in diagonal mode and dense W in Cartesian mode (where a zero weight is no entry: its gW is 0): (out, gW at the
    entries, G); G drawn from `seed` when not given."""
    from fsw_gnn_amd import synth
    dt = torch.float64
    nrows, n = len(degrees), X.shape[0]
    rec = np.repeat(np.arange(nrows), degrees)
    kw = dict(total_mass_pad_thresh=tau, learnable_slices=True, learnable_freqs=True, device="cpu", dtype=dt, load_custom_cuda_lib=False,
              enable_bias=False)
    if fn is not None:
        kw.update(encode_total_mass=True, total_mass_encoding_scale=mass_scale, total_mass_encoding_function=fn,
                  total_mass_encoding_method=method)
    if cartesian:
        E = emb.FSW_embedding(d_in=X.shape[1], nSlices=V.shape[0], nFreqs=fr.size, collapse_freqs=True, **kw)
    else:
        E = emb.FSW_embedding(d_in=X.shape[1], d_out=V.shape[0] + (fn is not None), **kw)
    with torch.no_grad():
        E.projVecs.copy_(torch.from_numpy(V))
        E.freqs.copy_(torch.from_numpy(fr))
    vals = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
    idx = torch.from_numpy(np.stack([rec, cols.astype(np.int64)]))
    if cartesian:
        W = torch.zeros((nrows, n), dtype=dt).index_put((idx[0], idx[1]), vals)
    else:
        W = torch.sparse_coo_tensor(idx, vals, (nrows, n), is_coalesced=True)
    out = E(torch.from_numpy(X.astype(np.float64)), W, graph_mode=True)
    if G is None:
        G = synth.normal(seed, 1, tuple(out.shape), dtype=np.float64)
    (out * torch.from_numpy(G)).sum().backward()
    return out.detach().numpy(), vals.grad.numpy(), G


def row_maxima(ref, rowptr):
    """max |ref| over every row, repeated per entry."""
    out = np.zeros(ref.shape[0])
    for a, b in zip(rowptr[:-1], rowptr[1:]):
        if b > a:
            out[a:b] = np.abs(ref[a:b]).max()
    return out


def per_entry_ratio(got, ref, rowptr):
    """Per row the largest |got - ref| / max |ref| over the row (0 for empty rows); rows whose reference vanishes count absolutely."""
    rm = row_maxima(ref, rowptr)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref) / np.where(rm > 0, rm, 1.0)
    return np.array([err[a:b].max() if b > a else 0.0 for a, b in zip(rowptr[:-1], rowptr[1:])])


def rank_shift_effect(rowptr, col, w, keys, freqs, tau, G, cartesian=False):
    """Per row the median over (entry, slice) of |gW_s[j'] - gW_s[j]| for j, j' adjacent in slice s's sorted order, over the row's
    largest |gW|: what handing an entry the value of its neighbour in rank (a rank off by one) does to it.  The difference of two
    adjacent reverse sums is one term H_t / M (M = max(m, tau), the row's divisor), so this is the median |H_t| / M over max |gW|
    without writing H_t down.  Returns (that, that times M = the median |H_t| over max |gW|), NaN for rows of fewer than two."""
    res = weight_grad_reference(rowptr, col, w, keys, freqs, tau, G, cartesian=cartesian)
    keys = np.asarray(keys, dtype=np.float64)
    Kn = keys if col is None else keys[np.asarray(col, dtype=np.int64)]
    out = np.full(len(rowptr) - 1, np.nan)
    M = np.maximum(res["mass"], tau)
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        if b - a < 2:
            continue
        diffs = []
        for s in range(Kn.shape[1]):
            order = np.lexsort((np.arange(b - a), Kn[a:b, s]))
            diffs.append(np.abs(np.diff(res["gW_s"][a:b, s][order])))
        out[r] = np.median(np.concatenate(diffs)) / np.abs(res["gW"][a:b]).max()
    return out, out * M
