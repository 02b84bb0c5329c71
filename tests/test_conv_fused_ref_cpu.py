"""tests/conv_fused_ref.py without a GPU: the float64 reference of the fused conv kernels against the oracle and the goldens, and the
per-entry bound against a plain float32 evaluation of the same formulae -- inside the bound as it stands (with a factor 2 to spare),
outside it once a coefficient, a column, a bias, a row or the k-interleave of the weights is wrong."""
import numpy as np
import pytest

from oracle import fsw_oracle as O
from tests import cases
from tests import conv_fused_ref as R
from tests.conftest import relerr
from tests.test_cartesian_cpu import case_csr, diagonal_expansion, load_cases

TOL64 = 1e-12


def edge_csr(edge_index, n):
    """Uncoalesced CSR by recipient of an edge_index (row 0 = sender, row 1 = recipient): parallel edges stay separate entries."""
    return R.csr_of(np.asarray(edge_index[1], dtype=np.int64), np.asarray(edge_index[0], dtype=np.int64), n)


def test_coefficients_and_layer_match_oracle_on_conv10k():
    """embed_rows on Xp = X V^T (float64) equals the oracle's embedding of the coalesced graph with its mass column (k parallel unit
    edges = one entry of weight k, DESIGN.md "duplicates"); Y_ref of the message half + x W2^T + b equals O.conv_tail."""
    c = cases.conv10k()
    n, S = c["n"], c["V"].shape[0]
    rowptr, col = edge_csr(c["edge_index"], n)
    deg = np.diff(rowptr)
    X64 = c["X"].astype(np.float64)
    Xp = X64 @ c["V"].astype(np.float64).T
    T = {int(D): R.unit_coeffs_deg(c["freqs"], int(D)) for D in np.unique(deg)}
    E, A = R.embed_rows(rowptr, col, Xp, T, None, 1.0, 1, 0, 1.0)
    crp, ccol, cw, _ = O.coalesce_edge_index(c["edge_index"], n)
    emb = O.fsw_embedding_forward(c["X"], crp, ccol, cw, c["V"], c["freqs"], encode_total_mass=True)
    assert E.shape == emb.shape == (n, 1 + S) and np.isfinite(E).all()
    assert relerr(E, emb) < TOL64
    assert (A >= np.abs(E) * (1 - 1e-12)).all()
    W = c["lin_w"].astype(np.float64)
    K = 1 + S
    yin = X64 @ W[:, K:].T + c["lin_b"].astype(np.float64)
    Y, bound = R.layer_reference(E, A, W[:, :K], deg, yin=yin, act=2, slope=0.2)
    want = O.conv_tail(emb, X64, linear_weight=c["lin_w"], linear_bias=c["lin_b"])
    assert relerr(Y, want) < TOL64
    assert (bound > 0).all()


def test_flat_table_row_order():
    fr = R.freqs(6)
    T, flat = R.unit_coeffs(fr), R.unit_coeffs_flat(fr)
    assert flat.shape == (32 * 33 // 2, 6)
    for D in (1, 2, 31, 32):
        for t in (0, D - 1):
            assert np.array_equal(flat[D * (D - 1) // 2 + t], T[D][t])
    assert np.array_equal(T[4][:, 0], np.full(4, 0.5)) and np.array_equal(T[4][:, 1], np.full(4, 0.5))   # xi = +-0: 2 w
    assert np.abs(T[7][:, 2]).max() == 0.0                                                               # xi = -1: (1 + xi) = 0


@pytest.mark.parametrize("mass_fn", [0, 1, 2])
def test_mass_functions_and_bias_match_oracle(mass_fn):
    """On a ladder with a random bias: embed_rows equals the oracle with projVecs = eye(S) for every total_mass_encoding_function."""
    S = 9
    rec, snd, nr, nc = R.ladder(0, counts=(1, 3), long_rows=True)
    rowptr, col = R.csr_of(rec, snd, nr)
    deg = np.diff(rowptr)
    Xp = R.keys(nc, S + 2)
    fr = R.freqs(S)
    bias = np.random.default_rng(3).standard_normal(1 + S).astype(np.float32)
    T = {int(D): R.unit_coeffs_deg(fr, int(D)) for D in np.unique(deg)}
    E, A = R.embed_rows(rowptr, col, Xp, T, bias, 0.5, 1, mass_fn, 0.7)
    want = 0.5 * O.fsw_embedding_forward(Xp[:, :S].astype(np.float64), rowptr, col, np.ones(col.size), np.eye(S), fr.astype(np.float64),
                                         bias=bias.astype(np.float64), encode_total_mass=True,
                                         total_mass_encoding_function=R.MASS_FN_NAMES[mass_fn], total_mass_encoding_scale=0.7)
    assert set(R.LONG_DEGREES) <= set(deg.tolist()) and (deg == 0).sum() == 1
    assert relerr(E, want) < TOL64
    assert np.abs(E[deg == 0] - 0.5 * bias.astype(np.float64)).max() == 0.0       # rows of degree 0: s b
    E32, _ = R.embed_rows(rowptr, col, Xp, R.unit_coeffs(fr), bias, 0.5, 1, mass_fn, 0.7)
    assert np.isnan(E32[deg > 32]).all() and np.array_equal(E32[deg <= 32], E[deg <= 32])


def test_cartesian_expansion_matches_golden():
    """The Cartesian expansion through embed_rows equals tests/golden/cartesian.npz (the unit-weight graph case, rows of up to 4500
    neighbours) and the diagonal identity tests/test_cartesian_cpu.py checks that golden with."""
    c = load_cases("cartesian")["graph_unit_collapsed"]
    X, rowptr, col, w = case_csr(c)
    assert (w == 1).all() and not bool(c["mass"])
    V, fr = c["V"], c["freqs"]
    S = V.shape[0]
    Xp = X.astype(np.float64) @ V.astype(np.float64).T
    Kx, frx = R.cartesian_expand(Xp, fr, S)
    assert Kx.shape[1] == frx.size == S * fr.size
    assert fr.dtype == np.float32 or np.array_equal(fr.astype(np.float32).astype(np.float64), fr)
    deg = np.diff(rowptr)
    T = {int(D): R.unit_coeffs_deg(frx, int(D)) for D in np.unique(deg)}
    E, _ = R.embed_rows(rowptr, col, Kx, T, c["bias"].reshape(-1), 1.0, 0, 0, 1.0)
    ref = diagonal_expansion(c)
    scale = max(1.0, np.abs(ref).max())
    assert np.abs(E - ref).max() <= 1e-12 * scale
    assert np.abs(E - c["out"].reshape(ref.shape)).max() <= 1e-12 * scale


@pytest.mark.parametrize("Hout,K", [(1, 1), (31, 7), (32, 8), (33, 9), (128, 64), (129, 65), (300, 257)])
@pytest.mark.parametrize("col0", [0, 5])
def test_pack_reference_round_trip(Hout, K, col0):
    ldw_in = col0 + K + 4
    W = np.random.default_rng(Hout + K).standard_normal((Hout, ldw_in)).astype(np.float32)
    W[W == 0] = 1.0
    Wq = R.pack_reference(W, ldw_in, Hout, col0, K)
    ldw = 32 * ((Hout + 31) // 32)
    assert Wq.size == ((K + 7) // 8 + 16) * ldw * 8 == R.packed_floats(K, Hout)
    assert np.array_equal(R.unpack_reference(Wq, Hout, K), W[:, col0:col0 + K])
    assert np.count_nonzero(Wq) == Hout * K                                       # every other element is 0
    q = Wq.reshape(-1, ldw, 8)
    assert not q[:, Hout:].any() and not q[(K + 7) // 8:].any()
    # the formula once more, element by element, on a few indices
    for g, j, h, i in [(0, 0, 0, 0), ((K - 1) // 8, Hout - 1, (K - 1) % 2, ((K - 1) % 8) // 2)]:
        assert Wq[((g * ldw + j) * 8) + 4 * h + i] == W[j, col0 + 8 * g + 2 * i + h]


# ---- the bound against float32 arithmetic -------------------------------------------------------------------------------------------
def fma32(acc, a, b):
    """float32 fused multiply-add: the product of two float32 is exact in float64."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def layer_f32(rowptr, col, Xp, fr, bias, out_scale, has_mass, mass_fn, mass_scale, W1, yin, act, slope, perturb=None):
    """The formulae of embed_rows and layer_reference in np.float32, naive order: coefficients rounded to float32 and scaled, a
    left-to-right sum over t, then over k.  perturb: one of the wrong evaluations of test_bound_has_teeth."""
    f32 = np.float32
    deg = np.diff(rowptr)
    S = fr.size
    hm = has_mass
    K = hm + S
    T = R.unit_coeffs(fr)
    s = f32(out_scale)
    b = np.zeros(K, dtype=f32) if bias is None else bias.astype(f32)
    E = np.zeros((deg.size, K), dtype=f32)
    for D in np.unique(deg):
        D = int(D)
        rows = np.nonzero(deg == D)[0]
        sb = s * b[hm:]
        if perturb == "no_bias_deg0" and D == 0:
            sb = np.zeros(S, dtype=f32)
        acc = np.broadcast_to(sb, (rows.size, S)).astype(f32)
        if D > 0:
            coef = s * T[D].astype(f32)
            if perturb == "swap_coef" and D == 32:
                coef[[15, 16]] = coef[[16, 15]]
            idx = rowptr[rows][:, None] + np.arange(D)[None, :]
            keys = np.sort(Xp[col[idx], :S], axis=1)
            for t in range(D):
                acc = fma32(acc, np.broadcast_to(coef[t], acc.shape), keys[:, t])
        E[rows, hm:] = acc
        if hm:
            m = f32(D)
            f = m if mass_fn == 0 else (f32(2) * (m / (np.sqrt(m + f32(1)) + f32(1))) if mass_fn == 1 else np.log1p(m))
            E[rows, 0] = s * (f32(f) * f32(mass_scale) + b[0])
    W = W1.astype(f32)
    if perturb == "swap_w_cols":
        W = W.copy()
        W[:, [2, 3]] = W[:, [3, 2]]
    Y = np.zeros((deg.size, W.shape[0]), dtype=f32)
    for k in range(K - 1 if perturb == "drop_last_col" else K):
        Y = fma32(Y, E[:, k:k + 1], W[None, :, k])
    if yin is not None:
        Y = Y + np.broadcast_to(yin.astype(f32), Y.shape)
    if act == 1:
        Y = np.maximum(Y, f32(0))
    elif act == 2:
        Y = np.where(Y >= 0, Y, f32(slope) * Y)
    if perturb == "rotate_tile":
        tile = np.nonzero(deg == 18)[0][:32]
        assert tile.size == 32
        Y[tile] = Y[np.roll(tile, 1)]
    return Y


_SETUP = {}


def ladder_a_setup(K, Hout=24):
    """Ladder A with a mass column, bias, Yin, LeakyReLU: (inputs, Y_ref, bound), computed once per K."""
    if K not in _SETUP:
        S = K - 1
        rec, snd, nr, nc = R.ladder(0)
        rowptr, col = R.csr_of(rec, snd, nr)
        rng = np.random.default_rng(100 + K)
        inp = dict(rowptr=rowptr, col=col, Xp=R.keys(nc, S), fr=R.freqs(S), bias=rng.standard_normal(K).astype(np.float32),
                   out_scale=np.float32(0.5), has_mass=1, mass_fn=1, mass_scale=np.float32(0.7),
                   W1=(rng.standard_normal((Hout, K)) / np.sqrt(K)).astype(np.float32),
                   yin=rng.standard_normal((nr, Hout)).astype(np.float32), act=2, slope=np.float32(0.2))
        E, A = R.embed_rows(rowptr, col, inp["Xp"], R.unit_coeffs(inp["fr"]), inp["bias"], float(inp["out_scale"]), 1, 1,
                            float(inp["mass_scale"]))
        Y, bound = R.layer_reference(E, A, inp["W1"], np.diff(rowptr), yin=inp["yin"], act=2, slope=float(inp["slope"]))
        for a in (Y, bound):
            a.setflags(write=False)
        _SETUP[K] = (inp, Y, bound)
    return _SETUP[K]


@pytest.mark.parametrize("K", [8, 65, 504])
def test_bound_is_achievable_in_float32(K):
    """A plain float32 evaluation stays inside the bound in every entry, and uses less than half of it."""
    inp, Y, bound = ladder_a_setup(K)
    got = layer_f32(**inp).astype(np.float64)
    assert np.isfinite(got).all() and (bound > 0).all()
    ratio = np.abs(got - Y) / bound
    print("K = %d: largest |err| / bound %.3f" % (K, ratio.max()))
    assert (ratio <= 1.0).all()
    assert ratio.max() < 0.5


def test_bound_has_teeth():
    """The same float32 evaluation with one thing wrong leaves the bound on at least one entry."""
    inp, Y, bound = ladder_a_setup(65)

    def leaves(perturb):
        return bool((np.abs(layer_f32(perturb=perturb, **inp).astype(np.float64) - Y) > bound).any())

    assert not leaves(None)
    assert leaves("swap_coef")          # (a) two adjacent coefficients of the D = 32 rows swapped
    assert leaves("drop_last_col")      # (b) embedding column K - 1 dropped from the product
    assert leaves("no_bias_deg0")       # (c) the bias of degree-0 rows omitted
    assert leaves("rotate_tile")        # (d) the rows of one 32-row tile rotated by one
    assert leaves("swap_w_cols")        # (e) W1 columns 2 and 3 exchanged: the even/odd interleave of the packed layout
