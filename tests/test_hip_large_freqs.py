"""Frequencies up to 2S - 1 and beyond: every kernel class against the oracle, per (row, frequency column) line.

'spread' frequencies reach 2 nFreqs - 1 (511 at S = 256, 2047 at S = 1024) and 'random' ones have a heavy tail; the per-entry suites
(tests/test_hip_ties.py, test_hip_signed_freqs.py, test_hip_edge_features.py, the Cartesian hub / giant / split suites) stop at
|xi| <= 13, and the norm-wise checks at larger xi hide one bad column behind the good ones.  Here every column has its own frequency
(tests/large_freq_cases.py: 0.37 and 13 as controls, 127, 511, 2047, -1500, 1e4, and 1024, 2048, 4096 which meet the unit rows of 2048
and 4096 neighbours at xi / D = 1/2, 1, 2), the keys are distinct and exact, the rows run from 1 to 32769 neighbours in three graphs,
and the weights come in four modes: unit at tau = 1, unit at tau = 3.3 (a non-integer pad weight on the rows of 1 .. 3 neighbours),
'deficient' (arbitrary float32 weights, every row's mass in (0.3, 0.9): every row carries the reference's pad element) and 'full'
(mass >= tau: no pad weight; separates the pad element from everything else).

The drivers are those of tests/test_hip_ties.py.  The reference is oracle/fsw_oracle.py on the same float32 inputs;
tests/test_large_freq_cases_cpu.py pins it to long double at these inputs within 1e-7 in the measures used here.

Measures and bounds (the project's: TOL 1e-5 forward, F32_BOUND 3e-5 gradients per line, PER_ENTRY 1e-5), never a norm over an array:
    forward    |got - ref| <= TOL * |ref| per (row, column), or the rounding of the line's own float32 sum where that is larger
               (forward_allowance: rows of thousands of neighbours)
    gkey       per entry <= PER_ENTRY of the largest reference entry of its (row, column) line; per row <= F32_BOUND
    gfreq      |got - ref| <= F32_BOUND * |ref| per column, |ref| floored at the size of the rows' terms (gfreq_terms)
    a line whose coefficients vanish analytically has a reference of pure float64 rounding: |ref| and the line maximum are floored at
    ZERO_LINE_FLOOR = 2e-4 of the line's scale (tests/test_large_freq_cases_cpu.py derives the figure from the oracle's rounding).
The kernels' float32 arithmetic does not depend on xi -- the phase is float64, the sine float32 (absolute error about 6e-8), and
(1 + xi) / (pi xi) tends to 1 / pi -- so these bounds hold at every frequency, provided the cumulative weight is exact to float64:
the pad element's weight max(tau - m, 0) rounded to float32 shifts the phase of every element behind the pad by 2 pi xi * 3e-8.
"""
import functools

import numpy as np
import pytest
import torch

from tests import large_freq_cases as C
from tests import test_hip_ties as T
from tests.test_hip_ties import F32_BOUND, G64_ROW, HAS_MASS, OUT_SCALE, TOL
from tests.test_large_freq_cases_cpu import ZERO_LINE_FLOOR

pytestmark = pytest.mark.gpu
S = len(C.FREQS)
KINDS = (T.CONTROL,) * S                  # every key column is a control column: distinct keys
LADDERS = {repr(l): l for l in C.LADDERS}
CART_COLS, CART_F = (0, 1, 2), S
ALL_SPLIT_FLAGS = 15                      # the four FSW_CART_SPLIT_* bits; each is ignored where its class has no row


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def fmt(freqs, values):
    return " ".join("%s: %.1e" % (k if isinstance(k, str) else "%g" % k, v) for k, v in zip(freqs, values))


U32 = 2.0 ** -24           # unit roundoff of float32
U64 = 2.0 ** -53
SUM_SIGMAS = 4.0           # forward_allowance


def phase_rounding(freqs, degrees):
    """[rows, L]: what float64 arithmetic itself can lose of a line's phase 2 pi xi c: c is a running float64 sum of up to D + 1
    weights (oracle: of D + 1 quotients), each addition rounding by U64 of a sum <= the denominator, so c is off by up to D U64 of the
    denominator in the kernel and in the oracle each: 4 pi |xi| D U64 between the two.  1.5e-11 for 9000 neighbours at xi = 13 (the
    older suites' largest), 4.6e-7 for 32769 at 1e4."""
    return 4 * np.pi * np.abs(np.asarray(freqs, dtype=np.float64))[None, :] * np.asarray(degrees, dtype=np.float64)[:, None] * U64


def forward_allowance(ref, scale, degrees, rel):
    """[rows, L] absolute error allowed per (row, column) line of the float32 kernels, the largest of
      rel * |ref|                       the project's bound TOL per line;
      rel * ZERO_LINE_FLOOR * scale     on a line that vanishes analytically (tests/test_large_freq_cases_cpu.py);
      SUM_SIGMAS * sum_sigma            the float32 sum of the line itself.  The kernels add D products in float32 (lane by lane, then
                                        across lanes): d_t k_t with d_t the difference of two consecutive sines, or B cos(phi_t) k_t in the
                                        unit-weight recurrence.  Scaled by the line's factor (1 + xi) / (pi xi), a partial sum is at most
                                        |sum d_t| max|k| <= 2 max|k| (the keys of tests/large_freq_cases.py sit in two clusters far from
                                        0, so a partial sum is as large as the output).  Every addition rounds by at most U32 of the
                                        partial sum, uniformly: standard deviation 2 U32 max|k| / sqrt(3) each, and over D additions
                                        sum_sigma = 2 U32 sqrt(D / 3) of the line's scale.  The bound is SUM_SIGMAS = 4 of them: the
                                        cases of this module hold some 3000 lines.  4 sum_sigma is 5.0e-5 of the scale for 32768
                                        neighbours, 2.6e-5 for 9000, 1.8e-6 for 40 and 4.8e-7 for 3.  It does not depend on xi, while the
                                        pad weight's rounding costs 1e-4 .. 1e-2 of the scale from xi = 511 on.  It decides two kinds of
                                        line: the long rows, and short rows whose output cancels to less than 4 sum_sigma / TOL of the
                                        scale (5e-2 at 3 neighbours) -- there it stands for the float32 sine's absolute error (6e-8 of
                                        the scale per term): the edge-feature line of 3 neighbours at xi = 2047, whose output is 4e-3 of
                                        its scale, is 3.6e-5 off relatively and 0.27 of this term."""
    D = np.asarray(degrees, dtype=np.float64)[:, None]
    return np.maximum(rel * np.maximum(np.abs(ref), ZERO_LINE_FLOOR * scale), SUM_SIGMAS * 2 * U32 * np.sqrt(D / 3) * scale) + 1e-300


def check_forward_lines(got, ref, scale, degrees, freqs, what, allowed=None):
    """got, ref [rows, 1 + L]: the mass column and L (row, column) lines; scale [rows, L] (large_freq_cases.forward_scale times
    OUT_SCALE); allowed [rows, L]: forward_allowance(TOL) unless given.  Prints the largest relative error of every column with its
    row, and the largest error / allowance."""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    assert degrees[0] == 0 and np.abs(got[0, HAS_MASS:]).max() == 0.0      # the empty row
    mass = np.abs(got[:, 0] - ref[:, 0]) / np.maximum(np.abs(ref[:, 0]), 1e-300)
    diff = np.abs(got[:, HAS_MASS:] - ref[:, HAS_MASS:])
    err = diff / np.maximum(np.abs(ref[:, HAS_MASS:]), ZERO_LINE_FLOOR * scale + 1e-300)
    ratio = diff / (forward_allowance(ref[:, HAS_MASS:], scale, degrees, TOL) if allowed is None else allowed)
    print("%s: forward per (row, column) relative, column max (worst D %s): %s" % (
        what, [degrees[r] for r in err.argmax(axis=0)], fmt(freqs, err.max(axis=0))))
    print("%s: forward error / allowance, column max: %s" % (what, fmt(freqs, ratio.max(axis=0))))
    r, k = np.unravel_index(ratio.argmax(), ratio.shape)
    assert mass.max() <= TOL, (what, "mass column", float(mass.max()))
    assert ratio.max() <= 1.0, (what, "row of %d, xi = %g" % (degrees[r], freqs[k]), float(ratio.max()), float(err[r, k]))


def check_gkey_lines(got, ref, rowptr, scale, freqs, what):
    """Per entry relative to the line maximum and per row (test_hip_ties.check_key_gradients, with the floor of this module); prints the
    largest per-entry ratio of every column."""
    lm = np.maximum(T.line_maxima(ref, rowptr), ZERO_LINE_FLOOR * np.repeat(scale, np.diff(rowptr), axis=0))
    print("%s: gkey per entry / line maximum, column max: %s" % (what, fmt(freqs, (np.abs(got - ref) / lm).max(axis=0))))
    T.check_key_gradients(got, ref, rowptr, KINDS[:got.shape[1]], what, scale, floor=ZERO_LINE_FLOOR)


def gfreq_terms(g, fscale):
    """[L]: root of the sum of squares of the rows' terms of a column's frequency gradient.  gfreq[k] = sum_r g[r, k] d out[r, k] / d xi;
    a row's term is, telescoped like the forward, (1 + xi) / (pi xi) * 2 pi sum_t c_t cos(2 pi xi c_t) (k_(t) - k_(t+1)) (the factor c
    is the cumulative weight, <= 1) plus the derivative of the factor: at most 2 pi |g| * 2 max|k| times the factor in size, 2 pi |g|
    of the line's scale typically.  The rows' terms have either sign; where they cancel in the sum, a kernel that has every term to
    F32_BOUND of its own size has the sum to F32_BOUND of this root, not of the sum."""
    return np.sqrt(((2 * np.pi * np.abs(g) * fscale) ** 2).sum(axis=0))


def check_gfreq(got, ref, terms, freqs, what, rel=F32_BOUND):
    """Per column: |got - ref| <= rel * max(|ref|, terms) (gfreq_terms; rel: a scalar or [L])."""
    err = np.abs(got - ref) / np.maximum(np.abs(ref), terms)
    print("%s: gfreq per column / max(|ref|, terms): %s   (|ref| / terms: %s)" % (what, fmt(freqs, err), fmt(freqs, np.abs(ref) / terms)))
    ratio = err / rel
    assert np.isfinite(got).all() and ratio.max() <= 1.0, (what, "xi = %g" % freqs[int(ratio.argmax())], float(err[int(ratio.argmax())]))


def diagonal(ladder, weights, tau):
    """Reference and scales of the diagonal layout: key column k at frequency k."""
    ref = T.diagonal_reference(weights, tau, S, C.FREQS, KINDS, ladder)
    c = T.tied_case(weights, KINDS, ladder, tau)
    fscale = OUT_SCALE * C.forward_scale(c["K"], c["rowptr"], C.FREQS)
    return ref, c["rowptr"], fscale, gfreq_terms(c["g"][:, HAS_MASS:HAS_MASS + S].astype(np.float64), fscale)


# ---- fsw_embed_f32, fsw_embed_backward_f32, fsw_embed_backward_keys_f32 ------------------------------------------------------------------
TUNED_MODES = [(w, C.TAU_B_F32 if tau == C.TAU_B else tau) for w, tau in C.MODES]       # tau is a float32 in fsw_embed_args
@functools.lru_cache(maxsize=None)
def tuned_run(name, weights, tau):
    return T.run_tuned_kernels(torch.device("cuda:0"), weights, tau, S, C.FREQS, KINDS, LADDERS[name])


@pytest.mark.parametrize("weights,tau", TUNED_MODES, ids=["%s-%.1f" % m for m in TUNED_MODES])
@pytest.mark.parametrize("name", sorted(LADDERS))
def test_tuned_kernels(dev, name, weights, tau):
    """Every degree class of the diagonal kernels, the four weight modes, all ten columns: forward per line, gkey of the atomic and of
    the stored form per entry and per row, against the oracle and against each other.  tau is a float32 in fsw_embed_args: the kernels
    and the oracle get float32(3.3)."""
    ladder = LADDERS[name]
    ref, rowptr, fscale, _terms = diagonal(ladder, weights, tau)
    what = "tuned %s %s tau %g" % (name, weights, tau)
    out, atomic, keys, _gfreq = tuned_run(name, weights, tau)
    check_forward_lines(out, ref["out"], fscale, ladder.degrees, C.FREQS, what)
    check_gkey_lines(atomic, ref["gkey"], rowptr, ref["scale"], C.FREQS, what + " atomics")
    check_gkey_lines(keys, ref["gkey"], rowptr, ref["scale"], C.FREQS, what + " stored")
    check_gkey_lines(keys, atomic, rowptr, ref["scale"], C.FREQS, what + " stored vs atomics")


@pytest.mark.parametrize("weights,tau", TUNED_MODES, ids=["%s-%.1f" % m for m in TUNED_MODES])
@pytest.mark.parametrize("name", sorted(LADDERS))
def test_tuned_kernels_gfreq(dev, name, weights, tau):
    """gfreq of both backward forms per column, on the same runs.  (xi = 4096 on 16384 unit-weight neighbours, xi / D = 1/4, was 3.4e-5
    off while walk_line of csrc/embed_wsort_bwd.hip summed a lane's terms in float32: 7.9e-8 with the float64 lane sum.)"""
    ladder = LADDERS[name]
    ref, _rowptr, _fscale, terms = diagonal(ladder, weights, tau)
    what = "tuned %s %s tau %g" % (name, weights, tau)
    failed = []
    for form, gf in tuned_run(name, weights, tau)[3].items():
        try:
            check_gfreq(gf, ref["gfreq"], terms, C.FREQS, "%s %s" % (what, form))
        except AssertionError as e:
            failed.append(e)
    if failed:
        raise failed[0]


# ---- fsw_embed_generic ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["float64", "float32"])
@pytest.mark.parametrize("weights,tau", C.MODES, ids=["%s-%.1f" % m for m in C.MODES])
@pytest.mark.parametrize("name", sorted(LADDERS))
def test_generic_kernel(dev, name, weights, tau, storage):
    """fsw_embed_generic keeps the pad weight in double: a second reference at long rows.  float32 storage at the bounds of the tuned
    kernels; float64 storage per line and per entry at G64_ROW plus the phase rounding of float64 itself (phase_rounding)."""
    ladder = LADDERS[name]
    ref, rowptr, fscale, terms = diagonal(ladder, weights, tau)
    what = "generic %s %s %s tau %g" % (storage, name, weights, tau)
    out, gkey, gf = T.run_generic_kernel(dev, weights, tau, storage, C.FREQS, KINDS, ladder, S)
    if storage == "float64":
        # G64_ROW, and what float64 arithmetic can lose of the phase on either side (phase_rounding), per line instead of per row
        rel = G64_ROW + phase_rounding(C.FREQS, ladder.degrees)
        check_forward_lines(out, ref["out"], fscale, ladder.degrees, C.FREQS, what, rel * np.maximum(np.abs(ref["out"][:, HAS_MASS:]), fscale) + 1e-300)
        lm = np.maximum(T.line_maxima(ref["gkey"], rowptr), np.repeat(ref["scale"], np.diff(rowptr), axis=0))
        ratio = np.abs(gkey - ref["gkey"]) / (np.repeat(rel, np.diff(rowptr), axis=0) * lm)
        print("%s: gkey per entry / allowance, column max: %s" % (what, fmt(C.FREQS, ratio.max(axis=0))))
        assert np.isfinite(gkey).all() and ratio.max() <= 1.0, (what, float(ratio.max()))
        check_gfreq(gf, ref["gfreq"], terms, C.FREQS, what, rel.max(axis=0))
    else:
        check_forward_lines(out, ref["out"], fscale, ladder.degrees, C.FREQS, what)
        check_gkey_lines(gkey, ref["gkey"], rowptr, ref["scale"], C.FREQS, what)
        check_gfreq(gf, ref["gfreq"], terms, C.FREQS, what)


# ---- fsw_embed_cart_f32, fsw_embed_cart_backward_keys_f32 ----------------------------------------------------------------------------------
CART_CASES = [(n, w, tau, f) for n in sorted(LADDERS) for w, tau in (C.MODES[0], C.MODES[2], C.MODES[3])
              for f in ((0,) if n == "ladder_ties" else (0, ALL_SPLIT_FLAGS))]


@pytest.mark.parametrize("name,weights,tau,flags", CART_CASES, ids=["%s-%s-flags%d" % (n, w, f) for n, w, _tau, f in CART_CASES])
def test_cartesian_kernels(dev, name, weights, tau, flags):
    """S = 3 slices x F = the ten frequencies: the tuned classes (ladder_ties), the hub classes (unit rows of 2049 .. 32768
    neighbours, weighted lines up to 16384 elements), the giant classes above them (one workgroup per line, flags 0) and their split
    forms (all four FSW_CART_SPLIT_* bits).  Forward per (row, slice, frequency) line, gkey (summed over the frequencies) per entry
    relative to its (row, slice) line and per row, gfreq per frequency."""
    ladder = LADDERS[name]
    ref = T.cartesian_reference(weights, tau, CART_COLS, CART_F, C.FREQS, KINDS, ladder)
    c = T.tied_case(weights, KINDS, ladder, tau)
    rowptr = c["rowptr"]
    freqs = C.FREQS * len(CART_COLS)
    fscale = OUT_SCALE * C.forward_scale(np.repeat(c["K"][:, list(CART_COLS)], CART_F, axis=1), rowptr, freqs)
    what = "cartesian %s %s tau %g flags %d" % (name, weights, tau, flags)
    out, gkey, gf = T.run_cartesian_kernels(dev, weights, tau, CART_COLS, CART_F, C.FREQS, KINDS, ladder, flags)
    check_forward_lines(out, ref["out"], fscale, ladder.degrees, freqs, what)
    check_gkey_lines(gkey, ref["gkey"], rowptr, ref["scale"], ["slice %d" % s for s in CART_COLS], what)
    gS = c["g"][:, HAS_MASS:HAS_MASS + len(freqs)].astype(np.float64)
    terms = np.sqrt((gfreq_terms(gS, fscale).reshape(len(CART_COLS), CART_F) ** 2).sum(axis=0))       # over the slices as well
    check_gfreq(gf, ref["gfreq"], terms, C.FREQS, what)


# ---- the edge-feature branch: fsw_embed_f32 / fsw_embed_backward_keys_f32 with efeat -------------------------------------------------------
EF_FREQS = (C.FREQS[3], C.FREQS[4])       # 511, 2047


def test_edge_feature_branch(dev):
    """d_edge = 3 on the 'deficient' weights of ladder_ties, one column at 511 and one at 2047: the only caller of the forward kernels of
    csrc/embed_wsort.hip (rows above 128 neighbours) and the efeat branch of the register and mid-size kernels.  The operands lie on the
    dyadic grids of tests/edge_feature_cases.py with the Xp grid refined to 2^-7: ef multiples of 1/4 in [-2, 2], Ve multiples of 1/8 in
    [-1, 1], so the edge term is a multiple of 2^-5 below 8, and Xp = key - term a multiple of 2^-7 below 1024 -- 17 significant bits, so
    every fma of the kernels is exact and the keys are those of large_freq_cases.place_keys bit for bit.  Same checks as the tuned
    kernels."""
    import ctypes

    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.graph import build_csr_coalesced
    from oracle import fsw_oracle as O
    from tests import edge_feature_cases as EC
    from tests import test_hip_edge_features as EF
    ladder, d_edge, tau, SE = C.LADDERS[0], 3, 1.0, len(EF_FREQS)
    rows, nnz = len(ladder.degrees), ladder.nnz
    rec, snd, w = ladder.edge_list("deficient")
    ef = (np.random.default_rng(171).integers(-8, 9, size=(nnz, d_edge)) / 4.0).astype(np.float32)
    graph = build_csr_coalesced(T.t(rec, dev, torch.int64), T.t(snd, dev, torch.int64), T.t(w, dev), T.t(ef, dev), rows, nnz)
    st = graph.read_stats()
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_NNZ] == nnz
    rowptr = graph.rowptr.cpu().numpy().astype(np.int64)
    col = graph.col[:nnz].cpu().numpy().astype(np.int64)
    wv, efv = graph.w[:nnz].cpu().numpy().astype(np.float64), graph.ef[:nnz].cpu().numpy()
    order = EC.csr_order(rec, snd)
    assert tuple(np.diff(rowptr)) == ladder.degrees and np.array_equal(wv, w[order].astype(np.float64)) and np.array_equal(efv, ef[order])
    Ve = EC.slice_vectors(SE, d_edge)
    term = EC.edge_term(efv, Ve)
    keys = C.place_keys(rowptr, wv, tau, SE, EF_FREQS, np.random.default_rng(172))
    xp = (keys.astype(np.float64) - term).astype(np.float32)
    assert np.array_equal(xp.astype(np.float64) + term, keys.astype(np.float64)) and np.array_equal(EC.keys_float32(xp, efv, Ve), keys)
    g = np.random.default_rng(173).standard_normal((rows, HAS_MASS + SE)).astype(np.float32)

    fr = np.array(EF_FREQS)
    V = np.concatenate([np.eye(SE), Ve.astype(np.float64)], axis=1)
    ident = np.arange(nnz)
    emb, mass = O.fsw_embed_csr(xp.astype(np.float64), rowptr, ident, wv, V, fr, total_mass_pad_thresh=tau, return_mass=True, edge_feat=efv)
    G = OUT_SCALE * g[:, HAS_MASS:].astype(np.float64)
    _, _, gxi, _, gkey_ref = O.fsw_embed_csr_backward(xp.astype(np.float64), rowptr, ident, wv, V, fr, G, total_mass_pad_thresh=tau,
                                                      edge_feat=efv, return_gkey=True)
    ref_out = OUT_SCALE * np.concatenate([EF.MASS_SCALE * mass[:, None], emb], axis=1)

    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    Xp_host = np.zeros((nnz, SE), dtype=np.float32)
    Xp_host[col] = xp
    Xp, Ved, frd, gd = T.t(Xp_host, dev), T.t(Ve, dev), T.t(fr, dev), T.t(g, dev)
    scratch = torch.empty(int(L.fsw_embed_scratch_bytes(max(ladder.degrees))), dtype=torch.uint8, device=dev)
    case = {"graph": graph, "st": st, "degrees": ladder.degrees}
    out = torch.full((rows, HAS_MASS + SE), float("nan"), device=dev)
    a = EF.embed_args(case, Xp, Ved, d_edge, frd, SE, tau, 0, None, scratch)
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    _lib.check(L.fsw_embed_f32(ctypes.byref(a), stream), "fsw_embed_f32")
    gkey = torch.full((nnz, SE), float("nan"), device=dev)
    gf = torch.zeros(SE, device=dev)
    a = EF.embed_args(case, Xp, Ved, d_edge, frd, SE, tau, 0, None, scratch)
    _lib.check(L.fsw_embed_backward_keys_f32(ctypes.byref(a), None, _lib.ptr(gd), gd.stride(0), _lib.ptr(gkey), gkey.stride(0),
                                             _lib.ptr(gf), stream), "fsw_embed_backward_keys_f32")
    torch.cuda.synchronize()
    what = "edge features d_edge 3, deficient"
    fscale = OUT_SCALE * C.forward_scale(keys, rowptr, EF_FREQS)
    check_forward_lines(out.cpu().numpy().astype(np.float64), ref_out, fscale, ladder.degrees, EF_FREQS, what)
    check_gkey_lines(gkey.cpu().numpy().astype(np.float64), gkey_ref, rowptr, T.coefficient_scale(G, fr), EF_FREQS, what)
    check_gfreq(gf.cpu().numpy().astype(np.float64), gxi, gfreq_terms(g[:, HAS_MASS:].astype(np.float64), fscale), EF_FREQS, what)


# ---- the fused layer ---------------------------------------------------------------------------------------------------------------------
def test_fused_layer_at_spread_frequencies(dev):
    """fsw_conv_fused_f32 at the 256 'spread' frequencies (0.002 .. 511) on the degree ladder of tests/test_hip_conv_fused.py (rows of
    0 .. 32 neighbours: the entry takes no longer ones, and unit weights with tau <= 1 only, so there is no 'gcn' form of this case), read
    out per (row, frequency column): W1 is the identity, so Y[i, k] is the embedding entry itself (every other product is an exact
    zero), against tests/conv_fused_ref.py (float64 coefficients and sums).  Per entry |Y - E| <= max(TOL |E|, (D + 4) 2^-24 A), A the
    sum of the absolute values of the line's terms -- the bound of test_conv_fused_selector_weights, which is what D float32
    multiply-adds of a float32 coefficient table can hold; it exceeds TOL |E| only on lines that cancel to less than (D + 4) 6e-3 of their
    terms (measured: 0.15 of the allowance; the plain relative error of the lines with |E| >= 1e-2 A that do not vanish analytically is
    printed: 1.3e-5 at most, 7.0e-6 in the column xi = 511)."""
    from fsw_gnn_amd import synth
    from tests import conv_fused_ref as R
    from tests import test_hip_conv_fused as FU
    K = 256
    fr = synth.spread_freqs(K)
    assert fr.dtype == np.float32 and fr.max() == 511.0
    g = FU.ladder_graph("A")
    r = FU.run_fused(dev, g, K, 0, K, W1=np.eye(K, dtype=np.float32), fr=fr)
    assert r["rc"] == 0, FU.last_error()
    deg = g["deg"]
    short = (deg >= 1) & (deg <= 32)
    got, E, A = r["Y"][short, :K].astype(np.float64), r["E"][short], r["A"][short]
    assert np.isfinite(got).all()
    diff = np.abs(got - E)
    # the line's scale (large_freq_cases.forward_scale): lines that vanish analytically -- xi = 511 is an integer, so every degree that
    # divides 511 or 1022 -- hold rounding only, in the table and in the reference alike
    rowptr = g["rowptr"]
    keys = R.keys(g["nc"], K + 3, seed=11 + K)[g["col"], :K]
    fscale = C.forward_scale(keys, rowptr, fr)[short]
    allowed = np.maximum(TOL * np.maximum(np.abs(E), ZERO_LINE_FLOOR * fscale), (deg[short][:, None] + 4.0) * R.U * A) + 1e-300
    rel = diff / np.maximum(np.abs(E), 1e-300)
    well = (np.abs(E) >= 1e-2 * A) & (np.abs(E) >= ZERO_LINE_FLOOR * fscale)      # lines that neither cancel nor vanish
    top = np.argsort(fr)[-4:]
    print("fused layer, spread S = 256: error / allowance max %.2f; relative error on the %d of %d lines with |E| >= 1e-2 A: max %.1e, "
          "in the columns xi = %s: %s" % ((diff / allowed).max(), well.sum(), well.size, rel[well].max(), fr[top].tolist(),
                                         ["%.1e" % np.where(well[:, k], rel[:, k], 0).max() for k in top]))
    i, k = np.unravel_index((diff / allowed).argmax(), diff.shape)
    assert (diff <= allowed).all(), ("row of %d, xi = %g" % (deg[short][i], fr[k]), float((diff / allowed).max()))


# ---- modules -----------------------------------------------------------------------------------------------------------------------------
# Exact keys.  A float32 module projects in float32 and a float64 module in float64; keys that differ in the last bit swap ranks in
# rows of thousands of neighbours, which moves single key gradients by 2 pi xi / D of the line maximum, and the forward's sensitivity
# to a key's rounding grows with xi -- neither is what these cases are about.  Features are multiples of 1/8 in [-4, 4] and slice
# vectors multiples of 1/8 in [-1, 1] (d = 8): every product is a multiple of 1/64 below 4 and every partial sum below 32, 11 bits, so
# both projections are exact and both modules sort the same keys (with many ties, ranked by the same rule).
MOD_N, MOD_D, MOD_S, MOD_HUB = 2600, 8, 256, 2500


def module_graph(n, hub_degree, seed, extra_short=0):
    """(senders, recipients, degrees) without repeated edges: recipient 0 has hub_degree senders, the next n - 1 have 1 .. 40, and
    extra_short more recipients have 1 .. 3; senders are among the first n vertices."""
    rng = np.random.default_rng(seed)
    deg = np.concatenate([rng.integers(1, 41, size=n), rng.integers(1, 4, size=extra_short)])
    deg[0] = hub_degree
    snd = np.concatenate([rng.choice(n, size=d, replace=False) for d in deg])
    return snd.astype(np.int64), np.repeat(np.arange(deg.size), deg).astype(np.int64), deg


def dyadic(seed, shape, top):
    return np.random.default_rng(seed).integers(-8 * top, 8 * top + 1, size=shape) / 8.0


def line_scales(snd, rec, nrows, keys, freqs):
    """[nrows, S]: large_freq_cases.forward_scale for an edge list: max |key| over the row's senders times the size of F(xi; c)."""
    order = np.argsort(rec, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rec, minlength=nrows))])
    return C.forward_scale(keys[snd[order]], rowptr, freqs)


def run_module(m, call, X, R):
    X = X.clone().requires_grad_(True)
    m.zero_grad()
    out = call(m, X)
    (out * R.to(out.dtype)).sum().backward()
    grads = {"X": X.grad} | {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    return out.detach().cpu().numpy().astype(np.float64), {n: v.detach().cpu().numpy().astype(np.float64) for n, v in grads.items()}


def check_module(dev, m32, m64, call, X, what, snd, rec, deg, hm, unwrap=lambda y: y):
    """The float32 module against the float64 module with the same parameters.  Forward per (row, frequency column) at forward_allowance
    (TOL of the entry, or the line's own float32 sum); the mass column, if any, at TOL; every gradient per row (matrices) or as a
    whole (vectors) norm-wise <= F32_BOUND.  unwrap: the module's output -> [rows, hm + S] embedding entries."""
    V = m64.state_dict()[[k for k in m64.state_dict() if k.endswith("projVecs")][0]].cpu().numpy()
    fr = m64.state_dict()[[k for k in m64.state_dict() if k.endswith("freqs")][0]].cpu().numpy().reshape(-1)
    Xh = X.cpu().numpy()
    keys = Xh @ V.T
    assert np.array_equal(keys, (Xh.astype(np.float32) @ V.T.astype(np.float32)).astype(np.float64)) and np.array_equal(keys, np.round(keys * 64) / 64)
    fscale = line_scales(snd, rec, deg.size, keys, fr)
    R = torch.from_numpy(np.random.default_rng(7).standard_normal((deg.size, hm + fr.size))).to(dev)
    out32, g32 = run_module(m32, call, X.to(torch.float32), R)
    out64, g64 = run_module(m64, call, X.to(torch.float64), R)
    e32, e64 = unwrap(out32), unwrap(out64)
    assert np.isfinite(e32).all() and e32.shape == (deg.size, hm + fr.size)
    if hm:
        assert (np.abs(e32[:, 0] - e64[:, 0]) <= TOL * np.abs(e64[:, 0])).all(), what
    diff = np.abs(e32[:, hm:] - e64[:, hm:])
    ratio = diff / forward_allowance(e64[:, hm:], fscale, deg, TOL)
    rel = diff / np.maximum(np.abs(e64[:, hm:]), ZERO_LINE_FLOOR * fscale + 1e-300)
    top = np.argsort(np.abs(fr))[-3:]
    r, k = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%s: forward error / allowance max %.2f (row of %d, xi = %g), by degree 1..3: %.2f, 4..40: %.2f, %d: %.2f; relative max %.1e; in the "
          "columns xi = %s: %s" % (what, ratio.max(), deg[r], fr[k], ratio[deg <= 3].max(), ratio[(deg > 3) & (deg <= 40)].max(), deg.max(),
                                   ratio[deg > 40].max(), rel.max(), fr[top].tolist(), ["%.1e" % rel[:, c].max() for c in top]))
    worst = {}
    for name in g64:
        a, b = g32[name], g64[name]
        assert np.isfinite(a).all(), name
        if a.ndim == 2:
            floor = 1e-6 * np.linalg.norm(b) / np.sqrt(len(b)) + 1e-300
            worst[name] = float((np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), floor)).max())
        else:
            worst[name] = float(T.relerr(a, b))
    print("%s: gradients, per row or whole: %s" % (what, {k: "%.1e" % v for k, v in worst.items()}))
    assert ratio.max() <= 1.0, (what, "row of %d, xi = %g" % (deg[r], fr[k]), float(ratio.max()))
    assert max(worst.values()) <= F32_BOUND, (what, worst)


def embedding_pair(dev, **kw):
    from fsw_gnn_amd import FSW_embedding
    mods = []
    for dtype in (torch.float32, torch.float64):
        E = FSW_embedding(d_in=MOD_D, d_out=MOD_S, freqs_init="spread", enable_bias=False, learnable_slices=True, learnable_freqs=True,
                          device=dev, dtype=dtype, **kw)
        with torch.no_grad():
            E.projVecs.copy_(torch.from_numpy(dyadic(191, (MOD_S, MOD_D), 1)).to(dev, dtype))
        mods.append(E)
    with torch.no_grad():
        mods[1].freqs.copy_(mods[0].freqs.to(torch.float64))      # the float32 values of 'spread', for both
    assert float(mods[0].freqs.max()) == 511.0 and float(mods[1].freqs.max()) == 511.0
    return mods


@pytest.mark.xfail(strict=True, reason="the float32 layer rounds its 'gcn' weights to float32: 88 times the allowance on rows of 1 .. 3 "
                                       "neighbours at xi = 511 (DESIGN.md, Frequencies)")
def test_module_conv_gcn_spread(dev):
    """FSW_conv(edge_weighting='gcn', embed_dim=257): 256 'spread' frequencies up to 511 through the layer's own dispatch, 2599 vertices
    of 1 .. 40 in-neighbours and one of 2500.  The first Linear layer is the selector [I | 0] with no bias and the activation
    LeakyReLU(0.2), so output column j is the embedding column j or 0.2 of it, exactly, in both modules.
    Finding ("Frequencies"): the float32 layer forms the 'gcn' weights 1 / sqrt(deg_i deg_j) in float32 and the float64 layer
    in float64; the two adjacency matrices differ by 6e-8 per weight, the cumulative weights by about 3e-8, and the phase by
    2 pi xi * 3e-8 -- the rounding of an input, which no kernel can take back.  Measured: 88 times the allowance on a row of 3 neighbours
    at xi = 511 (1.8e-2 of the entry), 38 on the rows of 4 .. 40, 0.11 on the row of 2500.  The two layers also list a row's entries in
    different orders (edge list against coalesced COO), so tied keys -- frequent on this grid -- rank differently and gX is not comparable
    per vertex (0.86).  test_module_embedding_gcn_like_weights_spread hands both modules the same float32 weights and passes."""
    from fsw_gnn_amd import FSW_conv
    snd, rec, deg = module_graph(MOD_N, MOD_HUB, 181)
    X = torch.from_numpy(dyadic(182, (MOD_N, MOD_D), 4)).to(dev)
    eid = torch.from_numpy(np.stack([snd, rec])).to(dev)
    mods = []
    for dtype in (torch.float32, torch.float64):
        m = FSW_conv(MOD_D, 257, embed_dim=257, edge_weighting="gcn", device=dev, dtype=dtype)
        with torch.no_grad():
            m.fsw_embed.projVecs.copy_(torch.from_numpy(dyadic(191, (MOD_S, MOD_D), 1)).to(dev, dtype))
            m.mlp[0].weight.zero_()
            m.mlp[0].weight[:, :257].copy_(torch.eye(257, device=dev, dtype=dtype))
            m.mlp[0].bias.zero_()
        mods.append(m)
    mods[1].load_state_dict({k: v.to(torch.float64) if v.is_floating_point() else v for k, v in mods[0].state_dict().items()})
    check_module(dev, mods[0], mods[1], lambda m, x: m(x, eid), X, "FSW_conv gcn embed_dim 257", snd, rec, deg, 1,
                 unwrap=lambda y: np.where(y >= 0, y, y / 0.2))


@pytest.mark.xfail(strict=True, reason="tau is a float32 in fsw_embed_args: float32(3.3) against 3.3, 19 times the allowance on rows of "
                                       "1 .. 3 neighbours at xi = 511 (DESIGN.md, Frequencies)")
def test_module_embedding_tau_3p3_spread(dev):
    """FSW_embedding(total_mass_pad_thresh=3.3, freqs_init='spread'), 256 slices, unit weights: 200 more rows of 1 .. 3 neighbours carry
    a pad element of non-integer weight.
    Finding ("Frequencies"): fsw_embed_args carries tau as a float32, so the float32 module pads to float32(3.3) and the
    float64 module to 3.3 -- 1.4e-8 of the denominator of every padded row, 2 pi xi * 1.4e-8 of phase.  Measured: 19 times the
    allowance on a row of 3 neighbours at xi = 511 (relative 1.1e-3 at most); rows of 4 neighbours and more, which have no pad weight,
    0.35 of the allowance, the row of 2500 0.06; every gradient <= 2.6e-6.  Widening the field changes the library's interface."""
    snd, rec, deg = module_graph(MOD_N, MOD_HUB, 183, extra_short=200)
    idx = torch.from_numpy(np.stack([rec, snd])).to(dev)
    X = torch.from_numpy(dyadic(186, (MOD_N, MOD_D), 4)).to(dev)
    m32, m64 = embedding_pair(dev, total_mass_pad_thresh=3.3)

    def call(m, x):
        return m(x, torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1], device=dev, dtype=x.dtype), (deg.size, MOD_N)).coalesce(), graph_mode=True)
    check_module(dev, m32, m64, call, X, "FSW_embedding tau 3.3 spread", snd, rec, deg, 0)


def test_module_embedding_gcn_like_weights_spread(dev):
    """FSW_embedding with 256 'spread' frequencies on a sparse W whose values are float32 'gcn'-like weights (every row's mass in
    (0.3, 0.9)), the same values for both modules: the float32 inputs are exact in float64, so what is compared is the kernels'
    arithmetic -- the pad weight above all -- through the module's dispatch, not the rounding of the weights."""
    snd, rec, deg = module_graph(MOD_N, MOD_HUB, 187)
    rng = np.random.default_rng(188)
    w = rng.uniform(0.05, 1.0, size=snd.size)
    w = (w * (rng.uniform(0.3, 0.9, size=deg.size) / np.bincount(rec, weights=w))[rec] * (1 - 1e-6)).astype(np.float32)
    idx = torch.from_numpy(np.stack([rec, snd])).to(dev)
    wd = torch.from_numpy(w).to(dev)
    X = torch.from_numpy(dyadic(189, (MOD_N, MOD_D), 4)).to(dev)
    m32, m64 = embedding_pair(dev)

    def call(m, x):
        return m(x, torch.sparse_coo_tensor(idx, wd.to(x.dtype), (deg.size, MOD_N)).coalesce(), graph_mode=True)
    check_module(dev, m32, m64, call, X, "FSW_embedding gcn-like float32 weights, spread", snd, rec, deg, 0)
