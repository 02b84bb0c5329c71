"""The restatement tests/weight_grad_ref.py (plain float64 forward + torch.autograd) against the reference's own float64 autograd of
d loss / d W: the four fixtures that store a gW, and the reference itself where it is present.  CPU only, always runs.

Metric: per entry, |gW - ref| over the largest |ref| of the entry's row; bound REF_BOUND = 1e-11 (the reference's own agreement
with a plain restatement on rows of up to 4500 neighbours is of order 1e-13; the bound leaves room for other seeds and longer sums).
The forward is held to the same bound per row (norm-wise).

Measured, largest ratio per fixture (gW per entry | forward per row):
    grads_w.npz            tau1 3.7e-13, tau3 8.2e-13, cloud 1.5e-12  | 7.0e-14     (frequencies up to 31: a weight's gradient carries
                           the factor 2 pi xi twice, once in the phase and once in its derivative)
    signed_freqs.npz       unit 6.8e-14, general 6.3e-14, general_tau3 6.3e-14  | 4.0e-14
    grads_cartesian.npz    weighted_mass_w 1.5e-15  | 1.8e-15
    grads_w_long.npz       diag_tau1_sqrt_homog 3.3e-13, diag_tau3_log_homog_alt 4.1e-13, nopad_tau1 1.3e-13, cart_tau1 1.7e-14,
                           cart_tau3 3.7e-14  | 4.5e-13   (rows of 2047 / 2048; the restatement's sequential cumsum is the larger part:
                           the GPU module agrees with the sparse-path cases to 7e-15)
    the reference itself   fresh graph (rows of 0 .. 1500), diagonal tau 1 and 3 without a mass column: 1.1e-13  | 1.1e-13
    restatement gkey / gfreq / out against the oracle on the kernel-level inputs of tests/test_hip_weight_grad.py: gkey 1.2e-11 of
                           the line maximum on a floored line (bound 5e-11, see the test), 1.6e-14 Cartesian; gfreq 8e-16, out 3e-15
    nopad_tau1             the clamp rule instead of the reference's global pad rule is off by 210 % on the row of 256 (m == tau)

The gap between bound and fault (test_rank_shift_effect): handing an entry the value of its neighbour in rank -- what a wrong rank
at a chunk seam does -- moves it by one term H_t / M (M = max(m, tau)).  Median per row over the row's largest |gW|, diagonal |
Cartesian, in brackets the median |H_t| / max |gW| without the divisor:
    row of 2: 5.6e-2 | 1.3e-2    255: 7.8e-4 | 1.6e-3    256: 4.4e-4 | 4.8e-4    257: 5.7e-4 | 1.9e-3    2047: 5.2e-5 | 2.3e-4
    2048: 6.8e-5 | 1.9e-4    2049: 8.8e-5 | 3.7e-4    4500: 5.5e-5 (1.4e-1) | 5.6e-5 (1.5e-1);    smallest: 5.2e-5 (1.1e-4)
The bounds of tests/test_hip_weight_grad.py beside it: float64 storage 1e-10 of the row maximum, five orders below; float32 storage
about 1e-6 of the row maximum on the long rows (measured error 1.5e-7 = 0.17 of the bound), a factor 50 below.
"""
import functools

import numpy as np
import pytest

from oracle import fsw_oracle as O
from oracle import ref_harness
from tests import weight_grad_ref as R
from tests.conftest import golden, relerr
from tests.test_hip_ties import coefficient_scale, line_maxima

REF_BOUND = 1e-11


def rowptr_of(rec, nrows):
    assert (np.diff(rec) >= 0).all()
    return np.concatenate([[0], np.cumsum(np.bincount(rec, minlength=nrows))]).astype(np.int64)


def compare(what, res, rowptr, gW, out):
    """Per entry against the row maximum (gW) and per row norm-wise (out); prints the largest ratios."""
    ratios = R.per_entry_ratio(res["gW"], gW, rowptr)
    fwd = max(relerr(res["out"][r], out[r]) for r in range(out.shape[0]))
    deg = np.diff(rowptr)
    print("%s: gW per entry / row maximum %.1e (row of %d), forward per row %.1e" % (what, ratios.max(), deg[ratios.argmax()], fwd))
    assert np.isfinite(res["gW"]).all() and ratios.max() <= REF_BOUND, (what, dict(zip(deg.tolist(), ratios.tolist())))
    assert fwd <= REF_BOUND, (what, fwd)
    return ratios.max(), fwd


def test_restatement_on_grads_w():
    g, gt, gw = golden("tiny_graph"), golden("grads_tiny"), golden("grads_w")
    idx = g["adj_indices"]
    rowptr = rowptr_of(idx[0], 64)
    keys = g["X"].astype(np.float64) @ g["V"].astype(np.float64).T
    for tag, tau, fn in (("tau1", 1.0, "identity"), ("tau3", 3.0, "log")):
        res = R.weight_grad_reference(rowptr, idx[1], g["adj3_values"], keys, gt["freqs"], tau, gt["R"], mass_fn=fn, mass_scale=0.7,
                                      per_slice=False)
        compare("grads_w " + tag, res, rowptr, gw["gW_" + tag], gw["out_" + tag] - g["bias"])
    B, npts, d = gw["cloud_X"].shape
    res = R.weight_grad_reference(np.arange(B + 1) * npts, None, gw["cloud_W"].reshape(-1),
                                  gw["cloud_X"].reshape(B * npts, d) @ g["V"].astype(np.float64).T, gt["freqs"], 1.0, gw["cloud_R"],
                                  per_slice=False)
    compare("grads_w cloud", res, np.arange(B + 1) * npts, gw["cloud_gW"].reshape(-1), gw["cloud_out"])


def test_restatement_on_signed_freqs():
    g = golden("signed_freqs")
    deg = g["degrees"]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    keys = g["X"].astype(np.float64) @ g["V"].astype(np.float64).T
    for tag, w, tau in (("unit", np.ones(int(deg.sum())), 1.0), ("general", g["w_general"], 1.0), ("general_tau3", g["w_general"], 3.0)):
        res = R.weight_grad_reference(rowptr, g["senders"], w, keys, g["freqs"], tau, g["R"], per_slice=False)
        compare("signed_freqs " + tag, res, rowptr, g["gW_" + tag], g["out_" + tag])


def test_restatement_on_grads_cartesian():
    g = golden("grads_cartesian")
    c = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith("weighted_mass_w/")}
    B, npts, d = c["X"].shape
    rowptr = np.arange(B + 1) * npts
    assert bool(c["mass"]) and bool(c["collapse"]) and str(c["fn"]) == "identity"
    res = R.weight_grad_reference(rowptr, None, c["W"].reshape(-1), c["X"].reshape(B * npts, d) @ c["V"].T, c["freqs"], 1.0, c["G"],
                                  cartesian=True, mass_fn="identity", mass_scale=float(c["scale"]), per_slice=False)
    compare("grads_cartesian weighted_mass_w", res, rowptr, c["gW"].reshape(-1), c["out"])


# ---- the new fixture ----------------------------------------------------------------------------------------------------------------
LONG_CASES = ("diag_tau1_sqrt_homog", "diag_tau3_log_homog_alt", "nopad_tau1", "cart_tau1", "cart_tau3")


@functools.lru_cache(maxsize=None)
def long_case(name):
    """Inputs of one case of grads_w_long.npz: rowptr, cols, w and X in float64, and the case's arrays."""
    g = golden("grads_w_long")
    c = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}
    which = str(c["graph"])
    deg = g["graph/degrees"].astype(np.int64)
    if which == "nopad":
        deg = deg[1:]
    c.update(rowptr=np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), cols=g["graph/cols"].astype(np.int64),
             w=g["graph/w_" + which].astype(np.float64), X=g["graph/X"].astype(np.float64), degrees=deg, cartesian=bool(c["cartesian"]),
             tau=float(c["tau"]), fn=str(c["fn"]) or None, method=str(c["method"]), scale=float(c["scale"]))
    return c


def test_fixture_holds_what_it_is_for():
    g = golden("grads_w_long")
    assert tuple(g["graph/degrees"]) == R.FIXTURE_DEGREES
    for which, deg in (("pad", R.FIXTURE_DEGREES), ("cart", R.FIXTURE_DEGREES), ("nopad", R.FIXTURE_DEGREES[1:])):
        w = g["graph/w_" + which]
        assert w.dtype == np.float32 and (w == 0).sum() >= 10
        m = np.add.reduceat(w.astype(np.float64), np.cumsum((0,) + tuple(d for d in deg if d))[:-1])
        mass = dict(zip([d for d in deg if d], m))
        assert mass[256] == 1.0 and np.all(w[np.repeat(deg, deg) == 256] == np.float32(1 / 256))
        if which != "nopad":
            assert abs(mass[2] - 0.4) < 1e-6 and abs(mass[257] - 2.0) < 1e-5 and abs(mass[2049] - 0.9) < 1e-5 and mass[1] < 1
        else:
            assert mass[1] == 1.0 and min(mass.values()) == 1.0
    for name in LONG_CASES:
        c = long_case(name)
        fr = c["freqs"]
        assert (fr == 0).any() and (fr < 0).sum() == 1 and (fr > 4).any(), name
        if c["method"] != "plain":
            # 'homog' differentiates |emb|: no readout of a non-empty row may vanish (weight_grad_ref.PAD_MASSES), or the gradient
            # is a choice among subgradients that rounding makes.  (The smallest, 4.7e-8 of its row's maximum in the row of two, is a
            # cosine at 1/2 + 1e-8: its sign comes from the float32 rounding of the weights, the same for every path.)
            emb = np.abs(c["out"][1:, 1:])
            assert (emb > 1e-9 * emb.max(axis=1, keepdims=True)).all(), name
        # a zero weight still has a gradient, in the reference's dense-W (Cartesian) cases too
        assert c["gW"].shape == c["w"].shape and np.abs(c["gW"][c["w"] == 0]).min() > 0


@pytest.mark.parametrize("name", LONG_CASES)
def test_restatement_on_the_long_rows(name):
    """Every case of grads_w_long.npz.  nopad_tau1: the rows of 1 and 256 neighbours have m == tau exactly and no row is deficient, so
    the reference divides by m; the clamp rule, forced by one extra empty recipient, must be far off on the row of 256."""
    c = long_case(name)
    rowptr, cols, w = c["rowptr"], c["cols"], c["w"]
    keys = c["X"] @ c["V"].T
    res = R.weight_grad_reference(rowptr, cols, w, keys, c["freqs"], c["tau"], c["G"], cartesian=c["cartesian"], mass_fn=c["fn"],
                                  mass_scale=c["scale"], method=c["method"], per_slice=False)
    compare("grads_w_long " + name, res, rowptr, c["gW"], c["out"])
    if name == "nopad_tau1":
        G1 = np.concatenate([c["G"], np.zeros((1, c["G"].shape[1]))])
        clamp = R.weight_grad_reference(np.append(rowptr, rowptr[-1]), cols, w, keys, c["freqs"], c["tau"], G1, per_slice=False)
        r = list(c["degrees"]).index(256)
        a, b = rowptr[r], rowptr[r + 1]
        off = np.abs(clamp["gW"][a:b] - c["gW"][a:b]).max() / np.abs(c["gW"][a:b]).max()
        print("nopad_tau1: the clamp rule on the row of 256 is off by %.0f %%" % (100 * off))
        assert off > 0.3


def test_the_fixture_forward_against_long_double():
    """The fixture's own error: the float64 module is held to 1e-12 per row against the stored forward (tests/test_hip_weight_grad.py),
    so the stored forward itself must be inside that.  Measure: the same forward in long double (64-bit mantissa); bound: half of
    the module's, 5e-13, which leaves the module the other half (measured: nopad_tau1 2.1e-15, cart_tau1 1.0e-14, cart_tau3 1.4e-13
    on the row of 256, whose division by tau = 3 is not exact: 256 terms are too few to matter more).
    The reference's sparse path (a segmented tree cumsum) is within 2.1e-15 on every row.  Its dense
    path, which the Cartesian cases have to take, divides by the mass and runs a sequential torch.cumsum over all 4600 senders of
    a row; with the 'pad' weights that put its stored forward off by 9.2e-13 / 1.3e-12 / 3.4e-13 on the rows of 2047 / 2048 / 4500
    (rows whose division is exact, m <= tau = 1, stayed at 1e-15).  Hence the 'cart' weights, whose long rows have a power-of-two
    mass (weight_grad_ref.long_row_weights): asserted here, with the figure they give."""
    g = golden("grads_w_long")
    deg = np.array(R.FIXTURE_DEGREES)
    m = np.add.reduceat(g["graph/w_cart"].astype(np.float64), np.concatenate([[0], np.cumsum(deg[deg > 0])[:-1]]))
    for d, mass in zip(deg[deg > 0], m):
        if d in (255, 2047, 2048, 4500):
            assert mass > 1 and np.log2(mass) == np.floor(np.log2(mass)), (d, mass)
    worst = {}
    for name in ("nopad_tau1", "cart_tau1", "cart_tau3"):
        c = long_case(name)
        ld = R.forward_longdouble(c["rowptr"], c["cols"], c["w"], c["X"].astype(np.longdouble) @ c["V"].astype(np.longdouble).T,
                                  c["freqs"], c["tau"], c["cartesian"])
        errs = np.array([relerr(c["out"][r], ld[r]) for r in range(ld.shape[0])])
        print("%s: stored forward vs long double per row: %s" % (name, "  ".join("%d: %.1e" % (d, e) for d, e in zip(c["degrees"], errs))))
        worst[name] = errs.max()
    if np.finfo(np.longdouble).nmant >= 63:          # x86: the 80-bit format; elsewhere long double may be float64 and tells nothing
        assert max(worst.values()) <= 5e-13, worst


def test_rank_shift_effect():
    """The smallest effect of a rank shifted by one (module docstring), from the fixture, diagonal (the nopad weights, tau 1) and
    Cartesian: per row the median over (entry, slice) of the change an entry sees when it gets its rank neighbour's value, H_t / M,
    and of H_t itself, both over the row's largest |gW|.  The float64 bound of the GPU tests (1e-10 of the row maximum) must stay four
    orders below the smaller of the two in every row."""
    low = []
    for name in ("nopad_tau1", "cart_tau1"):
        c = long_case(name)
        eff, h = R.rank_shift_effect(c["rowptr"], c["cols"], c["w"], c["X"] @ c["V"].T, c["freqs"], c["tau"], c["G"], cartesian=c["cartesian"])
        print("%s, median per row, |H_t| / M / max |gW| (|H_t| / max |gW|): %s" % (name, "  ".join(
            "%d: %.1e (%.1e)" % (d, e, hh) for d, e, hh in zip(c["degrees"], eff, h) if np.isfinite(e))))
        low.append(np.nanmin(eff))
    assert min(low) > 1e4 * 1e-10, low


# ---- the restatement's other outputs against the oracle, on the inputs of the GPU kernel tests ------------------------------------------
def test_restatement_gkey_gfreq_against_the_oracle():
    """gkey and gfreq of the restatement (the yardstick of the same launches in tests/test_hip_weight_grad.py) against
    oracle.fsw_oracle on the kernel-level inputs, diagonal with the edge term and Cartesian through the diagonal identity."""
    k = R.kernel_inputs()
    nnz, rowptr = k["w"].size, k["rowptr"]
    ident = np.arange(nnz)
    worst = 0.0
    for cart in (False, True):
        S, F = (R.S_CART, len(R.CART_FREQS)) if cart else (R.S_DIAG, 1)
        fr = np.array(R.CART_FREQS if cart else R.DIAG_FREQS, dtype=np.float32).astype(np.float64)
        K = k["K"][:, :S].astype(np.float64) + (0.0 if cart else k["Ke"].astype(np.float64))
        G = k["G"][:, 1:1 + S * F]
        res = R.weight_grad_reference(rowptr, None, k["w"], K, fr, 1.0, G, cartesian=cart, per_slice=False)
        Kd, frd = (np.repeat(K, F, axis=1), np.tile(fr, S)) if cart else (K, fr)
        emb = O.fsw_embed_csr(Kd, rowptr, ident, k["w"].astype(np.float64), np.eye(S * F), frd, total_mass_pad_thresh=1.0)
        _, _, gxi, gkey = O.fsw_embed_csr_backward(Kd, rowptr, ident, k["w"].astype(np.float64), np.eye(S * F), frd, G,
                                                   total_mass_pad_thresh=1.0, return_gkey=True)
        gkey, gxi = gkey.reshape(nnz, S, F).sum(axis=2), gxi.reshape(S, F).sum(axis=0) if cart else gxi
        # a line whose coefficients all vanish is pure rounding in both: the line maximum is floored as in tests/test_hip_ties.py, at
        # 2e-4 of the line's scale.  Each side rounds the argument of its sin / cos, an absolute error of 2 pi xi 2^-53 = 3.1e-15 of
        # the scale at xi = 4.5, i.e. 1.6e-11 of a floored line per side: the per-entry bound here is 5e-11 (both sides, factor 1.5),
        # half of what the GPU tests allow the kernel (1e-10)
        scale = coefficient_scale(G.astype(np.float64), frd).reshape(-1, S, F).sum(axis=2)
        lm = np.maximum(line_maxima(gkey, rowptr), 2e-4 * np.repeat(scale, k["degrees"], axis=0))
        ratio = (np.abs(res["gkey"] - gkey) / np.where(lm > 0, lm, 1.0)).max()
        print("restatement vs oracle, %s: gkey per entry / line maximum %.1e, gfreq %.1e, out %.1e" % (
            "Cartesian" if cart else "diagonal", ratio, relerr(res["gfreq"], gxi), relerr(res["out"], emb)))
        worst = max(worst, ratio)
        assert ratio <= 5e-11 and relerr(res["gfreq"], gxi) <= REF_BOUND and relerr(res["out"], emb) <= REF_BOUND
    assert worst > 0


# ---- the reference itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ref_harness.available(), reason="the reference implementation is not present")
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_restatement_against_the_reference_itself(tau):
    """A fresh graph (rows of 0 .. 3000 neighbours, other seeds than the fixture), diagonal mode without a mass column -- the cases the
    fixture has no room for -- run through the unmodified reference here and now."""
    from fsw_gnn_amd import synth
    emb, _ = ref_harness.load()
    degrees = (3, 0, 700, 1, 258, 1500, 64, 1100)      # the reference's pure-torch segcumsum needs nnz >= twice the longest row
    n, d, S = 3200, 4, 8
    cols = R.long_row_cols(degrees, n, seed=701)
    w = R.long_row_weights(degrees, {3: 0.4, 258: 0.9}, seed=702, zeros=8)
    X = synth.features(n, d, seed=703)
    V = synth.unit_slices(S, d, seed=704).astype(np.float64)
    fr = np.array(R.DIAG_FREQS, dtype=np.float32).astype(np.float64)
    out, gW, G = R.reference_run(emb, X, degrees, cols, w, V, fr, tau, False, None, "plain", seed=705)
    rowptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    res = R.weight_grad_reference(rowptr, cols, w, X.astype(np.float64) @ V.T, fr, tau, G, per_slice=False)
    compare("reference itself, tau %g" % tau, res, rowptr, gW, out)
