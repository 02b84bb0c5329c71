"""The yardstick of tests/test_hip_large_freqs.py, checked without a GPU.

1. oracle/fsw_oracle.py (float64) against the long-double restatement of tests/large_freq_cases.py at exactly the frequencies, degree
   ladders and weight modes of the GPU tests, in the GPU tests' own measure: the forward per (row, column), the key gradient per entry
   relative to the largest entry of its (row, column) line.  Condition: 1e-7, 1/100 of the GPU bounds (TOL, PER_ENTRY = 1e-5).
   The float64 oracle carries its own rounding into the phase pi xi (2c - w): c is a running float64 sum of D quotients w / denom,
   so the phase is off by up to 2 pi |xi| D 2^-53 (4e-11 for the row of 40 neighbours at xi = -1500; measured 1.0e-11 of the line's
   scale there).  On a line whose coefficients vanish analytically (unit weights, xi / D a multiple of 1/2: that row, 3 neighbours at
   -1500, 2048 at 1024 ...) that rounding is all the oracle returns, and a kernel that reduces the phase exactly returns 0.  Both
   measures therefore floor their denominator at ZERO_LINE_FLOOR = 2e-4 of the line's scale (large_freq_cases.forward_scale,
   test_hip_ties.coefficient_scale), the floor tests/test_hip_ties.py uses for the float64 kernel for the same reason: PIN times the
   floor, 2e-11 of the scale, covers the measured rounding.  The floor reaches two lines that do not vanish: the coefficients of the
   rows of 32768 and 32769 neighbours at xi = 0.37 are 2 (1 + xi) / D = 7e-5 of the scale, so those two control lines are checked
   at 2.9 times their line maximum; the next one (16385 neighbours, 1.4e-4) at 1.4 times; every other line at its own maximum.
2. The defect the GPU tests were written for, restated in float64: with the pad element's weight rounded to float32 before it enters
   the cumulative weight (what every float32 general-weight kernel did), the float64 forward leaves TOL = 1e-5 in the xi >= 511 columns
   of the 'deficient' mode; with the exact pad weight it stays inside it, as does the control mode without a pad.  (At xi = 13 the
   rounded pad costs up to 1.0e-5 here, at the bound: that column is printed, not asserted; 0.37 is asserted.)
"""
import functools

import numpy as np
import pytest

from oracle import fsw_oracle as O
from tests import large_freq_cases as C

PIN = 1e-7                    # oracle against long double: 1/100 of the GPU bounds
TOL = 1e-5                    # the GPU tests' forward bound
ZERO_LINE_FLOOR = 2e-4        # of the line's scale; see the module docstring

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).eps > 1e-18, reason="long double is no wider than double on this platform")


def line_maxima(ref, rowptr):
    out = np.zeros(ref.shape)
    for a, b in zip(rowptr[:-1], rowptr[1:]):
        if b > a:
            out[a:b] = np.abs(ref[a:b]).max(axis=0, keepdims=True)
    return out


CART_COLS = tuple(np.repeat(np.arange(3), len(C.FREQS)))     # Cartesian mode, 3 slices x every frequency, as diagonal columns
CART_FREQS = C.FREQS * 3
LAYOUTS = {"diagonal": (None, C.FREQS), "cartesian": (CART_COLS, CART_FREQS)}


def oracle(ladder, weights, tau, cols, freqs):
    """(out [rows, S], coefficients [nnz, S]) of the float64 oracle: the key gradient under G = 1 is the coefficient."""
    rowptr, _col, w, _w32 = C.csr(ladder, weights)
    K = C.cached_keys(ladder, weights, tau).astype(np.float64)[:, list(range(len(freqs)) if cols is None else cols)]
    S, ident, fr = len(freqs), np.arange(ladder.nnz), np.array(freqs)
    out = O.fsw_embed_csr(K, rowptr, ident, w, np.eye(S), fr, total_mass_pad_thresh=tau)
    G = np.ones((len(ladder.degrees), S))
    gkey = O.fsw_embed_csr_backward(K, rowptr, ident, w, np.eye(S), fr, G, total_mass_pad_thresh=tau, return_gkey=True)[-1]
    return out, gkey


def test_inputs():
    """Frequencies are float32 values; keys distinct, non-zero and exact; every 'deficient' row has mass in (0.3, 0.9), every 'full'
    row mass >= 1 and the mode holds exact zeros; tau = 3.3 leaves a non-integer pad on the rows of 1 .. 3 neighbours only."""
    assert all(float(np.float32(x)) == x for x in C.FREQS + (C.TAU_B_F32,))
    assert sorted(sum((l.degrees for l in C.LADDERS), ())) == sorted(C.TIES_DEGREES + (0, 16384, 16385, 0, 32768, 32769))
    for ladder in C.LADDERS:
        rowptr, col, _w, _ = C.csr(ladder, "unit")
        assert tuple(np.diff(rowptr)) == ladder.degrees and np.array_equal(np.sort(col), np.arange(ladder.nnz))
        for weights, tau in C.MODES:
            K = C.cached_keys(ladder, weights, tau)
            assert K.dtype == np.float32 and (np.abs(K) >= 128).all() and np.array_equal(K, np.round(K / C.KEY_STEP) * C.KEY_STEP)
            for a, b in zip(rowptr[:-1], rowptr[1:]):
                assert all(np.unique(K[a:b, c]).size == b - a for c in range(K.shape[1]))
        for weights in ("deficient", "full"):
            _, _, w, w32 = C.csr(ladder, weights)
            assert w32.dtype == np.float32
            mass = np.array([w[a:b].sum() for a, b in zip(rowptr[:-1], rowptr[1:]) if b > a])
            if weights == "deficient":
                assert (mass > 0.3).all() and (mass < 0.9).all() and (w > 0).all()
                assert (np.abs(np.log2(w[w > 0]) % 1) > 0).mean() > 0.99          # not dyadic
            else:
                assert (mass >= 1.0).all() and (w == 0).sum() >= 3
    pads = [C.TAU_B - d for d in (1, 2, 3)]
    assert all(p > 0 and p != round(p) for p in pads) and C.TAU_B < 4


@pytest.mark.parametrize("weights,tau", C.MODES + (("unit", C.TAU_B_F32),), ids=lambda v: str(v))
@pytest.mark.parametrize("ladder", C.LADDERS, ids=repr)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_oracle_against_long_double(layout, ladder, weights, tau):
    """Forward per (row, column) and key gradient per entry of the float64 oracle within PIN of long double, for the column layout
    of the diagonal kernels (key column k at frequency k) and of the Cartesian ones (key columns 0 .. 2 at every frequency)."""
    cols, freqs = LAYOUTS[layout]
    rowptr = C.csr(ladder, weights)[0]
    K = C.cached_keys(ladder, weights, tau)[:, list(range(len(freqs)) if cols is None else cols)]
    out_ld, coef_ld = C.reference(ladder, weights, tau, freqs, cols=cols)
    out, gkey = oracle(ladder, weights, tau, cols, freqs)
    scale = C.forward_scale(K, rowptr, freqs)
    fwd = np.abs(out - out_ld).astype(np.float64) / np.maximum(np.abs(out_ld).astype(np.float64), ZERO_LINE_FLOOR * scale + 1e-300)
    cscale = np.repeat(C.forward_scale(np.ones_like(K), rowptr, freqs), np.diff(rowptr), axis=0)
    lm = np.maximum(line_maxima(coef_ld.astype(np.float64), rowptr), ZERO_LINE_FLOOR * cscale)
    ent = np.abs(gkey - coef_ld).astype(np.float64) / lm
    print("%r %s tau %g: forward per column max " % (ladder, weights, tau) + " ".join("%g: %.1e" % (x, e) for x, e in zip(freqs, fwd.max(axis=0))))
    print("   key gradient per entry, per column max " + " ".join("%g: %.1e" % (x, e) for x, e in zip(freqs, ent.max(axis=0))))
    r, k = np.unravel_index(fwd.argmax(), fwd.shape)
    assert fwd.max() <= PIN, ("forward", ladder.degrees[r], freqs[k], float(fwd.max()))
    assert ent.max() <= PIN, ("key gradient", freqs[int(ent.max(axis=0).argmax())], float(ent.max()))


@pytest.mark.parametrize("ladder", C.LADDERS, ids=repr)
def test_float32_pad_weight_leaves_the_bound(ladder):
    """float64 forward with the pad weight rounded to float32 against long double: above TOL somewhere in every xi >= 511 column of the
    'deficient' mode (and of tau = 3.3 on the rows of 1 .. 3 neighbours), inside TOL at the control 0.37; with the exact pad
    weight, and in the mode without a pad, inside TOL everywhere."""
    big = np.array([abs(x) >= 511 for x in C.FREQS])
    ctrl = np.array([x == C.CONTROL_FREQS[0] for x in C.FREQS])
    f32 = lambda p: np.float64(np.float32(p))
    for weights, tau in C.MODES[1:]:
        rowptr = C.csr(ladder, weights)[0]
        K = C.cached_keys(ladder, weights, tau)
        floor = ZERO_LINE_FLOOR * C.forward_scale(K, rowptr, C.FREQS) + 1e-300
        ref = C.reference(ladder, weights, tau)[0]
        err = {}
        for name, fn in (("exact", None), ("float32", f32)):
            out = C.reference(ladder, weights, tau, pad_weight=fn, dtype=np.float64)[0]
            err[name] = np.abs(out - ref).astype(np.float64) / np.maximum(np.abs(ref).astype(np.float64), floor)
        print("%r %s tau %g: float32 pad, per column max " % (ladder, weights, tau) +
              " ".join("%g: %.1e" % (x, e) for x, e in zip(C.FREQS, err["float32"].max(axis=0))) + " | exact pad max %.1e" % err["exact"].max())
        assert err["exact"].max() <= TOL
        padded = np.array([d > 0 and (weights == "deficient" or (weights == "unit" and d < tau)) for d in ladder.degrees])
        if weights == "full":
            assert np.array_equal(err["float32"], err["exact"])           # no pad weight: nothing to round
        if not padded.any():
            continue
        over = err["float32"][padded][:, big].max(axis=0) > TOL
        assert over.all() if weights == "deficient" else over.any(), (weights, tau)      # three padded rows in all at tau = 3.3
        assert err["float32"][:, ctrl].max() <= TOL
        assert err["float32"][~padded].max() <= TOL
