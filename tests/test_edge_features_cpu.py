"""The claims the edge-feature kernel tests rest on (tests/test_hip_edge_features.py), checked without a GPU: the keys are exact in
float32 in every order of evaluation, the control column is distinct inside every row, the tie columns tie, and every row of the
degree ladder lands in the degree bin (include/fsw_hip.h) it is meant for."""
import numpy as np
import pytest

from tests import edge_feature_cases as EC
from tests.test_hip_ties import DEGREES

LADDER = DEGREES + (16384, 16385)
# the class every boundary row is meant for: the forward kernels of embed_wsort.hip change class at 128/129, 256/257, 512/513,
# 1024/1025, 2048/2049 and then per hub bin; the weighted backward also at 192/193 (bins mid192 / mid256)
INTENDED = {0: "reg0", 1: "reg1", 32: "reg32", 33: "mid40", 40: "mid40", 41: "mid48", 64: "mid64", 65: "mid80", 128: "mid128",
            129: "mid160", 192: "mid192", 193: "mid256", 255: "mid256", 256: "mid256", 257: "lds0", 511: "lds0", 512: "lds0",
            513: "lds1", 1023: "lds1", 1024: "lds1", 1025: "lds2", 2047: "lds2", 2048: "lds2", 2049: "hub0", 4096: "hub0",
            4097: "hub1", 9000: "hub2", 16384: "hub2", 16385: "hub3", 32768: "hub3", 32769: "global"}


def ladder_case(d_edge, S, degrees=LADDER):
    rec, snd, w, ef = EC.edge_list(degrees, d_edge)
    order = EC.csr_order(rec, snd)
    rowptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    assert np.array_equal(rec[order], np.repeat(np.arange(len(degrees)), degrees))
    ef, w = ef[order], w[order]
    Ve = EC.slice_vectors(S, d_edge)
    term = EC.edge_term(ef, Ve)
    return rowptr, w, ef, Ve, term, EC.xp_columns(rowptr, term)


@pytest.mark.parametrize("d_edge,S", [(1, 13), (3, 13), (5, 13), (3, 27)])
def test_keys_are_exact_in_every_order_of_evaluation(d_edge, S):
    rowptr, w, ef, Ve, term, xp = ladder_case(d_edge, S)
    assert np.array_equal(ef, np.round(ef * 4) / 4) and np.abs(ef).max() <= 2 and np.abs(ef).max() == 2
    assert np.array_equal(Ve, np.round(Ve * 8) / 8) and np.abs(Ve).max() <= 1
    assert np.array_equal(xp, np.round(xp * 64) / 64) and np.abs(xp).max() <= 512
    k64 = xp.astype(np.float64) + term
    fwd, rev = EC.keys_float32(xp, ef, Ve), EC.keys_float32(xp, ef, Ve, reverse=True)
    assert fwd.dtype == np.float32 and np.array_equal(fwd, rev)
    assert np.array_equal(fwd.astype(np.float64), k64)             # -0.0 == +0.0 here, as in the kernels' comparisons
    # one fused multiply-add per q in float64 arithmetic rounded to float32 once: the same values again
    fma = xp.astype(np.float64)
    for q in range(d_edge):
        fma = (fma + ef[:, q].astype(np.float64)[:, None] * Ve[:, q].astype(np.float64)[None, :]).astype(np.float32).astype(np.float64)
    assert np.array_equal(fma, k64)


@pytest.mark.parametrize("d_edge", [1, 5])
def test_columns_are_what_their_names_say(d_edge):
    S = 13
    rowptr, w, ef, Ve, term, xp = ladder_case(d_edge, S)
    keys = xp.astype(np.float64) + term
    names = EC.kinds(S)
    assert set(names) == set(EC.KIND_CYCLE)
    for c, kind in enumerate(names):
        for a, b in zip(rowptr[:-1], rowptr[1:]):
            if b - a < 2:
                continue
            distinct = np.unique(keys[a:b, c]).size
            if kind in ("e", "zero_ve"):
                assert distinct == b - a, (kind, b - a)            # the control really is distinct inside every row
            elif kind == "cancel":
                assert distinct == (b - a + 1) // 2, (kind, b - a)     # pairs tie on the sum ...
                if b - a >= 64:                                        # ... and only on the sum: the Xp of most pairs differ
                    n2 = (b - a) // 2 * 2
                    assert (xp[a:a + n2:2, c] != xp[a + 1:a + n2:2, c]).mean() > 0.5
            elif kind in ("d_up", "d_down"):                           # these kinds describe Xp; the edge term splits the runs
                assert np.unique(xp[a:b, c]).size == (b - a + 2) // 3
            elif kind == "a" and b - a >= 64:                          # constant Xp: the keys take the few values of the edge term
                assert distinct <= min(17 ** d_edge, 641) and distinct < b - a
        if kind == "zero_ve":
            assert not Ve[c].any() and np.array_equal(keys[:, c], xp[:, c].astype(np.float64))
        else:
            assert Ve[c].any()
    assert (w == 0).sum() >= 30
    for deg in EC.LOW_MASS_ROWS:
        r = LADDER.index(deg)
        assert abs(w[rowptr[r]:rowptr[r + 1]].astype(np.float64).sum() - 0.4) < 1e-5
    fr = EC.freqs(S)
    assert (fr == 0).sum() == 2 and np.signbit(fr[fr == 0]).sum() == 1 and (fr == -1).sum() == 1 and (fr < -0.1).sum() == 3


def test_every_ladder_row_lands_in_its_degree_bin():
    names = EC.bin_names()
    from fsw_gnn_amd import _lib
    assert len(names) == _lib.NUM_BINS
    for d in LADDER + (32768, 32769):
        assert names[EC.bin_of(d)] == INTENDED.get(d, names[EC.bin_of(d)]), d
    for d in (32, 33, 128, 129, 192, 193, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 16384, 16385):
        assert d in LADDER and d in INTENDED                        # both sides of every class boundary are rows of the ladder
    rows = EC.bin_rows(LADDER)
    assert sum(rows) == len(LADDER)
    assert rows[_lib.BIN_MID0:] == [2, 1, 1, 1, 0, 1, 1, 1, 3, 3, 3, 3, 2, 1, 2, 1, 0]    # mid, LDS, hub bins, global
    assert EC.bin_rows((0, 5, 32769))[-1] == 1
