"""The segmented-cumsum case generators (tests/segcumsum_cases.py) checked on the host: the exact reference against the oracle,
the bound that makes every summation order exact, and that each family places its boundaries where it says."""
import time

import numpy as np
import pytest

from oracle import fsw_oracle as O
from tests import segcumsum_cases as S

KEYS = sorted(S.GEOMETRIES)                       # the four (value type, id type) geometries


def geom(key):
    return S.geometry(*S.GEOMETRIES[key])


def small_cases(key):
    """every case of the small families for one geometry (runs up to 2 tiles per segment)"""
    g, vdt = geom(key), key[0]
    out = [S.single_head(p, g, vdt) for p in S.single_head_positions(g)]
    out += [S.single_head(p, g, vdt, n=3 * g.TILE + 8) for p in S.single_head_positions(g)]
    out += [S.runs(L, sh, g, vdt) for L in S.run_lengths(g) if L <= 2 * g.TILE for sh in S.run_shifts(g)]
    out += S.sizes(g, vdt) + S.sizes(g, vdt, kind="int")
    out += S.id_patterns(g, vdt, wide=key[1] == "int64")
    return out


def test_geometry_table():
    assert [geom(k) for k in KEYS] == [(4, 256, 1024, 4096), (2, 128, 1024, 4096), (2, 128, 512, 2048), (2, 128, 512, 2048)]


@pytest.mark.parametrize("key", KEYS, ids="-".join)
def test_exact_reference_equals_the_oracle(key):
    """The integer reference and the oracle's left-to-right floating sum agree to the bit on dyadic values, both directions."""
    for c in small_cases(key):
        assert c.values.dtype.name == key[0] and c.ids.dtype == np.int64
        S.assert_exact(c.values, c.ids)
        assert np.array_equal(S.exact_segcumsum(c.values, c.ids), O.segcumsum(c.values, c.ids)), c.name
        rev = O.segcumsum(c.values[::-1].copy(), c.ids[::-1].copy())[::-1]
        assert np.array_equal(S.exact_segcumsum(c.values, c.ids, reverse=True), rev), c.name
        S.assert_exact(c.values[::-1], c.ids[::-1])


def test_exact_reference_by_hand():
    v = np.array([1, 2, -1, 0.5, 0.25, 4, 1], dtype=np.float32)
    ids = np.array([5, 5, 9, 9, 5, 5, 5])
    assert S.exact_segcumsum(v, ids).tolist() == [1, 3, -1, -0.5, 0.25, 4.25, 5.25]
    assert S.exact_segcumsum(v, ids, reverse=True).tolist() == [3, 2, -0.5, 0.5, 5.25, 5, 1]
    assert S.exact_segcumsum(v[:0], ids[:0]).shape == (0,)
    with pytest.raises(AssertionError):
        S.exact_segcumsum(np.array([0.1]), np.array([0]))              # not dyadic
    with pytest.raises(AssertionError):
        S.assert_exact(np.full(2 ** 14, 1025.0 / 1024, dtype=np.float32), np.zeros(2 ** 14))   # 2^14 * 1025 units >= 2^24


@pytest.mark.parametrize("key", KEYS, ids="-".join)
def test_long_runs_and_nonfinite_satisfy_the_bound(key):
    g, vdt = geom(key), key[0]
    for L in S.run_lengths(g):
        if L > 2 * g.TILE:
            for sh in S.run_shifts(g):
                c = S.runs(L, sh, g, vdt)
                S.assert_exact(c.values, c.ids)
                assert S.longest_segment(c.ids) == L and len(c.ids) >= sh % L + 2 * L + 3
                if vdt == "float32":
                    assert np.abs(c.values).max() * 1024 >= 32          # still fractions of several bits, not zeros
    assert max(len(S.runs(L, 0, g, vdt).ids) for L in S.run_lengths(g)[-1:]) <= 131 * g.TILE
    for kind in S.NONFINITE_KINDS:
        c, want = S.nonfinite(kind, g, vdt)
        fin = np.isfinite(c.values)
        S.assert_exact(c.values, c.ids, finite_only=fin)
        assert np.array_equal(~fin & c.marked, ~fin) and (~fin).sum() == (8 if kind == "minus_inf_plus_inf" else 4)
        heads = S.segment_heads(c.ids)
        spans = S.nonfinite_segments(g)
        for a, b in spans.values():                                    # exactly one segment each
            assert heads[a] and heads[b] and not heads[a + 1:b].any() and c.marked[a:b].all()
        assert c.marked.sum() == sum(b - a for a, b in spans.values())
        a, b = spans["ends_on_tile_end"]
        assert b % g.TILE == 0
        a, b = spans["spans_tile_boundary"]
        assert a // g.TILE + 1 == (b - 1) // g.TILE
        a, b = spans["spans_over_64_tiles"]
        assert (b - 1) // g.TILE - a // g.TILE > 64
        a, b = spans["inside_halo_group"]
        assert g.TILE - g.GRP < a and b < g.TILE
        # outside the marked segments the expectation is finite and is the exact reference of the finite values
        assert np.isfinite(want[~c.marked]).all()
        assert np.array_equal(want[~c.marked], S.exact_segcumsum(np.where(fin, c.values, 0).astype(c.values.dtype), c.ids)[~c.marked])
        for a, b in spans.values():
            assert np.isfinite(want[a]) and not np.isfinite(want[a + 1:b]).any()
            assert np.isnan(want[b - 1]) == (kind != "inf")


@pytest.mark.parametrize("key", KEYS, ids="-".join)
def test_families_place_what_they_claim(key):
    g, vdt = geom(key), key[0]
    E, G, W, T = g
    pos = S.single_head_positions(g)
    assert {T - G, T - G + 1, T - 1, T, W, G, E, 2 * T, 3 * T + 4} <= set(pos)
    for p in pos:
        c = S.single_head(p, g, vdt)
        assert len(c.ids) == 3 * T + 5 and np.nonzero(S.segment_heads(c.ids))[0].tolist() == [0, p]
    # the halo of tile 1 is [T - G, T): its first element (deliberately "no head") and its second
    assert np.nonzero(S.segment_heads(S.single_head(T - G, g, vdt).ids))[0][1] - (T - G) == 0
    assert np.nonzero(S.segment_heads(S.single_head(T - G + 1, g, vdt).ids))[0][1] - (T - G) == 1
    for L in S.run_lengths(g):
        for sh in S.run_shifts(g):
            c = S.runs(L, sh, g, vdt, align_n=E) if L <= 2 * T else None
            if c is None:
                continue
            h = np.nonzero(S.segment_heads(c.ids))[0]
            lens = np.diff(np.append(h, len(c.ids)))
            lead = sh % L
            assert len(c.ids) % E == 0 and len(c.ids) > 2 * T
            assert (lens[0] == lead if lead else lens[0] == L) and (lens[1:-1] == L).all() and lens[-1] <= L and len(lens) >= 3
    assert {1, E, G - 1, G, G + 1, W, T - 1, T, T + 1, 2 * T, 64 * T, 64 * T + 1, 65 * T} == set(S.run_lengths(g))
    assert {1, 2, E, E + 1, G, T - 1, T, T + 1, 2 * T - 1, 2 * T + E} <= set(S.size_list(g))
    cs = S.sizes(g, vdt)
    assert sorted(len(c.ids) for c in cs) == sorted(2 * S.size_list(g))
    for c in cs:
        h = S.segment_heads(c.ids)
        assert h.sum() == 1 if c.name.endswith("one)") else np.array_equal(np.nonzero(h)[0], np.arange(0, len(h), 3))
    # id patterns: every relabelling keeps the layout's heads; what each one claims
    pats = {c.name: c for c in S.id_patterns(g, vdt, wide=key[1] == "int64")}
    assert len(pats) == (8 if key[1] == "int64" else 6)
    for layout in ("mean10", "all_heads"):
        ref_heads = S.segment_heads(pats["ids(%s,abab)" % layout].ids)
        assert ref_heads.sum() == len(ref_heads) if layout == "all_heads" else 0.07 < ref_heads.mean() < 0.14
        for name, c in pats.items():
            if layout in name:
                assert np.array_equal(S.segment_heads(c.ids), ref_heads), name
        labels = pats["ids(%s,abab)" % layout].ids[ref_heads]
        assert set(labels.tolist()) == {3, 7} and (labels[2:] == labels[:-2]).all()          # A B A: an id comes back
        labels = pats["ids(%s,negative_descending)" % layout].ids[ref_heads]
        assert (labels < 0).all() and (np.diff(labels) < 0).all()
        labels = pats["ids(%s,int32_extremes)" % layout].ids
        assert set(labels.tolist()) == set(S.INT32_EXTREMES) and np.array_equal(labels.astype(np.int32), labels)
        if key[1] == "int64":
            ids = pats["ids(%s,int64_halves)" % layout].ids
            a, b = ids[:-1][ref_heads[1:]], ids[1:][ref_heads[1:]]
            lo, hi = (a & 0xffffffff) != (b & 0xffffffff), (a >> 32) != (b >> 32)
            assert (lo & ~hi).any() and (hi & ~lo).any() and (lo & hi).any()
            if layout == "all_heads":
                # ... and each kind of neighbour at a lane boundary (EPL), a group boundary (GRP) and a chunk boundary (WCH)
                at = np.arange(1, len(ids))
                for step in (E, G, W):
                    for kind in (lo & ~hi, hi & ~lo):
                        assert (kind & (at % step == 0)).any()


def test_rounds_build_quickly_and_within_the_bound():
    g32, g64 = geom(("float32", "int64")), geom(("float64", "int64"))
    for grid in (768, 1536):
        for g, vdt in ((g32, "float32"), (g64, "float64")):
            for layout in S.ROUND_LAYOUTS:
                t0 = time.perf_counter()
                c = S.rounds(grid, g, vdt, layout)
                dt = time.perf_counter() - t0
                assert dt < 1.0, (grid, vdt, layout, dt)
                n = len(c.ids)
                assert n == (2 * grid + 3) * g.TILE + 5 and -(-n // g.TILE) >= 2 * grid + 3
                assert set(np.unique(c.values).tolist()) <= {-1.0, 0.0, 1.0}
                longest = S.longest_segment(c.ids)
                assert longest < 2 ** S.MANTISSA[vdt]                         # |v| <= 1: the bound, without the full pass
                if layout == "one_segment":
                    assert longest == n
                elif layout == "mean10":
                    assert 9 < n / S.segment_heads(c.ids).sum() < 11
                else:
                    assert 4000 < n / S.segment_heads(c.ids).sum() < 6000 and longest > g.TILE
    c = S.rounds(768, g32, "float32", "one_segment")
    S.assert_exact(c.values, c.ids)
    want = S.exact_segcumsum(c.values, c.ids)
    assert np.array_equal(want, np.cumsum(c.values.astype(np.float64)).astype(np.float32))
    with pytest.raises(ValueError):
        S.rounds(2047, g32, "float32", "one_segment")                         # 4097 tiles of 4096 > 2^24 elements
    assert S.rounds_size(2046, g32) < 2 ** 24 <= S.rounds_size(2047, g32)
