"""Case generators and an exact reference for the segmented cumulative sum (numpy only: no GPU, no torch).

Every value is dyadic and every segment is short enough that ANY order of summation is exact in the value type: all values of
a case are integer multiples of one power of two (the case's unit), and the sum of |value| over each segment stays below
2^24 units (float32) or 2^53 units (float64).  Every partial sum of elements of one segment, in whatever grouping a tree, a
chain, the halo or the look-back forms it, is then an integer below 2^mantissa units and is representable; all orders give the
same bits and a kernel's output is compared with `np.array_equal`, no tolerance.  `assert_exact` checks the bound.

Segment boundaries are placed from the kernel's geometry (EPL elements per lane and load, GRP = 64 * EPL elements per group
and halo, WCH elements per wavefront chunk, TILE elements per workgroup step), which the caller passes in: the GPU test reads
it from the library, the CPU test uses the table below.
"""
import collections

import numpy as np

Geometry = collections.namedtuple("Geometry", "EPL GRP WCH TILE")
Case = collections.namedtuple("Case", "name values ids marked")   # marked: bool mask of the non-finite segments, or None


def geometry(epl, grp, tile):
    """The kernel's tile shape; a tile is four wavefront chunks."""
    assert tile % 4 == 0 and grp == 64 * epl and (tile // 4) % grp == 0
    return Geometry(int(epl), int(grp), int(tile) // 4, int(tile))


# (value type, id type) -> (EPL, GRP, TILE) of k_segscan_chained; the GPU test asserts that the library reports exactly these
GEOMETRIES = {
    ("float32", "int32"): (4, 256, 4096),
    ("float32", "int64"): (2, 128, 4096),
    ("float64", "int32"): (2, 128, 2048),
    ("float64", "int64"): (2, 128, 2048),
}
MANTISSA = {"float32": 24, "float64": 53}
_FIX = 30   # every generated value is a multiple of 2^-30


# ---- exact reference -------------------------------------------------------------------------------------------------
def segment_heads(ids):
    """heads[i]: element i starts a segment (element 0 does; later ones when their id differs from the neighbour's)."""
    ids = np.asarray(ids)
    heads = np.ones(ids.shape[0], dtype=bool)
    heads[1:] = ids[1:] != ids[:-1]
    return heads


def _fixed(values):
    """values as int64 multiples of 2^-30 (asserts that they are)"""
    v = np.asarray(values, dtype=np.float64)
    k = np.rint(np.ldexp(v, _FIX))
    assert np.array_equal(np.ldexp(k, -_FIX), v), "values must be finite multiples of 2^-30"
    assert np.abs(k).max(initial=0) < 2.0 ** 40
    return k.astype(np.int64)


def exact_segcumsum(values, ids, reverse=False):
    """Inclusive segmented scan by integer arithmetic: the int64 cumulative sum minus its value before the segment's head.
    Returns the values' dtype; exact whenever `assert_exact` holds.  reverse: the same on the flipped arrays."""
    values = np.asarray(values)
    ids = np.asarray(ids)
    if reverse:
        return exact_segcumsum(values[::-1], ids[::-1])[::-1].copy()
    if values.shape[0] == 0:
        return values.copy()
    k = _fixed(values)
    c = np.cumsum(k)                                    # |c| < 2^40 * 2^24: no overflow
    heads = segment_heads(ids)
    before = np.where(heads, c - k, 0)[heads]           # cumulative sum just before each head
    seg = np.cumsum(heads) - 1
    r = c - before[seg]
    assert np.abs(r).max() < 2 ** 53
    out = np.ldexp(r.astype(np.float64), -_FIX).astype(values.dtype)
    assert np.array_equal(np.rint(np.ldexp(out.astype(np.float64), _FIX)).astype(np.int64), r), "result not representable"
    return out


def segment_abs_sums(values, ids):
    """(sum of |value| over each segment in units of 2^-30, the case's unit in the same units)"""
    k = np.abs(_fixed(values))
    heads = segment_heads(ids)
    sums = np.add.reduceat(k, np.nonzero(heads)[0]) if k.size else k
    nz = k[k != 0]
    unit = int(np.bitwise_or.reduce(nz) & -np.bitwise_or.reduce(nz)) if nz.size else 1   # lowest set bit of all values
    return sums, unit


def assert_exact(values, ids, finite_only=None):
    """The bound that makes every summation order exact: per segment, sum |v| < 2^mantissa units."""
    values = np.asarray(values)
    if finite_only is not None:
        values = np.where(finite_only, values, 0)
    sums, unit = segment_abs_sums(values, ids)
    limit = 2 ** MANTISSA[values.dtype.name]
    worst = int(sums.max(initial=0))
    assert worst < limit * unit, "segment of %d units of 2^-30 exceeds %d * %d" % (worst, limit, unit)


# ---- values ------------------------------------------------------------------------------------------------------------
def longest_segment(ids):
    h = np.nonzero(segment_heads(ids))[0]
    return int(np.diff(np.append(h, len(ids))).max(initial=0))


def dyadic_values(rng, ids, vdtype, kind=None):
    """Values for the layout `ids`.  kind:
      'int'   integers in {-2 .. 2};
      'sign'  {-1, 0, 1};
      'frac'  multiples of 2^-10 up to 2 in magnitude, fewer where the longest segment needs it (a kernel that truncates shows);
      'fine'  float64 only: k * 2^-30 with |k| < 2^20, so that sums fill both 32-bit halves of a double.
    Default: 'frac' for float32, 'fine' for float64."""
    n = len(ids)
    kind = kind or ("fine" if vdtype == "float64" else "frac")
    if kind in ("int", "sign"):     # unit 1: the bound is (largest magnitude) * (longest segment) < 2^mantissa
        top = 2 if kind == "int" else 1
        assert top * longest_segment(ids) < 2 ** MANTISSA[vdtype]
        return rng.integers(-top, top + 1, size=n, dtype=np.int8).astype(vdtype)
    if kind == "frac":
        kmax = max(1, min(2048, (2 ** MANTISSA[vdtype] - 1) // max(1, longest_segment(ids))))
        v = np.ldexp(rng.integers(-kmax, kmax + 1, size=n).astype(np.float64), -10).astype(vdtype)
    elif kind == "fine":
        assert vdtype == "float64"
        v = np.ldexp(rng.integers(-(2 ** 20) + 1, 2 ** 20, size=n).astype(np.float64), -30)
    else:
        raise ValueError(kind)
    assert_exact(v, ids)
    return v


def _case(name, rng, ids, vdtype, kind=None):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    return Case(name, dyadic_values(rng, ids, vdtype, kind), ids, None)


def random_heads(rng, n, mean):
    """Head mask with geometric segment lengths of the given mean (element 0 is a head)."""
    m = int(n / mean * 1.2) + 16
    pos = np.cumsum(rng.geometric(1.0 / mean, size=m))
    while pos[-1] < n:
        pos = np.concatenate([pos, pos[-1] + np.cumsum(rng.geometric(1.0 / mean, size=m))])
    heads = np.zeros(n, dtype=bool)
    heads[0] = True
    heads[pos[pos < n]] = True
    return heads


# ---- case families -----------------------------------------------------------------------------------------------------
def single_head_positions(g):
    E, G, W, T = g
    p = [1, E - 1, E, E + 1, G - 1, G, G + 1, W - 1, W, W + 1, T - G - 1, T - G, T - G + 1, T - G + E, T - E, T - 1, T, T + 1,
         T + G, 2 * T - G, 2 * T - G + 1, 2 * T - 1, 2 * T, 3 * T, 3 * T + 4]
    return sorted(set(p))


def single_head(p, g, vdtype, n=None, seed=0):
    """Two segments: [0, p) and [p, n).  n = 3 * TILE + 5 unless given."""
    n = 3 * g.TILE + 5 if n is None else n
    assert 0 < p < n
    ids = np.zeros(n, dtype=np.int64)
    ids[p:] = 1
    return _case("single_head(p=%d,n=%d)" % (p, n), np.random.default_rng([11, seed, p, n]), ids, vdtype)


def run_lengths(g):
    E, G, W, T = g
    return sorted(set([1, E, G - 1, G, G + 1, W, T - 1, T, T + 1, 2 * T, 64 * T, 64 * T + 1, 65 * T]))


def run_shifts(g):
    return [0, 1, g.GRP - 1]


def runs(L, shift, g, vdtype, kind=None, align_n=1, seed=0):
    """Segments of length L, the first one cut to `shift % L` elements (0: not cut).  At least two whole segments and a
    ragged tail, at least two and a half tiles; n is rounded up to a multiple of align_n."""
    assert L >= 1 and 0 <= shift
    lead = shift % L
    n = max(lead + 2 * L, 2 * g.TILE) + g.TILE // 2 + 3
    n = -(-n // align_n) * align_n
    i = np.arange(n, dtype=np.int64)
    ids = (i + (L - lead if lead else 0)) // L
    return _case("runs(L=%d,shift=%d,n=%d)" % (L, shift, n), np.random.default_rng([12, seed, L, shift]), ids, vdtype, kind)


def size_list(g):
    E, G, W, T = g
    return sorted(set(n for n in (1, 2, E - 1, E, E + 1, G, T - 1, T, T + 1, 2 * T - 1, 2 * T + E) if n >= 1))


def sizes(g, vdtype, kind=None, seed=0):
    """Every n of size_list in two id layouts: one segment, and a head every 3 elements."""
    out = []
    for n in size_list(g):
        rng = np.random.default_rng([13, seed, n])
        out.append(_case("sizes(n=%d,one)" % n, rng, np.zeros(n, dtype=np.int64), vdtype, kind))
        out.append(_case("sizes(n=%d,every3)" % n, rng, np.arange(n, dtype=np.int64) // 3, vdtype, kind))
    return out


INT32_EXTREMES = (-2 ** 31, -1, 0, 2 ** 31 - 1)
# consecutive labels (cyclically) differ in the low half only, the high half only, or both
INT64_HALVES = (0, 1, 2 ** 32 + 1, 2 ** 32, 2 ** 33, 1, 2 ** 32)


def id_patterns(g, vdtype, wide, seed=0):
    """Two layouts -- random segments of mean length 10, and every element its own segment -- relabelled so that the label of
    segment s is: alternating A B A B; negative and descending; the int32 extremes in turn; and, when `wide` (int64 ids),
    labels whose neighbours differ in one 32-bit half only."""
    n = 2 * g.TILE + 77
    out = []
    for layout in ("mean10", "all_heads"):
        rng = np.random.default_rng([14, seed, layout == "mean10"])
        heads = random_heads(rng, n, 10.0) if layout == "mean10" else np.ones(n, dtype=bool)
        s = np.cumsum(heads) - 1
        labels = {
            "abab": np.array([7, 3])[s % 2],
            "negative_descending": -5 * s - 1,
            "int32_extremes": np.array(INT32_EXTREMES, dtype=np.int64)[s % 4],
        }
        if wide:
            labels["int64_halves"] = np.array(INT64_HALVES, dtype=np.int64)[s % len(INT64_HALVES)]
        for name, ids in labels.items():
            assert np.array_equal(segment_heads(ids), heads)
            out.append(_case("ids(%s,%s)" % (layout, name), rng, ids, vdtype))
    return out


NONFINITE_KINDS = ("inf", "minus_inf_plus_inf", "nan")
NONFINITE_PLACES = ("ends_on_tile_end", "spans_tile_boundary", "spans_over_64_tiles", "inside_halo_group")


def nonfinite_segments(g):
    """{place: (first, one past last)} of the four marked segments"""
    E, G, W, T = g
    return {
        "inside_halo_group": (T - G + 3, T - G + 11),
        "ends_on_tile_end": (2 * T - 9, 2 * T),
        "spans_tile_boundary": (3 * T - 5, 3 * T + 6),
        "spans_over_64_tiles": (4 * T + 11, 69 * T + 20),
    }


def nonfinite(kind, g, vdtype, seed=0):
    """Random segments of mean length 10 with four marked segments (nonfinite_segments) that hold +inf, -inf followed by +inf
    (NaN from there on), or NaN; dyadic values elsewhere.  Returns (case, expected): expected is numpy's own cumsum per marked
    segment and the exact reference elsewhere."""
    n = 70 * g.TILE + 5
    rng = np.random.default_rng([15, seed, NONFINITE_KINDS.index(kind)])
    heads = random_heads(rng, n, 10.0)
    marked = np.zeros(n, dtype=bool)
    spans = nonfinite_segments(g)
    for a, b in spans.values():
        heads[a:b + 1] = False
        heads[a] = heads[b] = True
        marked[a:b] = True
    ids = np.cumsum(heads).astype(np.int64)
    v = dyadic_values(rng, ids, vdtype)
    finite = v.copy()
    for a, b in spans.values():
        if kind == "inf":
            v[a + 1] = np.inf
        elif kind == "nan":
            v[a + 1] = np.nan
        else:
            v[a + 1], v[a + 3] = -np.inf, np.inf
    expected = exact_segcumsum(np.where(np.isfinite(v), finite, 0).astype(v.dtype), ids)
    with np.errstate(invalid="ignore"):
        for a, b in spans.values():
            expected[a:b] = np.cumsum(v[a:b])
    return Case("nonfinite(%s)" % kind, v, ids, marked), expected


ROUND_LAYOUTS = ("mean10", "one_segment", "mean5000")


def rounds_size(grid, g):
    return (2 * grid + 3) * g.TILE + 5


def rounds(grid, g, vdtype, layout, seed=0):
    """n = (2 * grid + 3) * TILE + 5 elements, so that each of `grid` workgroups walks at least three tiles.  Values in
    {-1, 0, 1}: one segment of n elements is exact while n < 2^24 (float32), and a larger grid is refused."""
    n = rounds_size(grid, g)
    if n >= 2 ** MANTISSA[vdtype]:
        raise ValueError("rounds(%d): one segment of %d elements in {-1, 0, 1} is not exact in %s" % (grid, n, vdtype))
    rng = np.random.default_rng([16, seed, ROUND_LAYOUTS.index(layout)])
    if layout == "one_segment":
        ids = np.zeros(n, dtype=np.int64)
    else:
        ids = np.cumsum(random_heads(rng, n, 10.0 if layout == "mean10" else 5000.0), dtype=np.int64)
    return _case("rounds(grid=%d,%s)" % (grid, layout), rng, ids, vdtype, "sign")
