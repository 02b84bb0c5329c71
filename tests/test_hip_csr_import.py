"""fsw_graph_import_csr (csrc/graph_import.hip) against its numpy restatement tests/csr_import_ref.py, at the library level: the device
arrays are compared exactly (the 'gcn' weights within the four roundings of their expression), bins and perm through
graph_ref.ref_bins / perm_mismatch.  The shapes are the smallest that reach every branch: every degree class with its cut, more
than one block of FSW_BIN_BLOCK_ROWS rows, rows above the 2048 entries from which a workgroup walks a row together, both index
widths, unit and dyadic weights (every sum exact), the identity columns of a readout, row chunks, self loops appended and merged,
and every malformed input -- which is only ever inspected on the host here: no embedding kernel is launched on it."""
import numpy as np
import pytest
import torch

from tests import csr_import_ref as C
from tests import graph_ref as R

pytestmark = pytest.mark.gpu
NB = R.NUM_BINS
IDX = {"int32": torch.int32, "int64": torch.int64}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def t(a, dev, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.to(device=dev, dtype=dtype) if dtype is not None else x.to(dev)


def host(x):
    return x.cpu().numpy()


def dyadic(rng, n):
    return (rng.integers(1, 4096, n) / 1024.0).astype(np.float32)


def run(dev, rowptr, col, w, rows, cols, idx="int64", **kw):
    from fsw_gnn_amd import import_csr
    return import_csr(t(rowptr, dev, IDX[idx]), None if col is None else t(col, dev, IDX[idx]), None if w is None else t(w, dev),
                      rows, cols, want_invperm=True, want_slots=True, **kw)


def check(gr, ref, chunk_rows=0, gcn=False):
    """Every output array of an import against the restatement."""
    st = host(gr.stats_dev).tolist()
    nnz = ref["nnz"]
    assert st[R.STAT_FLAGS] == ref["flags"], (st[R.STAT_FLAGS], ref["flags"])
    assert st[R.STAT_NNZ] == nnz
    assert np.array_equal(host(gr.rowptr), ref["rowptr"])
    assert np.array_equal(host(gr.col[:nnz]), ref["col"])
    if ref["w"] is None:
        assert gr.w is None
    elif gcn:
        got, want = host(gr.w[:nnz]).astype(np.float64), ref["w64"]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin)
        # sqrt, sqrt, division, division: four roundings of at most 2^-23 relative each (the dyadic degree sums are exact)
        assert bool((np.abs(got[fin] - want[fin]) <= 2.0 ** -21 * np.abs(want[fin])).all()), np.abs(got[fin] / want[fin] - 1).max()
    else:
        assert np.array_equal(host(gr.w[:nnz]).view(np.int32), ref["w"].view(np.int32))
    if ref["slot"] is not None and ref["slot"].size:
        assert np.array_equal(host(gr.slot_of_edge[:ref["slot"].size]), ref["slot"])
    bins = R.ref_bins(ref["rowptr"], chunk_rows)
    bs = host(gr.bin_start).reshape(-1, NB + 1)
    assert np.array_equal(bs, bins["bin_start"])
    for word, want in bins["stats"].items():
        assert st[word] == want, (word, st[word], want)
    perm = host(gr.perm)
    bad = R.perm_mismatch(perm, bins, chunk_rows)
    assert bad is None, bad
    assert np.array_equal(host(gr.invperm)[perm], np.arange(perm.size))
    return st


# ---- every degree class, two blocks of rows -------------------------------------------------------------------------------------
CUTS = [0, 1, 32, 33, 40, 41, 256, 257, 2048, 2049, 4096, 4097, 32_768, 32_769]


def degree_case():
    def make():
        rng = np.random.default_rng(5)
        rows = 2040 + len(CUTS)
        deg = rng.integers(0, 4, rows)
        deg[:len(CUTS)] = CUTS
        deg = deg[rng.permutation(rows)]
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        col = rng.integers(0, rows, int(rowptr[-1])).astype(np.int64)
        return rows, rowptr, col, dyadic(rng, col.size)
    return cached("degrees", make)


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "dyadic"])
@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_plain_import_every_degree_class(dev, idx, weighted):
    rows, rowptr, col, w = degree_case()
    assert rows == 2054 > 2048 and 80_000 < col.size < 85_000
    ref = C.ref_import(rowptr, col, w if weighted else None, rows, rows)
    assert len(set(R.ref_bins(ref["rowptr"])["bin_of_row"].tolist())) == 14 and ref["flags"] == (C.FLAG_W_NONUNIT if weighted else 0)
    st = check(run(dev, rowptr, col, w if weighted else None, rows, rows, idx), ref)
    assert st[R.STAT_MAX_DEGREE] == 32_769


@pytest.mark.parametrize("gcn", [False, True], ids=["loops", "loops_gcn"])
@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_appended_loops_and_gcn_every_degree_class(dev, idx, gcn):
    """The row-cooperative copy: rows of up to 2048 entries by 8 lanes, the five longer ones by their whole workgroup."""
    rows, rowptr, col, w = degree_case()
    ref = C.ref_import(rowptr, col, w, rows, rows, self_loop_weight=0.5, gcn=gcn)
    assert ref["nnz"] == col.size + rows and not ref["flags"] & ~C.FLAG_W_NONUNIT
    check(run(dev, rowptr, col, w, rows, rows, idx, self_loop_weight=0.5, gcn=gcn), ref, gcn=gcn)


def test_unit_input_with_loops_becomes_weighted(dev):
    rows, rowptr, col, _ = degree_case()
    ref = C.ref_import(rowptr, col, None, rows, rows, self_loop_weight=2.0)
    gr = run(dev, rowptr, col, None, rows, rows, self_loop_weight=2.0)
    check(gr, ref)
    w = host(gr.w[:ref["nnz"]])
    assert set(np.unique(w).tolist()) == {1.0, 2.0} and int((w == 2.0).sum()) == rows


# ---- small and odd shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2049])
@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_import_without_entries(dev, rows, idx):
    rowptr = np.zeros(rows + 1, dtype=np.int64)
    col = np.zeros(0, dtype=np.int64)
    for kw in (dict(), dict(self_loop_weight=0.5), dict(self_loop_weight=0.5, strict_cols=True), dict(gcn=True)):
        ref = C.ref_import(rowptr, col, None, rows, rows, self_loop_weight=kw.get("self_loop_weight", 0.0), gcn=kw.get("gcn", False),
                           strict=kw.get("strict_cols", False))
        assert ref["nnz"] == (rows if "self_loop_weight" in kw else 0)
        check(run(dev, rowptr, col, None, rows, rows, idx, **kw), ref, gcn=kw.get("gcn", False))


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_rectangle_5_by_3(dev, idx):
    rowptr = np.array([0, 3, 3, 4, 9, 10], dtype=np.int64)
    col = np.array([2, 0, 2, 1, 0, 1, 2, 2, 0, 1], dtype=np.int64)
    w = (np.arange(1, 11) / 8.0).astype(np.float32)
    for ww in (None, w):
        check(run(dev, rowptr, col, ww, 5, 3, idx), C.ref_import(rowptr, col, ww, 5, 3))
    strict_col = np.array([0, 1, 2, 1, 0, 1, 2, 2, 0, 1], dtype=np.int64)          # row 3 = [0, 1, 2, 2, 0]: not increasing
    ref = C.ref_import(rowptr, strict_col, w, 5, 3, strict=True)
    assert ref["flags"] & C.BAD == C.FLAG_CSR_COL_ORDER
    gr = run(dev, rowptr, strict_col, w, 5, 3, idx, strict_cols=True)
    assert gr.flags & C.BAD == C.FLAG_CSR_COL_ORDER and gr.stats()[R.STAT_NNZ] == 0


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_identity_columns_of_a_readout(dev, idx):
    """col_in = NULL: segments of 0, 1, 2048, 2049 and 33 000 consecutive vertices."""
    seg = np.array([0, 1, 2048, 0, 2049, 33_000, 0], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(seg)])
    n = int(rowptr[-1])
    ref = C.ref_import(rowptr, None, None, seg.size, n)
    assert np.array_equal(ref["col"], np.arange(n)) and ref["flags"] == 0
    gr = run(dev, rowptr, None, None, seg.size, n, idx)
    st = check(gr, ref)
    assert gr.w is None and st[R.STAT_MAX_DEGREE] == 33_000 and st[R.STAT_NUM_ZERO] == 3


@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_row_chunks_of_2048(dev, idx):
    rows, chunk = 5 * 2048 + 77, 2048

    def make():
        rng = np.random.default_rng(9)
        deg = rng.integers(0, 8, rows)
        deg[rng.choice(rows, 6, replace=False)] = [33, 300, 2100, 40, 257, 4097]
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        return rowptr, rng.integers(0, rows, int(rowptr[-1])).astype(np.int64)
    rowptr, col = cached("chunks", make)
    ref = C.ref_import(rowptr, col, None, rows, rows)
    gr = run(dev, rowptr, col, None, rows, rows, idx, chunk_rows=chunk)
    assert gr.num_chunks == 6
    check(gr, ref, chunk_rows=chunk)
    perm, bs = host(gr.perm), host(gr.bin_start)
    for c in range(6):
        assert np.array_equal(np.sort(perm[bs[c, 0]:bs[c, NB]]), np.arange(c * chunk, min((c + 1) * chunk, rows)))


# ---- self loops on n = 2049: appended and strict --------------------------------------------------------------------------------
def strict_case(n, long_rows):
    """Strictly increasing columns; row r by r % 5: 0 empty, 1 the diagonal first, 2 the diagonal last, 3 no diagonal (columns on
    both sides where there are any), 4 the diagonal in the middle.  long_rows: {row: with_diagonal} rows that hold every column
    (but their own, without the diagonal)."""
    def make():
        rng = np.random.default_rng(n)
        rows_cols = []
        for r in range(n):
            below, above = np.arange(0, r), np.arange(r + 1, n)
            pick = lambda a, k: np.sort(rng.choice(a, min(k, a.size), replace=False))
            k = r % 5
            if r in long_rows:
                c = np.arange(n) if long_rows[r] else np.concatenate([below, above])
            elif k == 0:
                c = np.zeros(0, dtype=np.int64)
            elif k == 1:
                c = np.concatenate([[r], pick(above, 3)])
            elif k == 2:
                c = np.concatenate([pick(below, 3), [r]])
            elif k == 3:
                c = np.concatenate([pick(below, 2), pick(above, 2)])
            else:
                c = np.concatenate([pick(below, 2), [r], pick(above, 2)])
            rows_cols.append(c.astype(np.int64))
        rowptr = np.concatenate([[0], np.cumsum([c.size for c in rows_cols])]).astype(np.int64)
        col = np.concatenate(rows_cols)
        return rowptr, col, dyadic(rng, col.size)
    return cached(("strict", n), make)


@pytest.mark.parametrize("mode", ["appended", "strict", "strict_gcn"])
@pytest.mark.parametrize("idx", ["int32", "int64"])
def test_self_loops_on_2049_vertices(dev, idx, mode):
    n = 2049
    rowptr, col, w = strict_case(n, {7: True})                                 # row 7 holds all 2049 columns: walked by its workgroup
    strict, gcn = mode != "appended", mode == "strict_gcn"
    ref = C.ref_import(rowptr, col, w, n, n, self_loop_weight=0.25, gcn=gcn, strict=strict)
    deg = np.diff(rowptr)
    has = np.bincount(np.repeat(np.arange(n), deg)[col == np.repeat(np.arange(n), deg)], minlength=n) > 0
    assert (deg == 0).sum() > 400 and has.sum() > 1200 and (~has & (deg > 0)).sum() > 400
    assert ref["nnz"] == col.size + (int((~has).sum()) if strict else n) and not ref["flags"] & C.BAD
    gr = run(dev, rowptr, col, w, n, n, idx, self_loop_weight=0.25, gcn=gcn, strict_cols=strict)
    check(gr, ref, gcn=gcn)
    if strict:                                                                 # still strictly increasing, every row has its diagonal once
        oc, orow = ref["col"], np.repeat(np.arange(n), np.diff(ref["rowptr"]))
        assert bool(((orow[1:] != orow[:-1]) | (oc[1:] > oc[:-1])).all()) and int((oc == orow).sum()) == n


def test_strict_loops_in_rows_walked_by_a_workgroup(dev):
    """n = 4100: a row of all columns (the loop is merged) and one of all columns but its own (the loop is inserted in the middle)."""
    n = 4100
    rowptr, col, w = strict_case(n, {11: True, 3000: False})
    ref = C.ref_import(rowptr, col, w, n, n, self_loop_weight=0.25, strict=True)
    assert np.diff(rowptr)[[11, 3000]].tolist() == [4100, 4099]
    check(run(dev, rowptr, col, w, n, n, "int32", self_loop_weight=0.25, strict_cols=True), ref)


def test_gcn_isolated_sender_reports_nonfinite(dev):
    rowptr = np.array([0, 2, 2, 3], dtype=np.int64)                             # vertex 1 sends to 0 and has no incoming edge
    col = np.array([1, 2, 0], dtype=np.int64)
    ref = C.ref_import(rowptr, col, None, 3, 3, gcn=True)
    assert ref["flags"] == C.FLAG_W_NONFINITE
    check(run(dev, rowptr, col, None, 3, 3, gcn=True), ref, gcn=True)
    # with self loops every vertex has weight: finite
    check(run(dev, rowptr, col, None, 3, 3, gcn=True, self_loop_weight=1.0), C.ref_import(rowptr, col, None, 3, 3, self_loop_weight=1.0, gcn=True), gcn=True)


def test_final_weight_flags(dev):
    rowptr = np.array([0, 2, 3], dtype=np.int64)
    col = np.array([0, 1, 1], dtype=np.int64)
    for vals, want in (([1.0, -1.0, 2.0], C.FLAG_W_NEGATIVE), ([np.inf, 1.0, 1.0], C.FLAG_W_NONFINITE), ([1.0, 1.0, 1.0], 0)):
        w = np.array(vals, dtype=np.float32)
        for kw in (dict(), dict(self_loop_weight=0.5)):
            ref = C.ref_import(rowptr, col, w, 2, 2, self_loop_weight=kw.get("self_loop_weight", 0.0))
            assert ref["flags"] & ~C.FLAG_W_NONUNIT == want
            check(run(dev, rowptr, col, w, 2, 2, **kw), ref)
    # the merged diagonal weight overflows: reported on the FINAL weights
    big = np.array([3.0e38, 1.0, 1.0], dtype=np.float32)
    gr = run(dev, rowptr, col, big, 2, 2, self_loop_weight=3.0e38, strict_cols=True)
    assert gr.flags == C.FLAG_W_NONFINITE | C.FLAG_W_NONUNIT


# ---- malformed inputs: flagged, and the imported graph is empty -----------------------------------------------------------------
def malformed_case():
    def make():
        rng = np.random.default_rng(21)
        rows = 3000
        deg = rng.integers(1, 6, rows)
        deg[[1000, 2000]] = 4                                                   # the rows whose column order the strict cases break
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        col = np.concatenate([np.sort(rng.choice(rows, d, replace=False)) for d in deg]).astype(np.int64)
        return rows, rowptr, col
    return cached("malformed", make)


def _set(a, i, v):
    a = a.copy()
    a[i] = v
    return a


MALFORMED = [
    ("rowptr0_is_1", lambda rp, c: (_set(rp, 0, 1), c), False, C.FLAG_CSR_MALFORMED),
    ("decreasing_pair_in_the_middle", lambda rp, c: (_set(rp, 1500, rp[1499] - 1), c), False, C.FLAG_CSR_MALFORMED),
    ("last_is_nnz_plus_1", lambda rp, c: (_set(rp, -1, rp[-1] + 1), c), False, C.FLAG_CSR_MALFORMED),
    ("last_is_nnz_minus_1", lambda rp, c: (_set(rp, -1, rp[-1] - 1), c), False, C.FLAG_CSR_MALFORMED),
    ("negative_entry", lambda rp, c: (_set(rp, 2, -5), c), False, C.FLAG_CSR_MALFORMED),
    ("huge_entry", lambda rp, c: (_set(rp, 2000, 2 ** 31 - 1), c), False, C.FLAG_CSR_MALFORMED),
    ("col_minus_1", lambda rp, c: (rp, _set(c, 4097, -1)), False, C.FLAG_INDEX_RANGE),
    ("col_num_cols", lambda rp, c: (rp, _set(c, c.size - 1, 3000)), False, C.FLAG_INDEX_RANGE),
    ("strict_equal_pair", lambda rp, c: (rp, _set(c, rp[1000] + 1, c[rp[1000]])), True, C.FLAG_CSR_COL_ORDER),
    ("strict_decreasing_pair", lambda rp, c: (rp, _set(c, rp[2000], 2999)), True, C.FLAG_CSR_COL_ORDER),
]


@pytest.mark.parametrize("loops", [False, True], ids=["plain", "loops_gcn"])
@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("name,change,strict,flag", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_input_gives_its_flag_and_the_empty_graph(dev, name, change, strict, flag, idx, loops):
    rows, rowptr, col = malformed_case()
    rp, c = change(rowptr, col)
    kw = dict(self_loop_weight=0.5, gcn=True) if loops else dict()
    ref = C.ref_import(rp, c, None, rows, rows, strict=strict, **kw)
    assert ref["flags"] & C.BAD == flag and ref["nnz"] == 0
    gr = run(dev, rp, c, None, rows, rows, idx, strict_cols=strict, **kw)
    st = host(gr.stats_dev).tolist()
    bad = st[R.STAT_FLAGS] & C.BAD
    # COL_ORDER is only defined for a well-formed rowptr (the rows are not known otherwise)
    assert bad == flag or (flag == C.FLAG_CSR_MALFORMED and bad & ~C.FLAG_CSR_COL_ORDER == flag), (bad, flag)
    assert st[R.STAT_NNZ] == 0 and st[R.STAT_MAX_DEGREE] == 0 and st[R.STAT_NUM_ZERO] == rows
    assert int(gr.rowptr.abs().max()) == 0
    bs = host(gr.bin_start)
    assert bs[0] == 0 and bool((bs[1:] == rows).all())
    assert np.array_equal(np.sort(host(gr.perm)), np.arange(rows))
    # the same arrays are accepted where the rule does not apply
    if strict:
        ok = run(dev, rp, c, None, rows, rows, idx)
        assert ok.flags == 0 and ok.stats()[R.STAT_NNZ] == col.size


def test_malformed_flags_raise_the_documented_assertions(dev):
    """FSW_embedding._checked_stats on the imported (empty) graph: the messages of the public entries."""
    from fsw_gnn_amd import FSW_embedding
    rows, rowptr, col = malformed_case()
    E = FSW_embedding(d_in=3, d_out=4, device=dev)
    for rp, c, strict, msg in ((_set(rowptr, 0, 1), col, False, "CSR adjacency is malformed"), (rowptr, _set(col, 5, rows), False, "index out of range"),
                               (rowptr, _set(col, rowptr[2000], 2999), True, "strictly increasing column indices")):
        with pytest.raises(AssertionError, match=msg):
            E._checked_stats(run(dev, rp, c, None, rows, rows, strict_cols=strict))


# ---- refused arguments ----------------------------------------------------------------------------------------------------------
def raw_import(dev, rowptr, col, rows, cols, nnz=None, index_bytes=8, short=0):
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    nnz = col.numel() if nnz is None else nnz
    out = dict(rowptr=torch.full((rows + 1,), -7, dtype=torch.int32, device=dev), col=torch.empty(max(col.numel(), 1), dtype=torch.int32, device=dev),
               perm=torch.empty(rows, dtype=torch.int32, device=dev), bin_start=torch.empty(NB + 1, dtype=torch.int32, device=dev),
               stats=torch.full((_lib.NUM_STATS,), -7, dtype=torch.int32, device=dev))
    ws_bytes = int(L.fsw_graph_import_workspace_bytes(rows, min(nnz, 1 << 20)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rc = L.fsw_graph_import_csr(_lib.ptr(rowptr), _lib.ptr(col), None, index_bytes, nnz, rows, cols, 0, 0.0, 0, 0, _lib.ptr(out["rowptr"]),
                                _lib.ptr(out["col"]), None, None, _lib.ptr(out["perm"]), None, _lib.ptr(out["bin_start"]), _lib.ptr(out["stats"]),
                                _lib.ptr(ws), ws_bytes - short, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def test_refused_arguments_leave_the_next_import_intact(dev):
    from fsw_gnn_amd import _lib
    rows, rowptr, col = malformed_case()
    ref = C.ref_import(rowptr, col, None, rows, rows)
    rp, c = t(rowptr, dev), t(col, dev)
    for kw in (dict(short=1), dict(index_bytes=2), dict(nnz=2 ** 31 - rows), dict(nnz=2 ** 31)):
        rc, out = raw_import(dev, rp, c, rows, rows, **kw)
        assert rc != 0 and _lib.lib().fsw_last_error(), kw
        assert int((out["rowptr"] != -7).sum()) == 0 and int((out["stats"] != -7).sum()) == 0          # nothing ran
        rc, out = raw_import(dev, rp, c, rows, rows)
        assert rc == 0
        assert np.array_equal(host(out["rowptr"]), ref["rowptr"]) and np.array_equal(host(out["col"]), ref["col"])
        assert host(out["stats"])[R.STAT_NNZ] == col.size and host(out["stats"])[R.STAT_FLAGS] == 0
        assert R.perm_mismatch(host(out["perm"]), R.ref_bins(ref["rowptr"])) is None
