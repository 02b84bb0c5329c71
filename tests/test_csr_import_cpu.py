"""The numpy restatement of fsw_graph_import_csr (tests/csr_import_ref.py) against the references of the builds it has to agree with,
entry for entry -- graph_ref.ref_csr for the plain import and the appended self loops, graph_ref.ref_coalesced for the strict import --
on random multigraphs turned into CSR by a stable sort / by coalescing; and the host-side argument checks of the three public
entries, which raise before any device is touched (the modules live on the CPU here)."""
import numpy as np
import pytest
import torch

from tests import csr_import_ref as C
from tests import graph_ref as R


@pytest.fixture(autouse=True, scope="module")
def flag_bits_are_the_bindings():
    """The restatement speaks of the flags by value: they must be the ones fsw_gnn_amd/_lib.py and include/fsw_hip.h declare."""
    import os
    import re
    from fsw_gnn_amd import _lib
    assert (C.FLAG_CSR_MALFORMED, C.FLAG_CSR_COL_ORDER, C.FLAG_W_NONUNIT) == (_lib.FLAG_CSR_MALFORMED, _lib.FLAG_CSR_COL_ORDER, _lib.FLAG_W_NONUNIT)
    header = open(os.path.join(R.ROOT, "include", "fsw_hip.h")).read()
    for name, bit in (("CSR_MALFORMED", 16), ("CSR_COL_ORDER", 32), ("W_NONUNIT", 64)):
        assert re.search(r"#define FSW_FLAG_%s %d\b" % (name, bit), header), name


def dyadic(rng, n):
    return (rng.integers(1, 4096, n) / 1024.0).astype(np.float32)


def multigraph(seed, rows, cols, edges):
    """Random edges with ~20 % repeated pairs, some rows empty."""
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, rows, edges).astype(np.int64)
    snd = rng.integers(0, cols, edges).astype(np.int64)
    dup = rng.choice(edges, edges // 5, replace=False)
    src = rng.integers(0, edges, dup.size)
    rec[dup], snd[dup] = rec[src].copy(), snd[src].copy()
    rec[rec % 7 == 3] = (rec[rec % 7 == 3] + 1) % rows                      # rows 3, 10, 17, ... stay empty
    return rec, snd, dyadic(rng, edges)


SHAPES = [(1, 1, 1), (5, 3, 40), (64, 64, 10), (300, 300, 5000), (2049, 2049, 9000)]


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("rows,cols,edges", SHAPES)
def test_plain_import_is_ref_csr_of_the_edge_list(rows, cols, edges, weighted):
    rec, snd, w = multigraph(rows + edges, rows, cols, edges)
    rowptr, col, wc, _ = C.edges_to_csr(rec, snd, w if weighted else None, rows)
    got = C.ref_import(rowptr, col, wc, rows, cols)
    want = R.ref_csr(rec, snd, w if weighted else None, rows, cols)
    assert got["nnz"] == want["nnz"] == edges
    assert np.array_equal(got["rowptr"], want["rowptr"]) and np.array_equal(got["col"], want["col"])
    assert np.array_equal(got["slot"], np.arange(edges))
    if weighted:
        assert np.array_equal(got["w"].view(np.int32), want["w"].view(np.int32))
        assert got["flags"] == C.FLAG_W_NONUNIT
    else:
        assert got["w"] is None and got["flags"] == 0
    bins = R.ref_bins(got["rowptr"])
    assert np.array_equal(bins["bin_start"], R.ref_bins(want["rowptr"])["bin_start"]) and bins["stats"][R.STAT_NNZ] == edges


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("n,edges", [(1, 3), (64, 10), (300, 5000), (2049, 9000)])
def test_appended_self_loops_are_ref_csr_of_the_edge_list_with_the_loops_appended(n, edges, weighted):
    """What FSW_conv._weighted_edges + the stable build do: the loop is the LAST entry of every row, next to a diagonal entry or not."""
    rec, snd, w = multigraph(n + edges, n, n, edges)
    assert bool((rec == snd).any()) or edges != 5000                         # the 300-vertex case has rows with a diagonal entry
    sl = np.float32(0.5)
    rowptr, col, wc, order = C.edges_to_csr(rec, snd, w if weighted else None, n)
    got = C.ref_import(rowptr, col, wc, n, n, self_loop_weight=sl)
    loops = np.arange(n, dtype=np.int64)
    w_all = np.concatenate([w if weighted else np.ones(edges, dtype=np.float32), np.full(n, sl, dtype=np.float32)])
    want = R.ref_csr(np.concatenate([rec, loops]), np.concatenate([snd, loops]), w_all, n, n)
    assert got["nnz"] == want["nnz"] == edges + n
    assert np.array_equal(got["rowptr"], want["rowptr"]) and np.array_equal(got["col"], want["col"])
    assert np.array_equal(got["w"].view(np.int32), want["w"].view(np.int32))
    assert np.array_equal(got["rowptr"], rowptr + np.arange(n + 1))           # no scan needed
    # the slot of an input entry holds that entry
    assert np.array_equal(got["col"][got["slot"]], col) and np.array_equal(got["w"][got["slot"]], w_all[:edges][order])
    bins = R.ref_bins(got["rowptr"])
    assert np.array_equal(bins["bin_start"], R.ref_bins(want["rowptr"])["bin_start"])


@pytest.mark.parametrize("loops", [False, True], ids=["no_loops", "loops"])
@pytest.mark.parametrize("n,edges", [(1, 3), (64, 10), (300, 5000), (2049, 9000)])
def test_strict_import_is_ref_coalesced_of_the_edge_list(n, edges, loops):
    """The input is the coalesced adjacency of the multigraph; with self loops the result is the coalesced adjacency of the edge list
    with the loops appended, and slot_of_entry composes with the first coalescing to that build's slot_of_edge."""
    rec, snd, w = multigraph(n + edges + 1, n, n, edges)
    first = R.ref_coalesced(rec, snd, w, None, n, n)
    sl = np.float32(0.25) if loops else np.float32(0)
    got = C.ref_import(first["rowptr"].astype(np.int64), first["col"].astype(np.int64), first["w"], n, n, self_loop_weight=sl, strict=True)
    assert not got["flags"] & C.BAD
    if loops:
        ar = np.arange(n, dtype=np.int64)
        want = R.ref_coalesced(np.concatenate([rec, ar]), np.concatenate([snd, ar]), np.concatenate([w, np.full(n, sl, dtype=np.float32)]),
                               None, n, n)
        has_diag = np.bincount(rec[rec == snd], minlength=n) > 0
        assert got["nnz"] == first["nnz"] + int((~has_diag).sum())
    else:
        want = first
    assert got["nnz"] == want["nnz"]
    assert np.array_equal(got["rowptr"], want["rowptr"]) and np.array_equal(got["col"], want["col"])
    assert np.array_equal(got["w"], want["w"])                              # dyadic weights: every sum is exact
    assert np.array_equal(got["slot"][first["slot"]], want["slot"][:edges])
    assert np.array_equal(R.ref_bins(got["rowptr"])["bin_start"], R.ref_bins(want["rowptr"])["bin_start"])


def test_gcn_weights_are_those_of_the_edge_list_path():
    """w / sqrt(deg[recipient]) / sqrt(deg[sender]) with deg = the row sums of the final weights (FSW_conv._weighted_edges)."""
    n, edges = 300, 5000
    rec, snd, _ = multigraph(77, n, n, edges)
    rowptr, col, _, _ = C.edges_to_csr(rec, snd, None, n)
    got = C.ref_import(rowptr, col, None, n, n, self_loop_weight=0.5, gcn=True)
    ar = np.arange(n)
    r2, s2 = np.concatenate([rec, ar]), np.concatenate([snd, ar])
    w2 = np.concatenate([np.ones(edges), np.full(n, 0.5)])
    deg = np.bincount(r2, weights=w2, minlength=n)
    want = R.ref_csr(r2, s2, (w2 / np.sqrt(deg[r2]) / np.sqrt(deg[s2])).astype(np.float32), n, n)
    assert np.array_equal(got["col"], want["col"]) and np.array_equal(got["w"], want["w"]) and got["flags"] == 0
    # a sender without incoming weight: division by sqrt(0)
    rowptr = np.array([0, 1, 1], dtype=np.int64)
    iso = C.ref_import(rowptr, np.array([1], dtype=np.int64), None, 2, 2, gcn=True)
    assert iso["flags"] == C.FLAG_W_NONFINITE and iso["nnz"] == 1


MALFORMED = [
    ("rowptr0_is_1", dict(rowptr=[1, 2, 4, 6]), C.FLAG_CSR_MALFORMED),
    ("decreasing_pair", dict(rowptr=[0, 4, 2, 6]), C.FLAG_CSR_MALFORMED),
    ("last_is_nnz_plus_1", dict(rowptr=[0, 2, 4, 7]), C.FLAG_CSR_MALFORMED),
    ("last_is_nnz_minus_1", dict(rowptr=[0, 2, 4, 5]), C.FLAG_CSR_MALFORMED),
    ("negative_entry", dict(rowptr=[0, -1, 4, 6]), C.FLAG_CSR_MALFORMED),
    ("col_minus_1", dict(col=[0, 1, -1, 2, 0, 1]), C.FLAG_INDEX_RANGE),
    ("col_num_cols", dict(col=[0, 1, 0, 3, 0, 1]), C.FLAG_INDEX_RANGE),
    ("strict_equal_pair", dict(col=[1, 1, 0, 2, 0, 1], strict=True), C.FLAG_CSR_COL_ORDER),
    ("strict_decreasing_pair", dict(col=[0, 1, 2, 0, 0, 1], strict=True), C.FLAG_CSR_COL_ORDER),
]


@pytest.mark.parametrize("name,change,flag", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_empty_graph_rule(name, change, flag):
    rowptr = np.array(change.get("rowptr", [0, 2, 4, 6]), dtype=np.int64)
    col = np.array(change.get("col", [0, 1, 0, 2, 0, 1]), dtype=np.int64)
    got = C.ref_import(rowptr, col, None, 3, 3, strict=change.get("strict", False))
    assert got["flags"] & C.BAD == flag
    assert got["nnz"] == 0 and not got["rowptr"].any() and got["rowptr"].size == 4
    bins = R.ref_bins(got["rowptr"])
    assert bins["stats"][R.STAT_NUM_ZERO] == 3 and bins["stats"][R.STAT_NNZ] == 0
    # the same columns are fine without strict_cols (repeated columns are parallel edges)
    if "strict" in change:
        assert C.ref_import(rowptr, col, None, 3, 3)["flags"] == 0


# ---- host-side argument checks of the public entries: raised on CPU tensors, before any device is touched ------------------------
def csr_w(crow, col, vals, size):
    return torch.sparse_csr_tensor(torch.tensor(crow), torch.tensor(col), torch.tensor(vals, dtype=torch.float32), size=size)


def test_embedding_refuses_what_the_csr_layout_does_not_cover():
    from fsw_gnn_amd import FSW_embedding
    E = FSW_embedding(d_in=4, d_out=6, device="cpu")
    X = torch.zeros(3, 4)
    W = csr_w([0, 1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0], (3, 3))
    with pytest.raises(AssertionError, match="graph_mode=True"):
        E(X, W, graph_mode=False)
    batched = torch.sparse_csr_tensor(torch.tensor([[0, 1, 2, 3]] * 2), torch.tensor([[0, 1, 2]] * 2), torch.ones(2, 3), size=(2, 3, 3))
    with pytest.raises(AssertionError, match="batch dimensions are not supported"):
        E(torch.zeros(2, 3, 4), batched, graph_mode=True)
    with pytest.raises(AssertionError, match="unsupported sparsity layout.*torch.sparse_csr"):
        E(X, W.to_sparse_csc(), graph_mode=True)
    Wg = csr_w([0, 1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0], (3, 3)).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="torch.sparse_coo"):
        E(X, Wg, graph_mode=True)
    with pytest.raises(RuntimeError, match="no CPU path"):                   # a valid call gets as far as the device check
        E(X, W, graph_mode=True)


def test_conv_and_import_refuse_bad_csr_arguments():
    from fsw_gnn_amd import FSW_conv, import_csr
    conv = FSW_conv(4, 5, device="cpu")
    x = torch.zeros(3, 4)
    rowptr, col = torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])
    with pytest.raises(AssertionError, match="int32 or both be int64"):
        conv(x, (rowptr.to(torch.int16), col.to(torch.int16)))
    with pytest.raises(AssertionError, match="int32 or both be int64"):
        conv(x, (rowptr, col.to(torch.int32)))
    with pytest.raises(AssertionError, match=r"num_vertices \+ 1"):
        conv(x, (rowptr[:-1], col))
    with pytest.raises(AssertionError, match="num_vertices, num_vertices"):
        conv(x, csr_w([0, 1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0], (3, 4)))
    with pytest.raises(AssertionError, match="unsupported layout"):
        conv(x, csr_w([0, 1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0], (3, 3)).to_sparse_csc())
    conv._node_parallel = True
    with pytest.raises(NotImplementedError, match="CSR adjacency under"):
        conv(x, (rowptr, col))
    conv._node_parallel = False
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv(x, (rowptr, col))
    # graph.import_csr itself
    with pytest.raises(AssertionError, match="square adjacency"):            # self loops on a rectangular adjacency
        import_csr(torch.tensor([0, 1, 2, 3, 3, 3]), col, None, 5, 3, self_loop_weight=0.5)
    with pytest.raises(AssertionError, match="square adjacency"):
        import_csr(torch.tensor([0, 1, 2, 3, 3, 3]), col, None, 5, 3, gcn=True)
    with pytest.raises(AssertionError, match="int32 or int64"):
        import_csr(rowptr.to(torch.float32), col, None, 3, 3)
    with pytest.raises(AssertionError, match="dtype of rowptr"):
        import_csr(rowptr, col.to(torch.int32), None, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        import_csr(rowptr, col, None, 3, 3)


def test_readout_refuses_ptr_together_with_graph_index():
    from fsw_gnn_amd import FSW_readout
    ro = FSW_readout(4, 5, device="cpu")
    x = torch.zeros(3, 4)
    with pytest.raises(AssertionError, match="either graph_index or ptr"):
        ro(x, graph_index=torch.zeros(3, dtype=torch.int64), ptr=torch.tensor([0, 3]))
    with pytest.raises(AssertionError, match="int32 or int64"):
        ro(x, ptr=torch.tensor([0.0, 3.0]))
    with pytest.raises(AssertionError, match="batch_size must equal"):
        ro(x, batch_size=2, ptr=torch.tensor([0, 3]))
