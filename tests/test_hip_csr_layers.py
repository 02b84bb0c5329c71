"""CSR adjacency input of the public layers: a torch.sparse_csr W of FSW_embedding, the tuple (rowptr, col) and torch.sparse_csr forms
of FSW_conv's adjacency, FSW_readout(ptr=...).  Anchored to the reference's goldens (tiny_graph.npz, edgefeat_tiny.npz) at the bounds
the edge-list tests use, and to the edge-list path of the same graph BIT FOR BIT: the imported CSR arrays are identical to the built
ones and every row's output depends on its own entries only."""
import numpy as np
import pytest
import torch

from tests import csr_import_ref as C
from tests import graph_ref as R
from tests.conftest import golden, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5            # tests/test_hip_parity.py
F64 = 1e-12           # tests/test_hip_float64.py
GRAD = 3e-5           # tests/test_hip_parity.py: test_edge_features_conv_forward_and_backward


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def crow_of(rows, n):
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)


def csr_tensor(crow, col, vals, size, dev, idx=torch.int64, dtype=torch.float32):
    return torch.sparse_csr_tensor(t(crow, dev, idx), t(col, dev, idx), t(vals, dev, dtype), size=size)


def make_embedding(dev, V, freqs, bias=None, scale=None, dtype=torch.float32, **kw):
    from fsw_gnn_amd import FSW_embedding
    S, d = V.shape
    E = FSW_embedding(d_in=d, d_out=S + (1 if kw.get("encode_total_mass", False) else 0), device=dev, dtype=dtype, **kw)
    with torch.no_grad():
        E.projVecs.copy_(t(V, dev, dtype))
        E.freqs.copy_(t(freqs, dev, dtype))
        if bias is not None and E.enable_bias:
            E.bias.copy_(t(bias, dev, dtype))
        if scale is not None:
            E.total_mass_encoding_scale.fill_(scale)
    return E


def tiny_csr(g):
    """The coalesced adjacency of the golden as CSR: its indices are sorted by (recipient, sender)."""
    idx = g["adj_indices"]
    assert bool((np.diff(idx[0] * 64 + idx[1]) > 0).all())
    return crow_of(idx[0], 64), idx[1]


# ---- the reference's goldens ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_embedding_sparse_csr_W_against_the_goldens(dev, idx):
    g = golden("tiny_graph")
    crow, col = tiny_csr(g)
    X = t(g["X"], dev)
    W = csr_tensor(crow, col, g["adj_values"], (64, 64), dev, idx)
    W3 = csr_tensor(crow, col, g["adj3_values"], (64, 64), dev, idx)
    with torch.no_grad():
        E = make_embedding(dev, g["V"], g["freqs"], bias=g["bias"], scale=0.7, encode_total_mass=True, total_mass_encoding_function="identity",
                           total_mass_encoding_method="plain", total_mass_encoding_scale=0.7)
        assert relerr(E(X, W, graph_mode=True).cpu().numpy(), g["out_identity_plain"]) < TOL
        E = make_embedding(dev, g["V"], g["freqs"], enable_bias=False)
        assert relerr(E(X, W3, graph_mode=True).cpu().numpy(), g["out_weighted"]) < TOL
        E = make_embedding(dev, g["V"], g["freqs"], enable_bias=False, total_mass_pad_thresh=3.0)
        assert relerr(E(X, W, graph_mode=True).cpu().numpy(), g["out_tau3"]) < TOL


def test_float64_embedding_sparse_csr_W_against_the_goldens(dev):
    g = golden("tiny_graph")
    crow, col = tiny_csr(g)
    X = t(g["X"], dev, torch.float64)
    with torch.no_grad():
        E = make_embedding(dev, g["V"], g["freqs"], enable_bias=False, dtype=torch.float64)
        W3 = csr_tensor(crow, col, g["adj3_values"], (64, 64), dev, dtype=torch.float64)
        out = E(X, W3, graph_mode=True)
        assert out.dtype == torch.float64 and relerr(out.cpu().numpy(), g["out_weighted"]) < F64
        E = make_embedding(dev, g["V"], g["freqs"], enable_bias=False, total_mass_pad_thresh=3.0, dtype=torch.float64)
        W = csr_tensor(crow, col, g["adj_values"], (64, 64), dev, torch.int32, dtype=torch.float64)
        assert relerr(E(X, W, graph_mode=True).cpu().numpy(), g["out_tau3"]) < F64


@pytest.mark.parametrize("dtype,tol", [(torch.float32, TOL), (torch.float64, F64)], ids=["float32", "float64"])
def test_conv_gcn_selfloops_from_both_csr_forms(dev, dtype, tol):
    """out_gcn_selfloop from the tuple form of the raw edge list's CSR (parallel edges as repeated columns) and from the tensor form
    of the coalesced adjacency with the multiplicities as values."""
    from fsw_gnn_amd import FSW_conv
    g = golden("tiny_graph")
    conv = FSW_conv(8, 16, encode_vertex_degrees=False, mlp_layers=0, concat_self=False, bias=False, self_loop_weight=0.5,
                    edge_weighting="gcn", device=dev, dtype=dtype)
    ei = g["edge_index"]
    rowptr, col, _, _ = C.edges_to_csr(ei[1], ei[0], None, 64)
    assert col.size == 400 and int((np.diff(rowptr) > 0).sum()) == 56
    crow, ccol = tiny_csr(g)
    assert g["adj_values"].max() > 1                                          # the coalesced adjacency has merged parallel edges
    X = t(g["X"], dev, dtype)
    with torch.no_grad():
        conv.fsw_embed.projVecs.copy_(t(g["V"], dev, dtype))
        conv.fsw_embed.freqs.copy_(t(g["freqs"], dev, dtype))
        for idx in (torch.int32, torch.int64):
            y = conv(X, (t(rowptr, dev, idx), t(col, dev, idx)))
            assert relerr(y.cpu().numpy(), g["out_gcn_selfloop"]) < tol
            y = conv(X, csr_tensor(crow, ccol, g["adj_values"], (64, 64), dev, idx, dtype))
            assert relerr(y.cpu().numpy(), g["out_gcn_selfloop"]) < tol


@pytest.mark.parametrize("tag,slw", [("plain", 0.0), ("selfloop", 0.5)])
def test_edge_features_conv_on_the_coalesced_csr(dev, tag, slw):
    """edgefeat_tiny.npz: the coalesced adjacency (multiplicities as values) with the summed features of every entry; forward,
    gradients, and dL/d edge_features per entry = gEF[e] of any input edge e of that entry."""
    from fsw_gnn_amd import FSW_conv
    g, ge = golden("tiny_graph"), golden("edgefeat_tiny")
    d, de, out_ch, embed_dim = 8, 3, 5, 17
    ei = g["edge_index"]
    co = R.ref_coalesced(ei[1], ei[0], None, ge["edge_features"].astype(np.float32), 64, 64)
    nnz = co["nnz"]
    assert nnz == 371 and co["w"].max() > 1
    conv = FSW_conv(d, out_ch, edgefeat_dim=de, embed_dim=embed_dim, self_loop_weight=slw, device=dev)
    with torch.no_grad():
        conv.fsw_embed.projVecs.copy_(t(ge["V"], dev))
        conv.fsw_embed.freqs.copy_(t(ge["freqs"], dev))
        conv.mlp[0].weight.copy_(t(ge["lin_w"], dev))
        conv.mlp[0].bias.copy_(t(ge["lin_b"], dev))
    adj = csr_tensor(co["rowptr"], co["col"], co["w"], (64, 64), dev, torch.int32)
    with torch.no_grad():
        y = conv(t(g["X"], dev), adj, edge_features=t(co["ef"], dev))
    assert relerr(y.cpu().numpy(), ge["y_" + tag]) < TOL
    X = t(g["X"], dev).requires_grad_(True)
    EF = t(co["ef"], dev).requires_grad_(True)
    y2 = conv(X, adj, edge_features=EF)
    (y2 * t(ge["R"], dev)).sum().backward()
    assert relerr(X.grad.cpu().numpy(), ge["gX_" + tag]) < GRAD
    assert relerr(EF.grad.cpu().numpy()[co["slot"]], ge["gEF_" + tag]) < GRAD
    assert relerr(conv.fsw_embed.projVecs.grad.cpu().numpy(), ge["gV_" + tag]) < GRAD
    assert relerr(conv.fsw_embed.freqs.grad.cpu().numpy(), ge["gfreqs_" + tag]) < GRAD
    assert relerr(conv.mlp[0].weight.grad.cpu().numpy(), ge["gW_" + tag]) < GRAD


# ---- equality with the edge-list path -------------------------------------------------------------------------------------------
_CACHE = {}


def long_row_graph():
    """2600 vertices, ~6 neighbours a row, and rows of 33, 300 and 2100 neighbours (the fused kernel's long-row finishing)."""
    if "g" not in _CACHE:
        rng = np.random.default_rng(31)
        n = 2600
        long_rows = {5: 33, 6: 300, 7: 2100}
        rec = np.concatenate([rng.integers(8, n, 15_000)] + [np.full(k, r, dtype=np.int64) for r, k in long_rows.items()])
        snd = np.concatenate([rng.integers(0, n, 15_000)] + [rng.choice(n, k, replace=False) for k in long_rows.values()])
        p = rng.permutation(rec.size)
        rec, snd = rec[p], snd[p]
        rowptr, col, _, _ = C.edges_to_csr(rec, snd, None, n)
        assert np.diff(rowptr)[5:8].tolist() == [33, 300, 2100]
        _CACHE["g"] = (n, rec, snd, rowptr, col, rng.standard_normal((n, 16)).astype(np.float32))
    return _CACHE["g"]


def grads_of(f, X, params):
    """Output and gradients of X and params for the loss sum(f(X) * R), R fixed."""
    for p in params:
        p.grad = None
    Xg = X.clone().requires_grad_(True)
    y = f(Xg)
    R_ = torch.linspace(-1.0, 1.0, y.numel(), device=y.device).reshape(y.shape)
    (y * R_).sum().backward()
    return [y.detach(), Xg.grad.clone()] + [p.grad.clone() for p in params]


def assert_same_or_close(a, b, repro, bound):
    """Bit-identical where the edge-list path is itself reproducible run to run (repro), else within the bound of its gradient tests."""
    for x, y, same in zip(a, b, repro):
        if same:
            assert torch.equal(x, y)
        else:
            assert relerr(x.cpu().numpy(), y.cpu().numpy()) < bound


@pytest.mark.parametrize("cart", [False, True], ids=["diagonal_fused", "cartesian"])
def test_unit_conv_equals_the_edge_list_path_bit_for_bit(dev, cart):
    from fsw_gnn_amd import FSW_conv
    n, rec, snd, rowptr, col, X = long_row_graph()
    kw = dict(embed_slices=4, embed_freqs=8) if cart else dict()
    conv = FSW_conv(16, 24, device=dev, **kw)
    assert conv._fusable()
    ei = t(np.stack([snd, rec]), dev, torch.int64)
    Xd = t(X, dev)
    forms = [(t(rowptr, dev, torch.int32), t(col, dev, torch.int32)), (t(rowptr, dev, torch.int64), t(col, dev, torch.int64)),
             csr_tensor(rowptr, col, np.ones(col.size), (n, n), dev)]
    with torch.no_grad():
        want = conv(Xd, ei)
        for adj in forms:
            assert torch.equal(conv(Xd, adj), want)
    # training: the edge-list path twice first
    params = [conv.fsw_embed.projVecs, conv.fsw_embed.freqs, conv.mlp[0].weight]
    a, b = grads_of(lambda x: conv(x, ei), Xd, params), grads_of(lambda x: conv(x, ei), Xd, params)
    repro = [torch.equal(x, y) for x, y in zip(a, b)]
    assert repro[0]
    for adj in (forms[0], forms[2]):
        assert_same_or_close(grads_of(lambda x: conv(x, adj), Xd, params), a, repro, GRAD)


@pytest.mark.parametrize("slw", [0.0, 0.5], ids=["plain", "selfloop"])
@pytest.mark.parametrize("cart", [False, True], ids=["diagonal", "cartesian_edge_features"])
def test_edge_feature_conv_equals_the_edge_list_path_bit_for_bit(dev, cart, slw):
    """A graph without parallel edges, its edges listed in CSR order: the coalescing build of the edge-list path and the strict import
    give the same entries, weights (the loop's weight added to a diagonal entry) and feature rows (zeros for a new diagonal entry)."""
    from fsw_gnn_amd import FSW_conv
    n, rec, snd, _, _, X = long_row_graph()
    rec, snd = np.concatenate([rec, [20, 21, 22]]), np.concatenate([snd, [20, 21, 22]])         # some diagonal entries
    co = R.ref_coalesced(rec, snd, None, None, n, n)
    rows = np.repeat(np.arange(n), np.diff(co["rowptr"]))
    assert bool((np.diff(co["rowptr"])[5:8] >= [33, 300, 2100]).all()) and int((rows == co["col"]).sum()) >= 3
    ef = np.random.default_rng(34).standard_normal((co["nnz"], 2)).astype(np.float32)
    kw = dict(embed_slices=4, embed_freqs=8, cartesian_edge_features=True) if cart else dict()
    conv = FSW_conv(16, 24, edgefeat_dim=2, self_loop_weight=slw, device=dev, **kw)
    ei = t(np.stack([co["col"], rows]), dev, torch.int64)
    Xd, efd = t(X, dev), t(ef, dev)
    adj = (t(co["rowptr"], dev, torch.int32), t(co["col"], dev, torch.int32))
    with torch.no_grad():
        want = conv(Xd, ei, edge_features=efd)
        assert torch.equal(conv(Xd, adj, edge_features=efd), want)
        assert torch.equal(conv(Xd, csr_tensor(co["rowptr"], co["col"], np.ones(co["nnz"]), (n, n), dev), edge_features=efd), want)
    # dL/d edge_features through slot_of_entry
    def grad_ef(a):
        e = efd.clone().requires_grad_(True)
        y = conv(Xd, a, edge_features=e)
        (y * torch.linspace(-1.0, 1.0, y.numel(), device=dev).reshape(y.shape)).sum().backward()
        return e.grad
    a, b = grad_ef(ei), grad_ef(ei)
    if torch.equal(a, b):
        assert torch.equal(grad_ef(adj), a)
    else:
        assert relerr(grad_ef(adj).cpu().numpy(), a.cpu().numpy()) < GRAD


def test_unit_sparse_csr_adjacency_keeps_the_unit_kernels(dev):
    """No weight array after the import of a unit torch.sparse_csr adjacency; a non-unit one keeps it; the tuple form never has one."""
    from fsw_gnn_amd import FSW_conv
    n, rec, snd, rowptr, col, X = long_row_graph()
    conv = FSW_conv(16, 24, device=dev)
    unit = conv._csr_adjacency(csr_tensor(rowptr, col, np.ones(col.size), (n, n), dev), n)
    vals = np.ones(col.size)
    vals[col.size // 2] = 2.0
    nonunit = conv._csr_adjacency(csr_tensor(rowptr, col, vals, (n, n), dev), n)
    tup = conv._csr_adjacency((t(rowptr, dev, torch.int64), t(col, dev, torch.int64)), n)
    assert conv.build_graph_csr(unit, n).w is None and conv.build_graph_csr(tup, n).w is None
    gw = conv.build_graph_csr(nonunit, n)
    assert gw.w is not None and float(gw.w[col.size // 2]) == 2.0 and gw.flags & C.FLAG_W_NONUNIT
    assert conv.fsw_embed._unit_fast(conv.build_graph_csr(unit, n)) and not conv.fsw_embed._unit_fast(gw)


@pytest.mark.parametrize("cart", [False, True], ids=["diagonal", "cartesian"])
def test_embedding_sparse_csr_W_equals_the_coo_W_bit_for_bit(dev, cart):
    from fsw_gnn_amd import FSW_embedding
    n, rec, snd, _, _, X = long_row_graph()
    co = R.ref_coalesced(rec, snd, None, None, n, n)
    rng = np.random.default_rng(32)
    w = (rng.random(co["nnz"]) + 0.25).astype(np.float32)
    rows = np.repeat(np.arange(n), np.diff(co["rowptr"]))
    Wcoo = torch.sparse_coo_tensor(t(np.stack([rows, co["col"]]), dev, torch.int64), t(w, dev), (n, n)).coalesce()
    Wcsr = csr_tensor(co["rowptr"], co["col"], w, (n, n), dev, torch.int32)
    E = FSW_embedding(d_in=16, nSlices=4, nFreqs=6, collapse_freqs=True, encode_total_mass=True, device=dev) if cart else \
        FSW_embedding(d_in=16, d_out=33, encode_total_mass=True, device=dev)
    Xd = t(X, dev)
    with torch.no_grad():
        want = E(Xd, Wcoo, graph_mode=True)
        assert torch.equal(E(Xd, Wcsr, graph_mode=True), want)
    params = [p for p in (E.projVecs, E.freqs) if p.requires_grad]
    a, b = grads_of(lambda x: E(x, Wcoo, graph_mode=True), Xd, params), grads_of(lambda x: E(x, Wcoo, graph_mode=True), Xd, params)
    repro = [torch.equal(x, y) for x, y in zip(a, b)]
    assert repro[0]
    assert_same_or_close(grads_of(lambda x: E(x, Wcsr, graph_mode=True), Xd, params), a, repro, GRAD)


@pytest.mark.parametrize("cart", [False, True], ids=["diagonal", "cartesian"])
def test_embedding_sparse_csr_X_edge_equals_the_coo_inputs_bit_for_bit(dev, cart):
    """d_edge = 2: W and X_edge as torch.sparse_csr (values [nnz, 2], the indices of W) against the coalesced COO pair; an X_edge with
    other indices is refused."""
    from fsw_gnn_amd import FSW_embedding
    n, rec, snd, _, _, X = long_row_graph()
    co = R.ref_coalesced(rec, snd, None, None, n, n)
    rng = np.random.default_rng(35)
    nnz = co["nnz"]
    w = (rng.random(nnz) + 0.25).astype(np.float32)
    ef = rng.standard_normal((nnz, 2)).astype(np.float32)
    rows = np.repeat(np.arange(n), np.diff(co["rowptr"]))
    ij = t(np.stack([rows, co["col"]]), dev, torch.int64)
    Wcoo = torch.sparse_coo_tensor(ij, t(w, dev), (n, n)).coalesce()
    Ecoo = torch.sparse_coo_tensor(ij, t(ef, dev), (n, n, 2)).coalesce()
    Wcsr = csr_tensor(co["rowptr"], co["col"], w, (n, n), dev, torch.int32)
    Ecsr = csr_tensor(co["rowptr"], co["col"], ef, (n, n, 2), dev, torch.int32)
    kw = dict(nSlices=4, nFreqs=6, collapse_freqs=True, cartesian_edge_features=True) if cart else dict(d_out=33)
    E = FSW_embedding(d_in=16, d_edge=2, encode_total_mass=True, device=dev, **kw)
    Xd = t(X, dev)
    with torch.no_grad():
        want = E(Xd, Wcoo, Ecoo, graph_mode=True)
        assert torch.equal(E(Xd, Wcsr, Ecsr, graph_mode=True), want)
        other = co["col"].copy()
        other[0] = (other[0] + 1) % n                                          # compared on the host: never imported
        with pytest.raises(AssertionError, match="same nonzero pattern"):
            E(Xd, Wcsr, csr_tensor(co["rowptr"], other, ef, (n, n, 2), dev, torch.int32), graph_mode=True)
    a = grads_of(lambda x: E(x, Wcoo, Ecoo, graph_mode=True), Xd, [])
    b = grads_of(lambda x: E(x, Wcoo, Ecoo, graph_mode=True), Xd, [])
    repro = [torch.equal(x, y) for x, y in zip(a, b)]
    assert repro[0]
    assert_same_or_close(grads_of(lambda x: E(x, Wcsr, Ecsr, graph_mode=True), Xd, []), a, repro, GRAD)


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_readout_ptr_equals_graph_index_bit_for_bit(dev, idx):
    from fsw_gnn_amd import FSW_readout
    sizes = [0, 1, 40, 2100, 0]
    n, d = sum(sizes), 8
    gi = t(np.repeat(np.arange(len(sizes)), sizes), dev, torch.int64)
    ptr = t(np.concatenate([[0], np.cumsum(sizes)]), dev, idx)
    X = t(np.random.default_rng(33).standard_normal((n, d)).astype(np.float32), dev)
    ro = FSW_readout(d, 12, concat_self=False, mlp_layers=0, bias=False, encode_vertex_degrees=False, device=dev)
    with torch.no_grad():
        want = ro(X, gi, len(sizes))
        got = ro(X, ptr=ptr)
        assert got.shape == (len(sizes), 12) and torch.equal(got, want)
    params = [ro.fsw_embed.projVecs, ro.fsw_embed.freqs]
    a, b = grads_of(lambda x: ro(x, gi, len(sizes)), X, params), grads_of(lambda x: ro(x, gi, len(sizes)), X, params)
    repro = [torch.equal(x, y) for x, y in zip(a, b)]
    assert repro[0]
    assert_same_or_close(grads_of(lambda x: ro(x, ptr=ptr), X, params), a, repro, 2e-5)
    # ptr that does not end at the number of vertices
    with pytest.raises(AssertionError, match="CSR adjacency is malformed"):
        with torch.no_grad():
            ro(X, ptr=ptr - 1)


def test_float64_layers_take_the_csr_forms(dev):
    """float64 layers get (rec, snd) from the CSR with torch ops and run the generic kernels: equal to the edge-list call."""
    from fsw_gnn_amd import FSW_conv, FSW_readout
    g = golden("tiny_graph")
    ei = g["edge_index"]
    rowptr, col, _, _ = C.edges_to_csr(ei[1], ei[0], None, 64)
    X = t(g["X"], dev, torch.float64)
    conv = FSW_conv(8, 6, device=dev, dtype=torch.float64)
    ro = FSW_readout(8, 6, concat_self=False, mlp_layers=0, bias=False, device=dev, dtype=torch.float64)
    with torch.no_grad():
        want = conv(X, t(ei, dev, torch.int64))
        got = conv(X, (t(rowptr, dev, torch.int32), t(col, dev, torch.int32)))
        assert relerr(got.cpu().numpy(), want.cpu().numpy()) < F64
        gi = t(np.repeat(np.arange(3), [20, 0, 44]), dev, torch.int64)
        assert relerr(ro(X, ptr=t(np.array([0, 20, 20, 64]), dev, torch.int64)).cpu().numpy(), ro(X, gi, 3).cpu().numpy()) < F64


# ---- the new assertions, from the public entries --------------------------------------------------------------------------------
def test_malformed_and_unsorted_adjacencies_raise_from_the_public_entries(dev):
    from fsw_gnn_amd import FSW_conv, FSW_embedding
    g = golden("tiny_graph")
    crow, col = tiny_csr(g)
    X = t(g["X"], dev)
    bad_crow = crow.copy()
    bad_crow[10] = crow[9] - 1 if crow[9] > 0 else crow[11] + 1
    E = FSW_embedding(d_in=8, d_out=9, device=dev)
    conv = FSW_conv(8, 6, device=dev)
    with torch.no_grad():
        with pytest.raises(AssertionError, match="CSR adjacency is malformed"):
            E(X, csr_tensor(bad_crow, col, g["adj_values"], (64, 64), dev), graph_mode=True)
        with pytest.raises(AssertionError, match="CSR adjacency is malformed"):
            conv(X, (t(bad_crow, dev, torch.int64), t(col, dev, torch.int64)))
        with pytest.raises(AssertionError, match="index out of range"):
            conv(X, (t(crow, dev, torch.int64), t(np.where(np.arange(col.size) == 7, 64, col), dev, torch.int64)))
        # unsorted columns: fine as parallel-edge structure, refused with edge features
        row = int(np.argmax(np.diff(crow) >= 2))
        swapped = col.copy()
        swapped[[crow[row], crow[row] + 1]] = col[[crow[row] + 1, crow[row]]]
        adj = (t(crow, dev, torch.int64), t(swapped, dev, torch.int64))
        assert bool(torch.isfinite(conv(X, adj)).all())
        conv_e = FSW_conv(8, 6, edgefeat_dim=2, device=dev)
        ef = torch.zeros(col.size, 2, device=dev)
        with pytest.raises(AssertionError, match="strictly increasing column indices"):
            conv_e(X, adj, edge_features=ef)
        assert bool(torch.isfinite(conv_e(X, (adj[0], t(col, dev, torch.int64)), edge_features=ef)).all())
