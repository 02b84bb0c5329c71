"""Pins the CPU oracle (oracle/fsw_oracle.py, oracle/fsw_oracle.c) to golden vectors captured from the
reference's own CPU path (oracle/make_goldens.py).  Runs without a GPU.

Tolerances: the oracle computes in float64 like the float64 goldens, with a different (CSR, per-row)
evaluation order, so agreement is expected near 1e-13; 1e-10 norm-wise is asserted.
"""
import numpy as np
import pytest

from oracle import fsw_oracle as O
from tests import cases
from tests.conftest import golden, relerr

TOL64 = 1e-10


def test_pointcloud_1k_config1():
    g = golden("pointcloud_1k")
    c = cases.pointcloud_1k()
    out = O.point_cloud_forward(c["X"][None], None, c["V"], c["freqs"])[0]
    assert relerr(out, g["out_f64"]) < TOL64
    # the reference's own float32 output sits within its float32 accuracy floor of the float64 one
    assert relerr(g["out_f32"], g["out_f64"]) < 1e-5


def test_pointcloud_batch_weighted_padding_zero_weight():
    g = golden("pointcloud_batch")
    out = O.point_cloud_forward(g["X"], g["W"], g["V"], g["freqs"]) + g["bias"].astype(np.float64)
    assert relerr(out, g["out_f64"]) < TOL64
    n = g["X"].shape[1]
    outu = O.point_cloud_forward(g["X"], np.full(g["W"].shape, 1.0 / n), g["V"], g["freqs"]) + g["bias"].astype(np.float64)
    assert relerr(outu, g["out_f64_uniform"]) < TOL64


def _tiny_csr(g, which="adj"):
    idx = g["adj_indices"] if which != "adj2" else g["adj2_indices"]
    vals = {"adj": g["adj_values"], "adj2": g["adj2_values"], "adj3": g["adj3_values"]}[which]
    return O.csr_from_coo(idx[0], idx[1], vals, 64)


def test_tiny_graph_adjacency_matches_reference_coalesce():
    g = golden("tiny_graph")
    rowptr, col, w, indeg = O.coalesce_edge_index(g["edge_index"], 64)
    rp, cl, vv = _tiny_csr(g)
    assert np.array_equal(rowptr, rp) and np.array_equal(col, cl) and np.array_equal(w, vv)
    assert np.array_equal(indeg, g["in_degrees"])
    assert (np.diff(rowptr)[56:] == 0).all() and w.max() >= 2.0      # isolated rows and duplicate edges exist
    rowptr2, col2, w2, _ = O.coalesce_edge_index(g["edge_index"], 64, self_loop_weight=0.5, edge_weighting="gcn")
    rp2, cl2, vv2 = _tiny_csr(g, "adj2")
    assert np.array_equal(rowptr2, rp2) and np.array_equal(col2, cl2)
    assert relerr(w2, vv2) < 1e-14


@pytest.mark.parametrize("fn", ["identity", "sqrt", "log"])
@pytest.mark.parametrize("method", ["plain", "homog", "homog_alt"])
def test_tiny_graph_total_mass_encodings(fn, method):
    g = golden("tiny_graph")
    rp, cl, vv = _tiny_csr(g)
    out = O.fsw_embedding_forward(g["X"], rp, cl, vv, g["V"], g["freqs"], bias=g["bias"], encode_total_mass=True,
                                  total_mass_encoding_function=fn, total_mass_encoding_method=method,
                                  total_mass_encoding_scale=0.7)
    assert relerr(out, g["out_%s_%s" % (fn, method)]) < TOL64


def test_tiny_graph_variants():
    g = golden("tiny_graph")
    rp, cl, vv = _tiny_csr(g)
    base = O.fsw_embedding_forward(g["X"], rp, cl, vv, g["V"], g["freqs"])
    assert relerr(base, g["out_plain_nomass_nobias"]) < TOL64
    assert np.abs(base[56:]).max() == 0.0                            # zero in-degree -> zero embedding row
    tau3 = O.fsw_embedding_forward(g["X"], rp, cl, vv, g["V"], g["freqs"], total_mass_pad_thresh=3.0)
    assert relerr(tau3, g["out_tau3"]) < TOL64
    rp2, cl2, vv2 = _tiny_csr(g, "adj2")
    assert relerr(O.fsw_embedding_forward(g["X"], rp2, cl2, vv2, g["V"], g["freqs"]), g["out_gcn_selfloop"]) < TOL64
    rp3, cl3, vv3 = _tiny_csr(g, "adj3")
    assert relerr(O.fsw_embedding_forward(g["X"], rp3, cl3, vv3, g["V"], g["freqs"]), g["out_weighted"]) < TOL64
    wm = O.fsw_embedding_forward(g["X"], rp3, cl3, vv3, g["V"], g["freqs"], bias=g["bias"], encode_total_mass=True,
                                 total_mass_encoding_scale=0.7)
    assert relerr(wm, g["out_weighted_mass"]) < TOL64


def test_duplicates_equal_separate_unit_elements():
    """Property used by the HIP CSR build: k parallel edges == one edge of weight k."""
    g = golden("tiny_graph")
    ei = g["edge_index"]
    order = np.argsort(ei[1], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=64))])
    out = O.fsw_embedding_forward(g["X"], rowptr, ei[0][order], np.ones(ei.shape[1]), g["V"], g["freqs"])
    assert relerr(out, g["out_plain_nomass_nobias"]) < TOL64


def test_conv10k_config2():
    g = golden("conv10k")
    c = cases.conv10k()
    rowptr, col, w, indeg = O.coalesce_edge_index(c["edge_index"], c["n"])
    assert w.shape[0] == int(g["nnz_coalesced"])
    emb = O.fsw_embedding_forward(c["X"], rowptr, col, w, c["V"], c["freqs"], encode_total_mass=True)
    rows = g["rows"]
    assert relerr(emb[rows], g["emb_rows_f64"]) < TOL64
    assert relerr(np.linalg.norm(emb, axis=0), g["emb_colnorm_f64"]) < TOL64
    y = O.conv_tail(emb, c["X"].astype(np.float64), linear_weight=c["lin_w"], linear_bias=c["lin_b"])
    assert relerr(y[rows], g["conv_rows_f64"]) < TOL64
    assert abs(np.linalg.norm(y) - float(g["conv_norm_f64"])) / float(g["conv_norm_f64"]) < TOL64
    # accuracy floor of the reference's float32 path against its own float64 path (documented in DESIGN.md)
    assert relerr(g["emb_rows_f32"], g["emb_rows_f64"]) < 1e-5


def test_rmat14_skewed_degrees():
    g = golden("rmat14")
    c = cases.rmat(14)
    rowptr, col, w, indeg = O.coalesce_edge_index(c["edge_index"], c["n"])
    assert w.shape[0] == int(g["nnz_coalesced"])
    assert np.diff(rowptr).max() > 1000                               # hubs present
    rows = g["rows"]
    # evaluate only the sampled rows (plus nothing else): build a sub-CSR
    deg = np.diff(rowptr)[rows]
    sub_rp = np.concatenate([[0], np.cumsum(deg)])
    idx = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows])
    emb = O.fsw_embedding_forward(c["X"], sub_rp, col[idx], w[idx], c["V"], c["freqs"], encode_total_mass=True)
    assert relerr(emb, g["emb_rows_f64"]) < TOL64


def test_segcumsum_vectors():
    g = golden("segcumsum")
    for tag, tol in (("f64", 1e-13), ("f32", 1e-5)):
        got = O.segcumsum(g["values_" + tag], g["ids"])
        assert relerr(got, g["slow_" + tag]) == 0.0                   # same left-to-right order as segcumsum_slow
        assert relerr(got, g["out_" + tag]) < tol                     # reference log-step scan, different rounding


@pytest.mark.parametrize("tag,which", [("unit", "adj"), ("weighted", "adj3")])
def test_backward_oracle_matches_reference_autograd(tag, which):
    """The analytic gradients of the oracle against the reference's autograd (float64 goldens, tiny graph)."""
    g = golden("tiny_graph")
    gg = golden("grads_tiny")
    rp, cl, vv = _tiny_csr(g, which)
    R = gg["R"]
    gX, gV, gxi = O.fsw_embed_csr_backward(g["X"], rp, cl, vv, g["V"], gg["freqs"], R[:, 1:])
    assert relerr(gX, gg["gX_" + tag]) < 1e-10
    assert relerr(gV, gg["gV_" + tag]) < 1e-10
    assert relerr(gxi, gg["gfreqs_" + tag]) < 1e-10
    assert relerr(R.sum(axis=0), gg["gbias_" + tag]) < 1e-12
    mass = np.zeros(64)
    np.add.at(mass, np.repeat(np.arange(64), np.diff(rp)), vv)
    assert abs((R[:, 0] * mass).sum() - float(gg["gscale_" + tag])) < 1e-10 * abs(float(gg["gscale_" + tag]))


def test_backward_oracle_conv10k():
    gg = golden("grads_conv10k")
    c = cases.conv10k()
    rowptr, col, w, _ = O.coalesce_edge_index(c["edge_index"], c["n"])
    X = c["X"].astype(np.float64)
    emb = O.fsw_embedding_forward(X, rowptr, col, w, c["V"], c["freqs"], encode_total_mass=True)
    Rc = cases.synth.normal(92, 1, (c["n"], c["out_ch"]), dtype=np.float64)
    h = np.concatenate([emb, X], axis=1)
    Wl, bl = c["lin_w"].astype(np.float64), c["lin_b"].astype(np.float64)
    pre = h @ Wl.T + bl
    gpre = Rc * np.where(pre >= 0, 1.0, 0.2)                                   # LeakyReLU(0.2) backward
    gh = gpre @ Wl
    E = c["embed_dim"]
    gX_e, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, col, w, c["V"], c["freqs"], gh[:, 1:E])
    gX = gX_e + gh[:, E:]
    assert relerr(gX[gg["rows"]], gg["gX_rows"]) < 1e-9
    assert relerr(gV, gg["gV"]) < 1e-9 and relerr(gxi, gg["gfreqs"]) < 1e-9
    assert relerr(gpre.T @ h, gg["gW"]) < 1e-9


@pytest.mark.parametrize("tag,slw", [("plain", 0.0), ("selfloop", 0.5)])
def test_edge_features_oracle_forward_and_backward(tag, slw):
    """Edge features (reference fsw_embedding.py:934-968, fsw_conv.py:419-439) incl. duplicate edges and self loops."""
    g, ge = golden("tiny_graph"), golden("edgefeat_tiny")
    n, d, de = 64, 8, 3
    rowptr, col, w, _, ef, slot = O.coalesce_edge_index(g["edge_index"], n, self_loop_weight=slw, edge_features=ge["edge_features"])
    X = g["X"].astype(np.float64)
    emb = O.fsw_embedding_forward(X, rowptr, col, w, ge["V"], ge["freqs"], encode_total_mass=True, edge_feat=ef)
    assert relerr(emb, ge["emb_" + tag]) < TOL64
    Wl, bl = ge["lin_w"].astype(np.float64), ge["lin_b"].astype(np.float64)
    pre = np.concatenate([emb, X], axis=1) @ Wl.T + bl
    assert relerr(np.where(pre >= 0, pre, 0.2 * pre), ge["y_" + tag]) < TOL64
    gpre = ge["R"] * np.where(pre >= 0, 1.0, 0.2)
    gh = gpre @ Wl
    E = emb.shape[1]
    gX, gV, gxi, gef = O.fsw_embed_csr_backward(X, rowptr, col, w, ge["V"], ge["freqs"], gh[:, 1:E], edge_feat=ef)
    assert relerr(gX + gh[:, E:], ge["gX_" + tag]) < 1e-10
    assert relerr(gV, ge["gV_" + tag]) < 1e-10 and relerr(gxi, ge["gfreqs_" + tag]) < 1e-10
    assert relerr(gef[slot], ge["gEF_" + tag]) < 1e-10                       # every duplicate receives its slot's gradient


@pytest.mark.parametrize("tag", ["unit", "general"])
def test_tied_keys_contract(tag):
    """Equal keys (tests/golden/ties.npz: rows of 0 .. 130 neighbours, keys from {-1, -0.0, 0.0, 0.5, 2.0}, projVecs = I, one sender
    per entry, so gX is the gradient of every key).  The reference's order among equal keys is unspecified (an unstable
    torch.sort): when the fixture was generated its per-entry gX differed from entry order already in the row of 5 neighbours, so
    no per-entry gradient of the reference is pinned here.  Pinned at 1e-12 is what every order agrees on -- out, gfreqs and the sum
    of the key gradients over every group of equal keys (for the zero keys of a mass-deficient row the pad element is part of the
    group and takes an order-dependent share: those groups are left out, see oracle/make_goldens.py::case_ties).
    Entry order among equal keys (a stable sort, -0.0 == 0.0, the pad element last) is this project's own rule; the oracle states
    it, and the second half of this test pins the oracle to it with a direct evaluation that does not sort at all."""
    g = golden("ties")
    degs, X, V, fr, R = g["degrees"], g["X"], g["V"], g["freqs"], g["R"]
    n, S = X.shape
    rowptr = np.concatenate([[0], np.cumsum(degs)])
    col = np.arange(n)
    w = np.ones(n) if tag == "unit" else g["w_general"]
    assert 0 in degs and w.min() == (1.0 if tag == "unit" else 0.0) and np.signbit(X[X == 0]).any() and not np.signbit(X[X == 0]).all()
    out = O.fsw_embedding_forward(X, rowptr, col, w, V, fr)
    gX, gV, gxi, gkey = O.fsw_embed_csr_backward(X, rowptr, col, w, V, fr, R, return_gkey=True)
    assert np.array_equal(gX, gkey)                                  # projVecs = I, one sender per entry
    scale = np.abs(gkey).max()
    assert np.abs(out - g["out_" + tag]).max() <= 1e-12 * np.abs(g["out_" + tag]).max()
    assert np.abs(gxi - g["gfreqs_" + tag]).max() <= 1e-12 * np.abs(g["gfreqs_" + tag]).max()
    valid = g["tie_sums_valid_general"] if tag == "general" else np.ones((n, S), dtype=bool)
    rec = np.repeat(np.arange(degs.size), degs)
    deficient = np.bincount(rec, weights=w, minlength=degs.size) < 1.0
    assert np.array_equal(~valid, deficient[rec][:, None] & (X == 0.0))   # the zero keys of the deficient rows, nothing else
    assert (deficient & (degs > 0)).sum() == (0 if tag == "unit" else 3) and valid[X == 0.0].any()
    sums = np.zeros_like(gkey)
    # the rule itself, without a sort: the rank of an element is the number of elements that are smaller or equal and earlier
    direct = np.zeros_like(gkey)
    for r, (a, b) in enumerate(zip(rowptr[:-1], rowptr[1:])):
        if a == b:
            continue
        m = w[a:b].sum()
        wt = np.concatenate([w[a:b], [max(1.0 - m, 0.0)]]) / max(m, 1.0)
        for s in range(S):
            k = np.concatenate([X[a:b, s], [0.0]])
            sums[a:b, s] = ((k[:-1, None] == k[None, :-1]) * gkey[a:b, s][None, :]).sum(axis=1)
            pos = np.arange(k.size)
            ahead = (k[None, :] < k[:, None]) | ((k[None, :] == k[:, None]) & (pos[None, :] <= pos[:, None]))   # [t, u]: u not after t
            c = (ahead * wt[None, :]).sum(axis=1)
            delta = 2 * wt * np.sinc(fr[s] * wt) * np.cos(np.pi * fr[s] * (2 * c - wt))
            direct[a:b, s] = (R[r, s] * (1 + fr[s]) * delta)[:-1]
    assert np.abs(sums - g["tie_sums_" + tag])[valid].max() <= 1e-12 * scale
    assert np.abs(direct - gkey).max() <= 1e-12 * scale


def test_signed_frequencies():
    """Frequencies of both signs (tests/golden/signed_freqs.npz, oracle/make_goldens.py::case_signed_freqs): the reference's float64
    autograd at xi = -13 .. 13 with -1, -0.0 and +-1e-3 among them, rows of 1 .. 50 neighbours, unit weights, general weights with a
    row of total mass 0.4, and the general weights at tau = 3.  Python oracle forward and backward, C oracle forward (the fixture's
    inputs are float32 values, which the C oracle reads).  Every coefficient carries the factor (1 + xi): the column at xi = -1 is
    exactly zero in the reference and in both oracles.  The oracle has no dL/dW: gW is compared on the GPU
    (tests/test_hip_signed_freqs.py)."""
    from oracle import c_oracle as C
    g = golden("signed_freqs")
    degs, snd, X, V, fr, R = g["degrees"], g["senders"], g["X"], g["V"], g["freqs"], g["R"]
    rowptr = np.concatenate([[0], np.cumsum(degs)])
    assert (fr < 0).sum() == 5 and np.signbit(fr[5]) and fr[5] == 0 and fr[2] == -1.0 and 2 * degs.max() <= snd.size
    mass = np.add.reduceat(g["w_general"], rowptr[:-1])
    assert abs(mass[2] - 0.4) < 1e-7 and (mass[3:] > 3).all()
    for tag, w, tau in (("unit", np.ones(snd.size), 1.0), ("general", g["w_general"], 1.0), ("general_tau3", g["w_general"], 3.0)):
        ref = g["out_" + tag]
        assert np.abs(ref[:, 2]).max() == 0.0 and np.abs(ref[:, [0, 1, 3, 4]]).min() > 0
        out = O.fsw_embedding_forward(X, rowptr, snd, w, V, fr, total_mass_pad_thresh=tau)
        assert relerr(out, ref) < TOL64, tag
        cout = C.embed(X, rowptr, snd, w, V, fr, tau=tau)
        assert relerr(cout, ref) < TOL64, tag
        assert np.abs(out[:, 2]).max() == 0.0 and np.abs(cout[:, 2]).max() == 0.0
        for c in range(fr.size):                                       # per column: no frequency hides in a row norm
            if c != 2:
                assert relerr(out[:, c], ref[:, c]) < TOL64 and relerr(cout[:, c], ref[:, c]) < TOL64, (tag, c)
        gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, snd, w, V, fr, R, total_mass_pad_thresh=tau)
        assert relerr(gX, g["gX_" + tag]) < 1e-10 and relerr(gV, g["gV_" + tag]) < 1e-10, tag
        assert relerr(gxi, g["gfreqs_" + tag]) < 1e-10 and np.abs(gxi - g["gfreqs_" + tag]).max() < 1e-10 * np.abs(gxi).max(), tag
        assert g["gfreqs_" + tag][2] != 0 and np.abs(gV[2]).max() == 0.0 and np.abs(g["gV_" + tag][2]).max() == 0.0
