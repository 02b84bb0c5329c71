"""Cartesian mode (nSlices x nFreqs) on the HIP kernels (csrc/embed_cart.hip): parity with the reference's goldens in float64 and
float32, every degree class, the input forms, gradients, and config-3-sized graphs against the diagonal module and the C oracle."""
import os

import numpy as np
import pytest
import torch

from fsw_gnn_amd import FSW_embedding, synth
from fsw_gnn_amd.graph import build_csr
from oracle import c_oracle

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")


def load_cases(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cases = {}
    for key in z.files:
        case, field = key.split("/")
        cases.setdefault(case, {})[field] = z[key]
    return cases


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def module_for(c, dt, **kw):
    S, F = c["V"].shape[0], c["freqs"].shape[0]
    mass = bool(c["mass"]) if "mass" in c else False
    E = FSW_embedding(d_in=c["X"].shape[-1], nSlices=S, nFreqs=F, collapse_freqs=bool(c["collapse"]), encode_total_mass=mass,
                      total_mass_encoding_method=str(c["method"]) if "method" in c else "plain",
                      total_mass_encoding_function=str(c["fn"]), total_mass_encoding_scale=float(c["scale"]),
                      enable_bias="bias" in c, device=DEV, dtype=dt, **kw)
    with torch.no_grad():
        E.projVecs.copy_(torch.from_numpy(c["V"]))
        E.freqs.copy_(torch.from_numpy(c["freqs"]))
        if "bias" in c:
            E.bias.copy_(torch.from_numpy(c["bias"]).reshape(E.bias.shape))
    return E


def case_inputs(c, dt, sparse=False):
    X = torch.from_numpy(c["X"]).to(dt).to(DEV)
    if "rows" in c:
        nr = c["out"].shape[0]
        idx = torch.from_numpy(np.stack([c["rows"], c["cols"]]).astype(np.int64)).to(DEV)
        W = torch.sparse_coo_tensor(idx, torch.from_numpy(c["vals"]).to(dt).to(DEV), (nr, c["X"].shape[0])).coalesce()
        return X, (W if sparse else W.to_dense()), True
    if "W" in c:
        return X, torch.from_numpy(c["W"]).to(dt).to(DEV), False
    return X, str(c["Wmode"]), False


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_cartesian_goldens(dt):
    for name, c in load_cases("cartesian").items():
        E = module_for(c, dt)
        X, W, gm = case_inputs(c, dt)
        with torch.no_grad():
            out = E(X, W, graph_mode=gm).cpu().numpy()
        ref = c["out"]
        assert out.shape == ref.shape, name
        bound = 1e-12 if dt == torch.float64 else 3e-5
        assert np.abs(out - ref).max() <= bound * max(1.0, np.abs(ref).max()), (name, np.abs(out - ref).max())
        if "rows" in c:
            # every class of the tuned forward on this graph: zero rows, register path, wavefront lines of 33 .. 2048 elements
            # (unit and weighted), generic kernel above
            deg = np.bincount(c["rows"], minlength=ref.shape[0])
            assert {0, 1, 32, 33, 256, 257, 2047, 2048, 2049} <= set(deg.tolist()) and deg.max() > 4096


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_sparse_w_equals_dense_w(dt):
    for name in ("graph_weighted", "graph_unit_collapsed"):
        c = load_cases("cartesian")[name]
        E = module_for(c, dt)
        X, Wd, _ = case_inputs(c, dt)
        _, Ws, _ = case_inputs(c, dt, sparse=True)
        with torch.no_grad():
            a, b = E(X, Wd, graph_mode=True), E(X, Ws, graph_mode=True)
        assert torch.equal(a, b), name


def test_collapse_order_and_shapes():
    c = load_cases("cartesian")["pc_batch_weighted"]
    X, W, _ = case_inputs(c, torch.float32)
    E = module_for(c, torch.float32)
    c2 = dict(c, collapse=np.array(True), bias=c["bias"].reshape(-1))
    E2 = module_for(c2, torch.float32)
    with torch.no_grad():
        a, b = E(X, W), E2(X, W)
    assert tuple(a.shape) == (3, 6, 4) and tuple(b.shape) == (3, 24)
    assert torch.equal(a.reshape(3, 24), b)                   # column s * F + f
    assert tuple(E.bias.shape) == (6, 4) and tuple(E2.bias.shape) == (24,)


def test_bias_shapes_and_state_dict_from_reference_arrays():
    E = FSW_embedding(d_in=5, nSlices=6, nFreqs=4, device=DEV, dtype=torch.float64)
    assert {k: tuple(v.shape) for k, v in E.state_dict().items()} == {"projVecs": (6, 5), "freqs": (4,), "bias": (6, 4)}
    Em = FSW_embedding(d_in=5, nSlices=6, nFreqs=4, collapse_freqs=True, encode_total_mass=True, device=DEV)
    assert tuple(Em.bias.shape) == (25,) and Em.d_out == 25     # the reference creates this shape and then fails on it
    c = load_cases("cartesian")["pc_batch_weighted"]
    E.load_state_dict({"projVecs": torch.from_numpy(c["V"]), "freqs": torch.from_numpy(c["freqs"]), "bias": torch.from_numpy(c["bias"])})
    X, W, _ = case_inputs(c, torch.float64)
    with torch.no_grad():
        assert np.abs(E(X, W).cpu().numpy() - c["out"]).max() < 1e-12
    # collapsed + mass + bias: column 0 gets bias[0], the others bias[1:]
    with torch.no_grad():
        Em.bias.copy_(torch.arange(25, dtype=torch.float32, device=DEV) * 0.01)
        Z = Em(torch.from_numpy(c["X"]).float().to(DEV), W.float())
        Em.bias.zero_()
        Z0 = Em(torch.from_numpy(c["X"]).float().to(DEV), W.float())
    assert torch.allclose(Z - Z0, (torch.arange(25, device=DEV) * 0.01).expand_as(Z), atol=1e-6)


def test_serialize_num_slices_matches():
    g = synth.er_multigraph(3000, 40000, seed=41)
    X = torch.from_numpy(synth.features(3000, 32, seed=42)).to(DEV)
    idx = torch.from_numpy(np.stack([g[1], g[0]]).astype(np.int64)).to(DEV)
    W = torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1], device=DEV), (3000, 3000)).coalesce()
    E = FSW_embedding(d_in=32, nSlices=16, nFreqs=5, collapse_freqs=True, encode_total_mass=True, device=DEV)
    with torch.no_grad():
        E.bias.normal_()
        a = E(X, W, graph_mode=True)
        b = E(X, W, graph_mode=True, serialize_num_slices=3)
    assert tuple(a.shape) == (3000, 81) and torch.allclose(a, b, rtol=0, atol=1e-6 * float(a.abs().max()))


def expanded_diagonal(E, d_in):
    D = FSW_embedding(d_in=d_in, d_out=E.nSlices * E.nFreqs, enable_bias=False, device=DEV)
    with torch.no_grad():
        D.projVecs.copy_(E.projVecs.repeat_interleave(E.nFreqs, dim=0))
        D.freqs.copy_(E.freqs.repeat(E.nSlices))
    return D


def test_config3_er_graph_against_diagonal_oracle_and_invariances():
    n, num_e, d, S, F = 1_000_000, 10_000_000, 128, 16, 16
    ei = torch.from_numpy(synth.er_multigraph(n, num_e, seed=51)).to(DEV)
    X = torch.from_numpy(synth.features(n, d, seed=52)).to(DEV)
    E = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, collapse_freqs=True, enable_bias=False, freqs_init='spread', device=DEV)
    D = expanded_diagonal(E, d)
    graph = build_csr(ei[1].contiguous(), ei[0].contiguous(), None, n, n)
    out = torch.empty((n, S * F), device=DEV)
    ref = torch.empty((n, S * F), device=DEV)
    with torch.no_grad():
        E.embed_cartesian_into(X, graph, out)
        D.embed_into(X, graph, ref)
    assert graph.max_degree > 0 and torch.isfinite(out).all()
    assert float((out - ref).abs().max()) < 3e-5 * float(ref.abs().max())
    # sampled rows against the C oracle (float64, expanded parameters), the longest row included
    deg = (graph.rowptr[1:] - graph.rowptr[:-1]).cpu().numpy()
    rows = np.unique(np.concatenate([np.arange(0, n, 7919), [int(deg.argmax())], np.nonzero(deg == 0)[0][:3]]))
    o = c_oracle.embed(X.cpu().numpy(), graph.rowptr.cpu().numpy(), graph.col[:num_e].cpu().numpy(), None,
                       D.projVecs.detach().cpu().numpy(), D.freqs.detach().cpu().numpy(), rows=rows)
    assert relerr(out[torch.from_numpy(rows).to(DEV)].cpu().numpy(), o) < 2e-5
    # edge order and x2 homogeneity
    p = torch.randperm(num_e, device=DEV)
    graph2 = build_csr(ei[1][p].contiguous(), ei[0][p].contiguous(), None, n, n)
    out2 = torch.empty_like(out)
    out3 = torch.empty_like(out)
    with torch.no_grad():
        E.embed_cartesian_into(X, graph2, out2)
        E.embed_cartesian_into((2 * X).contiguous(), graph, out3)
    assert float((out2 - out).abs().max()) <= 1e-6 * float(out.abs().max())
    assert float((out3 - 2 * out).abs().max()) <= 1e-6 * float(out.abs().max())


@pytest.mark.parametrize("weighted", [False, True])
def test_rmat_hub_rows_against_oracle(weighted):
    ei = synth.rmat_graph(14, 400_000, seed=61)
    n = 1 << 14
    rec, snd = torch.from_numpy(ei[1].astype(np.int64)).to(DEV), torch.from_numpy(ei[0].astype(np.int64)).to(DEV)
    w = torch.from_numpy(synth.edge_weights(rec.numel(), seed=62)).to(DEV) if weighted else None
    X = torch.from_numpy(synth.features(n, 32, seed=63)).to(DEV)
    E = FSW_embedding(d_in=32, nSlices=8, nFreqs=12, collapse_freqs=True, enable_bias=False, device=DEV)
    graph = build_csr(rec, snd, w, n, n)
    out = torch.empty((n, 96), device=DEV)
    with torch.no_grad():
        E.embed_cartesian_into(X, graph, out)
    deg = (graph.rowptr[1:] - graph.rowptr[:-1]).cpu().numpy()
    assert deg.max() > 2048
    rows = np.unique(np.concatenate([np.nonzero(deg > 32)[0][:300], np.argsort(deg)[-20:], np.arange(0, n, 331)]))
    nnz = int(graph.rowptr[-1])
    o = c_oracle.embed(X.cpu().numpy(), graph.rowptr.cpu().numpy(), graph.col[:nnz].cpu().numpy(),
                       graph.w[:nnz].cpu().numpy() if weighted else None, E.projVecs.detach().repeat_interleave(12, 0).cpu().numpy(),
                       E.freqs.detach().repeat(8).cpu().numpy(), rows=rows)
    got = out[torch.from_numpy(rows).to(DEV)].cpu().numpy()
    assert np.abs(got - o).max() < 3e-5 * np.abs(o).max()


def grad_module(c, dt):
    c = dict(c, method=np.array("plain"))
    E = module_for(c, dt, learnable_slices=True, learnable_freqs=True, learnable_total_mass_encoding_scale=bool(c["mass"]))
    return E


def run_grads(c, dt):
    E = grad_module(c, dt)
    X = torch.from_numpy(c["X"]).to(dt).to(DEV).requires_grad_(True)
    W = torch.from_numpy(c["W"]).to(dt).to(DEV).requires_grad_("gW" in c) if "W" in c else "unit"
    out = E(X, W)
    (out * torch.from_numpy(c["G"]).to(dt).to(DEV)).sum().backward()
    g = {"out": out.detach(), "gX": X.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad}
    if "gbias" in c:
        g["gbias"] = E.bias.grad
    if "gscale" in c:
        g["gscale"] = E.total_mass_encoding_scale.grad
    if "gW" in c:
        g["gW"] = W.grad
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def test_gradients_float64_against_reference():
    for name, c in load_cases("grads_cartesian").items():
        g = run_grads(c, torch.float64)
        for k, v in g.items():
            assert relerr(v, c[k]) < 1e-10, (name, k, relerr(v, c[k]))


def test_gradients_float32_against_float64():
    for name, c in load_cases("grads_cartesian").items():
        g64, g32 = run_grads(c, torch.float64), run_grads(c, torch.float32)
        for k in g64:
            assert relerr(g32[k], g64[k]) < 3e-5, (name, k, relerr(g32[k], g64[k]))


def test_gradcheck_small():
    E = FSW_embedding(d_in=3, nSlices=2, nFreqs=3, collapse_freqs=True, encode_total_mass=True, enable_bias=False,
                      learnable_slices=True, learnable_freqs=True, device=DEV, dtype=torch.float64)
    with torch.no_grad():
        E.freqs.copy_(torch.tensor([0.3, 0.9, 1.7], dtype=torch.float64))
    X = torch.from_numpy(synth.features(2 * 7, 3, seed=71).astype(np.float64).reshape(2, 7, 3)).to(DEV).requires_grad_(True)
    W = (torch.from_numpy(synth.edge_weights(14, seed=72).astype(np.float64)).reshape(2, 7).to(DEV) + 0.2).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x, w: E(x, w), (X, W), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_edge_features_with_cartesian_mode_raise():
    with pytest.raises(NotImplementedError, match="edge features"):
        FSW_embedding(d_in=4, d_edge=2, nSlices=2, nFreqs=3, device=DEV)


def mass_fn(m, fn):
    return m if fn == "identity" else (2 * m / (np.sqrt(m + 1) + 1) if fn == "sqrt" else np.log1p(m))


@pytest.mark.parametrize("F", [5, 8])
def test_unit_weights_with_mass_column_against_oracle(F):
    """Unit weights, collapsed output with the total-mass column and a bias: the register path's per-frequency (non-vector) form and
    the wavefront path, against the C oracle (expanded parameters) and f(degree) * scale + bias[0]."""
    S, d, n, num_e = 6, 16, 20000, 200_000
    E = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, collapse_freqs=True, encode_total_mass=True, total_mass_encoding_function="sqrt",
                      total_mass_encoding_scale=0.6, device=DEV)
    with torch.no_grad():
        E.bias.copy_(torch.from_numpy(synth.normal(81, 1, (S * F + 1,))).to(DEV))
    bias = E.bias.detach().cpu().numpy().astype(np.float64)
    Vx = E.projVecs.detach().repeat_interleave(F, 0).cpu().numpy()
    fx = E.freqs.detach().repeat(S).cpu().numpy()
    # a graph: ER rows (degrees 0 .. ~30) plus rows of 33 .. 80 neighbours (wavefront lines)
    ei = synth.er_multigraph(n, num_e, seed=82)
    extra_rec = np.repeat(np.arange(100), 33 + np.arange(100) % 48)
    extra_snd = synth.randint(83, 0, n, extra_rec.size)
    rec = torch.from_numpy(np.concatenate([ei[1], extra_rec]).astype(np.int64)).to(DEV)
    snd = torch.from_numpy(np.concatenate([ei[0], extra_snd]).astype(np.int64)).to(DEV)
    X = torch.from_numpy(synth.features(n, d, seed=84)).to(DEV)
    graph = build_csr(rec, snd, None, n, n)
    out = torch.empty((n, S * F + 1), device=DEV)
    with torch.no_grad():
        E.embed_cartesian_into(X, graph, out, bias=E.bias.detach())
    deg = (graph.rowptr[1:] - graph.rowptr[:-1]).cpu().numpy()
    assert deg.max() >= 80 and (deg == 0).any()
    rows = np.unique(np.concatenate([np.arange(0, n, 97), np.arange(100), np.nonzero(deg == 0)[0][:5]]))
    nnz = int(graph.rowptr[-1])
    o = c_oracle.embed(X.cpu().numpy(), graph.rowptr.cpu().numpy(), graph.col[:nnz].cpu().numpy(), None, Vx, fx, rows=rows)
    got = out[torch.from_numpy(rows).to(DEV)].cpu().numpy().astype(np.float64)
    assert np.abs(got[:, 1:] - (o + bias[1:])).max() < 3e-5 * np.abs(o).max()
    np.testing.assert_allclose(got[:, 0], mass_fn(deg[rows].astype(np.float64), "sqrt") * 0.6 + bias[0], rtol=1e-6, atol=1e-6)
    # the same through the public forward: point clouds of unit weights, one degree per call (register and wavefront lengths)
    for npts in (7, 32, 45):
        Xb = torch.from_numpy(synth.features(3 * npts, d, seed=85 + npts)).to(DEV).reshape(3, npts, d)
        with torch.no_grad():
            y = E(Xb).cpu().numpy().astype(np.float64)
        o = c_oracle.embed(Xb.reshape(-1, d).cpu().numpy(), np.arange(4) * npts, np.arange(3 * npts), None, Vx, fx)
        assert np.abs(y[:, 1:] - (o + bias[1:])).max() < 3e-5 * np.abs(o).max(), npts
        np.testing.assert_allclose(y[:, 0], mass_fn(float(npts), "sqrt") * 0.6 + bias[0], rtol=1e-6)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_empty_multisets_give_the_bias(dt):
    for kw in (dict(), dict(collapse_freqs=True, encode_total_mass=True, total_mass_encoding_method="homog_alt")):
        E = FSW_embedding(d_in=5, nSlices=3, nFreqs=4, device=DEV, dtype=dt, **kw)
        with torch.no_grad():
            E.bias.normal_()
        y = E(torch.zeros((2, 0, 5), dtype=dt, device=DEV))
        assert torch.equal(y, E.bias.detach().expand_as(y)), kw
