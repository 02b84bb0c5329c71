"""GPU parity tests: the HIP path (through the C ABI of libfsw_hip.so) against golden vectors captured from
the reference's CPU path and against the CPU oracle on the same seeded inputs.

Tolerance: the north star asks for 1e-5 relative in float32.  As SURVEY.md 8(c) records, the reference's own
float32 output differs from its float64 output by ~5e-6 norm-wise at S=256 'spread' frequencies, so the
criterion is norm-wise relative error <= 1e-5 against the float64 golden (TOL below).
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import fsw_oracle as O
from tests import cases
from tests.conftest import golden, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def make_embedding(dev, V, freqs, bias=None, scale=None, **kw):
    from fsw_gnn_amd import FSW_embedding
    S, d = V.shape
    encode = kw.get("encode_total_mass", False)
    E = FSW_embedding(d_in=d, d_out=S + (1 if encode else 0), device=dev, **kw)
    with torch.no_grad():
        if E.d_edge == 0:
            E.projVecs.copy_(t(V, dev))
        E.freqs.copy_(t(freqs, dev))
        if bias is not None and E.enable_bias:
            E.bias.copy_(t(bias, dev))
        if scale is not None:
            E.total_mass_encoding_scale.fill_(scale)
    return E


def sparse_adj(idx, vals, shape, dev):
    return torch.sparse_coo_tensor(torch.from_numpy(idx).to(dev), t(vals, dev), shape).coalesce()


# ---------------------------------------------------------------------------------------------------
def test_projection_mfma_vs_float64(dev):
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(0)
    # d <= 256 with 16-byte aligned rows: bf16x3 matrix-core kernels (k-blocked weight slabs above 128); the rest: generic kernel
    for n, d, S in ((1000, 64, 32), (777, 13, 70), (4096, 128, 256), (130, 3, 129), (3000, 192, 256), (5000, 256, 256), (999, 256, 40),
                    (640, 200, 130), (300, 260, 64)):
        X = rng.standard_normal((n, d)).astype(np.float32)
        V = rng.standard_normal((S, d)).astype(np.float32)
        Xd, Vd = t(X, dev), t(V, dev)
        ldp = (S + 63) // 64 * 64
        Xp = torch.full((n, ldp), float("nan"), device=dev)
        stats = torch.zeros(8, dtype=torch.int32, device=dev)
        xc = torch.full((n, d + 3), -1.0, device=dev)
        rc = L.fsw_project_f32(Xd.data_ptr(), n, d, d, Vd.data_ptr(), S, d, Xp.data_ptr(), ldp, xc.data_ptr() + 4, d + 3,
                               stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert torch.equal(xc[:, 1:d + 1], Xd) and (xc[:, 0] == -1).all() and (xc[:, d + 1:] == -1).all()
        ref = X.astype(np.float64) @ V.astype(np.float64).T
        assert relerr(Xp[:, :S].cpu().numpy(), ref) < 5e-7      # fp32 fma chain over d terms
        assert int(stats[0]) == 0
    Xd[5, 1] = float("inf")
    L.fsw_project_f32(Xd.data_ptr(), n, d, d, Vd.data_ptr(), S, d, Xp.data_ptr(), ldp, None, 0, stats.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    assert int(stats[0]) & _lib.FLAG_X_NONFINITE
    # narrow outputs without the feature copy (one rank's block of a slice-sharded layer): k_project_narrow, a wavefront per 32-row
    # tile, no LDS -- one and two slabs, row counts that are no multiple of 32, padded row strides, the non-finite flag
    for n, d, S, ldx in ((1000, 64, 32, 64), (5003, 128, 33, 128), (70, 16, 5, 20), (4097, 128, 64, 132), (33, 32, 64, 32)):
        X = rng.standard_normal((n, ldx)).astype(np.float32)
        V = rng.standard_normal((S, d)).astype(np.float32)
        Xd, Vd = t(X, dev), t(V, dev)
        ldp = (S + 31) // 32 * 32
        Xp = torch.full((n, ldp), float("nan"), device=dev)
        stats = torch.zeros(8, dtype=torch.int32, device=dev)
        rc = L.fsw_project_f32(Xd.data_ptr(), n, d, ldx, Vd.data_ptr(), S, d, Xp.data_ptr(), ldp, None, 0, stats.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        ref = X[:, :d].astype(np.float64) @ V.astype(np.float64).T
        assert relerr(Xp[:, :S].cpu().numpy(), ref) < 5e-7
        assert torch.isfinite(Xp).all() and int(stats[0]) == 0
        Xd[n - 1, d - 1] = float("nan")
        L.fsw_project_f32(Xd.data_ptr(), n, d, ldx, Vd.data_ptr(), S, d, Xp.data_ptr(), ldp, None, 0, stats.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
        assert int(stats[0]) & _lib.FLAG_X_NONFINITE


def test_graph_build_matches_oracle_adjacency(dev):
    from fsw_gnn_amd import build_csr
    g = golden("tiny_graph")
    ei = g["edge_index"]
    gr = build_csr(t(ei[1], dev, torch.int64), t(ei[0], dev, torch.int64), None, 64, 64)
    rowptr = gr.rowptr.cpu().numpy()
    col = gr.col.cpu().numpy()
    deg_ref = np.bincount(ei[1], minlength=64)
    assert np.array_equal(np.diff(rowptr), deg_ref)
    for r in range(64):                                   # same multiset of senders per recipient
        assert sorted(col[rowptr[r]:rowptr[r + 1]]) == sorted(ei[0][ei[1] == r])
    perm = gr.perm.cpu().numpy()
    bins = gr.bin_start.cpu().numpy()
    assert sorted(perm) == list(range(64))
    for b in range(len(bins) - 1):
        for r in perm[bins[b]:bins[b + 1]]:
            assert min(deg_ref[r], 33) == b
    assert gr.max_degree == deg_ref.max() and gr.stats()[2] == (deg_ref == 0).sum()
    # out-of-range endpoints are flagged, not dereferenced
    bad = ei.copy()
    bad[0, 3] = 64
    gr2 = build_csr(t(bad[1], dev, torch.int64), t(bad[0], dev, torch.int64), None, 64, 64)
    assert gr2.flags & 1


@pytest.mark.parametrize("rows,edges,weighted,bad", [
    (200_000, 1_000_000, False, 0),       # one partition pass (7 upper bits), 98 buckets
    (65_535, 400_000, True, 17),          # rows + 1 (the sentinel) starts a bucket of its own; weights; invalid edges
    (70_001, 300_000, False, 5),          # last bucket partly filled, invalid edges share it with valid rows
    (3_000_000, 2_000_000, False, 0),     # 11 upper bits: two partition passes, bucket starts from the sorted keys
    (100_000, 600_000, True, 0),
])
def test_two_level_graph_build_equals_lsd_build(dev, rows, edges, weighted, bad):
    """fsw_graph_build_two_level (partition pass + one workgroup per bucket of 2048 rows) against fsw_graph_build (three LSD
    passes): the same rowptr / col / w / perm / bin_start / stats, entry for entry, including a hub row and out-of-range
    edges (which both builds drop and flag)."""
    from fsw_gnn_amd import build_csr
    g = torch.Generator(device="cpu").manual_seed(rows + edges)
    rec = torch.randint(0, rows, (edges,), generator=g)
    snd = torch.randint(0, rows, (edges,), generator=g)
    rec[:5000] = 12345                                    # a hub row: 5000 edges in one bucket
    if bad:
        idx = torch.randint(0, edges, (bad,), generator=g)
        rec[idx[: bad // 2]] = rows + 3
        snd[idx[bad // 2:]] = -1
    w = (torch.rand(edges, generator=g) + 0.01) if weighted else None
    rec, snd = rec.to(dev), snd.to(dev)
    wd = None if w is None else w.to(dev)
    a = build_csr(rec, snd, wd, rows, rows, want_invperm=True, algo="lsd")
    b = build_csr(rec, snd, wd, rows, rows, want_invperm=True, algo="two_level")
    sa, sb = a.stats_dev.cpu().tolist(), b.stats_dev.cpu().tolist()
    assert sa == sb, (sa, sb)
    nnz = sa[6]
    assert nnz == edges - bad and bool(sa[0] & 1) == bool(bad)
    assert torch.equal(a.rowptr, b.rowptr)
    assert torch.equal(a.col[:nnz], b.col[:nnz])
    if weighted:
        assert torch.equal(a.w[:nnz], b.w[:nnz])
    assert torch.equal(a.bin_start, b.bin_start)
    # perm lists every bin's rows in an order that depends on atomics between workgroups: compare as sets per bin
    bs = a.bin_start.cpu().tolist()
    pa, pb = a.perm.cpu(), b.perm.cpu()
    for lo, hi in zip(bs[:-1], bs[1:]):
        if hi > lo:
            assert torch.equal(torch.sort(pa[lo:hi]).values, torch.sort(pb[lo:hi]).values)
    # and against torch: stable sort by recipient
    ok = (rec >= 0) & (rec < rows) & (snd >= 0) & (snd < rows)
    order = torch.sort(rec[ok], stable=True).indices
    assert torch.equal(b.col[:nnz].long(), snd[ok][order])
    assert torch.equal(b.rowptr.long(), torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.bincount(rec[ok], minlength=rows).cumsum(0)]))
    # row chunks (the multi-GPU pipeline bins the rows per chunk): the same tables from both builds
    if rows == 200_000:
        ca = build_csr(rec, snd, wd, rows, rows, want_invperm=True, chunk_rows=65536, algo="lsd")
        cb = build_csr(rec, snd, wd, rows, rows, want_invperm=True, chunk_rows=65536, algo="two_level")
        assert ca.num_chunks == 4 and torch.equal(ca.bin_start, cb.bin_start) and torch.equal(ca.col[:nnz], cb.col[:nnz])
        assert torch.equal(torch.sort(ca.perm).values, torch.sort(cb.perm).values)


def test_tiny_graph_all_variants(dev):
    g = golden("tiny_graph")
    X = t(g["X"], dev)
    adj = sparse_adj(g["adj_indices"], g["adj_values"], (64, 64), dev)
    with torch.no_grad():
        E = make_embedding(dev, g["V"], g["freqs"], enable_bias=False)
        out = E(X, adj, graph_mode=True).cpu().numpy()
        assert relerr(out, g["out_plain_nomass_nobias"]) < TOL
        assert np.abs(out[56:]).max() == 0.0                                  # isolated recipients
        for fn in ("identity", "sqrt", "log"):
            for method in ("plain", "homog", "homog_alt"):
                E = make_embedding(dev, g["V"], g["freqs"], bias=g["bias"], scale=0.7, encode_total_mass=True,
                                   total_mass_encoding_function=fn, total_mass_encoding_method=method,
                                   total_mass_encoding_scale=0.7)
                got = E(X, adj, graph_mode=True).cpu().numpy()
                assert relerr(got, g["out_%s_%s" % (fn, method)]) < TOL, (fn, method)
        E = make_embedding(dev, g["V"], g["freqs"], enable_bias=False, total_mass_pad_thresh=3.0)
        assert relerr(E(X, adj, graph_mode=True).cpu().numpy(), g["out_tau3"]) < TOL
        E = make_embedding(dev, g["V"], g["freqs"], enable_bias=False)
        adj2 = sparse_adj(g["adj2_indices"], g["adj2_values"], (64, 64), dev)
        assert relerr(E(X, adj2, graph_mode=True).cpu().numpy(), g["out_gcn_selfloop"]) < TOL
        adj3 = sparse_adj(g["adj_indices"], g["adj3_values"], (64, 64), dev)
        assert relerr(E(X, adj3, graph_mode=True).cpu().numpy(), g["out_weighted"]) < TOL
        assert relerr(E(X, adj3.to_dense(), graph_mode=True).cpu().numpy(), g["out_weighted"]) < TOL   # dense W
        E = make_embedding(dev, g["V"], g["freqs"], bias=g["bias"], scale=0.7, encode_total_mass=True,
                           total_mass_encoding_scale=0.7)
        assert relerr(E(X, adj3, graph_mode=True).cpu().numpy(), g["out_weighted_mass"]) < TOL
        # serialize_num_slices changes nothing (property 2)
        a = E(X, adj3, graph_mode=True)
        b = E(X, adj3, graph_mode=True, serialize_num_slices=5)
        assert torch.equal(a, b)


def test_conv_layer_gcn_selfloops_matches_reference_adjacency(dev):
    """FSW_conv.build_graph with self loops + 'gcn' weighting == the reference's coalesced adjacency."""
    from fsw_gnn_amd import FSW_conv
    g = golden("tiny_graph")
    conv = FSW_conv(8, 16, encode_vertex_degrees=False, mlp_layers=0, concat_self=False, bias=False,
                    self_loop_weight=0.5, edge_weighting="gcn", device=dev)
    with torch.no_grad():
        conv.fsw_embed.projVecs.copy_(t(g["V"], dev))
        conv.fsw_embed.freqs.copy_(t(g["freqs"], dev))
        out = conv(t(g["X"], dev), t(g["edge_index"], dev, torch.int64)).cpu().numpy()
    assert relerr(out, g["out_gcn_selfloop"]) < TOL


def test_pointcloud_config1_and_batches(dev):
    g = golden("pointcloud_1k")
    c = cases.pointcloud_1k()
    with torch.no_grad():
        E = make_embedding(dev, c["V"], c["freqs"])
        out = E(t(c["X"], dev)).cpu().numpy()
    assert out.shape == (32,)
    assert relerr(out, g["out_f64"]) < TOL
    gb = golden("pointcloud_batch")
    with torch.no_grad():
        E = make_embedding(dev, gb["V"], gb["freqs"], bias=gb["bias"])
        out = E(t(gb["X"], dev), t(gb["W"], dev)).cpu().numpy()
        outu = E(t(gb["X"], dev), "uniform").cpu().numpy()
        # graph mode == expanded non-graph mode (reference docstring fsw_embedding.py:603-605)
        Wg = t(gb["W"], dev)
        outg = E(t(gb["X"][0], dev), Wg[0:1].expand(3, -1).contiguous() * 1.0, graph_mode=True).cpu().numpy()
    assert relerr(out, gb["out_f64"]) < TOL
    assert relerr(outu, gb["out_f64_uniform"]) < TOL
    assert relerr(outg[0], gb["out_f64"][0]) < TOL


def _conv_from_case(c, dev):
    from fsw_gnn_amd import FSW_conv
    conv = FSW_conv(c["d"], c["out_ch"], embed_dim=c["embed_dim"], device=dev)
    with torch.no_grad():
        conv.fsw_embed.projVecs.copy_(t(c["V"], dev))
        conv.fsw_embed.freqs.copy_(t(c["freqs"], dev))
        conv.mlp[0].weight.copy_(t(c["lin_w"], dev))
        conv.mlp[0].bias.copy_(t(c["lin_b"], dev))
    return conv


def test_conv10k_config2(dev):
    g = golden("conv10k")
    c = cases.conv10k()
    conv = _conv_from_case(c, dev)
    X, ei = t(c["X"], dev), t(c["edge_index"], dev, torch.int64)
    with torch.no_grad():
        y = conv(X, ei)
        graph = conv.build_graph(ei, c["n"])
        emb = torch.empty((c["n"], c["embed_dim"]), device=dev)
        conv.fsw_embed.embed_into(X, graph, emb)
    rows = g["rows"]
    emb = emb.cpu().numpy()
    assert relerr(emb[rows], g["emb_rows_f64"]) < TOL
    assert relerr(np.linalg.norm(emb.astype(np.float64), axis=0), g["emb_colnorm_f64"]) < TOL
    assert np.array_equal(emb[:, 0], g["in_degrees"])                       # degree column is exact
    y = y.cpu().numpy()
    assert conv._fusable()                                                   # default FSW_conv -> fused Linear kernel
    assert relerr(y[rows], g["conv_rows_f64"]) < TOL
    conv.fuse_linear = False                                                 # unfused kernels + stock torch Linear
    with torch.no_grad():
        y2 = conv(X, ei).cpu().numpy()
    assert relerr(y2[rows], g["conv_rows_f64"]) < 2e-5
    assert relerr(y2, y) < 2e-6
    # not worse than the reference's own float32 path measured against its float64 path
    assert relerr(emb[rows], g["emb_rows_f64"]) <= 1.5 * relerr(g["emb_rows_f32"], g["emb_rows_f64"]) + 1e-6


def test_rmat14_long_rows_lds_and_global_paths(dev):
    g = golden("rmat14")
    c = cases.rmat(14)
    E = make_embedding(dev, c["V"], c["freqs"], encode_total_mass=True, enable_bias=False)
    from fsw_gnn_amd import build_csr
    ei = t(c["edge_index"], dev, torch.int64)
    with torch.no_grad():
        graph = build_csr(ei[1].contiguous(), ei[0].contiguous(), None, c["n"], c["n"])
        emb = torch.empty((c["n"], c["S"] + 1), device=dev)
        E.embed_into(t(c["X"], dev), graph, emb)
    st = graph.stats()
    assert st[4] > 0, "expected rows on the LDS path"
    emb = emb.cpu().numpy()
    assert relerr(emb[g["rows"]], g["emb_rows_f64"]) < TOL
    assert relerr(np.linalg.norm(emb.astype(np.float64), axis=0), g["emb_colnorm_f64"]) < TOL


def test_long_rows_weighted_and_global_scratch_path(dev):
    """Few very long neighbourhoods (FSW_readout shape): 3 graphs of 700 / 3000 / 5000 vertices, weighted and unit."""
    from fsw_gnn_amd import build_csr
    rng = np.random.default_rng(3)
    sizes = [700, 3000, 5000]
    n, d, S = sum(sizes), 16, 24
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=81)
    fr = cases.random_freqs(S, seed=82)
    gi = np.repeat(np.arange(3), sizes).astype(np.int64)
    w = (rng.random(n) + 0.1).astype(np.float32)
    w[gi == 0] *= 0.5 / w[gi == 0].sum()                        # first graph: total mass 0.5 < tau -> pad element
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    col = np.arange(n)
    for weights in (None, w):
        E = make_embedding(dev, V, fr, enable_bias=False)
        with torch.no_grad():
            graph = build_csr(t(gi, dev, torch.int64), t(col, dev, torch.int64), None if weights is None else t(weights, dev), 3, n)
            out = torch.empty((3, S), device=dev)
            E.embed_into(t(X, dev), graph, out)
        assert graph.stats()[5] == 2 and graph.stats()[4] == 1                # two global-path rows, one LDS row
        ref = C.embed(X, rowptr, col, weights, V, fr)
        assert relerr(out.cpu().numpy(), ref) < TOL


def test_merge_path_rows_beyond_one_partition_chunk_and_with_ties(dev):
    """csrc/merge_path.h on one neighbourhood of 2.2M vertices (an FSW_readout of a whole graph): 269 sorted blocks of 8192, nine
    merge levels with runs without a partner on several of them, more tile boundaries per level (538) than the 512 kept in LDS at a
    time; a second, shorter row whose features are drawn from 40 distinct vectors, so that almost every key is tied (merge path keeps
    ties in any order -- the readout must not care).  General weights (k_embed_mergepath_w, incl. a mass-deficient row) and unit
    weights (k_embed_giant on the same rows)."""
    from fsw_gnn_amd import build_csr
    rng = np.random.default_rng(41)
    sizes = [2_200_000, 50_000]
    n, d, S = sizes[0], 5, 4
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[:sizes[1]] = X[rng.integers(0, 40, size=sizes[1])]          # the second row reads vertices 0 .. 49 999: 40 distinct feature vectors
    V = cases.synth.unit_slices(S, d, seed=91)
    fr = cases.random_freqs(S, seed=92)
    rec = np.repeat(np.arange(2), sizes).astype(np.int64)
    snd = np.concatenate([rng.permutation(n), np.arange(sizes[1])]).astype(np.int64)
    w = (rng.random(rec.size) + 0.1).astype(np.float32)
    w[rec == 1] *= 0.7 / w[rec == 1].sum()                         # mass 0.7 < tau: the pad element carries 0.3
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    for weights in (w, None):
        E = make_embedding(dev, V, fr, enable_bias=False)
        with torch.no_grad():
            graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None if weights is None else t(weights, dev), 2, n)
            out = torch.empty((2, S), device=dev)
            E.embed_into(t(X, dev), graph, out)
        ref = C.embed(X, rowptr, snd, weights, V, fr)
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        assert relerr(got, ref) < TOL, (weights is None, merge_path, relerr(got, ref))
        assert np.abs(got - ref).max() < 3e-5 * np.abs(ref).max()


def test_mid_degree_rows_every_padded_network_size(dev):
    """Rows of in-degree 33..300: both ends of every padded register-path bin (csrc/embed_mid.hip, FSW_MID_SIZES), one
    row past the last bin on the LDS path; unit weights, general weights (incl. a mass-deficient row that receives the
    reference's pad element, and the weighted bins above 128 that stay on the LDS path), S not a multiple of 64, a zero
    frequency, bias and total-mass column."""
    from fsw_gnn_amd import build_csr, _lib
    rng = np.random.default_rng(21)
    sizes = [33, 40, 41, 48, 49, 64, 65, 80, 81, 96, 97, 128, 129, 160, 161, 192, 193, 255, 256, 257, 300, 35, 100]
    assert set(_lib.MID_SIZES) <= set(sizes)
    nrows, n, d, S = len(sizes), 600, 12, 270                     # > 256 slices: two chunk groups
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=85)
    fr = cases.random_freqs(S, seed=86)
    fr[5] = 0.0
    bias = rng.standard_normal(S + 1).astype(np.float32)
    rec = np.repeat(np.arange(nrows), sizes).astype(np.int64)
    snd = np.concatenate([rng.choice(n, size=k, replace=False) for k in sizes]).astype(np.int64)
    order = rng.permutation(rec.size)                           # edge list in random order: the build groups it
    w = (rng.random(rec.size) + 0.1).astype(np.float32)
    w[rec == 2] *= 0.4 / w[rec == 2].sum()                      # row 2: total mass 0.4 < tau = 1 -> pad element carries 0.6
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    for weights in (None, w):
        E = make_embedding(dev, V, fr, bias=bias, scale=0.7, encode_total_mass=True)
        with torch.no_grad():
            graph = build_csr(t(rec[order], dev, torch.int64), t(snd[order], dev, torch.int64),
                              None if weights is None else t(weights[order], dev), nrows, n)
            out = torch.empty((nrows, S + 1), device=dev)
            E.embed_into(t(X, dev), graph, out)
        st = graph.stats()
        assert st[_lib.STAT_NUM_LDS] == nrows and st[_lib.STAT_NUM_REG] == 0 and st[_lib.STAT_NUM_GLOBAL] == 0
        bs = graph.bin_start.cpu().numpy()
        assert bs[_lib.NUM_BINS] == nrows and bs[_lib.REG_MAX_DEG + 1] == 0
        assert np.diff(bs)[_lib.REG_MAX_DEG + 1:].tolist() == [3, 2, 2, 2, 2, 3, 2, 2, 3, 2, 0, 0, 0, 0, 0, 0, 0]   # rows per mid bin, three LDS bins, four hub bins, global
        ref = O.fsw_embedding_forward(X, rowptr, snd, np.ones(rec.size) if weights is None else weights.astype(np.float64), V, fr,
                                      bias=bias, encode_total_mass=True, total_mass_encoding_scale=0.7)
        assert relerr(out.cpu().numpy(), ref) < TOL
        assert np.abs(out.cpu().numpy() - ref).max() < 2e-5 * np.abs(ref).max()


@pytest.mark.parametrize("S", [277, 280])
def test_wave_sort_rows_every_size_class(dev, S):
    """Rows of 257..2048 neighbours at both ends of the three wave-sort classes (csrc/embed_hub.hip: k_embed_rowlines -- four lines
    of 16 lanes x 32 keys per wavefront -- and k_embed_hub<1, M> / k_embed_hub_quad<M> -- a wavefront holds a slice's line in
    registers, 16 / 32 keys per lane), unit and general weights (the general-weight kernels run one size class up for the pad
    element; row 0 is mass-deficient), a zero frequency.  S = 277: not a multiple of the slice-group size, 4-byte gathers; S = 280:
    a multiple of 4, so the unit-weight kernels gather 16 bytes per lane (four slices) and deal the lines out in registers
    (v_permlane swaps) / through LDS."""
    from fsw_gnn_amd import build_csr, _lib
    rng = np.random.default_rng(23)
    sizes = [257, 512, 513, 1024, 1025, 2048, 600, 300, 384, 385, 700, 768, 769, 1500, 1536, 1537]
    nrows, n, d = len(sizes), 2300, 8                            # > 256 slices: several chunk groups on every path
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=89)
    fr = cases.random_freqs(S, seed=90)
    fr[3] = 0.0
    rec = np.repeat(np.arange(nrows), sizes).astype(np.int64)
    snd = np.concatenate([rng.choice(n, size=k, replace=False) for k in sizes]).astype(np.int64)
    w = (rng.random(rec.size) + 0.1).astype(np.float32)
    w[rec == 0] *= 0.3 / w[rec == 0].sum()
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    for weights in (None, w):
        E = make_embedding(dev, V, fr, enable_bias=False, encode_total_mass=True)
        with torch.no_grad():
            graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None if weights is None else t(weights, dev), nrows, n)
            out = torch.empty((nrows, S + 1), device=dev)
            E.embed_into(t(X, dev), graph, out)
        bs = np.diff(graph.bin_start.cpu().numpy())
        assert bs[-8:].tolist() == [5, 6, 5, 0, 0, 0, 0, 0] and bs[:-8].sum() == 0
        ref = O.fsw_embedding_forward(X, rowptr, snd, np.ones(rec.size) if weights is None else weights.astype(np.float64), V, fr,
                                      encode_total_mass=True)
        assert relerr(out.cpu().numpy(), ref) < TOL
        assert np.abs(out.cpu().numpy() - ref).max() < 2e-5 * np.abs(ref).max()


@pytest.mark.parametrize("S", [11, 12])
def test_hub_rows_every_size_class(dev, S):
    """Rows of 2049..70001 neighbours at both ends of the four hub classes (csrc/embed_hub.hip: a workgroup of 2 / 4 / 8 / 16
    wavefronts holds one slice's line, 2048 keys per wavefront, merge levels above a wavefront through LDS) and two rows above
    them (k_embed_giant: blocks of 16384 keys + block sweeps); general weights: k_embed_hub_w's capacity classes up to 8191
    neighbours, above them k_embed_mergepath_w ((key, weight) blocks of 8192 + merge-path levels, csrc/merge_path.h: 5 and 9 blocks =
    runs without a partner at two levels); a zero
    frequency; a mass-deficient row; several rows per class so that the XCD-interleaved block order is exercised.
    S = 11: 4-byte gathers; S = 12 (a multiple of 4): the 16-byte gather forms."""
    from fsw_gnn_amd import build_csr, _lib
    rng = np.random.default_rng(29)
    sizes = [2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 33000, 3000, 5000, 6000, 7000, 4100, 9000, 9001, 9002, 2500, 70001,
             8191, 6143, 6144, 3071, 3072, 4095]
    nrows, n, d = len(sizes), 80_000, 6
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=87)
    fr = cases.random_freqs(S, seed=88)
    fr[2] = 0.0
    rec = np.repeat(np.arange(nrows), sizes).astype(np.int64)
    snd = np.concatenate([rng.choice(n, size=k, replace=False) for k in sizes]).astype(np.int64)
    w = (rng.random(rec.size) + 0.1).astype(np.float32)
    w[rec == 0] *= 0.3 / w[rec == 0].sum()
    w[rec == 18] *= 0.4 / w[rec == 18].sum()          # the longest row is mass-deficient too: its pad element carries weight
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    for weights in (None, w):
        E = make_embedding(dev, V, fr, enable_bias=False, encode_total_mass=True)
        with torch.no_grad():
            graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None if weights is None else t(weights, dev), nrows, n)
            out = torch.empty((nrows, S + 1), device=dev)
            E.embed_into(t(X, dev), graph, out)
        bs = np.diff(graph.bin_start.cpu().numpy())
        assert bs[-5:].tolist() == [7, 9, 5, 2, 2] and bs[:-5].sum() == 0 and graph.stats()[_lib.STAT_NUM_GLOBAL] == nrows
        ref = C.embed(X, rowptr, snd, weights, V, fr)
        got = out.cpu().numpy()
        assert relerr(got[:, 1:], ref) < TOL
        assert np.abs(got[:, 1:] - ref).max() < 2e-5 * np.abs(ref).max()
        mass = np.array(sizes, dtype=np.float64) if weights is None else np.bincount(rec, weights=weights.astype(np.float64))
        assert np.allclose(got[:, 0], mass, rtol=1e-5)


def test_mid_degree_rows_backward(dev):
    """Gradients through rows of 33..256 neighbours (forward on the padded register path, backward on the long-row kernels)."""
    from fsw_gnn_amd import build_csr
    rng = np.random.default_rng(22)
    sizes = [33, 64, 100, 129, 200, 256]
    nrows, n, d, S = len(sizes), 400, 10, 24
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=87)
    fr = cases.random_freqs(S, seed=88)
    rec = np.repeat(np.arange(nrows), sizes).astype(np.int64)
    snd = np.concatenate([rng.choice(n, size=k, replace=False) for k in sizes]).astype(np.int64)
    wts = (rng.random(rec.size) + 0.1).astype(np.float32)
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    R = rng.standard_normal((nrows, S))
    for weights in (None, wts):
        E = make_embedding(dev, V, fr, enable_bias=False, learnable_slices=True, learnable_freqs=True)
        Xd = t(X, dev).requires_grad_(True)
        graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None if weights is None else t(weights, dev), nrows, n)
        out = E.embed_autograd(Xd, graph)
        (out * t(R, dev)).sum().backward()
        wv = np.ones(rec.size) if weights is None else weights.astype(np.float64)
        gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, snd, wv, V, fr, R, Xp_override=_hip_projection(E, Xd))
        assert relerr(out.detach().cpu().numpy(), O.fsw_embedding_forward(X, rowptr, snd, wv, V, fr)) < TOL
        assert relerr(Xd.grad.cpu().numpy(), gX) < 2e-5
        assert relerr(E.projVecs.grad.cpu().numpy(), gV) < 2e-5
        assert relerr(E.freqs.grad.cpu().numpy(), gxi) < 2e-5


@pytest.mark.parametrize("seed", [101, 102, 103, 104, 105, 106])
def test_random_mix_of_degree_classes(dev, seed):
    """Randomised cases: every row draws its in-degree from a mix that touches all degree classes (0, 1..32, the padded
    networks, the three wave-sort classes, the chunked path), random slice counts incl. 1 and non-multiples of 64, random
    choice of unit / general weights, total-mass column and bias; forward against the numpy oracle."""
    from fsw_gnn_amd import build_csr
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.arange(0, 41), [48, 49, 64, 65, 100, 128, 129, 200, 256, 257, 511, 512, 513, 1024, 1025, 2048, 2049, 4097]])
    nrows = 60
    deg = rng.choice(pool, size=nrows)
    deg[rng.integers(0, nrows, 3)] = rng.choice([2049, 3000, 4097], size=3)
    n = int(max(deg.max(), 300)) + 10
    d = int(rng.choice([3, 8, 17]))
    S = int(rng.choice([1, 7, 64, 65, 130]))
    weighted = bool(rng.integers(0, 2))
    mass = bool(rng.integers(0, 2))
    use_bias = bool(rng.integers(0, 2))
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=seed)
    fr = cases.random_freqs(S, seed=seed + 1)
    if S > 2 and rng.integers(0, 2):
        fr[0] = 0.0
    rec = np.repeat(np.arange(nrows), deg).astype(np.int64)
    snd = np.concatenate([rng.choice(n, size=k, replace=False) for k in deg] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    w = (rng.random(rec.size) * 0.2 + 0.001).astype(np.float32) if weighted else None      # many rows below tau = 1: pad element
    bias = rng.standard_normal(S + (1 if mass else 0)).astype(np.float32) if use_bias else None
    order = rng.permutation(rec.size)
    E = make_embedding(dev, V, fr, bias=bias, scale=1.3 if mass else None, encode_total_mass=mass, enable_bias=use_bias)
    with torch.no_grad():
        graph = build_csr(t(rec[order], dev, torch.int64), t(snd[order], dev, torch.int64), None if w is None else t(w[order], dev), nrows, n)
        out = torch.empty((nrows, S + (1 if mass else 0)), device=dev)
        E.embed_into(t(X, dev), graph, out)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    ref = O.fsw_embedding_forward(X, rowptr, snd, np.ones(rec.size) if w is None else w.astype(np.float64), V, fr, bias=bias,
                                  encode_total_mass=mass, total_mass_encoding_scale=1.3)
    got = out.cpu().numpy()
    assert relerr(got, ref) < TOL, (seed, S, d, weighted, mass, use_bias)
    assert np.abs(got - ref).max() < 3e-5 * max(np.abs(ref).max(), 1e-3)


@pytest.mark.parametrize("seed", [201, 202, 203, 204])
def test_random_mix_of_degree_classes_backward(dev, seed):
    """The same kind of random mix through the backward kernels (register, lane-per-slice, wave-sort, chunked scratch
    paths in one graph) against the oracle's analytic backward with the float32 projection of the path under test."""
    from fsw_gnn_amd import build_csr
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.arange(0, 41), [48, 64, 65, 100, 128, 129, 200, 256, 257, 512, 513, 1024, 1025, 2048, 2049]])
    nrows = 40
    deg = rng.choice(pool, size=nrows)
    deg[rng.integers(0, nrows, 2)] = rng.choice([2049, 3000, 4097], size=2)
    n = int(max(deg.max(), 300)) + 10
    d, S = int(rng.choice([4, 9])), int(rng.choice([5, 33, 70]))
    weighted = bool(seed % 2)
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=seed)
    fr = cases.random_freqs(S, seed=seed + 1)
    rec = np.repeat(np.arange(nrows), deg).astype(np.int64)
    snd = np.concatenate([rng.choice(n, size=k, replace=False) for k in deg]).astype(np.int64)
    w = (rng.random(rec.size) * 0.2 + 0.001).astype(np.float32) if weighted else None
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    R = rng.standard_normal((nrows, S))
    E = make_embedding(dev, V, fr, enable_bias=False, learnable_slices=True, learnable_freqs=True)
    Xd = t(X, dev).requires_grad_(True)
    graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None if w is None else t(w, dev), nrows, n)
    out = E.embed_autograd(Xd, graph)
    (out * t(R, dev)).sum().backward()
    wv = np.ones(rec.size) if w is None else w.astype(np.float64)
    assert relerr(out.detach().cpu().numpy(), O.fsw_embedding_forward(X, rowptr, snd, wv, V, fr)) < TOL
    gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, snd, wv, V, fr, R, Xp_override=_hip_projection(E, Xd))
    assert relerr(Xd.grad.cpu().numpy(), gX) < 3e-5, (seed, S, d, weighted)
    assert relerr(E.projVecs.grad.cpu().numpy(), gV) < 3e-5
    assert relerr(E.freqs.grad.cpu().numpy(), gxi) < 3e-5


def test_degenerate_graphs(dev):
    """No edges at all, a single vertex, a single self loop, every edge into one vertex: the layer must run and match
    what the oracle says about rows without neighbours (zero embedding, mass 0) and about the rest."""
    from fsw_gnn_amd import FSW_conv
    torch.manual_seed(11)
    d, out_ch, embed_dim = 6, 5, 9
    conv = FSW_conv(d, out_ch, embed_dim=embed_dim, device=dev)
    V = conv.fsw_embed.projVecs.detach().cpu().numpy()
    fr = conv.fsw_embed.freqs.detach().cpu().numpy()
    lw, lb = conv.mlp[0].weight.detach().cpu().numpy().astype(np.float64), conv.mlp[0].bias.detach().cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(12)
    for n, edges in ((5, np.zeros((2, 0), dtype=np.int64)), (1, np.zeros((2, 0), dtype=np.int64)), (1, np.array([[0], [0]])),
                     (40, np.stack([np.arange(40), np.full(40, 7)]))):
        X = rng.standard_normal((n, d)).astype(np.float32)
        with torch.no_grad():
            y = conv(t(X, dev), t(edges, dev, torch.int64)).cpu().numpy()
        order = np.argsort(edges[1], kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(edges[1], minlength=n))])
        emb = O.fsw_embedding_forward(X, rowptr, edges[0][order], np.ones(edges.shape[1]), V, fr, encode_total_mass=True)
        ref = O.conv_tail(emb, X.astype(np.float64), linear_weight=lw, linear_bias=lb)
        assert y.shape == (n, out_ch) and relerr(y, ref) < 1e-5 and np.isfinite(y).all()


def test_readout_layer(dev):
    from fsw_gnn_amd import FSW_readout
    rng = np.random.default_rng(4)
    sizes = [40, 1, 300, 0, 77]                                  # includes an empty graph
    n, d = sum(sizes), 8
    gi = np.repeat(np.arange(5), sizes).astype(np.int64)
    X = rng.standard_normal((n, d)).astype(np.float32)
    ro = FSW_readout(d, 20, concat_self=False, mlp_layers=0, bias=False, device=dev)   # embed_dim = out_channels (fsw_conv.py:228-229)
    with torch.no_grad():
        out = ro(t(X, dev), t(gi, dev, torch.int64), 5).cpu().numpy()
    V = ro.fsw_embed.projVecs.detach().cpu().numpy()
    fr = ro.fsw_embed.freqs.detach().cpu().numpy()
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    ref = O.fsw_embedding_forward(X, rowptr, np.arange(n), np.ones(n), V, fr, encode_total_mass=True)
    assert out.shape == (5, 20)
    assert relerr(out, ref) < TOL
    assert np.abs(out[3]).max() == 0.0


def test_readout_layer_is_differentiable(dev):
    """Training through FSW_readout (reference fsw_conv.py:503-515 is differentiable through self.fsw_embed): gradients
    of the vertex features and of the slices / frequencies against the oracle's analytic backward."""
    from fsw_gnn_amd import FSW_readout
    rng = np.random.default_rng(14)
    sizes = [40, 1, 300, 0, 77, 2500]
    n, d, out_ch = sum(sizes), 8, 12
    gi = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    X = rng.standard_normal((n, d)).astype(np.float32)
    ro = FSW_readout(d, out_ch, concat_self=False, mlp_layers=0, bias=False, encode_vertex_degrees=False, device=dev)
    assert ro.fsw_embed.projVecs.requires_grad and ro.fsw_embed.freqs.requires_grad
    Xd = t(X, dev).requires_grad_(True)
    out = ro(Xd, t(gi, dev, torch.int64), len(sizes))
    assert out.grad_fn is not None
    R = rng.standard_normal((len(sizes), out_ch))
    (out * t(R, dev)).sum().backward()
    V = ro.fsw_embed.projVecs.detach().cpu().numpy()
    fr = ro.fsw_embed.freqs.detach().cpu().numpy()
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, np.arange(n), np.ones(n), V, fr, R, Xp_override=_hip_projection(ro.fsw_embed, Xd))
    assert relerr(Xd.grad.cpu().numpy(), gX) < 2e-5
    assert relerr(ro.fsw_embed.projVecs.grad.cpu().numpy(), gV) < 2e-5
    assert relerr(ro.fsw_embed.freqs.grad.cpu().numpy(), gxi) < 2e-5
    # an empty batch / no vertices at all: empty result instead of an error
    with torch.no_grad():
        assert tuple(ro(torch.zeros((0, d), device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 0).shape) == (0, out_ch)


def test_in_place_weight_edits_are_seen_and_graph_cache_is_safe(dev):
    """Nothing derived from the parameters is cached on the host: edits through .data (which do not bump _version) change
    the next forward; the optional CSR cache is keyed on the edge_index tensor itself and forgets old input flags."""
    from fsw_gnn_amd import FSW_conv
    n, E, d = 2000, 16000, 16
    ei = t(cases.synth.er_multigraph(n, E, seed=3), dev, torch.int64)
    X = t(cases.synth.features(n, d, seed=4), dev)
    torch.manual_seed(0)
    conv = FSW_conv(d, 8, embed_dim=33, device=dev)
    conv2 = FSW_conv(d, 8, embed_dim=33, device=dev)
    conv2.load_state_dict(conv.state_dict())
    with torch.no_grad():
        y0 = conv(X, ei)
        conv.mlp[0].weight.data.mul_(2.0)                       # _version stays 0
        conv.fsw_embed.total_mass_encoding_scale.data.fill_(3.0)
        conv2.mlp[0].weight.mul_(2.0)
        conv2.fsw_embed.total_mass_encoding_scale.fill_(3.0)
        y1, y2 = conv(X, ei), conv2(X, ei)
        assert not torch.allclose(y1, y0) and torch.equal(y1, y2)
        conv.fuse_linear = False
        assert float((conv(X, ei) - y1).abs().max()) < 1e-5 * float(y1.abs().max())
        conv.fuse_linear = True
        # CSR cache: same tensor -> hit; an equal-sized new tensor -> rebuilt; bad input once does not poison later calls
        conv.cache_graph = True
        ya = conv(X, ei)
        g1 = conv._graph_cache[2]
        assert conv(X, ei) is not None and conv._graph_cache[2] is g1
        Xbad = X.clone()
        Xbad[5, 3] = float("nan")
        with pytest.raises(AssertionError, match="NaNs or infs"):
            conv(Xbad, ei)
        assert torch.equal(conv(X, ei), ya)                     # the flag of the bad input is gone
        ei2 = ei.flip(1).contiguous()
        yb = conv(X, ei2)
        assert conv._graph_cache[2] is not g1 and float((yb - ya).abs().max()) < 1e-5 * float(ya.abs().max())
        assert tuple(conv(torch.zeros((0, d), device=dev), torch.zeros((2, 0), dtype=torch.int64, device=dev)).shape) == (0, 8)


def test_sparse_weights_outside_graph_mode(dev):
    """Coalesced COO weights with graph_mode=False (reference fsw_embedding.py:664-668): same result as the dense tensor."""
    rng = np.random.default_rng(6)
    B, n, d, S = 3, 50, 7, 12
    X = rng.standard_normal((B, n, d)).astype(np.float32)
    W = (rng.random((B, n)) * (rng.random((B, n)) < 0.6)).astype(np.float32)
    E = make_embedding(dev, cases.synth.unit_slices(S, d, seed=5), cases.random_freqs(S, seed=6), encode_total_mass=True)
    with torch.no_grad():
        dense = E(t(X, dev), t(W, dev))
        sparse = E(t(X, dev), t(W, dev).to_sparse().coalesce())
    assert tuple(dense.shape) == (B, S + 1) and float((dense - sparse).abs().max()) < 1e-6 * float(dense.abs().max())


def test_er1m_config3_full_size(dev):
    """BASELINE config 3 at full size against rows sampled from the reference's float64 run."""
    g = golden("er1m")
    c = cases.er1m()
    conv = _conv_from_case(c, dev)
    X, ei = t(c["X"], dev), t(c["edge_index"], dev, torch.int64)
    with torch.no_grad():
        graph = conv.build_graph(ei, c["n"])
        emb = torch.empty((c["n"], c["embed_dim"]), device=dev)
        conv.fsw_embed.embed_into(X, graph, emb)
        y = conv(X, ei)
        torch.cuda.synchronize()
    st = graph.stats()
    assert st[2] == int(g["num_zero_degree"]) and st[1] >= int(g["max_degree"])
    rows = g["rows"]
    er = emb[t(rows, dev, torch.int64)].cpu().numpy()
    assert relerr(er, g["emb_rows_f64"]) < TOL
    coln = torch.linalg.vector_norm(emb.double(), dim=0).cpu().numpy()
    assert relerr(coln, g["emb_colnorm_f64"]) < TOL
    assert abs(float(torch.linalg.vector_norm(emb.double())) - float(g["emb_norm_f64"])) / float(g["emb_norm_f64"]) < TOL
    zero_rows = rows[np.abs(g["emb_rows_f64"]).max(axis=1) == 0]
    assert zero_rows.size == int(g["num_zero_degree"])
    assert float(emb[t(zero_rows, dev, torch.int64)].abs().max()) == 0.0
    # conv tail on the sampled rows through the oracle's restatement of fsw_conv.py:357-362
    ref_y = O.conv_tail(g["emb_rows_f64"], c["X"][rows].astype(np.float64), linear_weight=c["lin_w"], linear_bias=c["lin_b"])
    assert relerr(y[t(rows, dev, torch.int64)].cpu().numpy(), ref_y) < 2e-5
    # size-independent properties at full size: positive homogeneity and edge-order invariance
    with torch.no_grad():
        emb2 = torch.empty_like(emb)
        conv.fsw_embed.embed_into(X * 4.0, graph, emb2)
        assert relerr((emb2[:, 1:] / 4.0).cpu().numpy()[::97], emb[:, 1:].cpu().numpy()[::97]) < 1e-6
        perm = torch.randperm(ei.shape[1], device=dev)
        graph3 = conv.build_graph(ei[:, perm].contiguous(), c["n"])
        emb3 = torch.empty_like(emb)
        conv.fsw_embed.embed_into(X, graph3, emb3)
        assert torch.equal(emb3, emb)                     # unit path: bitwise independent of the edge order


# ---------------------------------------------------------------------------------------------------
def test_segcumsum_golden_and_reverse(dev):
    from fsw_gnn_amd import segcumsum
    g = golden("segcumsum")
    ids = g["ids"]
    for tag, dt, tol in (("f32", torch.float32, 2e-6), ("f64", torch.float64, 1e-14)):
        v = t(g["values_" + tag], dev, dt)
        for idt in (torch.int64, torch.int32):
            got = segcumsum(v, t(ids, dev, idt))
            assert relerr(got.cpu().numpy(), g["slow_" + tag]) < tol
            assert relerr(got.cpu().numpy(), g["out_" + tag]) < max(tol, 1e-5 if tag == "f32" else tol)
        rev = segcumsum(v, t(ids, dev, torch.int64), reverse=True).cpu().numpy()
        ref = O.segcumsum(g["values_" + tag][::-1].copy(), ids[::-1].copy())[::-1]
        assert relerr(rev, ref) < tol
        vc = v.clone()
        same = segcumsum(vc, t(ids, dev, torch.int64), in_place=True)
        assert same.data_ptr() == vc.data_ptr() and relerr(vc.cpu().numpy(), g["slow_" + tag]) < tol


def test_segcumsum_large_random(dev):
    from fsw_gnn_amd import segcumsum
    rng = np.random.default_rng(7)
    n = 3_000_017
    lens = rng.integers(1, 40, size=n // 10)
    lens[100] = 50_000                                      # spans many tiles
    ids = np.repeat(np.arange(lens.size), lens)[:n]
    vals = rng.standard_normal(ids.size)
    got = segcumsum(t(vals, dev, torch.float64), t(ids, dev, torch.int64)).cpu().numpy()
    assert relerr(got, O.segcumsum(vals, ids)) < 1e-13


@pytest.mark.parametrize("case", ["short", "one_segment", "long_runs", "all_heads"])
def test_segcumsum_chained_scan_cases(dev, case):
    """The single-pass chained scan across many tiles: segment structures that end the look-back at once (short
    segments), never (one segment: every tile waits for a published prefix) and in between; sizes that are and are not
    multiples of the vector width / tile, forward and reverse, both id widths, in place, unaligned views."""
    from fsw_gnn_amd import segcumsum
    rng = np.random.default_rng({"short": 1, "one_segment": 2, "long_runs": 3, "all_heads": 4}[case])
    for n in (1, 7, 4096, 4097, 1_000_003, 2_500_000):
        if case == "short":
            ids = np.cumsum(rng.random(n) < 0.12)
        elif case == "one_segment":
            ids = np.zeros(n, dtype=np.int64)
        elif case == "long_runs":
            ids = np.cumsum(rng.random(n) < 1.0 / 30000.0)
        else:
            ids = np.arange(n)
        ids = ids.astype(np.int64)
        vals = rng.standard_normal(n)
        ref = O.segcumsum(vals, ids)
        refr = O.segcumsum(vals[::-1].copy(), ids[::-1].copy())[::-1]
        scale = np.abs(ref).max() + 1e-300
        for vdt, tol in ((torch.float64, 1e-12), (torch.float32, 3e-5)):      # float32: sums of up to 2.5M terms
            v = t(vals, dev, vdt)
            for idt in (torch.int64, torch.int32):
                i = t(ids, dev, idt)
                assert np.abs(segcumsum(v, i).cpu().numpy() - ref).max() / scale < tol, (case, n, vdt, idt)
                assert np.abs(segcumsum(v, i, reverse=True).cpu().numpy() - refr).max() / scale < tol, (case, n, vdt, idt, "rev")
        # unaligned views (scalar path) and in place
        vp = torch.zeros(n + 3, device=dev, dtype=torch.float32)
        vp[3:] = t(vals, dev)
        ip = torch.zeros(n + 1, device=dev, dtype=torch.int64)
        ip[1:] = t(ids, dev, torch.int64)
        got = segcumsum(vp[3:], ip[1:])
        assert np.abs(got.cpu().numpy() - ref).max() / scale < 3e-5
        # in place: every tile takes the descriptor path (the halo shortcut would read values that another workgroup may already
        # have overwritten with its results).  With segments shorter than a tile the carry is the predecessor's aggregate either
        # way -- the same operations in the same order -- so in place and out of place give the same bits; with segments that span
        # tiles the look-back adds aggregates and prefixes in whatever state it finds them (sums equal to rounding, not to the bit)
        w = t(vals, dev, torch.float64)
        sep = segcumsum(w, t(ids, dev, torch.int64))
        assert segcumsum(w, t(ids, dev, torch.int64), in_place=True).data_ptr() == w.data_ptr()
        assert np.abs(w.cpu().numpy() - ref).max() / scale < 1e-12
        w32 = t(vals, dev, torch.float32)
        sep32 = segcumsum(w32, t(ids, dev, torch.int32), reverse=True)
        segcumsum(w32, t(ids, dev, torch.int32), in_place=True, reverse=True)
        if case in ("short", "all_heads"):
            assert torch.equal(w, sep) and torch.equal(w32, sep32)
        else:
            assert float((w32 - sep32).abs().max()) <= 3e-5 * scale


def test_legacy_abi_drives_reference_hierarchy(dev):
    """segcumsum_wrapper / add_block_sums_wrapper with the reference's driver loop (fsw_embedding.py:2905-3010)."""
    import ctypes
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    g = golden("segcumsum")
    ids = t(g["ids"], dev, torch.int64)
    for tag, dt, dnum in (("f32", torch.float32, 0), ("f64", torch.float64, 1)):
        vals = t(g["values_" + tag], dev, dt)
        tpb = 256
        sizes, max_seg = [vals.numel()], [1300]
        while sizes[-1] > tpb:
            sizes.append((sizes[-1] + tpb - 1) // tpb)
            max_seg.append((max_seg[-1] + tpb - 1) // tpb)
        nblocks = sizes[1:] + [1]
        outs = [vals.clone()] + [torch.empty(s, device=dev, dtype=dt) for s in sizes[1:]]
        idts = [ids] + [torch.empty(s, device=dev, dtype=torch.int64) for s in sizes[1:]]
        torch.cuda.synchronize()
        for i, s in enumerate(sizes):
            nxt = i < len(sizes) - 1
            L.segcumsum_wrapper(dnum, outs[i].data_ptr(), idts[i].data_ptr(), s, max_seg[i],
                                outs[i + 1].data_ptr() if nxt else None, idts[i + 1].data_ptr() if nxt else None,
                                nxt, nblocks[i], tpb, tpb * vals.element_size())
        for i in reversed(range(len(sizes) - 1)):
            L.add_block_sums_wrapper(dnum, outs[i].data_ptr(), outs[i + 1].data_ptr(), idts[i].data_ptr(),
                                     idts[i + 1].data_ptr(), sizes[i], nblocks[i], tpb)
        assert relerr(outs[0].cpu().numpy(), g["slow_" + tag]) < (2e-6 if tag == "f32" else 1e-14)
    assert L.get_max_threads_per_block(0) == 1024


def test_legacy_wrappers_wait_for_work_on_a_non_blocking_side_stream(dev):
    """The reference's wrappers synchronise the DEVICE before they launch on the null stream (fsw_embedding.cu:197, 215): the
    caller's producer may sit on a non-blocking side stream, which does not order itself against the null stream.  Here the
    values are produced on such a stream behind ~100 ms of queued work and NOT synchronised by the caller."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    n, tpb = 1 << 16, 256
    ids = torch.arange(n, device=dev, dtype=torch.int64) // 100              # segments of 100 <= tpb: one level suffices per block
    side = torch.cuda.Stream(device=dev)                                      # torch side streams are created non-blocking
    vals = torch.zeros(n, device=dev, dtype=torch.float32)
    big = torch.randn((4096, 4096), device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        acc = big
        for _ in range(60):
            acc = acc @ big * 1e-2                                            # queued producer work
        vals.fill_(1.0)                                                       # the values the scan must see
    nblocks = n // tpb
    sums = torch.empty(nblocks, device=dev, dtype=torch.float32)
    last = torch.empty(nblocks, device=dev, dtype=torch.int64)
    L.segcumsum_wrapper(0, vals.data_ptr(), ids.data_ptr(), n, 100, sums.data_ptr(), last.data_ptr(), True, nblocks, tpb, tpb * 4)
    # the wrapper is synchronous like the reference's: the result is complete here without any caller-side synchronisation
    got = vals.cpu().numpy()
    i = np.arange(n)
    want = np.minimum(i % 100, i % tpb) + 1.0                                 # block-local restart (the next level adds the carry)
    assert np.array_equal(got, want)
    with torch.cuda.stream(side):
        for _ in range(60):
            acc = acc @ big * 1e-2
        sums.fill_(1000.0)
        last.copy_(ids[tpb - 1::tpb])
    L.add_block_sums_wrapper(0, vals.data_ptr(), sums.data_ptr(), ids.data_ptr(), last.data_ptr(), n, nblocks, tpb)
    got2 = vals.cpu().numpy()
    carried = (i >= tpb) & ((i // 100) == ((i // tpb * tpb - 1) // 100))
    assert np.array_equal(got2, want + 1000.0 * carried)
    del acc


# ---------------------------------------------------------------------------------------------------
def _hip_projection(E, X):
    """float32 projections of the path under test (decide the sort order in the oracle: see fsw_embed_csr_backward)."""
    from fsw_gnn_amd import build_csr
    dev = X.device
    n = X.shape[0]
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    with torch.no_grad():
        return E.prepare(X.detach().contiguous(), build_csr(idx, idx, None, n, n))["Xp"][:, :E.nSlices].cpu().numpy()


def _hip_projection_cols(E, X, d):
    """float32 X . projVecs[:, :d]^T from the kernel under test (module with edge features: vertex part of the slices)."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    Xc = X.detach().contiguous()
    n, S = Xc.shape[0], E.nSlices
    V = E.projVecs.detach()
    Xp = torch.empty((n, (S + 63) // 64 * 64), dtype=torch.float32, device=Xc.device)
    _lib.check(L.fsw_project_f32(Xc.data_ptr(), n, d, d, V.data_ptr(), S, V.stride(0), Xp.data_ptr(), Xp.stride(0), None, 0, None,
                                 torch.cuda.current_stream(Xc.device).cuda_stream), "project")
    return Xp[:, :S].cpu().numpy().astype(np.float64)


def test_backward_tiny_graph_vs_reference_autograd(dev):
    """Gradients of the HIP backward kernel against the reference's own autograd (float64 goldens)."""
    from fsw_gnn_amd import build_csr
    g, gg = golden("tiny_graph"), golden("grads_tiny")
    ei = g["edge_index"]
    E = make_embedding(dev, g["V"], gg["freqs"], bias=g["bias"], scale=0.7, encode_total_mass=True,
                       total_mass_encoding_scale=0.7, learnable_slices=True, learnable_freqs=True,
                       learnable_total_mass_encoding_scale=True)
    X = t(g["X"], dev).requires_grad_(True)
    graph = build_csr(t(ei[1], dev, torch.int64), t(ei[0], dev, torch.int64), None, 64, 64)   # unit multigraph
    out = E.embed_autograd(X, graph)
    assert relerr(out.detach().cpu().numpy(), gg["out_unit"]) < TOL
    (out * t(gg["R"], dev)).sum().backward()
    assert relerr(X.grad.cpu().numpy(), gg["gX_unit"]) < 2e-5
    assert relerr(E.projVecs.grad.cpu().numpy(), gg["gV_unit"]) < 2e-5
    assert relerr(E.freqs.grad.cpu().numpy(), gg["gfreqs_unit"]) < 2e-5
    assert relerr(E.bias.grad.cpu().numpy(), gg["gbias_unit"]) < 1e-6
    assert abs(float(E.total_mass_encoding_scale.grad) - float(gg["gscale_unit"])) < 1e-5 * abs(float(gg["gscale_unit"]))
    # explicit non-unit sparse weights (rows below tau get the pad element): weighted backward kernel
    E.zero_grad()
    X2 = t(g["X"], dev).requires_grad_(True)
    adj3 = sparse_adj(g["adj_indices"], g["adj3_values"], (64, 64), dev)
    out3 = E(X2, adj3, graph_mode=True)
    assert relerr(out3.detach().cpu().numpy(), gg["out_weighted"]) < TOL
    (out3 * t(gg["R"], dev)).sum().backward()
    assert relerr(X2.grad.cpu().numpy(), gg["gX_weighted"]) < 2e-5
    assert relerr(E.projVecs.grad.cpu().numpy(), gg["gV_weighted"]) < 2e-5
    assert relerr(E.freqs.grad.cpu().numpy(), gg["gfreqs_weighted"]) < 2e-5
    assert abs(float(E.total_mass_encoding_scale.grad) - float(gg["gscale_weighted"])) < 1e-5 * abs(float(gg["gscale_weighted"]))
    # gradients w.r.t. the weights: tests/test_hip_float64.py::test_weight_gradients_vs_reference_autograd


@pytest.mark.parametrize("method", ["homog", "homog_alt"])
def test_backward_homog_mass_encodings_vs_reference_autograd(dev, method):
    """total_mass_encoding_method 'homog' / 'homog_alt' under autograd (reference fsw_embedding.py:874-882, 1136-1144):
    forward and every gradient against the reference's float64 autograd (tests/golden/grads_homog.npz)."""
    from fsw_gnn_amd import build_csr
    g, gt, gh = golden("tiny_graph"), golden("grads_tiny"), golden("grads_homog")
    ei = g["edge_index"]
    E = make_embedding(dev, g["V"], gt["freqs"], bias=g["bias"], scale=0.7, encode_total_mass=True, total_mass_encoding_scale=0.7,
                       total_mass_encoding_method=method, learnable_slices=True, learnable_freqs=True,
                       learnable_total_mass_encoding_scale=True)
    R = t(gt["R"], dev)
    for tag in ("unit", "weighted"):
        E.zero_grad()
        X = t(g["X"], dev).requires_grad_(True)
        if tag == "unit":
            out = E.embed_autograd(X, build_csr(t(ei[1], dev, torch.int64), t(ei[0], dev, torch.int64), None, 64, 64))
        else:
            out = E(X, sparse_adj(g["adj_indices"], g["adj3_values"], (64, 64), dev), graph_mode=True)
        k = method + "_" + tag
        assert relerr(out.detach().cpu().numpy(), gh["out_" + k]) < TOL
        with torch.no_grad():                                               # the inference path applies the same epilogue in place
            assert relerr(E(X.detach(), sparse_adj(g["adj_indices"], g["adj_values"] if tag == "unit" else g["adj3_values"], (64, 64), dev),
                            graph_mode=True).cpu().numpy(), gh["out_" + k]) < TOL
        (out * R).sum().backward()
        assert relerr(X.grad.cpu().numpy(), gh["gX_" + k]) < 2e-5
        assert relerr(E.projVecs.grad.cpu().numpy(), gh["gV_" + k]) < 2e-5
        assert relerr(E.freqs.grad.cpu().numpy(), gh["gfreqs_" + k]) < 2e-5
        assert relerr(E.bias.grad.cpu().numpy(), gh["gbias_" + k]) < 1e-6
        assert abs(float(E.total_mass_encoding_scale.grad) - float(gh["gscale_" + k])) < 2e-5 * abs(float(gh["gscale_" + k]))


def test_backward_long_rows_lds_and_global_paths(dev):
    """Readout-shaped input (segments of 700 / 3000 / 5000 points), unit and weighted: LDS and global backward kernels
    against the oracle's analytic backward evaluated with the same float32 sort order."""
    from fsw_gnn_amd import build_csr
    rng = np.random.default_rng(13)
    sizes = [700, 3000, 5000]
    n, d, S = sum(sizes), 16, 24
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=83)
    fr = cases.random_freqs(S, seed=84)
    gi = np.repeat(np.arange(3), sizes).astype(np.int64)
    wts = (rng.random(n) + 0.1).astype(np.float32)
    wts[gi == 0] *= 0.5 / wts[gi == 0].sum()
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    col = np.arange(n)
    R = rng.standard_normal((3, S))
    for weights in (None, wts):
        E = make_embedding(dev, V, fr, enable_bias=False, learnable_slices=True, learnable_freqs=True)
        Xd = t(X, dev).requires_grad_(True)
        graph = build_csr(t(gi, dev, torch.int64), t(col, dev, torch.int64), None if weights is None else t(weights, dev), 3, n)
        out = E.embed_autograd(Xd, graph)
        (out * t(R, dev)).sum().backward()
        wv = np.ones(n) if weights is None else weights.astype(np.float64)
        gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, col, wv, V, fr, R, Xp_override=_hip_projection(E, Xd))
        assert relerr(out.detach().cpu().numpy(), C.embed(X, rowptr, col, weights, V, fr)) < TOL
        assert relerr(Xd.grad.cpu().numpy(), gX) < 2e-5
        assert relerr(E.projVecs.grad.cpu().numpy(), gV) < 2e-5
        assert relerr(E.freqs.grad.cpu().numpy(), gxi) < 2e-5


@pytest.mark.parametrize("S", [10, 12])
def test_backward_rows_of_129_to_2048_neighbours_every_class(dev, S):
    """Gradients through rows at both ends of the classes 129..256 / ..512 / ..1024 / ..2048, unit weights, against the oracle's
    analytic backward evaluated with the same float32 sort order.  S = 12 (a multiple of 4): the store-and-sum backward takes
    k_embed_quad_bwd (16-byte gathers dealt through LDS, packed (key, index) lines in registers, 16-byte stores of the key gradients);
    S = 10: the LDS-tile kernels k_embed_wsort_bwd.  Both must give the same gradients to rounding."""
    from fsw_gnn_amd import build_csr
    rng = np.random.default_rng(31)
    sizes = [129, 256, 257, 512, 513, 1024, 1025, 2048, 200, 300, 700, 1500]
    nrows, n, d = len(sizes), 2100, 9
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=91)
    fr = cases.random_freqs(S, seed=92)
    fr[1] = 0.0
    rec = np.repeat(np.arange(nrows), sizes).astype(np.int64)
    snd = np.concatenate([rng.choice(n, size=k, replace=False) for k in sizes]).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(sizes)])
    R = rng.standard_normal((nrows, S))
    E = make_embedding(dev, V, fr, enable_bias=False, learnable_slices=True, learnable_freqs=True)
    Xd = t(X, dev).requires_grad_(True)
    graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None, nrows, n)
    out = E.embed_autograd(Xd, graph)
    (out * t(R, dev)).sum().backward()
    gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, snd, np.ones(rec.size), V, fr, R, Xp_override=_hip_projection(E, Xd))
    assert relerr(Xd.grad.cpu().numpy(), gX) < 2e-5
    assert relerr(E.projVecs.grad.cpu().numpy(), gV) < 2e-5
    assert relerr(E.freqs.grad.cpu().numpy(), gxi) < 2e-5


def test_hub_row_with_100k_neighbours_forward_and_backward(dev):
    """A star: 100 000 leaves send to vertex 0 (64 register-sorted chunks, six merge levels over the scratch line), a
    second row of 9 000; unit and general weights; forward against the C oracle, gradients against the oracle's analytic
    backward with the same float32 projection."""
    from fsw_gnn_amd import build_csr
    rng = np.random.default_rng(31)
    sizes = [100_000, 9_000]
    n, d, S = sum(sizes) + 2, 6, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=91)
    fr = cases.random_freqs(S, seed=92)
    rec = np.repeat(np.arange(2), sizes).astype(np.int64)
    snd = (2 + np.arange(sum(sizes))).astype(np.int64)
    wts = (rng.random(rec.size) + 0.1).astype(np.float32)
    rowptr = np.concatenate([[0], np.cumsum(sizes), [sum(sizes)] * (n - 2)])
    R = rng.standard_normal((n, S))
    R[2:] = 0.0
    for weights in (None, wts):
        E = make_embedding(dev, V, fr, enable_bias=False, learnable_slices=True, learnable_freqs=True)
        Xd = t(X, dev).requires_grad_(True)
        graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None if weights is None else t(weights, dev), n, n)
        assert graph.stats()[5] == 2 and graph.stats()[1] == 100_000
        out = E.embed_autograd(Xd, graph)
        (out * t(R, dev)).sum().backward()
        ref = C.embed(X, rowptr, snd, weights, V, fr)
        assert relerr(out.detach().cpu().numpy()[:2], ref[:2]) < TOL and float(out.detach()[2:].abs().max()) == 0.0
        wv = np.ones(rec.size) if weights is None else weights.astype(np.float64)
        gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, snd, wv, V, fr, R, Xp_override=_hip_projection(E, Xd))
        assert relerr(Xd.grad.cpu().numpy(), gX) < 2e-5
        assert relerr(E.projVecs.grad.cpu().numpy(), gV) < 2e-5
        assert relerr(E.freqs.grad.cpu().numpy(), gxi) < 2e-5


def test_store_and_sum_backward_matches_atomic_backward_and_is_reproducible(dev):
    """Unit-weight graphs store every neighbour's key gradient and sum them over the sender-major entry list
    (fsw_graph_transpose + fsw_segment_sum_rows_f32) instead of float atomics.  A graph with a sender of out-degree 6000 (its
    list crosses 24 segments), senders without out-edges, every in-degree class up to the scratch rows: the C entry points
    against torch's stable sort / index_add, the gradients against the atomic form (store_sum_backward_max_bytes = 0) and
    the oracle, and two runs of an ER graph bitwise equal."""
    import ctypes
    from fsw_gnn_amd import build_csr, _lib
    rng = np.random.default_rng(77)
    n, d, S = 9000, 7, 70
    deg = rng.choice([0, 1, 2, 3, 5, 9, 17, 33, 40, 70, 130, 300, 2100], size=n, p=[.1, .2, .2, .15, .1, .08, .06, .05, .03, .02, .006, .003, .001])
    deg[:6000] = np.maximum(deg[:6000], 1)
    rec = np.repeat(np.arange(n), deg).astype(np.int64)
    snd = rng.integers(100, n, size=rec.size).astype(np.int64)      # senders 0..99 mostly without out-edges
    first = np.concatenate([[0], np.cumsum(deg)[:-1]])[:6000]
    snd[first] = 7                                                   # one sender of out-degree 6000, no duplicates inside a row
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d, seed=5)
    fr = cases.random_freqs(S, seed=6)
    R = rng.standard_normal((n, S))
    graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None, n, n)
    nnz = graph.stats()[_lib.STAT_NNZ]
    # the two C entry points on their own
    cptr, order = graph.sender_major()
    col = graph.col[:nnz].long()
    ref_order = torch.sort(col, stable=True).indices
    assert torch.equal(order[:nnz].long(), ref_order)
    assert torch.equal(cptr.long(), torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.bincount(col, minlength=n).cumsum(0)]))
    src = torch.randn(nnz, S, device=dev)
    got = torch.zeros(n, 128, device=dev)
    L = _lib.lib()
    _lib.check(L.fsw_segment_sum_rows_f32(_lib.ptr(src), S, _lib.ptr(cptr), _lib.ptr(order), n, nnz, S, _lib.ptr(got), 128,
                                          torch.cuda.current_stream().cuda_stream), "fsw_segment_sum_rows_f32")
    torch.cuda.synchronize()
    want = torch.zeros(n, S, device=dev, dtype=torch.float64).index_add_(0, col, src.double())
    assert float((got[:, :S].double() - want).abs().max()) < 1e-4 * float(want.abs().max())
    assert float(got[:, S:].abs().max()) == 0.0
    # gradients: store-and-sum against atomics against the oracle
    grads = {}
    for mode, limit in (("store", 32 << 30), ("atomic", 0)):
        E = make_embedding(dev, V, fr, enable_bias=False, learnable_slices=True, learnable_freqs=True)
        E.store_sum_backward_max_bytes = limit
        Xd = t(X, dev).requires_grad_(True)
        out = E.embed_autograd(Xd, graph)
        (out * t(R, dev)).sum().backward()
        grads[mode] = (Xd.grad.cpu().numpy(), E.projVecs.grad.cpu().numpy(), E.freqs.grad.cpu().numpy())
        xp = _hip_projection(E, Xd)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, graph.col[:nnz].cpu().numpy().astype(np.int64), np.ones(nnz), V, fr, R, Xp_override=xp)
    for mode in grads:
        assert relerr(grads[mode][0], gX) < 3e-5 and relerr(grads[mode][1], gV) < 3e-5 and relerr(grads[mode][2], gxi) < 3e-5, mode
    assert relerr(grads["store"][0], grads["atomic"][0]) < 1e-5
    # bitwise reproducible where no sender's list spans more than two segments
    m = 20000
    rec2 = rng.integers(0, m, size=200000).astype(np.int64)
    snd2 = rng.integers(0, m, size=200000).astype(np.int64)
    g2 = build_csr(t(rec2, dev, torch.int64), t(snd2, dev, torch.int64), None, m, m)
    X2 = rng.standard_normal((m, d)).astype(np.float32)
    R2 = t(rng.standard_normal((m, S)), dev)
    runs = []
    for _ in range(2):
        E = make_embedding(dev, V, fr, enable_bias=False, learnable_slices=True, learnable_freqs=True)
        Xd = t(X2, dev).requires_grad_(True)
        (E.embed_autograd(Xd, g2) * R2).sum().backward()
        runs.append(Xd.grad.clone())
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("concat_self,act", [(True, "leaky"), (False, "relu")])
def test_fused_layer_with_a_few_long_rows_matches_unfused(dev, concat_self, act):
    """A graph whose rows mostly fit the fused kernel (<= 32 neighbours) plus rows of 33 .. 40 000 neighbours: the layer keeps
    the fused kernel for the short rows and finishes the long ones with the long-row kernels + one GEMM on those rows; the
    result must equal the unfused layer (every row through the embedding kernels + torch Linear), itself pinned to the oracle
    by the tests above."""
    from fsw_gnn_amd import FSW_conv
    rng = np.random.default_rng(5)
    n = 45_000
    rec = rng.integers(0, n, size=300_000)
    snd = rng.integers(0, n, size=300_000)
    extra_r, extra_s = [], []
    for row, deg in ((11, 33), (12, 100), (13, 257), (14, 700), (15, 1500), (16, 2049), (17, 9000), (18, 40_000), (n - 1, 64)):
        extra_r.append(np.full(deg, row))
        extra_s.append(rng.choice(n, size=deg, replace=False))
    ei = torch.from_numpy(np.stack([np.concatenate([snd] + extra_s), np.concatenate([rec] + extra_r)])).to(dev)
    x = torch.from_numpy(rng.standard_normal((n, 24)).astype(np.float32)).to(dev)
    torch.manual_seed(3)
    conv = FSW_conv(24, 40, embed_dim=65, concat_self=concat_self, mlp_layers=2, mlp_hidden_dim=56,
                    mlp_activation_hidden=torch.nn.LeakyReLU(0.2) if act == "leaky" else torch.nn.ReLU(), device=dev)
    with torch.no_grad():
        assert conv._fusable()
        y = conv(x, ei)
        conv.fuse_linear = False
        ref = conv(x, ei)
    assert torch.isfinite(y).all()
    err = float((y - ref).abs().max() / ref.abs().max())
    assert err < 1e-5, err
    rows = torch.tensor([11, 12, 13, 14, 15, 16, 17, 18, n - 1, 0, 1, 2], device=dev)
    assert float((y[rows] - ref[rows]).abs().max() / ref[rows].abs().max()) < 1e-5


def test_backward_conv10k_training_step(dev):
    gg = golden("grads_conv10k")
    c = cases.conv10k()
    conv = _conv_from_case(c, dev)                     # learnable_embedding=True by default (fsw_conv.py:167)
    X = t(c["X"], dev).requires_grad_(True)
    ei = t(c["edge_index"], dev, torch.int64)
    y = conv(X, ei)
    Rc = cases.synth.normal(92, 1, (c["n"], c["out_ch"]), dtype=np.float64)
    (y * t(Rc, dev)).sum().backward()
    gV, gfr = conv.fsw_embed.projVecs.grad.cpu().numpy(), conv.fsw_embed.freqs.grad.cpu().numpy()
    # (1) against the reference's float64 autograd.  The gradient is discontinuous where two neighbours' projections
    #     coincide: a pair that agrees to float32 rounding can take swapped ranks in float32 and float64, which moves
    #     g (C[s] - C[s+1]) between two entries of gXp (3 such pairs among 12.8M here).  Per-slice medians are tight,
    #     the norm-wise bound allows for those pairs.
    assert relerr(conv.mlp[0].weight.grad.cpu().numpy(), gg["gW"]) < 2e-5
    assert relerr(conv.mlp[0].bias.grad.cpu().numpy(), gg["gb"]) < 2e-5
    assert relerr(gfr, gg["gfreqs"]) < 5e-5
    per_slice = np.array([relerr(gV[k], gg["gV"][k]) for k in range(gV.shape[0])])
    assert np.median(per_slice) < 1e-5 and (per_slice > 1e-4).sum() <= 8 and relerr(gV, gg["gV"]) < 1e-2
    # ... and the allowance is CONFINED to the slices that hold such a pair: over all other slices together the gradient matches the
    # reference's norm-wise at the forward's own tolerance
    clean = per_slice <= 1e-4
    assert clean.sum() >= gV.shape[0] - 8 and relerr(gV[clean], gg["gV"][clean]) < 5e-5, relerr(gV[clean], gg["gV"][clean])
    assert relerr(X.grad[t(gg["rows"], dev, torch.int64)].cpu().numpy(), gg["gX_rows"]) < 1e-2
    # (2) against the oracle's analytic backward evaluated with the SAME float32 sort order: tight everywhere
    rowptr, col, w, _ = O.coalesce_edge_index(c["edge_index"], c["n"])
    Xd = c["X"].astype(np.float64)
    emb = O.fsw_embedding_forward(Xd, rowptr, col, w, c["V"], c["freqs"], encode_total_mass=True)
    Wl, bl = c["lin_w"].astype(np.float64), c["lin_b"].astype(np.float64)
    E_ = c["embed_dim"]
    pre = np.concatenate([emb, Xd], axis=1) @ Wl.T + bl
    gh = (Rc * np.where(pre >= 0, 1.0, 0.2)) @ Wl
    gX_o, gV_o, gxi_o = O.fsw_embed_csr_backward(Xd, rowptr, col, w, c["V"], c["freqs"], gh[:, 1:E_],
                                                 Xp_override=_hip_projection(conv.fsw_embed, X))
    assert relerr(gV, gV_o) < 2e-5 and relerr(gfr, gxi_o) < 2e-5
    assert relerr(X.grad.cpu().numpy(), gX_o + gh[:, E_:]) < 2e-5
    # forward under no_grad (fused kernels) and under autograd (unfused kernels) agree
    with torch.no_grad():
        y2 = conv(X.detach(), ei)
    assert relerr(y2.cpu().numpy(), y.detach().cpu().numpy()) < 2e-6


@pytest.mark.parametrize("K,M,N", [(100_000, 256, 128), (70_001, 128, 385), (65_536, 40, 17), (200_003, 257, 129)])
def test_gemm_tn_weight_gradient_shape(dev, K, M, N):
    """csrc/gemm_tn.hip: A^T . B for tall A [K, M], B [K, N] (the weight gradients of the backward pass: gV = gXp^T . X and the first
    Linear layer's gW, reductions over the rows) against float64; strided operands (gXp is read with its padded row stride); the
    result is bitwise reproducible (partial sums combined in a fixed order); LinearTallFn's gradients equal torch's."""
    from fsw_gnn_amd.fsw_embedding import gemm_tn, LinearTallFn
    g = torch.Generator(device=dev).manual_seed(K)
    Abig = torch.randn((K, M + 7), device=dev, generator=g)
    A = Abig[:, :M]                                                  # row stride M + 7
    B = torch.randn((K, N), device=dev, generator=g)
    C = gemm_tn(A, B)
    ref = A.double().t() @ B.double()
    assert tuple(C.shape) == (M, N)
    assert float((C.double() - ref).abs().max() / ref.abs().max()) < 2e-6
    assert torch.equal(C, gemm_tn(A, B))
    if M <= 128 and N > 64:
        # the split form: y = [s * e | x] . W^T + b without the concatenation
        from fsw_gnn_amd.fsw_embedding import LinearSplitTallFn
        Ne = N - 33
        e = torch.randn((K, Ne), device=dev, generator=g, requires_grad=True)
        x = torch.randn((K, 33), device=dev, generator=g, requires_grad=True)
        W = torch.randn((M, N), device=dev, generator=g, requires_grad=True)
        b = torch.randn(M, device=dev, generator=g, requires_grad=True)
        R = torch.randn((K, M), device=dev, generator=g)
        y1 = LinearSplitTallFn.apply(e, x, W, b, 0.7)
        (y1 * R).sum().backward()
        got = [t_.grad.clone() for t_ in (e, x, W, b)]
        e.grad = x.grad = W.grad = b.grad = None
        y2 = torch.nn.functional.linear(torch.cat((0.7 * e, x), dim=1), W, b)
        (y2 * R).sum().backward()
        assert float((y1 - y2).abs().max() / y2.abs().max()) < 2e-6
        for a_, r_ in zip(got, (e.grad, x.grad, W.grad, b.grad)):
            assert float((a_ - r_).abs().max() / r_.abs().max()) < 2e-5
    if M <= 128:
        h = torch.randn((K, N), device=dev, generator=g, requires_grad=True)
        W = torch.randn((M, N), device=dev, generator=g, requires_grad=True)
        b = torch.randn(M, device=dev, generator=g, requires_grad=True)
        R = torch.randn((K, M), device=dev, generator=g)
        (LinearTallFn.apply(h, W, b) * R).sum().backward()
        got = (h.grad.clone(), W.grad.clone(), b.grad.clone())
        h.grad = W.grad = b.grad = None
        (torch.nn.functional.linear(h, W, b) * R).sum().backward()
        for a_, r_ in zip(got, (h.grad, W.grad, b.grad)):
            assert float((a_ - r_).abs().max() / r_.abs().max()) < 2e-5


@pytest.mark.parametrize("n,E,d,out_ch,embed_dim,kw", [
    (500, 4000, 6, 10, None, {}),                                   # default embed_dim = 20 -> 19 slices, d % 4 != 0
    (1200, 9000, 64, 64, None, {}),                                 # default embed_dim = 128 -> 127 slices (odd)
    (800, 7000, 20, 40, 97, {"mlp_layers": 2}),                     # two-layer MLP: only the first Linear is fused
    (700, 5000, 16, 8, 33, {"concat_self": False}),                 # no vertex-feature block
    (900, 8000, 12, 24, 70, {"encode_vertex_degrees": False, "mlp_activation_final": torch.nn.ReLU()}),
    (600, 5000, 8, 300, 41, {"vertex_degree_encoding_function": "log", "message_weight_vs_self": 0.5}),   # > 256 outputs
    (600, 5000, 160, 32, 65, {}),                                   # > 128 features: x . W2^T by BLAS + row permutation
])
def test_fused_conv_odd_shapes_match_unfused_and_oracle(dev, n, E, d, out_ch, embed_dim, kw):
    """The fused Linear kernel, the unfused kernels and the oracle agree on shapes off the aligned fast paths."""
    from fsw_gnn_amd import FSW_conv
    ei = cases.synth.er_multigraph(n, E, seed=n)
    X = cases.synth.features(n, d, seed=n + 1)
    torch.manual_seed(n)
    conv = FSW_conv(d, out_ch, embed_dim=embed_dim, device=dev, **kw)
    Xd, eid = t(X, dev), t(ei, dev, torch.int64)
    with torch.no_grad():
        assert conv._fusable()
        y_f = conv(Xd, eid).cpu().numpy()
        conv.fuse_linear = False
        y_u = conv(Xd, eid).cpu().numpy()
    assert relerr(y_f, y_u) < 3e-6
    conv.cache_graph = True                                                   # CSR reuse gives the same result
    with torch.no_grad():
        y_c1 = conv(Xd, eid)
        g1 = conv._graph_cache[1]
        y_c2 = conv(Xd, eid)
    assert conv._graph_cache[1] is g1 and torch.equal(y_c1, y_c2) and relerr(y_c1.cpu().numpy(), y_u) == 0.0
    em = conv.fsw_embed
    rowptr, col, w, _ = O.coalesce_edge_index(ei, n)
    emb = O.fsw_embedding_forward(X, rowptr, col, w, em.projVecs.detach().cpu().numpy(), em.freqs.detach().cpu().numpy(),
                                  encode_total_mass=em.encode_total_mass,
                                  total_mass_encoding_function=em.total_mass_encoding_function)
    h = torch.from_numpy(np.concatenate([conv.message_weight_vs_self * emb, X.astype(np.float64)], axis=1) if conv.concat_self else emb)
    with torch.no_grad():
        ref = conv.mlp.double().cpu()(h).numpy()
    assert relerr(y_f, ref) < TOL


@pytest.mark.parametrize("tag,slw", [("plain", 0.0), ("selfloop", 0.5)])
def test_edge_features_conv_forward_and_backward(dev, tag, slw):
    """FSW_conv with edgefeat_dim = 3 on the tiny multigraph (duplicate edges are coalesced: features and weights summed)
    against the reference's forward and autograd (float64 goldens)."""
    from fsw_gnn_amd import FSW_conv
    g, ge = golden("tiny_graph"), golden("edgefeat_tiny")
    d, de, out_ch, embed_dim = 8, 3, 5, 17
    conv = FSW_conv(d, out_ch, edgefeat_dim=de, embed_dim=embed_dim, self_loop_weight=slw, device=dev)
    with torch.no_grad():
        conv.fsw_embed.projVecs.copy_(t(ge["V"], dev))
        conv.fsw_embed.freqs.copy_(t(ge["freqs"], dev))
        conv.mlp[0].weight.copy_(t(ge["lin_w"], dev))
        conv.mlp[0].bias.copy_(t(ge["lin_b"], dev))
    ei = t(g["edge_index"], dev, torch.int64)
    with torch.no_grad():
        y = conv(t(g["X"], dev), ei, edge_features=t(ge["edge_features"], dev))
        graph = conv.build_graph(ei, 64, t(ge["edge_features"], dev))
        emb = torch.empty((64, embed_dim), device=dev)
        conv.fsw_embed.embed_into(t(g["X"], dev), graph, emb)
    assert relerr(emb.cpu().numpy(), ge["emb_" + tag]) < TOL
    assert relerr(y.cpu().numpy(), ge["y_" + tag]) < TOL
    # coalesced adjacency == the oracle's (and the reference's) sorted, merged entries
    rowptr, col, w, _, ef, slot = O.coalesce_edge_index(g["edge_index"], 64, self_loop_weight=slw, edge_features=ge["edge_features"])
    nnz = graph.stats()[6]
    assert nnz == col.shape[0] and np.array_equal(graph.rowptr.cpu().numpy(), rowptr) and np.array_equal(graph.col[:nnz].cpu().numpy(), col)
    assert relerr(graph.w[:nnz].cpu().numpy(), w) < 1e-7 and relerr(graph.ef[:nnz].cpu().numpy(), ef) < 1e-6
    assert np.array_equal(graph.slot_of_edge[:400].cpu().numpy(), slot)
    # training step: gradients for vertex features, edge features, slices (vertex and edge part), frequencies, MLP
    X = t(g["X"], dev).requires_grad_(True)
    EF = t(ge["edge_features"], dev).requires_grad_(True)
    y2 = conv(X, ei, edge_features=EF)
    (y2 * t(ge["R"], dev)).sum().backward()
    assert relerr(X.grad.cpu().numpy(), ge["gX_" + tag]) < 3e-5
    assert relerr(EF.grad.cpu().numpy(), ge["gEF_" + tag]) < 3e-5
    assert relerr(conv.fsw_embed.projVecs.grad.cpu().numpy(), ge["gV_" + tag]) < 3e-5
    assert relerr(conv.fsw_embed.freqs.grad.cpu().numpy(), ge["gfreqs_" + tag]) < 3e-5
    assert relerr(conv.mlp[0].weight.grad.cpu().numpy(), ge["gW_" + tag]) < 3e-5


def test_edge_features_embedding_sparse_inputs_and_long_rows(dev):
    """FSW_embedding(d_edge > 0).forward(X, W sparse, X_edge sparse) incl. rows of 60 / 150 / 300 / 2500 neighbours
    (padded register path, wave-sort path with 8 and 16 keys per lane, chunked scratch path; all with general weights)."""
    rng = np.random.default_rng(5)
    n, d, de, S = 2600, 6, 2, 12
    long_rows = {0: 300, 1: 60, 2: 150, 3: 2500}
    src = np.concatenate([rng.integers(0, n, 1500)] + [rng.choice(n, size=k, replace=False) for k in long_rows.values()])
    dst = np.concatenate([rng.integers(4, n, 1500)] + [np.full(k, r, dtype=np.int64) for r, k in long_rows.items()])
    key = np.unique(dst * n + src)
    dst, src = key // n, key % n
    wv = (rng.random(key.shape[0]) + 0.2).astype(np.float32)
    ef = rng.standard_normal((key.shape[0], de)).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(S, d + de, seed=85)
    fr = cases.random_freqs(S, seed=86)
    E = make_embedding(dev, V[:, :d], fr, enable_bias=False, d_edge=de)
    with torch.no_grad():
        E.projVecs.copy_(t(V, dev))
        idx = torch.from_numpy(np.stack([dst, src])).to(dev)
        W = torch.sparse_coo_tensor(idx, t(wv, dev), (n, n)).coalesce()
        Xe = torch.sparse_coo_tensor(idx, t(ef, dev), (n, n, de)).coalesce()
        out = E(t(X, dev), W, Xe, graph_mode=True).cpu().numpy()
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    ref = O.fsw_embedding_forward(X, rowptr, src, wv, V, fr, edge_feat=ef)
    assert np.diff(rowptr)[:4].tolist() == [300, 60, 150, 2500]
    assert relerr(out, ref) < TOL and relerr(out[:4], ref[:4]) < TOL
    # backward through the key-gradient form of every long-row kernel (gradients for X, both parts of projVecs, freqs).
    # The oracle sorts with the float32 keys of the path under test up to the rounding of the edge term; a rare near-tie
    # swap between the two moves a small amount of gradient between two entries, hence the looser bound.
    E2 = make_embedding(dev, V[:, :d], fr, enable_bias=False, d_edge=de, learnable_slices=True, learnable_freqs=True)
    with torch.no_grad():
        E2.projVecs.copy_(t(V, dev))
    Xd = t(X, dev).requires_grad_(True)
    R = rng.standard_normal((n, S))
    R[4:] *= 0.05                                               # weight the long rows
    (E2(Xd, W, Xe, graph_mode=True) * t(R, dev)).sum().backward()
    keys = (_hip_projection_cols(E2, Xd, d)[src] + ef.astype(np.float64) @ V[:, d:].astype(np.float64).T).astype(np.float32)
    gX, gV, gxi, _ = O.fsw_embed_csr_backward(X, rowptr, src, wv, V, fr, R, edge_feat=ef, keys_override=keys)
    assert relerr(Xd.grad.cpu().numpy(), gX) < 1e-3
    assert relerr(E2.projVecs.grad.cpu().numpy(), gV) < 1e-3
    assert relerr(E2.freqs.grad.cpu().numpy(), gxi) < 1e-3
    m = 400                                                  # dense W / X_edge on a sub-block (dense n x n x de would be 54 MB)
    keep = (dst < m) & (src < m)
    with torch.no_grad():
        idx2 = torch.from_numpy(np.stack([dst[keep], src[keep]])).to(dev)
        Wd = torch.sparse_coo_tensor(idx2, t(wv[keep], dev), (m, m)).to_dense()
        Xed = torch.sparse_coo_tensor(idx2, t(ef[keep], dev), (m, m, de)).to_dense()
        out_d = E(t(X[:m], dev), Wd, Xed, graph_mode=True).cpu().numpy()
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(dst[keep], minlength=m))])
    assert relerr(out_d, O.fsw_embedding_forward(X[:m], rp2, src[keep], wv[keep], V, fr, edge_feat=ef[keep])) < TOL


@pytest.mark.parametrize("n,E,d,S", [(3000, 25000, 128, 1000), (2000, 15000, 256, 96), (1500, 12000, 100, 300)])
def test_wide_slice_axis_and_feature_dims(dev, n, E, d, S):
    """BASELINE config 4 shape class (1024 slices: several column groups in the projection, several chunk groups in the
    neighbourhood kernels), d > 128 (generic projection kernel) and d % 16 != 0, against the C oracle."""
    from fsw_gnn_amd import build_csr
    ei = cases.synth.er_multigraph(n, E, seed=S)
    X = cases.synth.features(n, d, seed=S + 1)
    V = cases.synth.unit_slices(S, d, seed=S + 2)
    fr = cases.synth.spread_freqs(S)
    Em = make_embedding(dev, V, fr, encode_total_mass=True, enable_bias=False)
    with torch.no_grad():
        graph = build_csr(t(ei[1], dev, torch.int64), t(ei[0], dev, torch.int64), None, n, n)
        out = torch.empty((n, S + 1), device=dev)
        Em.embed_into(t(X, dev), graph, out)
    order = np.argsort(ei[1], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=n))])
    ref = C.embed(X, rowptr, ei[0][order], None, V, fr)
    assert relerr(out[:, 1:].cpu().numpy(), ref) < TOL
    assert np.array_equal(out[:, 0].cpu().numpy(), np.bincount(ei[1], minlength=n).astype(np.float32))


_DIST_WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from fsw_gnn_amd import FSW_conv, synth
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)       # ranks share cuda:0 here; RCCL needs one GPU per rank
dev = torch.device("cuda:0")
n, E, d = 3000, 30000, 16
ei = torch.from_numpy(synth.er_multigraph(n, E, seed=7)).to(dev)
X = torch.from_numpy(synth.features(n, d, seed=8)).to(dev)
torch.manual_seed(3)
conv = FSW_conv(d, 12, embed_dim=31, device=dev)                   # 30 slices: uneven blocks over 4 ranks
rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
with torch.no_grad():
    ref = conv(X, ei)                                              # single-GPU fused path
    conv.fuse_linear = False
    ref_u = conv(X, ei)
    conv.fuse_linear = True
    # 1. gather form: this rank's block of slices + all-gather, pipelined over 2 node-range chunks
    st = {}
    conv.enable_slice_parallel(None, mode="gather", chunks=2, stats=st)
    y = conv(X, ei)
    assert st["mode"] == "gather" and st["collective"] == "all_gather", st
    assert torch.equal(y, ref_u), float((y - ref_u).abs().max())  # no reduction anywhere: bit-identical to one GPU
    conv.enable_slice_parallel(None, mode="gather", chunks=1)
    assert torch.equal(conv(X, ei), ref_u)
    # 2. sharded-consumer form: W1 column block inside the fused kernel, reduce-scatter of the partial sums
    for chunks in (1, 2):
        conv.enable_slice_parallel(None, mode="consumer", chunks=chunks, stats=st)
        yc = conv(X, ei)
        assert st["mode"] == "consumer" and st["collective"] == "reduce_scatter+all_gather", st
        assert tuple(yc.shape) == tuple(ref.shape) and rel(yc, ref) < 1e-6, rel(yc, ref)   # sums over the ranks: order differs
    conv.enable_slice_parallel(None, mode="consumer", chunks=2, output="sharded")
    R, row0 = conv(X, ei)
    m = R.shape[1]
    for c in range(R.shape[0]):
        r0 = int(row0[c]); r1 = min(r0 + m, n)
        if r1 > r0:
            assert rel(R[c, :r1 - r0], ref[r0:r1]) < 1e-6
    # 2b. sharded output of a layer whose tail is Linear -> BatchNorm1d -> act -> Linear: the remaining modules see [rows, H]
    # (eval-mode BatchNorm is row-wise); pad rows past the last node come back as zeros; batch statistics mode is refused
    torch.manual_seed(5)
    conv2 = FSW_conv(d, 12, embed_dim=31, mlp_layers=2, mlp_hidden_dim=12, batchNorm_hidden=True, device=dev)
    conv2.mlp[1].running_mean.copy_(torch.randn(12, device=dev) * 0.1)
    conv2.mlp[1].running_var.copy_(torch.rand(12, device=dev) + 0.5)
    conv2.eval()
    ref_bn = conv2(X, ei)
    conv2.enable_slice_parallel(None, mode="consumer", chunks=2, output="sharded")
    Rb, row0b = conv2(X, ei)
    assert Rb.dim() == 3 and Rb.shape[2] == 12
    for c in range(Rb.shape[0]):
        r0 = int(row0b[c]); r1 = min(r0 + Rb.shape[1], n)
        if r1 > r0:
            assert rel(Rb[c, :r1 - r0], ref_bn[r0:r1]) < 1e-5, rel(Rb[c, :r1 - r0], ref_bn[r0:r1])
        assert not Rb[c, max(r1 - r0, 0):].any()
    conv2.train()
    try:
        conv2(X, ei)
        raise SystemExit("batch-statistics BatchNorm on a row shard must be refused")
    except NotImplementedError:
        pass
    # 2c. exchange form: all-to-all of the slice blocks to the row owners, the tail on the owned rows, all-gather of the output
    for chunks in (1, 2):
        conv.enable_slice_parallel(None, mode="exchange", chunks=chunks, stats=st)
        yx = conv(X, ei)
        assert st["mode"] == "exchange" and st["collective"] == "all_to_all+all_gather", st
        assert tuple(yx.shape) == tuple(ref_u.shape) and rel(yx, ref_u) < 1e-6, rel(yx, ref_u)   # same embedding bits, GEMM on a row subset
    conv.enable_slice_parallel(None, mode="exchange", chunks=2, output="sharded", stats=st)
    Rx, row0x = conv(X, ei)
    assert st["collective"] == "all_to_all"
    for c in range(Rx.shape[0]):
        r0 = int(row0x[c]); r1 = min(r0 + Rx.shape[1], n)
        if r1 > r0:
            assert rel(Rx[c, :r1 - r0], ref_u[r0:r1]) < 1e-6
    conv2.eval()
    conv2.enable_slice_parallel(None, mode="exchange", chunks=2)
    assert rel(conv2(X, ei), ref_bn) < 1e-5                        # Linear -> BatchNorm (eval) -> act -> Linear tail on the owned rows
    conv2.enable_slice_parallel(None, enabled=False)
    # 2d. a layer too wide for the fused tile on ONE GPU (512 slices) takes the consumer form once its slices are spread over the
    # ranks (BASELINE config 4's situation: 1024 slices as 128 per GPU)
    torch.manual_seed(9)
    convw_ = FSW_conv(d, 12, embed_dim=513, device=dev)
    assert not convw_._fusable() and convw_._fusable(512 // world)
    ref_w = convw_(X, ei)
    convw_.enable_slice_parallel(None, mode="consumer", chunks=2, stats=st)
    yw_ = convw_(X, ei)
    assert st["mode"] == "consumer" and rel(yw_, ref_w) < 2e-6, rel(yw_, ref_w)
    del convw_
    # 3. auto on a graph with long rows: the consumer form does not apply, the gather form takes over
    ei2 = torch.cat([ei, torch.stack([torch.arange(300, device=dev), torch.full((300,), 2999, device=dev)]),
                     torch.stack([torch.arange(50, device=dev), torch.full((50,), 5, device=dev)])], dim=1)
    conv.enable_slice_parallel(None, mode="auto", stats=st)
    y2 = conv(X, ei2)
    assert st["mode"] == "gather"
    conv.enable_slice_parallel(None, enabled=False)
    ref2 = conv(X, ei2)
    assert rel(y2, ref2) < 1e-6
    conv.enable_slice_parallel(None, mode="exchange", stats=st)   # the exchange form covers long rows too
    y2x = conv(X, ei2)
    assert st["mode"] == "exchange" and rel(y2x, ref2) < 1e-6
    convw = FSW_conv(d, 12, embed_dim=31, edge_weighting="gcn", self_loop_weight=0.5, mlp_layers=0, device=dev)   # general weights, dim_reduct tail
    refw = convw(X, ei)
    convw.enable_slice_parallel(None, mode="exchange", chunks=2, stats=st)
    yw = convw(X, ei)
    assert st["mode"] == "exchange" and rel(yw, refw) < 1e-6, rel(yw, refw)
    conv.enable_slice_parallel(None, mode="auto", stats=st)
    ya = conv(X, ei)
    assert st["mode"] == "consumer" and rel(ya, ref) < 1e-6
torch.cuda.synchronize()
# 4. training in slice mode: gradients equal the single-GPU gradients on every rank
def grads(sharded):
    conv.enable_slice_parallel(None, enabled=sharded)
    conv.zero_grad()
    Xg = X.clone().requires_grad_(True)
    out = conv(Xg, ei)
    torch.manual_seed(11)
    (out * torch.randn_like(out)).sum().backward()
    ps = {k: p.grad.clone() for k, p in conv.named_parameters() if p.grad is not None}
    ps["X"] = Xg.grad.clone()
    return out.detach(), ps
o1, g1 = grads(False)
o2, g2 = grads(True)
assert rel(o2, o1) < 1e-6
assert set(g1) == set(g2) and {"fsw_embed.projVecs", "fsw_embed.freqs", "mlp.0.weight", "X"} <= set(g1), sorted(g1)
for k in g1:
    assert rel(g2[k], g1[k]) < 2e-4, (k, rel(g2[k], g1[k]))        # float atomics: the order of the sums differs run to run
# inference-only forms are refused under autograd instead of silently returning the replicated gather form
conv.enable_slice_parallel(None, mode="consumer", output="sharded")
try:
    conv(X.clone().requires_grad_(True), ei)
    raise SystemExit("output='sharded' under autograd must be refused")
except NotImplementedError:
    pass
conv.enable_slice_parallel(None, enabled=False)
# node-range sharding (extra, behind its flag): every rank runs the fused layer on its rows, one all-gather of the OUTPUT
conv.enable_node_parallel(None)
with torch.no_grad():
    yn = conv(X, ei)
    yn2 = conv(X, ei2)
    conv.enable_node_parallel(None, enabled=False)
torch.cuda.synchronize()
assert float((yn - ref).abs().max()) < 2e-6 * float(ref.abs().max())     # same kernel on the same rows; only x . W2^T comes from a BLAS GEMM here
assert float((yn2 - ref2).abs().max()) < 2e-5 * float(ref2.abs().max())
dist.barrier()
if rank == 0:
    print("DIST_OK")
'''


@pytest.mark.parametrize("world", [2, 4])
def test_slice_parallel_conv_matches_single_gpu(dev, world, tmp_path):
    """FSW_conv.enable_slice_parallel (gather / sharded-consumer / auto forms, inference and training) and
    enable_node_parallel over `world` ranks (gloo, ranks sharing the one GPU of the test box)."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    script = tmp_path / "dist_worker.py"
    script.write_text(_DIST_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29700 + world), WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-2000:] for o in outs]
    assert "DIST_OK" in outs[0][0]


_RCCL_WORKER = """
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)     # "nccl" is RCCL on ROCm
from fsw_gnn_amd.dist import all_gather_slice_blocks, slice_partition
n, S = 1000, 37
local = torch.randn((n, 1 + S), device=dev)
out = torch.empty((n, 1 + S + 5), device=dev)
all_gather_slice_blocks(local, slice_partition(S, 1), 1, out)
torch.cuda.synchronize()
assert torch.equal(out[:, :1 + S], local)
# the reduce-scatter / all-gather pipeline of the sharded-consumer form on the same backend (asynchronous collectives)
from fsw_gnn_amd.dist import reduce_scatter_pipeline
P = torch.randn((3 * 2048, 8), device=dev)
def part(c, Pc): Pc.copy_(P[c * 2048:(c + 1) * 2048])
def fin(r0, r1, R): R.mul_(2.0)
st = {}
Y = reduce_scatter_pipeline(part, fin, 3, 2048, 5000, 8, torch.float32, dev, None, "replicated", st)
torch.cuda.synchronize()
assert torch.equal(Y, 2.0 * P[:5000]) and st["collective"] == "reduce_scatter+all_gather"
dist.barrier()
dist.destroy_process_group()
print("RCCL_OK")
"""


def test_rccl_backend_runs_the_gather_collective(dev, tmp_path):
    """The collective of the slice-parallel path on the real backend (RCCL; one rank is all a one-GPU box allows --
    the multi-rank logic is covered by the gloo tests above and in tests/test_host_cpu.py)."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    script = tmp_path / "rccl_worker.py"
    script.write_text(_RCCL_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29731", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RCCL_OK" in r.stdout, r.stderr[-2000:]
