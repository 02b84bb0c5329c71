"""Edge-feature kernels (fsw_embed_args.efeat / Ve / ldve / d_edge): every degree class against the float64 oracle, per entry.

With edge features fsw_embed_f32 runs k_embed_wsort<8|16|32|64, true> and k_embed_wsort_global<32, true> (embed_wsort.hip), which
nothing else launches, and fsw_embed_backward_keys_f32 takes the efeat branches of embed_bwd.hip, embed_mid_bwd.hip,
k_embed_wsort_bwd<4 .. 64, true> and k_embed_wsort_global_bwd<32, true>.  The graph holds one recipient per degree of LADDER (the
DEGREES of tests/test_hip_ties.py, plus 16384 and 16385: both sides of every class boundary of both directions), built by
fsw_graph_build_coalesced from a shuffled edge list in which every sender occurs once.

Exact keys (tests/edge_feature_cases.py, tests/test_edge_features_cpu.py): Xp, the edge features and Ve lie on dyadic grids narrow
enough that the key Xp + <ef, Ve> has no rounding in float32 in any order of evaluation, so the oracle (oracle/fsw_oracle.py,
edge_feat=) ranks bit-identical keys without a keys_override and the project's own bounds apply: forward per row <= TOL (1e-5),
stored gkey per row <= F32_BOUND (3e-5) and per entry <= PER_ENTRY (1e-5) of the line maximum, gfreq <= F32_BOUND -- check_forward
and check_key_gradients of tests/test_hip_ties.py, unchanged.

Slice groups, from the code (LINE = 64 M + 65 floats per line; forward: 69 KiB - 64 floats - one weight line; backward: 69 KiB,
140 KiB at M = 64, - one weight line; groups of kTileLines & ~3 lines, or kTileLines below 4), four workgroups per row (gridDim.y):
    forward   k_embed_wsort      M = 8 / 16 / 32 / 64:      28 / 12 / 4 / 3 lines
    backward  k_embed_wsort_bwd  M = 4 / 8 / 16 / 32 / 64:  52 / 28 / 12 / 4 / 4 lines
S = 13: the forward's M = 64 class has 5 groups (the gridDim.y loop wraps) and a last group of one slice, M = 16 and M = 32 a last group
of one slice, M = 8 one partial group; the backward's classes likewise, without a wrap.  S = 211 = 4 * 52 + 3: every class of both
directions has more than four groups (wraps) and a partial last group (the clamped tail kcl = min(k0 + kk, S - 1)).

Measured on an MI355X, largest per-entry error / line maximum of the stored gkey over all cases, tied columns | control column:
    fsw_embed_backward_keys_f32 with efeat   rows of total mass 0.4: 1.9e-6 | 4.3e-7 (D = 31), 2.4e-6 | 2.0e-6 (D = 193), 2.4e-6 | 2.1e-6 (D = 2049)
                                             every other class (D = 1 .. 32769): 8.3e-8 .. 1.7e-7 | 3.4e-8 .. 1.5e-7
    fsw_embed_generic with Ke                float32 storage <= 5.9e-8 | 5.6e-8 in every class; float64 storage <= 9.8e-12 (D = 1) | 5.5e-12
    per row: gkey <= 1.0e-6 (generic float64 2.4e-12), gfreq <= 4.2e-7 (9.8e-13), forward generic 3.7e-8 (3.4e-12), module 2.9e-7
    forward per row, tuned kernels: <= 1.1e-6 except the rows of total mass 0.4: D = 31 1.9e-6, D = 193 5.1e-6, D = 2049 5.3e-6 at
    tau = 1 and 8.3e-6 at tau = 3
No class has a bound of its own.  The rows of total mass 0.4 carry the largest figures in both directions, as in
tests/test_hip_ties.py (the pad element's weight rounded to float32); in the forward of embed_wsort.hip their readout also differences
float32 sines of neighbouring ranks, (s - sprev) with |s - sprev| ~ 2 pi xi w / max(m, tau), which at tau = 3 leaves the row of 2049
within a factor 1.2 of TOL -- the closest any row comes.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests import edge_feature_cases as EC
from tests.conftest import relerr
from tests.test_hip_ties import (CONTROL, DEGREES, F32_BOUND, G64_ROW, OUT_SCALE, PER_ENTRY, TOL, check_forward, check_key_gradients,
                                 coefficient_scale, hip_projection, make_module)

pytestmark = pytest.mark.gpu

LADDER = DEGREES + (16384, 16385)
GIANT = (0, 5, 32769)               # FSW_BIN_GLOBAL: above FSW_HUB_MAX_DEG
WIDE_LADDER = (0, 1, 32, 33, 128, 129, 192, 193, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4097)
HAS_MASS, MASS_SCALE = 1, 1.25
MASS_FNS = ("identity", "sqrt", "log")
S_WIDE = 211


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


# ---- the graph on the device and the oracle's answers, computed once -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ef_case(d_edge, degrees=LADDER):
    """The coalesced graph of `degrees` with d_edge features per edge; everything the oracle needs is read back from the device."""
    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.graph import build_csr_coalesced
    dev = torch.device("cuda:0")
    rows, nnz = len(degrees), int(sum(degrees))
    rec, snd, w, ef = EC.edge_list(degrees, d_edge)
    graph = build_csr_coalesced(t(rec, dev, torch.int64), t(snd, dev, torch.int64), t(w, dev), t(ef, dev), rows, nnz)
    st = graph.read_stats()
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_NNZ] == nnz and st[_lib.STAT_MAX_DEGREE] == max(degrees)
    rowptr = graph.rowptr.cpu().numpy().astype(np.int64)
    assert tuple(np.diff(rowptr)) == tuple(degrees)
    bins = np.diff(graph.bin_start_host[0]).tolist()
    print("bin occupancy (d_edge %d): %s" % (d_edge, {n: b for n, b in zip(EC.bin_names(), bins) if b}))
    assert bins == EC.bin_rows(degrees)
    order = EC.csr_order(rec, snd)
    col = graph.col[:nnz].cpu().numpy().astype(np.int64)
    assert np.array_equal(col, snd[order]) and np.array_equal(np.sort(col), np.arange(nnz))      # every sender exactly once
    wv, efv = graph.w[:nnz].cpu().numpy(), graph.ef[:nnz].cpu().numpy()
    assert np.array_equal(wv, w[order]) and np.array_equal(efv, ef[order])
    if degrees == LADDER:
        assert bins[_lib.BIN_MID0:] == [2, 1, 1, 1, 0, 1, 1, 1, 3, 3, 3, 3, 2, 1, 2, 1, 0]      # mid, LDS, hub bins, global
        assert (wv == 0).sum() >= 30
        for deg in EC.LOW_MASS_ROWS:
            r = degrees.index(deg)
            assert abs(wv[rowptr[r]:rowptr[r + 1]].astype(np.float64).sum() - 0.4) < 1e-5
    g = np.random.default_rng(43).standard_normal((rows, HAS_MASS + S_WIDE)).astype(np.float32)
    return {"graph": graph, "st": st, "rowptr": rowptr, "col": col, "w": wv.astype(np.float64), "ef": efv, "g": g, "degrees": degrees}


@functools.lru_cache(maxsize=None)
def key_case(d_edge, S, degrees=LADDER):
    """Ve [S, d_edge], the edge term and Xp of every entry [nnz, S], the keys in float64."""
    c = ef_case(d_edge, degrees)
    Ve = EC.slice_vectors(S, d_edge)
    term = EC.edge_term(c["ef"], Ve)
    xp = EC.xp_columns(c["rowptr"], term)
    keys = xp.astype(np.float64) + term
    assert np.array_equal(EC.keys_float32(xp, c["ef"], Ve).astype(np.float64), keys)
    return {"Ve": Ve, "term": term, "xp": xp, "keys": keys, "kinds": EC.kinds(S), "freqs": EC.freqs(S)}


@functools.lru_cache(maxsize=None)
def reference(d_edge, S, tau, degrees=LADDER):
    """Oracle (float64) on the same arrays: the 'features' of entry e are its Xp values, the slices the unit vectors next to Ve."""
    c, k = ef_case(d_edge, degrees), key_case(d_edge, S, degrees)
    nnz, rowptr, fr = c["col"].size, c["rowptr"], k["freqs"].astype(np.float64)
    X, V = k["xp"].astype(np.float64), np.concatenate([np.eye(S), k["Ve"].astype(np.float64)], axis=1)
    ident = np.arange(nnz)
    emb, mass = O.fsw_embed_csr(X, rowptr, ident, c["w"], V, fr, total_mass_pad_thresh=tau, return_mass=True, edge_feat=c["ef"])
    G = OUT_SCALE * c["g"][:, HAS_MASS:HAS_MASS + S].astype(np.float64)
    _, _, gxi, _, gkey = O.fsw_embed_csr_backward(X, rowptr, ident, c["w"], V, fr, G, total_mass_pad_thresh=tau, edge_feat=c["ef"],
                                                  return_gkey=True)
    # a slice whose Ve row is zero: the oracle without edge features on the same Xp.  Same keys, same order; numpy sums the D terms of a
    # row in another association when the slice axis has another length, D * 2^-53 <= 4e-12 for the longest row here
    zc = [i for i, kind in enumerate(k["kinds"]) if kind == "zero_ve"]
    plain = O.fsw_embed_csr(X[:, zc], rowptr, ident, c["w"], np.eye(len(zc)), fr[zc], total_mass_pad_thresh=tau)
    assert len(zc) >= 1 and relerr(emb[:, zc], plain) <= max(degrees) * 2.0 ** -53
    for a in (emb, mass, gkey, gxi):
        a.setflags(write=False)
    return {"emb": emb, "mass": mass, "gkey": gkey, "gfreq": gxi, "scale": coefficient_scale(G, fr)}


def bias_vector(S):
    return (np.random.default_rng(46).integers(-8, 9, size=HAS_MASS + S) / 8.0).astype(np.float32)


def expected_out(ref, mass_fn, bias):
    full = np.concatenate([(O.mass_value(ref["mass"], MASS_FNS[mass_fn]) * MASS_SCALE)[:, None], ref["emb"]], axis=1)
    return OUT_SCALE * (full if bias is None else full + bias.astype(np.float64))


# ---- the tuned kernels ---------------------------------------------------------------------------------------------------------------
def embed_args(c, Xp, Ve, d_edge, fr, S, tau, mass_fn, bias, scratch, host_bins=True):
    from fsw_gnn_amd import _lib
    graph, st = c["graph"], c["st"]
    a = _lib.EmbedArgs()
    a.rowptr, a.col, a.perm, a.bin_start = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.perm.data_ptr(), graph.bin_start.data_ptr()
    a.w, a.num_rows = graph.w.data_ptr(), len(c["degrees"])
    a.bin_start_host = graph.bin_start_host[0].ctypes.data if host_bins else None
    a.Xp, a.ldp, a.freqs, a.S, a.tau = Xp.data_ptr(), Xp.stride(0), fr.data_ptr(), S, tau
    a.unit_table, a.ldt = None, 0
    a.bias = bias.data_ptr() if bias is not None else None
    a.out_scale, a.has_mass, a.mass_fn, a.mass_scale = OUT_SCALE, HAS_MASS, mass_fn, MASS_SCALE
    a.num_reg_rows, a.num_lds_rows = st[_lib.STAT_NUM_REG], st[_lib.STAT_NUM_LDS]
    a.num_global_rows, a.num_zero_rows, a.max_degree = st[_lib.STAT_NUM_GLOBAL], st[_lib.STAT_NUM_ZERO], st[_lib.STAT_MAX_DEGREE]
    a.scratch, a.scratch_bytes = (scratch.data_ptr(), scratch.numel()) if scratch is not None else (None, 0)
    a.efeat, a.Ve, a.ldve, a.d_edge = graph.ef.data_ptr(), Ve.data_ptr(), Ve.stride(0), d_edge
    return a


def device_inputs(dev, d_edge, pad, S, degrees=LADDER):
    """Xp [nnz, S + 5] (sender col[e] carries the Xp of entry e; the columns from S on hold NaN), Ve [S, d_edge + pad] with NaN in
    the padding, the frequencies, the output gradient."""
    c, k = ef_case(d_edge, degrees), key_case(d_edge, S, degrees)
    Xp = np.full((c["col"].size, S + 5), np.nan, dtype=np.float32)
    Xp[c["col"], :S] = k["xp"]
    Ve = np.full((S, d_edge + pad), np.nan, dtype=np.float32)
    Ve[:, :d_edge] = k["Ve"]
    return t(Xp, dev), t(Ve, dev), t(k["freqs"], dev), t(c["g"][:, :HAS_MASS + S], dev)


def run_tuned_kernels(dev, d_edge, pad, S, tau, mass_fn, with_bias, host_bins=True, degrees=LADDER):
    """fsw_embed_f32 and fsw_embed_backward_keys_f32 with edge features: (out [rows, 1 + S + 2], gkey [nnz, S + 2], gfreq [S]); the two
    columns past the end of out and gkey keep their NaN."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    c = ef_case(d_edge, degrees)
    nnz = c["col"].size
    stream = torch.cuda.current_stream(dev).cuda_stream
    Xp, Ve, fr, g = device_inputs(dev, d_edge, pad, S, degrees)
    bias = t(bias_vector(S), dev) if with_bias else None
    scratch = torch.empty(int(L.fsw_embed_scratch_bytes(max(degrees))), dtype=torch.uint8, device=dev)
    out = torch.full((len(degrees), HAS_MASS + S + 2), float("nan"), device=dev)
    a = embed_args(c, Xp, Ve, d_edge, fr, S, tau, mass_fn, bias, scratch, host_bins)
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    _lib.check(L.fsw_embed_f32(ctypes.byref(a), stream), "fsw_embed_f32")
    gkey = torch.full((nnz, S + 2), float("nan"), device=dev)
    gf = torch.zeros(S, device=dev)
    a = embed_args(c, Xp, Ve, d_edge, fr, S, tau, mass_fn, bias, scratch, host_bins)
    _lib.check(L.fsw_embed_backward_keys_f32(ctypes.byref(a), None, _lib.ptr(g), g.stride(0), _lib.ptr(gkey), gkey.stride(0),
                                             _lib.ptr(gf), stream), "fsw_embed_backward_keys_f32")
    torch.cuda.synchronize()
    res = out.cpu().numpy().astype(np.float64), gkey.cpu().numpy().astype(np.float64), gf.cpu().numpy().astype(np.float64)
    del scratch, out, gkey
    return res


def check_all_rows_forward(got, ref, degrees, what, bound=TOL):
    """Per row norm-wise <= bound, for every row (check_forward of tests/test_hip_ties.py stops at the rows of DEGREES)."""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    errs = np.array([relerr(got[r], ref[r]) for r in range(len(degrees))])
    print("%s: forward per row max %.2e (D = %d)   %s" % (what, errs.max(), degrees[errs.argmax()],
                                                          "  ".join("%d: %.1e" % de for de in zip(degrees, errs))))
    assert errs.max() <= bound, (what, dict(zip(degrees, errs.tolist())))


def check_case(out, gkey, gf, d_edge, S, tau, mass_fn, with_bias, what, degrees=LADDER, row_bound=F32_BOUND, entry_bound=PER_ENTRY,
               fwd_bound=TOL, floor=1e-6, padded=2):
    c, k, ref = ef_case(d_edge, degrees), key_case(d_edge, S, degrees), reference(d_edge, S, tau, degrees)
    bias = bias_vector(S) if with_bias else None
    want = expected_out(ref, mass_fn, bias)
    K = HAS_MASS + S
    if padded:
        assert np.isnan(out[:, K:]).all() and np.isnan(gkey[:, S:]).all(), what      # columns past the end are untouched
    out, gkey = out[:, :K], gkey[:, :S]
    check_all_rows_forward(out, want, degrees, what, fwd_bound)
    if degrees == LADDER and bias is None and fwd_bound == TOL:
        check_forward(out[:len(DEGREES)], want[:len(DEGREES)], what)
    dead = [i for i in range(S) if k["freqs"][i] == -1.0]
    keep = [i for i in range(S) if k["freqs"][i] != -1.0]
    if fwd_bound == TOL:                                            # xi = -1: out_scale * bias, nothing else
        dead_out = np.float32(OUT_SCALE) * (bias[[HAS_MASS + i for i in dead]] if with_bias else np.zeros(len(dead), dtype=np.float32))
        assert np.array_equal(out[:, [HAS_MASS + i for i in dead]], np.broadcast_to(dead_out.astype(np.float64), (len(degrees), len(dead)))), what
    assert np.isfinite(gkey).all(), what
    assert np.abs(gkey[:, dead]).max() == 0.0 and CONTROL in k["kinds"], what
    names = [k["kinds"][i] for i in keep]
    check_key_gradients(gkey[:, keep], ref["gkey"][:, keep], c["rowptr"], names, what, ref["scale"][:, keep], row_bound=row_bound,
                        entry_bound=entry_bound, floor=floor)
    e = relerr(gf, ref["gfreq"])
    print("%s: gfreq %.2e" % (what, e))
    assert np.isfinite(gf).all() and e <= row_bound, (what, e)


# (d_edge, ldve - d_edge, S, tau, mass_fn, bias, host copy of the bins)
TUNED_CASES = [
    (1, 0, 13, 1.0, 0, False, True),
    (1, 3, 13, 1.0, 1, True, True),
    (3, 0, 13, 1.0, 2, True, True),
    (3, 3, 13, 1.0, 0, False, True),
    (5, 0, 13, 1.0, 1, False, True),
    (5, 3, 13, 1.0, 2, True, True),
    (5, 3, 13, 3.0, 0, True, True),                 # tau = 3: every row carries a pad element of positive weight
    (3, 3, 13, 1.0, 1, False, False),               # no host copy of the bins: the launchers skip the bins max_degree cannot reach
]


@pytest.mark.parametrize("d_edge,pad,S,tau,mass_fn,with_bias,host_bins", TUNED_CASES)
def test_tuned_kernels_with_edge_features(dev, d_edge, pad, S, tau, mass_fn, with_bias, host_bins):
    """fsw_embed_f32 and fsw_embed_backward_keys_f32 with efeat on the graph of LADDER, general weights with exact zeros and three rows
    of total mass 0.4 (their pad element ties with every zero key), key columns of every kind of tests/edge_feature_cases.py, frequencies
    of either sign, both zeros and -1, has_mass with every mass_fn, bias, out_scale 0.7, Ve rows padded with NaN (ldve > d_edge), out and
    gkey pre-filled with NaN.  Forward per row <= TOL; gkey finite, per row <= F32_BOUND, per entry <= PER_ENTRY of the line maximum;
    gfreq <= F32_BOUND; the columns past S of out and gkey untouched; at xi = -1 out is out_scale * bias and gkey 0."""
    what = "edge features d_edge %d ldve %d S %d tau %g mass_fn %d%s%s" % (d_edge, d_edge + pad, S, tau, mass_fn, " bias" if with_bias else "",
                                                                         "" if host_bins else " no host bins")
    out, gkey, gf = run_tuned_kernels(dev, d_edge, pad, S, tau, mass_fn, with_bias, host_bins)
    check_case(out, gkey, gf, d_edge, S, tau, mass_fn, with_bias, what)


def test_wide_slice_axis_with_edge_features(dev):
    """S = 211 on WIDE_LADDER (both sides of every boundary between two slice-group kernels; the rows above 2048 neighbours run one
    wavefront per line, without slice groups): every slice-group loop of both directions wraps and ends in a partial group."""
    S = S_WIDE
    assert all(S > 4 * sc and S % sc for sc in (28, 12, 4, 3, 52))
    out, gkey, gf = run_tuned_kernels(dev, 3, 3, S, 1.0, 2, True, True, WIDE_LADDER)
    check_case(out, gkey, gf, 3, S, 1.0, 2, True, "edge features, S %d" % S, WIDE_LADDER)


def test_rows_above_the_hub_bins_with_edge_features(dev):
    """Rows of 0, 5 and 32769 neighbours: FSW_BIN_GLOBAL of k_embed_wsort_global / _bwd (scratch lines of 65536 elements, 1.6 GB by
    fsw_embed_scratch_bytes, allocated here and dropped), S = 13, d_edge 3 with ldve 6.  Same assertions."""
    from fsw_gnn_amd import _lib
    c = ef_case(3, GIANT)
    assert np.diff(c["graph"].bin_start_host[0]).tolist()[-1] == 1 and c["st"][_lib.STAT_NUM_GLOBAL] == 1
    out, gkey, gf = run_tuned_kernels(dev, 3, 3, 13, 1.0, 2, True, True, GIANT)
    torch.cuda.empty_cache()
    check_case(out, gkey, gf, 3, 13, 1.0, 2, True, "edge features, rows of 0 / 5 / 32769", GIANT)


def test_backward_without_key_gradients_refuses_edge_features(dev):
    """fsw_embed_backward_f32 (atomic form, no gkey) with efeat set: non-zero status, a message, and nothing written to gXp."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    d_edge, S = 3, 13
    c = ef_case(d_edge)
    Xp, Ve, fr, g = device_inputs(dev, d_edge, 0, S)
    scratch = torch.empty(int(L.fsw_embed_scratch_bytes(max(LADDER))), dtype=torch.uint8, device=dev)
    a = embed_args(c, Xp, Ve, d_edge, fr, S, 1.0, 0, None, scratch)
    gXp = torch.zeros((c["col"].size, S), device=dev)
    gf = torch.zeros(S, device=dev)
    rc = L.fsw_embed_backward_f32(ctypes.byref(a), None, _lib.ptr(g), g.stride(0), _lib.ptr(gXp), gXp.stride(0), _lib.ptr(gf),
                                  torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0
    assert b"edge features" in L.fsw_last_error()
    assert not gXp.any().item() and not gf.any().item()


# ---- the generic kernel: a second implementation of the oracle's edge-feature branch -------------------------------------------------
def run_generic_kernel(dev, d_edge, S, tau, storage):
    """fsw_embed_generic with Ke = ef . Ve^T (computed on the host, exact on the grids): (out [rows, 1 + S], gkey [nnz, S], gfreq)."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    c, k = ef_case(d_edge), key_case(d_edge, S)
    graph, nnz = c["graph"], c["col"].size
    dt = torch.float64 if storage == "float64" else torch.float32
    stream = torch.cuda.current_stream(dev).cuda_stream
    Xp_host = np.zeros((nnz, S))
    Xp_host[c["col"]] = k["xp"]
    Xp, Ke, fr = t(Xp_host, dev, dt), t(k["term"], dev, dt), t(k["freqs"], dev, dt)
    g = t(c["g"][:, :HAS_MASS + S], dev, dt)
    w = graph.w[:nnz].to(dt).contiguous()
    scratch = torch.empty(int(L.fsw_embed_generic_scratch_bytes(max(LADDER), len(LADDER))), dtype=torch.uint8, device=dev)
    out = torch.full((len(LADDER), HAS_MASS + S), float("nan"), dtype=dt, device=dev)
    gkey = torch.full((nnz, S), float("nan"), dtype=dt, device=dev)
    gf = torch.zeros(S, dtype=dt, device=dev)

    def args(**fields):
        a = _lib.GenericArgs()
        a.value_dtype, a.S = (1 if dt == torch.float64 else 0), S
        a.rowptr, a.col, a.w = graph.rowptr.data_ptr(), graph.col.data_ptr(), w.data_ptr()
        a.num_rows, a.max_degree = len(LADDER), max(LADDER)
        a.Xp, a.ldp, a.Ke, a.ldke, a.freqs, a.tau = Xp.data_ptr(), Xp.stride(0), Ke.data_ptr(), Ke.stride(0), fr.data_ptr(), tau
        a.out_scale, a.has_mass, a.mass_fn, a.mass_scale = OUT_SCALE, HAS_MASS, 0, MASS_SCALE
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        for name, v in fields.items():
            setattr(a, name, v)
        return a

    _lib.check(L.fsw_embed_generic(ctypes.byref(args(out=out.data_ptr(), ldo=out.stride(0))), stream), "fsw_embed_generic")
    _lib.check(L.fsw_embed_generic(ctypes.byref(args(g=g.data_ptr(), ldg=g.stride(0), gkey=gkey.data_ptr(), ldk=S, gfreq=gf.data_ptr())),
                                   stream), "fsw_embed_generic (backward)")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), gkey.cpu().numpy().astype(np.float64), gf.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("storage", ["float64", "float32"])
@pytest.mark.parametrize("d_edge,tau", [(3, 1.0), (5, 3.0)])
def test_generic_kernel_with_edge_term(dev, d_edge, tau, storage):
    """fsw_embed_generic with Ke on the same ladder, S = 13: float64 storage per row <= G64_ROW (1e-10) forward and backward and per
    entry 1e-10 of the line maximum (floored at 2e-4 of the line's scale, as in tests/test_hip_ties.py); float32 storage at the bounds of
    the tuned kernels.  Two implementations of the edge-feature branch, the oracle's and this kernel's, agree."""
    S = 13
    out, gkey, gf = run_generic_kernel(dev, d_edge, S, tau, storage)
    what = "generic %s with Ke, d_edge %d tau %g" % (storage, d_edge, tau)
    if storage == "float64":
        check_case(out, gkey, gf, d_edge, S, tau, 0, False, what, row_bound=G64_ROW, entry_bound=G64_ROW, fwd_bound=G64_ROW, floor=2e-4,
                   padded=0)
    else:
        check_case(out, gkey, gf, d_edge, S, tau, 0, False, what, padded=0)


# ---- module level: host routing at the project's own bound ---------------------------------------------------------------------------
MODULE_LADDER = (32, 33, 128, 129, 256, 257, 2048, 2049, 4097)
MODULE_LONG = (2048, 2049, 4097)


@functools.lru_cache(maxsize=None)
def module_case():
    """One recipient per degree of MODULE_LADDER, every node sends to one recipient; an eighth of the (recipient, sender) pairs occurs
    twice in the edge list, so the coalescing build sums two weights and two feature vectors.  X multiples of 1/8 in [-4, 4], projVecs
    multiples of 1/8 in [-1, 1] (d_in 8 + d_edge 3), features multiples of 1/4 whose sums stay in [-2, 2]: exact projection, exact keys."""
    rng = np.random.default_rng(61)
    n, d, de, S = sum(MODULE_LADDER), 8, 3, 13
    rec = np.repeat(np.arange(len(MODULE_LADDER)), MODULE_LADDER).astype(np.int64)
    snd = rng.permutation(n).astype(np.int64)
    dup = rng.random(n) < 0.125
    rec, snd = np.concatenate([rec, rec[dup]]), np.concatenate([snd, snd[dup]])
    E = rec.size
    twice = np.concatenate([dup, np.ones(int(dup.sum()), dtype=bool)])
    w = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), size=E)
    w[rng.choice(E, size=40, replace=False)] = 0.0
    ef = (np.where(twice[:, None], rng.integers(-4, 5, size=(E, de)), rng.integers(-8, 9, size=(E, de))) / 4.0).astype(np.float32)
    order = rng.permutation(E)
    rec, snd, w, ef = rec[order], snd[order], w[order], ef[order]
    # the coalesced entries on the host: sorted by (recipient, sender), weights and features summed (exact: few dyadic terms)
    key, slot = np.unique(rec * n + snd, return_inverse=True)
    crec, col = key // n, key % n
    cw, cef = np.zeros(key.size), np.zeros((key.size, de))
    np.add.at(cw, slot, w.astype(np.float64))
    np.add.at(cef, slot, ef.astype(np.float64))
    assert key.size == n and np.abs(cef).max() <= 2.0
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(crec, minlength=len(MODULE_LADDER)))]).astype(np.int64)
    assert tuple(np.diff(rowptr)) == MODULE_LADDER
    X = (rng.integers(-32, 33, size=(n, d)) / 8.0).astype(np.float32)
    V = (rng.integers(-8, 9, size=(S, d + de)) / 8.0).astype(np.float32)
    V[7, d:] = 0.0                                                   # one slice without an edge part
    R = rng.standard_normal((len(MODULE_LADDER), S))
    return {"n": n, "d": d, "de": de, "S": S, "rec": rec, "snd": snd, "w": w, "ef": ef, "slot": slot, "rowptr": rowptr, "col": col,
            "cw": cw, "cef": cef, "X": X, "V": V, "fr": EC.freqs(S), "R": R}


def test_module_edge_features_on_exact_keys(dev):
    """FSW_embedding(d_edge=3, learnable_slices, learnable_freqs).embed_autograd on the coalesced graph of MODULE_LADDER (both sides of
    32/33, 128/129, 256/257, 2048/2049 and a row of 4097), duplicate (recipient, sender) pairs in the edge list.  The projection is exact
    (asserted bit for bit against float64), so are the keys: the oracle gets no override.  Forward per row <= TOL; gX, both halves of
    projVecs.grad, freqs.grad and the gradient of every input edge's features (routed through slot_of_edge to both copies of a duplicate)
    <= F32_BOUND norm-wise; gX and the feature gradient also per long recipient <= F32_BOUND."""
    from fsw_gnn_amd.graph import build_csr_coalesced
    m = module_case()
    n, d, S, rowptr, col = m["n"], m["d"], m["S"], m["rowptr"], m["col"]
    E = make_module(dev, m["V"], m["fr"], d_edge=m["de"])
    Xd = t(m["X"], dev).requires_grad_(True)
    efd = t(m["ef"], dev).requires_grad_(True)
    graph = build_csr_coalesced(t(m["rec"], dev, torch.int64), t(m["snd"], dev, torch.int64), t(m["w"], dev), efd.detach(),
                                len(MODULE_LADDER), n, want_slots=True)
    assert graph.read_stats()[6] == n
    assert np.array_equal(graph.slot_of_edge.cpu().numpy()[:m["rec"].size], m["slot"])
    assert np.array_equal(graph.col[:n].cpu().numpy(), col)
    assert np.array_equal(graph.w[:n].cpu().numpy().astype(np.float64), m["cw"])
    assert np.array_equal(graph.ef[:n].cpu().numpy().astype(np.float64), m["cef"])
    print("module bins: %s" % {b: c for b, c in zip(EC.bin_names(), np.diff(graph.bin_start_host[0]).tolist()) if c})
    out = E.embed_autograd(Xd, graph, edge_feat=efd)
    (out * t(m["R"], dev)).sum().backward()
    X64, V64 = m["X"].astype(np.float64), m["V"].astype(np.float64)
    xp = hip_projection(E, Xd, d)
    assert np.array_equal(xp.astype(np.float64), X64 @ V64[:, :d].T)          # operands of 6 and 4 significant bits: bf16x3 is exact
    ref_out = O.fsw_embed_csr(m["X"], rowptr, col, m["cw"], m["V"], m["fr"], edge_feat=m["cef"])
    gX, gV, gxi, gef = O.fsw_embed_csr_backward(m["X"], rowptr, col, m["cw"], m["V"], m["fr"], m["R"], edge_feat=m["cef"])
    what = "module, exact keys"
    check_all_rows_forward(out.detach().cpu().numpy().astype(np.float64), ref_out, MODULE_LADDER, what)
    got_gX, got_gef = Xd.grad.cpu().numpy().astype(np.float64), efd.grad.cpu().numpy().astype(np.float64)
    got_gV, got_gf = E.projVecs.grad.cpu().numpy().astype(np.float64), E.freqs.grad.cpu().numpy().astype(np.float64)
    gef_in = gef[m["slot"]]                                          # every copy of a duplicate receives its entry's gradient
    errs = {"gX": relerr(got_gX, gX), "gV vertex part": relerr(got_gV[:, :d], gV[:, :d]), "gV edge part": relerr(got_gV[:, d:], gV[:, d:]),
            "gfreqs": relerr(got_gf, gxi), "g_edge_feat": relerr(got_gef, gef_in)}
    print("%s: %s" % (what, "  ".join("%s %.2e" % kv for kv in errs.items())))
    assert np.isfinite(got_gX).all() and np.isfinite(got_gef).all() and np.isfinite(got_gV).all()
    assert max(errs.values()) <= F32_BOUND, errs
    crow = np.searchsorted(rowptr, np.arange(n), side="right") - 1      # recipient of every entry
    for deg in MODULE_LONG:
        r = MODULE_LADDER.index(deg)
        senders = col[rowptr[r]:rowptr[r + 1]]                         # they send to this row only
        edges = crow[m["slot"]] == r
        ex, ee = relerr(got_gX[senders], gX[senders]), relerr(got_gef[edges], gef_in[edges])
        print("%s: row of %d: gX %.2e g_edge_feat %.2e" % (what, deg, ex, ee))
        assert ex <= F32_BOUND and ee <= F32_BOUND, (deg, ex, ee)


def test_conv_layer_edge_features_on_exact_keys(dev):
    """FSW_conv(edgefeat_dim=3) on the same graph seen as n x n (nodes 0 .. 8 are the recipients of MODULE_LADDER, all other nodes have
    no in-edges; unit weighting, so a duplicate pair weighs 2), forward and one backward against the oracle plus the layer's own MLP in
    float64 (as test_fused_conv_odd_shapes_match_unfused_and_oracle does): y <= TOL; gX, the gradient of every input edge's features,
    projVecs.grad, freqs.grad and the first Linear layer's weight gradient <= F32_BOUND."""
    import copy
    from fsw_gnn_amd import FSW_conv
    m = module_case()
    n, d, de, out_ch = m["n"], m["d"], m["de"], 6
    torch.manual_seed(62)
    conv = FSW_conv(d, out_ch, edgefeat_dim=de, embed_dim=m["S"] + 1, device=dev)
    em = conv.fsw_embed
    assert em.nSlices == m["S"] and em.encode_total_mass and tuple(em.projVecs.shape) == m["V"].shape
    with torch.no_grad():
        em.projVecs.copy_(t(m["V"], dev))
        em.freqs.copy_(t(m["fr"], dev))
    ei = np.stack([m["snd"], m["rec"]])
    Xd = t(m["X"], dev).requires_grad_(True)
    efd = t(m["ef"], dev).requires_grad_(True)
    R = np.random.default_rng(63).standard_normal((n, out_ch))
    R[len(MODULE_LADDER):] *= 0.01                                  # rows without in-edges: the MLP of [mass 0 | 0 | x] only
    y = conv(Xd, t(ei, dev, torch.int64), edge_features=efd)
    (y * t(R, dev)).sum().backward()
    rowptr, col, w, _, ef, slot = O.coalesce_edge_index(ei, n, edge_features=m["ef"])
    assert np.array_equal(np.diff(rowptr)[:len(MODULE_LADDER)], MODULE_LADDER) and np.array_equal(ef[:m["cef"].shape[0]], m["cef"])
    bias = em.bias.detach().cpu().numpy().astype(np.float64) if em.enable_bias else None
    emb = O.fsw_embedding_forward(m["X"], rowptr, col, w, m["V"], m["fr"], bias=bias, encode_total_mass=True,
                                  total_mass_encoding_function=em.total_mass_encoding_function,
                                  total_mass_encoding_method=em.total_mass_encoding_method,
                                  total_mass_encoding_scale=float(em.total_mass_encoding_scale),
                                  total_mass_pad_thresh=em.total_mass_pad_thresh, edge_feat=ef)
    assert em.total_mass_encoding_method == "plain" and conv.concat_self
    mw, K = conv.message_weight_vs_self, m["S"] + 1
    h = torch.from_numpy(np.concatenate([mw * emb, m["X"].astype(np.float64)], axis=1)).requires_grad_(True)
    mlp64 = copy.deepcopy(conv.mlp).double().cpu()
    y_ref = mlp64(h)
    (y_ref * torch.from_numpy(R)).sum().backward()
    what = "conv layer, exact keys"
    e_y = relerr(y.detach().cpu().numpy(), y_ref.detach().numpy())
    e_rows = relerr(y.detach().cpu().numpy()[:len(MODULE_LADDER)], y_ref.detach().numpy()[:len(MODULE_LADDER)])
    print("%s: forward %.2e, recipients only %.2e" % (what, e_y, e_rows))
    assert e_y <= TOL and e_rows <= TOL
    gh = h.grad.numpy()
    G = mw * gh[:, 1:K]                                             # the mass column does not depend on X, V, freqs or the features
    gX, gV, gxi, gef = O.fsw_embed_csr_backward(m["X"], rowptr, col, w, m["V"], m["fr"], G, total_mass_pad_thresh=em.total_mass_pad_thresh,
                                                edge_feat=ef)
    errs = {"gX": relerr(Xd.grad.cpu().numpy(), gX + gh[:, K:]), "g_edge_feat": relerr(efd.grad.cpu().numpy(), gef[slot]),
            "gV": relerr(em.projVecs.grad.cpu().numpy(), gV), "gfreqs": relerr(em.freqs.grad.cpu().numpy(), gxi),
            "gW": relerr(conv.mlp[0].weight.grad.cpu().numpy(), mlp64[0].weight.grad.numpy())}
    print("%s: %s" % (what, "  ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= F32_BOUND, errs
