"""Cartesian mode on unit-weight hub rows (2049 .. 32768 neighbours): k_cart_hub (forward, no scratch) and k_cart_bwd_long (backward, one
scratch line per wavefront) through fsw_embed_cart_f32 / fsw_embed_cart_backward_keys_f32 and through the modules.

One graph with one recipient per degree: the class edges of the four workgroup sizes (2, 4, 8, 16 wavefronts per line) and one row
inside a class, next to rows of the register and wavefront classes.  The keys hold 200 sender pairs with bit-identical keys, one
constant column and one control column without ties.  Yardsticks: the float64 oracle through the diagonal identity (forward) and the
generic kernel with float64 storage on the same inputs (backward).  Bounds: the project's TOL, F32_BOUND and PER_ENTRY of
tests/test_hip_ties.py; FWD_BOUND / F32_BOUND of tests/test_hip_cartesian_conv.py at module level.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests.conftest import relerr
from tests.test_hip_ties import F32_BOUND, FREQS, PER_ENTRY, TOL, check_key_gradients, coefficient_scale

pytestmark = pytest.mark.gpu

DEGREES = (0, 7, 2048, 2049, 3000, 4096, 4097, 8192, 8193, 16384, 16385, 32768)
BEYOND = 32769                     # one row past the hub bins: stays on the generic kernel
SENDERS = 33000
TIED_PAIRS = 200
SHAPES = [(3, 5), (4, 8)]
COLUMN_KINDS = ("t", "a", "e", "t")        # tied pairs | constant | control (CONTROL of test_hip_ties) | tied pairs
OUT_SCALE, HAS_MASS = 0.7, 1
DEV = torch.device("cuda:0")


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


@functools.lru_cache(maxsize=None)
def edges():
    """(recipients, senders) of DEGREES + (BEYOND,), every row drawn without replacement."""
    rng = np.random.default_rng(71)
    rec, snd = [], []
    for r, deg in enumerate(DEGREES + (BEYOND,)):
        rec.append(np.full(deg, r, dtype=np.int64))
        snd.append(rng.choice(SENDERS, size=deg, replace=False).astype(np.int64))
    return np.concatenate(rec), np.concatenate(snd)


@functools.lru_cache(maxsize=None)
def graph_case(beyond):
    from fsw_gnn_amd import _lib, build_csr
    degrees = DEGREES + ((BEYOND,) if beyond else ())
    rec, snd = edges()
    nnz = sum(degrees)
    graph = build_csr(t(rec[:nnz], torch.int64), t(snd[:nnz], torch.int64), None, len(degrees), SENDERS)
    st = graph.read_stats()
    rowptr = graph.rowptr.cpu().numpy().astype(np.int64)
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_NNZ] == nnz and tuple(np.diff(rowptr)) == degrees
    assert st[_lib.STAT_MAX_DEGREE] == max(degrees)
    hub0 = _lib.BIN_MID0 + len(_lib.MID_SIZES) + _lib.NUM_LDS_BINS
    assert np.diff(graph.bin_start_host[0])[hub0:].tolist() == [3, 2, 2, 2, 1 if beyond else 0]
    col = graph.col[:nnz].cpu().numpy().astype(np.int64)
    assert np.array_equal(col, snd[:nnz])                          # the rows keep the order of the edge list
    return {"graph": graph, "st": st, "rowptr": rowptr, "col": col, "nnz": nnz, "degrees": degrees}


@functools.lru_cache(maxsize=None)
def inputs(S, F, freqs=FREQS):
    """Xp [SENDERS, round_up(S, 32)] float32, frequencies freqs[:F], bias, output gradient (for the graph with the row of BEYOND)."""
    rng = np.random.default_rng(72 + S)
    ldp = (S + 31) // 32 * 32
    Xp = rng.standard_normal((SENDERS, ldp)).astype(np.float32)
    pairs = rng.permutation(SENDERS)[:2 * TIED_PAIRS].reshape(2, TIED_PAIRS)
    Xp[pairs[1]] = Xp[pairs[0]]                                    # exactly tied keys in every column ...
    kinds = COLUMN_KINDS[:S]
    for c, kind in enumerate(kinds):
        if kind == "a":
            Xp[:, c] = 0.75
        elif kind == "e":                                           # ... but the control column: distinct, exact in float32
            Xp[:, c] = (rng.permutation(SENDERS).astype(np.float32) - 16500.0) / 4096.0
    assert np.unique(Xp[:, kinds.index("e")]).size == SENDERS and np.array_equal(Xp[pairs[0], 0], Xp[pairs[1], 0])
    fr = np.array(freqs[:F], dtype=np.float32)
    width = HAS_MASS + S * F
    bias = (0.1 * rng.standard_normal(width)).astype(np.float32)
    g = rng.standard_normal((len(DEGREES) + 1, width)).astype(np.float32)
    for a in (Xp, fr, bias, g):
        a.setflags(write=False)
    return {"Xp": Xp, "fr": fr, "bias": bias, "g": g, "kinds": kinds, "ldp": ldp}


@functools.lru_cache(maxsize=None)
def forward_reference(S, F, freqs=FREQS):
    """The float64 oracle through the diagonal identity, on the graph with the row of BEYOND (its first rows are the other graph's):
    [rows, HAS_MASS + S F] with bias and out_scale."""
    c, x = graph_case(True), inputs(S, F, freqs)
    X = x["Xp"][:, :S].astype(np.float64)
    V = np.repeat(np.eye(S), F, axis=0)
    emb, mass = O.fsw_embed_csr(X, c["rowptr"], c["col"], np.ones(c["nnz"]), V, np.tile(x["fr"].astype(np.float64), S), return_mass=True)
    ref = OUT_SCALE * (np.concatenate([mass[:, None], emb], axis=1) + x["bias"].astype(np.float64)[None, :])
    ref.setflags(write=False)
    return ref


def cart_args(c, x, S, F, Xp, fr, table, scratch, dtype=0):
    from fsw_gnn_amd import _lib
    graph = c["graph"]
    a = _lib.CartArgs()
    a.value_dtype, a.S, a.F, a.has_mass = dtype, S, F, HAS_MASS
    a.rowptr, a.col, a.w = graph.rowptr.data_ptr(), graph.col.data_ptr(), None
    a.perm, a.bin_start, a.bin_start_host = graph.perm.data_ptr(), graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data
    a.num_rows, a.max_degree = len(c["degrees"]), c["st"][_lib.STAT_MAX_DEGREE]
    a.Xp, a.ldp, a.freqs, a.tau, a.out_scale = Xp.data_ptr(), Xp.stride(0), fr.data_ptr(), 1.0, OUT_SCALE
    a.mass_fn, a.mass_scale = 0, 1.0
    if table is not None:
        a.unit_table, a.ldt = table.data_ptr(), F
    if scratch is not None:
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    return a


def unit_tables(fr, F, stream):
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    table = torch.empty((int(L.fsw_unit_table_rows(_lib.REG_MAX_DEG)), F), device=DEV)
    dtable = torch.empty_like(table)
    _lib.check(L.fsw_unit_coeff_table(_lib.ptr(fr), F, _lib.REG_MAX_DEG, _lib.ptr(table), F, stream), "fsw_unit_coeff_table")
    _lib.check(L.fsw_unit_dcoeff_table(_lib.ptr(fr), F, _lib.REG_MAX_DEG, _lib.ptr(dtable), F, stream), "fsw_unit_dcoeff_table")
    return table, dtable


def run_forward(c, S, F, scratch, freqs=FREQS):
    """(status, out) of fsw_embed_cart_f32; out pre-filled with NaN."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    x = inputs(S, F, freqs)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    Xp, fr, bias = t(x["Xp"]), t(x["fr"]), t(x["bias"])
    table, _ = unit_tables(fr, F, stream)
    out = torch.full((len(c["degrees"]), HAS_MASS + S * F), float("nan"), device=DEV)
    a = cart_args(c, x, S, F, Xp, fr, table, scratch)
    a.out, a.ldo, a.bias = out.data_ptr(), out.stride(0), bias.data_ptr()
    rc = L.fsw_embed_cart_f32(ctypes.byref(a), stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().astype(np.float64)


def check_rows(got, ref, degrees, what):
    """Per row: the S F embedding columns norm-wise <= TOL, and the mass column on its own (D * out_scale would hide the rest)."""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    errs = np.array([relerr(got[r, HAS_MASS:], ref[r, HAS_MASS:]) for r in range(len(degrees))])
    mass = np.abs(got[:, 0] - ref[:, 0]) / np.maximum(np.abs(ref[:, 0]), 1e-300)
    print("%s: forward per row max %.2e (D = %d), mass column max %.2e" % (what, errs.max(), degrees[errs.argmax()], mass.max()))
    print("   per row D: " + "  ".join("%d: %.1e" % (d, e) for d, e in zip(degrees, errs)))
    assert errs.max() <= TOL, (what, dict(zip(degrees, errs.tolist())))
    assert mass.max() <= TOL, (what, dict(zip(degrees, mass.tolist())))


@pytest.mark.parametrize("S,F", SHAPES)
def test_forward_without_scratch(S, F):
    """fsw_embed_cart_f32 with scratch = NULL on rows of up to 32768 neighbours: status 0, every row (mass column included) within TOL
    of the float64 oracle."""
    c = graph_case(False)
    rc, out = run_forward(c, S, F, None)
    from fsw_gnn_amd import _lib
    assert rc == 0, _lib.lib().fsw_last_error().decode()
    check_rows(out, forward_reference(S, F)[:len(DEGREES)], DEGREES, "hub forward S %d F %d, no scratch" % (S, F))


def test_boundary_row_stays_on_the_generic_kernel():
    """One row of 32769 neighbours: with scratch the call succeeds and the row matches; without scratch the call is refused."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    S, F = SHAPES[0]
    c = graph_case(True)
    scratch = torch.empty(int(L.fsw_embed_cart_generic_scratch_bytes(BEYOND, 1)), dtype=torch.uint8, device=DEV)
    rc, out = run_forward(c, S, F, scratch)
    assert rc == 0, L.fsw_last_error().decode()
    check_rows(out, forward_reference(S, F), c["degrees"], "hub forward with a row of %d" % BEYOND)
    rc, _ = run_forward(c, S, F, None)
    assert rc != 0


@pytest.mark.parametrize("S,F", SHAPES)
def test_backward(S, F):
    """fsw_embed_cart_backward_keys_f32 with the scratch of fsw_embed_cart_backward_scratch_bytes and with the smallest scratch that
    was valid before (fsw_embed_cart_generic_scratch_bytes(max_degree, 1)): bit-identical gkey; against the generic kernel with
    float64 storage per row <= F32_BOUND, per entry <= PER_ENTRY of the line maximum, gfreq <= F32_BOUND."""
    check_backward(S, F)


def check_backward(S, F, freqs=FREQS):
    """The body of test_backward at the frequencies freqs[:F]."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    c, x = graph_case(False), inputs(S, F, freqs)
    nnz, nrows, rowptr = c["nnz"], len(DEGREES), c["rowptr"]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    g_host = x["g"][:nrows]

    # reference: the generic kernel, float64 storage, backward mode
    Xp64, fr64, g64 = t(x["Xp"], torch.float64), t(x["fr"], torch.float64), t(g_host, torch.float64)
    gkey_ref = torch.full((nnz, S), float("nan"), dtype=torch.float64, device=DEV)
    gf_ref = torch.zeros(F, dtype=torch.float64, device=DEV)
    gscratch = torch.empty(int(L.fsw_embed_cart_generic_scratch_bytes(max(DEGREES), nrows)), dtype=torch.uint8, device=DEV)
    a = cart_args(c, x, S, F, Xp64, fr64, None, gscratch, dtype=1)
    a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g64.data_ptr(), g64.stride(0), gkey_ref.data_ptr(), S, gf_ref.data_ptr()
    _lib.check(L.fsw_embed_cart_generic(ctypes.byref(a), stream), "fsw_embed_cart_generic (backward, float64)")

    Xp, fr, g = t(x["Xp"]), t(x["fr"]), t(g_host)
    table, dtable = unit_tables(fr, F, stream)
    sizes = {"new size function": int(L.fsw_embed_cart_backward_scratch_bytes(max(DEGREES), 9, S)),
             "smallest valid before": int(L.fsw_embed_cart_generic_scratch_bytes(max(DEGREES), 1))}
    assert sizes["new size function"] >= 12 * 32768 and sizes["smallest valid before"] >= 12 * 32768
    got = {}
    for name, nbytes in sizes.items():
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        gkey = torch.full((nnz, S), float("nan"), device=DEV)
        gf = torch.zeros(F, device=DEV)
        a = cart_args(c, x, S, F, Xp, fr, table, scratch)
        a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g.data_ptr(), g.stride(0), gkey.data_ptr(), S, gf.data_ptr()
        _lib.check(L.fsw_embed_cart_backward_keys_f32(ctypes.byref(a), _lib.ptr(dtable), F, stream), "fsw_embed_cart_backward_keys_f32")
        torch.cuda.synchronize()
        got[name] = (gkey.cpu().numpy(), gf.cpu().numpy())
    (k_new, f_new), (k_old, f_old) = got["new size function"], got["smallest valid before"]
    assert np.isfinite(k_new).all() and np.array_equal(k_new, k_old)

    ref = gkey_ref.cpu().numpy()
    assert np.isfinite(ref).all()
    G = OUT_SCALE * g_host[:, HAS_MASS:].astype(np.float64)
    scale = coefficient_scale(G, np.tile(x["fr"].astype(np.float64), S)).reshape(nrows, S, F).sum(axis=2)
    what = "hub backward S %d F %d" % (S, F)
    check_key_gradients(k_new.astype(np.float64), ref, rowptr, list(x["kinds"]), what, scale, row_bound=F32_BOUND, entry_bound=PER_ENTRY)
    for name, gf in (("new size function", f_new), ("smallest valid before", f_old)):
        e = relerr(gf, gf_ref.cpu().numpy())
        print("%s, %s: gfreq %.2e" % (what, name, e))
        assert e <= F32_BOUND, (what, name, e)


# ---- module level -------------------------------------------------------------------------------------------------------------------
def test_embedding_module_on_the_fixture_graph():
    """FSW_embedding float32 on the unit_bias case of tests/golden/grads_cartesian_graph.npz (rows of 2049 and 4500 neighbours), on the
    unit-weight CSR graph (no weight tensor: what FSW_readout and a default FSW_conv build), through _CartEmbedFn: output and all
    gradients against the stored float64 reference values <= F32_BOUND; the forward allocates no scratch."""
    from fsw_gnn_amd import build_csr
    from tests.test_hip_cartesian_train import assert_close, autograd_functions, graph_cases, make_module
    gr, cases = graph_cases()
    c = cases["unit_bias"]
    assert bool(c["unit"]) and not bool(c["mass"])
    E = make_module(c, torch.float32)
    X = torch.from_numpy(gr["X"]).float().to(DEV).contiguous()
    graph = build_csr(torch.from_numpy(gr["rows"]).long().to(DEV), torch.from_numpy(gr["cols"]).long().to(DEV), None, 12, X.shape[0])
    deg = np.diff(graph.rowptr.cpu().numpy())
    assert 2049 in deg and 4500 in deg and deg.max() == 4500 and graph.w is None
    assert E.prepare_cartesian(X, graph)["scratch"] is None
    Xl = X.clone().requires_grad_(True)
    out = E.embed_cartesian_autograd(Xl, graph)
    assert "_CartEmbedFnBackward" in autograd_functions(out)
    (out * torch.from_numpy(c["G"]).to(DEV).to(out.dtype)).sum().backward()
    got = {"out": out.detach(), "gX": Xl.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad, "gbias": E.bias.grad.reshape(-1)}
    got = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in got.items()}
    want = {k: c[k] for k in ("out", "gX", "gV", "gfreqs", "gbias")}
    assert_close(got, want, F32_BOUND, "float32 module (unit-weight graph) vs reference, unit_bias")


def test_readout_on_graphs_with_hub_rows():
    """FSW_readout(embed_slices=4, embed_freqs=8) on a batch of graphs of 40, 2500 and 5000 vertices: float32 against the float64 layer
    with the same state, forward and gradients at the bounds of tests/test_hip_cartesian_conv.py."""
    from fsw_gnn_amd import FSW_readout
    from tests.test_hip_cartesian_conv import F32_BOUND as CONV_F32, FWD_BOUND, _loss_grads, features, make_pair
    from tests.test_hip_cartesian_conv import relerr as rel
    S, F, in_ch, out_ch = 4, 8, 6, 8
    sizes = {0: 40, 1: 2500, 2: 5000}
    gi = torch.cat([torch.full((m,), g, dtype=torch.int64) for g, m in sizes.items()])
    gi = gi[torch.randperm(gi.numel(), generator=torch.Generator().manual_seed(6))].to(DEV)
    n = gi.numel()
    ref, low = make_pair(FSW_readout, in_ch, out_ch, S, F, concat_self=False, mlp_layers=2, learnable_vertex_degree_encoding_scale=True)
    x64, G = features(n, in_ch), features(3, out_ch, seed=36)
    want_y, want = _loss_grads(ref, x64, G, gi, 3)
    got_y, got = _loss_grads(low, x64.float(), G, gi, 3)
    with torch.no_grad():
        inference = low(x64.float(), gi, 3)
    assert set(got) == set(want)
    errs = {"out": rel(got_y, want_y), "inference": rel(inference, want_y), **{k: rel(got[k], want[k]) for k in want}}
    print("readout with hub rows, float32 vs float64:", errs)
    assert errs.pop("out") < FWD_BOUND and errs.pop("inference") < FWD_BOUND
    assert max(errs.values()) < CONV_F32, errs
