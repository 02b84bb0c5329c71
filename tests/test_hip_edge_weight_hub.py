"""The weight gradient of rows above 1024 neighbours on csrc/embed_w_long_bwd.hip, on the GPU.  The yardstick is
tests/weight_grad_ref.py (autograd of a plain float64 forward) everywhere, never the generic kernel and never the kernel under test.

Kernel level: fsw_embed_backward_w_f32 / fsw_embed_backward_w_lo_f32 through ctypes on the hand-made CSR of
tests/edge_weight_hub_cases.py (graph.import_csr keeps the entries in place): one recipient per degree 0, 1024, 1025, 2047, 2048, 2049,
4095, 4096, 4097, 6001, 8192, 8193, 16384, 16385, 32768, 32769 -- both sides of the hand-over from the wave-sort class, D + 1 at one
chunk, two chunks and every power of two (every merge level), both sides of every bin edge up to the first row of FSW_BIN_GLOBAL, a
partly filled last chunk; keys exact in float32, distinct or tied on the grid of 1/8 with the pad key; weights from {0, 1/4, 1/2, 1},
rows of mass below tau (many exact zero weights), tau exactly and above, tau 1 and 3; out_scale 0.7, a mass column in g, scattered
zero readouts and one zero row (4096 neighbours); S = 3 (less than one task's G = 4 slices), 8, 70 (18 tasks per row, the last of
two slices).

(1) test_kernel_weight_gradients: every degree, into a zeroed gw and into a gw pre-filled with 0.5.
      gw per entry  <= 2 [G64_ROW (row max |gW|) + (A + 2) 2^-24 sum_s |gW_s[j]| + (S + 1) 2^-24 |fill|]
                    (edge_weight_long_cases.gw_bound) with A = ceil(S / G) float32 adds above 1024 neighbours, G read from the
                    library; the row of 1024: min(4, ceil(S / 4)).  The arithmetic before the add is float64.
      the zero row  adds exactly nothing (also to the fill); no entry is left out of the comparison;
      gkey / gfreq  the bounds of test_hip_edge_weight.check_keys_and_freqs (F32_BOUND norm-wise, PER_ENTRY of the line maximum), on
                    this file's rows.
(2) test_w_lo_on_hub_rows: fsw_embed_backward_w_lo_f32 with the w_lo of the cases on every row; the reference is computed on
    w + w_lo in float64, the bound is that of (1).  Fails on the parent commit: its generic kernel reads w alone above 1024
    neighbours, and tests/test_edge_weight_hub_cpu.py shows that this misses the bound on every such row.
(3) test_one_wave_of_scratch: scratch_bytes = 20 * 65536, exactly one wavefront's line of the largest bin, S = 8: every line of that
    bin runs in sequence on one wavefront; the call returns 0 and meets the bounds of (1).  With one byte less it returns a non-zero
    status before anything is launched and leaves gw untouched.
(4) test_layer_learnable_edge_weights_hub_rows: a float32 FSW_conv with edge_weight.requires_grad against its float64 twin as
    test_hip_edge_weight.run_training_case does, at the module-level bounds (output 1e-5 per row; gx, parameters and g edge_weight
    per recipient 2e-5).  4400 vertices: vertex 0 a recipient of 4200 distinct senders, vertex 1 of 1500, the rest 25 .. 64, 200
    parallel edges on top; S = 9 and 70, unit scheme and self_loop_weight 0.5 with 'gcn'.  Keys exact in float32, as in
    tests/test_hip_edge_weight_long.py (4): x on the grid of 1/8 in [-4, 4], slice vectors rounded to the grid of 1/64.

Measured on an MI355X:
    (1) gw per entry err / bound, largest over tau 1 and 3, distinct and tied keys: S = 3: 0.21, S = 8: 0.26, S = 70: 0.06;
        pre-filled with 0.5: 0.28, 0.25, 0.08; err / row maximum 7.2e-8 (S = 3) .. 1.9e-6 (S = 70).
        per degree, tau 1, distinct keys, S = 70:  1024: 0.06 (wave-sort class) | 1025: 0.02  2047: 0.02  2048: 0.01  2049: 0.02
        4095: 0.02  (4096: the zero row)  4097: 0.02  6001: 0.02  8192: 0.02  8193: 0.01  16384: 0.03  16385: 0.02  32768: 0.02
        32769: 0.03;      S = 3, same case: 0.20 .. 0.21 on every row above 1024, 0.16 on the row of 1024.
        gkey per row 9.0e-8, per entry 1.6e-7 of the line maximum, gfreq 1.9e-7 (all cases of (1) - (3)).
    (2) err / bound 0.21 / 0.26 / 0.06 for S = 3 / 8 / 70.      (3) 0.26 (every degree 0.11 .. 0.26).
    (4) unit S 9 / S 70: out per row 3.3e-7 / 4.8e-7, gx 7.7e-7 / 7.7e-7, g edge_weight per recipient 3.4e-7 / 1.9e-7 (the hubs of
        4200 and 1500: 2.9e-8, 3.2e-8 / 1.1e-7, 9.8e-8); gcn_loops S 9 / S 70: out 1.7e-6 / 5.0e-7, gx 6.2e-7 / 1.0e-6, g edge_weight
        1.8e-7 / 2.3e-7 (the hubs: 6.7e-8, 7.2e-8 / 1.1e-7, 1.0e-7); parameters <= 3.0e-6.
    The whole file: 32 tests in 12.6 s, of which the float64 references on the CPU (computed once per (tau, keys, w_lo)) take half.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import edge_weight_hub_cases as HC
from tests import test_hip_edge_weight as T
from tests.conftest import relerr
from tests.test_hip_ties import F32_BOUND, PER_ENTRY, dev, line_maxima, per_row, t  # noqa: F401
from tests.weight_grad_ref import per_entry_ratio, row_maxima

pytestmark = pytest.mark.gpu
OUT_SCALE, HAS_MASS, FILL = 0.7, 1, 0.5
ONE_LINE = HC.BYTES_PER_ELEM * HC.pow2ceil(max(HC.DEGREES) + 1)


@pytest.fixture(scope="module", autouse=True)
def release_the_cached_cases():
    """The inputs and references of this module (some 200 MB of float64 arrays) are not kept for the rest of the session."""
    yield
    HC.base_reference.cache_clear()
    HC.kernel_inputs.cache_clear()


def run_kernel(dev, tau, tied, S, fill=0.0, lo=False, nbytes=None, expect_ok=True):
    """One launch on every recipient: {"gw" [nnz], "gkey" [nnz, S], "gfreq" [S]} as float64 numpy arrays and the status "rc".
    nbytes: the scratch size (None: the library's query)."""
    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.graph import import_csr
    L = _lib.lib()
    k = HC.kernel_inputs(tau, tied)
    Xp_h, fr_h, G_h = HC.expand(k, S)
    nrows, nnz, maxdeg = len(HC.DEGREES), k["w"].size, max(HC.DEGREES)
    stream = torch.cuda.current_stream(dev).cuda_stream
    graph = import_csr(t(k["rowptr"], dev, torch.int32), t(k["col"], dev, torch.int32), t(k["w"], dev), nrows, nnz)
    st = graph.read_stats()
    assert not (st[_lib.STAT_FLAGS] & ~_lib.FLAG_W_NONUNIT) and st[_lib.STAT_NNZ] == nnz and st[_lib.STAT_MAX_DEGREE] == maxdeg
    assert np.array_equal(graph.col[:nnz].cpu().numpy(), k["col"]) and np.array_equal(graph.w[:nnz].cpu().numpy(), k["w"])
    Xp, fr, g = t(Xp_h, dev), t(fr_h, dev), t(G_h, dev)
    a = _lib.EmbedArgs()
    a.rowptr, a.col, a.w, a.perm = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.w.data_ptr(), graph.perm.data_ptr()
    a.bin_start, a.bin_start_host, a.num_rows = graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data, nrows
    a.Xp, a.ldp, a.freqs, a.S, a.tau = Xp.data_ptr(), Xp.stride(0), fr.data_ptr(), S, tau
    a.out_scale, a.has_mass, a.mass_fn, a.mass_scale = OUT_SCALE, HAS_MASS, 0, 1.0
    a.num_reg_rows, a.num_lds_rows = st[_lib.STAT_NUM_REG], st[_lib.STAT_NUM_LDS]
    a.num_global_rows, a.num_zero_rows, a.max_degree = st[_lib.STAT_NUM_GLOBAL], st[_lib.STAT_NUM_ZERO], maxdeg
    if nbytes is None:
        nbytes = int(L.fsw_embed_backward_w_scratch_bytes(maxdeg, nrows))
    assert nbytes >= ONE_LINE - 1
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    gkey = torch.full((nnz, S), float("nan"), device=dev)
    gf = torch.zeros(S, device=dev)
    gw = torch.full((nnz,), fill, device=dev)
    w_lo = t(k["w_lo"], dev) if lo else None
    rc = L.fsw_embed_backward_w_lo_f32(ctypes.byref(a), _lib.ptr(w_lo), maxdeg, _lib.ptr(g), g.stride(0), _lib.ptr(gkey), S, _lib.ptr(gf),
                                       _lib.ptr(gw), _lib.ptr(buf), nbytes, stream)
    assert (rc == 0) == expect_ok, (rc, L.fsw_last_error())
    torch.cuda.synchronize()
    res = {name: v.cpu().numpy().astype(np.float64) for name, v in (("gw", gw), ("gkey", gkey), ("gfreq", gf))}
    res["rc"] = rc
    return res


def check_gw(got, ref, S, what, fill=0.0):
    """(1) of the module docstring: every entry is compared."""
    k = HC.kernel_inputs(1.0, False)
    rowptr, deg = k["rowptr"], k["degrees"]
    got = got - fill
    assert got.shape == ref["gW"].shape == (k["w"].size,) and np.isfinite(got).all(), what
    adds = np.repeat([HC.float32_adds(int(d), S) for d in deg], deg)
    bound = HC.gw_bound(ref, rowptr, S, adds, fill)
    err = np.abs(got - ref["gW"])
    zero = row_maxima(ref["gW"], rowptr) == 0                 # the row whose output gradient is zero: the kernel adds nothing
    assert zero[rowptr[HC.ZERO_ROW]:rowptr[HC.ZERO_ROW + 1]].all() and zero.sum() == HC.DEGREES[HC.ZERO_ROW] and not got[zero].any(), what
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    cls = per_row(lambda a, b: ratio[a:b].max(), rowptr)
    rel = per_entry_ratio(got, ref["gW"], rowptr)
    print("%s: gw per entry err / bound %.2f, err / row maximum %.2e" % (what, ratio.max(), rel.max()))
    print("   per degree err / bound:  " + "  ".join("%d: %.2f" % (d, c) for d, c in zip(deg, cls) if d))
    worst = int(ratio.argmax())
    rowdeg = np.repeat(deg, deg)
    assert ratio.max() <= 1.0, (what, "entry %d (row of %d)" % (worst, rowdeg[worst]), float(ratio.max()), float(got[worst]),
                                float(ref["gW"][worst]))


def check_keys_and_freqs(res, ref, what):
    """test_hip_edge_weight.check_keys_and_freqs on this file's rows (float32 storage)."""
    k = HC.kernel_inputs(1.0, False)
    rowptr, deg = k["rowptr"], k["degrees"]
    got = res["gkey"]
    assert got.shape == ref["gkey"].shape and np.isfinite(got).all(), what
    rows = per_row(lambda a, b: relerr(got[a:b], ref["gkey"][a:b]), rowptr)
    lm = np.maximum(line_maxima(ref["gkey"], rowptr), 1e-6 * np.repeat(ref["scale"], deg, axis=0))
    assert not got[lm == 0].any(), what
    ratio = np.abs(got - ref["gkey"]) / np.where(lm > 0, lm, 1.0)
    egf = relerr(res["gfreq"], ref["gfreq"])
    print("%s: gkey per row %.2e, per entry / line maximum %.2e, gfreq %.2e" % (what, rows.max(), ratio.max(), egf))
    assert rows.max() <= F32_BOUND, (what, dict(zip(deg.tolist(), rows.tolist())))
    assert ratio.max() <= PER_ENTRY, (what, float(ratio.max()))
    assert egf <= F32_BOUND, (what, egf)


@pytest.mark.parametrize("S", HC.S_VALUES)
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_kernel_weight_gradients(dev, tau, tied, S):
    """(1) of the module docstring."""
    ref = HC.reference(tau, tied, OUT_SCALE, S)
    what = "tau %g %s S %d" % (tau, "tied" if tied else "distinct", S)
    res = run_kernel(dev, tau, tied, S)
    check_gw(res["gw"], ref, S, what)
    check_keys_and_freqs(res, ref, what)
    filled = run_kernel(dev, tau, tied, S, fill=FILL)
    check_gw(filled["gw"], ref, S, what + " pre-filled", fill=FILL)
    assert np.array_equal(filled["gkey"], res["gkey"]), what


@pytest.mark.parametrize("S", HC.S_VALUES)
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_w_lo_on_hub_rows(dev, tau, tied, S):
    """(2) of the module docstring; fails on the parent commit (its rows above 1024 neighbours read w alone)."""
    ref = HC.reference(tau, tied, OUT_SCALE, S, lo=True)
    what = "w_lo, tau %g %s S %d" % (tau, "tied" if tied else "distinct", S)
    res = run_kernel(dev, tau, tied, S, lo=True)
    check_gw(res["gw"], ref, S, what)
    check_keys_and_freqs(res, ref, what)


@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_one_wave_of_scratch(dev, tau, tied):
    """(3) of the module docstring."""
    S = 8
    ref = HC.reference(tau, tied, OUT_SCALE, S)
    what = "one line of scratch, tau %g %s S %d" % (tau, "tied" if tied else "distinct", S)
    res = run_kernel(dev, tau, tied, S, nbytes=ONE_LINE)
    check_gw(res["gw"], ref, S, what)
    check_keys_and_freqs(res, ref, what)
    from fsw_gnn_amd import _lib
    refused = run_kernel(dev, tau, tied, S, fill=FILL, nbytes=ONE_LINE - 1, expect_ok=False)   # refused on the host: no launch
    assert refused["rc"] != 0 and b"scratch" in _lib.lib().fsw_last_error()
    assert (refused["gw"] == FILL).all() and not refused["gfreq"].any() and np.isnan(refused["gkey"]).all()


# ---- (4) layer level ------------------------------------------------------------------------------------------------------------------
N_VERT, HUB_DEG, SECOND_DEG = 4400, 4200, 1500


def layer_graph():
    """(edge_index [2, E] int64, weights [E] float64 exact in float32): module docstring (4); weights in [0.05, 1): rows below and
    above tau = 1."""
    rng = np.random.default_rng(6300)
    deg = np.concatenate([[HUB_DEG, SECOND_DEG], rng.integers(25, 65, size=N_VERT - 2)])
    dst = np.repeat(np.arange(N_VERT), deg)
    src = np.concatenate([rng.permutation(N_VERT)[:d] for d in deg])              # distinct senders per recipient
    dup = rng.integers(0, dst.size, size=200)
    dst, src = np.concatenate([dst, dst[dup]]), np.concatenate([src, src[dup]])
    order = rng.permutation(dst.size)
    w = rng.uniform(0.05, 1.0, dst.size)
    return np.stack([src[order], dst[order]]).astype(np.int64), w.astype(np.float32).astype(np.float64)


def run_hub_training_case(dev, what, **kw):
    """test_hip_edge_weight.run_training_case on layer_graph()."""
    conv, twin = T.make_pair(dev, torch.float32, **kw)
    with torch.no_grad():                                 # keys exact in float32: tests/test_hip_edge_weight_long.py (4)
        V = torch.round(conv.fsw_embed.projVecs * 64.0) / 64.0
        conv.fsw_embed.projVecs.copy_(V)
        twin.fsw_embed.projVecs.copy_(V.double())
    ei_h, w_h = layer_graph()
    coalesced = np.unique(ei_h[1] * N_VERT + ei_h[0]) // N_VERT
    indeg = np.bincount(coalesced, minlength=N_VERT)      # rows of the coalesced adjacency
    assert indeg[0] == HUB_DEG and indeg[1] == SECOND_DEG and 25 <= indeg[2:].min() and indeg[2:].max() <= 64
    rng = np.random.default_rng(6400)
    x_h = (np.round(np.clip(rng.standard_normal((N_VERT, 6)), -4, 4) * 8.0) / 8.0).astype(np.float32)
    r_h = rng.standard_normal((N_VERT, 5)).astype(np.float32)
    ei = torch.from_numpy(ei_h).to(dev)
    x64, w64 = t(x_h, dev, torch.float64).requires_grad_(True), t(w_h, dev, torch.float64).requires_grad_(True)
    x, w = t(x_h, dev).requires_grad_(True), t(w_h, dev).requires_grad_(True)
    ref = T.anchor_forward(twin, x64, ei, w64)
    (ref * t(r_h, dev, torch.float64)).sum().backward()
    out = conv(x, ei, edge_weight=w)
    (out * t(r_h, dev)).sum().backward()
    assert w.grad is not None and tuple(w.grad.shape) == tuple(w.shape) and bool(torch.isfinite(w.grad).all())
    e_out, e_x = T.rows_err(out, ref), T.rows_err(x.grad, x64.grad)
    got, want = w.grad.detach().cpu().numpy().astype(np.float64), w64.grad.detach().cpu().numpy()
    order = np.argsort(ei_h[1], kind="stable")
    cuts = np.concatenate([[0], np.cumsum(np.bincount(ei_h[1], minlength=N_VERT))])
    e_w = np.array([relerr(got[order[a:b]], want[order[a:b]]) if b > a else 0.0 for a, b in zip(cuts[:-1], cuts[1:])])
    e_p = {name: relerr(p.grad.cpu().numpy().astype(np.float64), dict(twin.named_parameters())[name].grad.cpu().numpy())
           for name, p in conv.named_parameters() if p.grad is not None}
    print("%s: out per row %.2e, gx per row %.2e, g edge_weight per recipient %.2e (in-degree %d; the hubs: %.2e, %.2e), parameters %s" % (
        what, e_out.max(), e_x.max(), e_w.max(), indeg[e_w.argmax()], e_w[0], e_w[1], "  ".join("%s %.1e" % kv for kv in sorted(e_p.items()))))
    assert {"fsw_embed.projVecs", "fsw_embed.freqs", "mlp.0.weight"} <= set(e_p)
    assert e_out.max() <= T.F32_FWD, (what, int(e_out.argmax()), float(e_out.max()))
    assert e_x.max() <= T.F32_GRAD, (what, int(e_x.argmax()), float(e_x.max()))
    assert e_w.max() <= T.F32_GRAD, (what, int(e_w.argmax()), int(indeg[e_w.argmax()]), float(e_w.max()))
    assert max(e_p.values()) <= T.F32_GRAD, (what, e_p)


@pytest.mark.parametrize("embed_dim", [10, 71], ids=["S9", "S70"])
@pytest.mark.parametrize("scheme", ["unit", "gcn_loops"])
def test_layer_learnable_edge_weights_hub_rows(dev, scheme, embed_dim):
    """(4) of the module docstring."""
    kw = dict(self_loop_weight=0.5, edge_weighting='gcn') if scheme == "gcn_loops" else {}
    run_hub_training_case(dev, "hub rows, %s S %d" % (scheme, embed_dim - 1), embed_dim=embed_dim, **kw)
