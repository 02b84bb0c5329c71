"""The weight gradient of rows of 25 .. 1024 neighbours on csrc/embed_w_sort_bwd.hip, on the GPU.  The yardstick is
tests/weight_grad_ref.py (autograd of a plain float64 forward) everywhere, never the generic kernel and never the kernel under test.

Kernel level: fsw_embed_backward_w_f32 / fsw_embed_backward_w_lo_f32 through ctypes on the hand-made CSR of
tests/edge_weight_long_cases.py (graph.import_csr keeps the entries in place): one recipient per degree 0, 24, 25, .. 2049 at both
sides of the register class, of every instance's first and last bin, of D + 1 crossing 64 M and of the hand-over to the generic
kernel at 1024 | 1025; keys exact in float32, distinct or tied on the grid of 1/8 with the pad key; weights from {0, 1/4, 1/2, 1},
rows of mass below tau (many exact zero weights), tau exactly and above, tau 1 and 3; out_scale 0.7, a mass column in g, scattered
zero readouts and one zero row (257 neighbours); S = 3 (fewer slices than wavefronts), 8, 70 (18 slice groups on 4 y-blocks for the
rows of 513 .. 1024: one workgroup accumulates over several groups).

(1) test_kernel_weight_gradients: every degree, into a zeroed gw and into a gw pre-filled with 0.5.
      gw per entry  <= 2 [G64_ROW (row max |gW|) + (A + 2) 2^-24 sum_s |gW_s[j]| + (S + 1) 2^-24 |fill|].  A, the float32 adds an
                    entry receives (edge_weight_long_cases.float32_adds): register rows (24) ceil(S / 64); rows of 25 .. 1024 one
                    per workgroup that visits the row, gridDim.y = min(4, ceil(S / SC)) with SC = 48 / 24 / 12 / 4 slices per group
                    for rows of up to 192 / 256 / 512 / 1024 neighbours -- A = 1 for S = 3, 1 | 1 | 1 | 2 for S = 8, 2 | 3 | 4 | 4 for
                    S = 70; rows above 1024 (the generic kernel) A = S.  The arithmetic before the add is float64.
      the zero row  adds exactly nothing (also to the fill); no entry is left out of the comparison;
      gkey / gfreq  the bounds of test_hip_edge_weight.check_keys_and_freqs (F32_BOUND norm-wise, PER_ENTRY of the line maximum).
(2) test_no_scratch_inside_the_class: the recipients of at most 300 neighbours, scratch = NULL, scratch_bytes = 0: the call returns 0
    and meets the bounds of (1); fsw_embed_backward_w_tuned_max_degree() >= 1024.  (The parent refuses: "need scratch".)
(3) test_w_lo_on_long_rows: fsw_embed_backward_w_lo_f32 with the w_lo of the cases (multiples of 2^-12, |w_lo| <= 2^-6, w + w_lo >= 0
    exact in float64, cancelling in pairs on the rows of mass tau exactly); the reference is computed on w + w_lo in float64, the
    bound is that of (1).  The recipients above the class limit of 1024 run on the generic kernel, which reads w alone: they are
    excluded from this test only (the launch is made on the recipients of at most 1024 neighbours).
    tests/test_edge_weight_long_cpu.py shows that dropping w_lo misses this bound on every row above 24 neighbours.
(4) test_layer_learnable_edge_weights_long_rows: a float32 FSW_conv with edge_weight.requires_grad against its float64 twin as
    test_hip_edge_weight.run_training_case does, at the module-level bounds (output 1e-5 per row; gx, parameters and g edge_weight
    per recipient 2e-5).  2100 vertices: vertex 0 a recipient of 2048 distinct senders (the layer coalesces parallel edges, so a
    row of 2048 entries needs that many vertices), vertex 1 without in-edges, 300 vertices of in-degree 25 .. 600, the rest 25 .. 64,
    200 parallel edges on top (every recipient but vertex 1 is a row of the new class or, the hub, of the generic kernel); S = 9 and 70, unit scheme and self_loop_weight 0.5 with 'gcn'.
    The keys are exact in float32, as at the kernel level: x on the grid of 1/8 in [-4, 4] and the slice vectors rounded to the grid
    of 1/64 (a key is a sum of six products of 13 significant bits).  The key gradient is piecewise constant in the ranks, so on
    rounded keys every pair of neighbours in rank that float32 orders differently from float64 exchanges two coefficients: with
    random keys this graph (the sum of D^2 S over its rows is 3e9) has more than a hundred such pairs at S = 70, and the first run
    of this test showed gx off by 5.4e-3 on one sender while g edge_weight, which is continuous in the keys, stood at 5.3e-6.  With
    exact keys the float32-keys-only estimate of the error is zero.
    Recipients of one or two neighbours are left to tests/test_hip_edge_weight.py (the register kernels): a first version of this graph
    gave the vertices that only serve as the hub's senders 1 .. 9 in-edges, and under 'gcn' at S = 70 one recipient of a single
    in-edge from a sender of high degree stood at 2.3e-5 against the 2e-5 -- its weight 1 / sqrt(d_i d_j) is small, the pad element
    holds nearly all of the row's mass and the slices cancel (that file's docstring has the mechanism); no row of that kind runs code
    this file is about.

Measured on an MI355X:
    (1) gw per entry err / bound, largest over tau 1 and 3, distinct and tied keys: S = 3: 0.23, S = 8: 0.22, S = 70: 0.07;
        pre-filled with 0.5: 0.35, 0.27, 0.16; err / row maximum 1.3e-7 (S = 3) .. 1.6e-6 (S = 70).
        per degree, tau 1, distinct keys, S = 70:  24: 0.00  25: 0.02  32: 0.02  33: 0.02  40: 0.01  41: 0.01  48: 0.01  49: 0.01
        63: 0.01  64: 0.01  65: 0.02  96: 0.01  97: 0.02  127: 0.01  128: 0.01  129: 0.01  192: 0.02  193: 0.02  255: 0.01  256: 0.02
        (257: the zero row)  511: 0.02  512: 0.02  513: 0.04  1023: 0.07  1024: 0.04 | generic kernel, A = S:  1025: 0.01  2047: 0.01
        2048: 0.01  2049: 0.01;      S = 3, same case:  25: 0.15  32: 0.17  33: 0.15  192: 0.16  193: 0.17  256: 0.20  511: 0.20
        513: 0.20  1023: 0.21  1024: 0.20  1025: 0.21  2049: 0.19.
        gkey per row 1.1e-7, per entry 1.6e-7 of the line maximum, gfreq 1.2e-6 (all cases of (1) - (3)).
    (2) err / bound 0.21 / 0.20 / 0.03 for S = 3 / 8 / 70.      (3) 0.21 / 0.22 / 0.07.
    (4) unit S 9 / S 70: out per row 3.9e-7 / 5.7e-7, gx 5.2e-7 / 7.9e-7, g edge_weight per recipient 5.6e-7 / 1.9e-7;
        gcn_loops S 9 / S 70: out 1.9e-6 / 4.9e-7, gx 1.0e-6 / 7.7e-7, g edge_weight per recipient 1.9e-7 / 2.0e-7 (the hub, on the
        generic kernel: 1.0e-7 / 1.9e-7); parameters <= 2.0e-6.
    The whole file: 34 tests in 6.2 s.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import edge_weight_long_cases as LC
from tests import test_hip_edge_weight as T
from tests.conftest import relerr
from tests.test_hip_ties import F32_BOUND, PER_ENTRY, dev, line_maxima, per_row, t  # noqa: F401
from tests.weight_grad_ref import per_entry_ratio, row_maxima

pytestmark = pytest.mark.gpu
OUT_SCALE, HAS_MASS, FILL = 0.7, 1, 0.5


def run_kernel(dev, tau, tied, S, fill=0.0, lo=False, top=None, scratch=True):
    """One launch on the recipients of at most `top` neighbours (None: all): {"gw" [nnz], "gkey" [nnz, S], "gfreq" [S]} as float64
    numpy arrays.  scratch False: scratch = NULL, scratch_bytes = 0."""
    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.graph import import_csr
    L = _lib.lib()
    k = LC.kernel_inputs(tau, tied)
    Xp_h, fr_h, G_h = LC.expand(k, S)
    nrows, nnz = LC.rows_up_to(top)
    maxdeg = LC.DEGREES[nrows - 1]
    stream = torch.cuda.current_stream(dev).cuda_stream
    graph = import_csr(t(k["rowptr"][:nrows + 1], dev, torch.int32), t(k["col"][:nnz], dev, torch.int32), t(k["w"][:nnz], dev), nrows,
                       k["w"].size)
    st = graph.read_stats()
    assert not (st[_lib.STAT_FLAGS] & ~_lib.FLAG_W_NONUNIT) and st[_lib.STAT_NNZ] == nnz and st[_lib.STAT_MAX_DEGREE] == maxdeg
    assert np.array_equal(graph.col[:nnz].cpu().numpy(), k["col"][:nnz]) and np.array_equal(graph.w[:nnz].cpu().numpy(), k["w"][:nnz])
    Xp, fr, g = t(Xp_h, dev), t(fr_h, dev), t(G_h[:nrows], dev)
    a = _lib.EmbedArgs()
    a.rowptr, a.col, a.w, a.perm = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.w.data_ptr(), graph.perm.data_ptr()
    a.bin_start, a.bin_start_host, a.num_rows = graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data, nrows
    a.Xp, a.ldp, a.freqs, a.S, a.tau = Xp.data_ptr(), Xp.stride(0), fr.data_ptr(), S, tau
    a.out_scale, a.has_mass, a.mass_fn, a.mass_scale = OUT_SCALE, HAS_MASS, 0, 1.0
    a.num_reg_rows, a.num_lds_rows = st[_lib.STAT_NUM_REG], st[_lib.STAT_NUM_LDS]
    a.num_global_rows, a.num_zero_rows, a.max_degree = st[_lib.STAT_NUM_GLOBAL], st[_lib.STAT_NUM_ZERO], maxdeg
    nbytes = int(L.fsw_embed_backward_w_scratch_bytes(maxdeg, nrows)) if scratch else 0
    assert nbytes > 0 or not scratch
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev) if scratch else None
    gkey = torch.full((nnz, S), float("nan"), device=dev)
    gf = torch.zeros(S, device=dev)
    gw = torch.full((nnz,), fill, device=dev)
    if lo:
        w_lo = t(k["w_lo"][:nnz], dev)
        rc = L.fsw_embed_backward_w_lo_f32(ctypes.byref(a), _lib.ptr(w_lo), maxdeg, _lib.ptr(g), g.stride(0), _lib.ptr(gkey), S, _lib.ptr(gf),
                                           _lib.ptr(gw), _lib.ptr(buf), nbytes, stream)
    else:
        rc = L.fsw_embed_backward_w_f32(ctypes.byref(a), maxdeg, _lib.ptr(g), g.stride(0), _lib.ptr(gkey), S, _lib.ptr(gf), _lib.ptr(gw),
                                        _lib.ptr(buf), nbytes, stream)
    assert rc == 0, L.fsw_last_error()
    torch.cuda.synchronize()
    return {name: v.cpu().numpy().astype(np.float64) for name, v in (("gw", gw), ("gkey", gkey), ("gfreq", gf))}


def check_gw(got, ref, S, what, fill=0.0, top=None):
    """(1) of the module docstring on the recipients of at most `top` neighbours: every entry is compared."""
    nrows, nnz = LC.rows_up_to(top)
    k = LC.kernel_inputs(1.0, False)
    rowptr, deg = k["rowptr"][:nrows + 1], k["degrees"][:nrows]
    got = got - fill
    assert got.shape == ref["gW"].shape == (nnz,) and np.isfinite(got).all(), what
    adds = np.repeat([LC.float32_adds(int(d), S) for d in deg], deg)
    bound = LC.gw_bound(ref, rowptr, S, adds, fill)
    err = np.abs(got - ref["gW"])
    zero = row_maxima(ref["gW"], rowptr) == 0                 # the row whose output gradient is zero: the kernel adds nothing
    assert zero[rowptr[LC.ZERO_ROW]:rowptr[LC.ZERO_ROW + 1]].all() and not got[zero].any(), what
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    cls = per_row(lambda a, b: ratio[a:b].max(), rowptr)
    rel = per_entry_ratio(got, ref["gW"], rowptr)
    print("%s: gw per entry err / bound %.2f, err / row maximum %.2e" % (what, ratio.max(), rel.max()))
    print("   per degree err / bound:  " + "  ".join("%d: %.2f" % (d, c) for d, c in zip(deg, cls) if d))
    worst = int(ratio.argmax())
    rowdeg = np.repeat(deg, deg)
    assert ratio.max() <= 1.0, (what, "entry %d (row of %d)" % (worst, rowdeg[worst]), float(ratio.max()), float(got[worst]),
                                float(ref["gW"][worst]))


def check_keys_and_freqs(res, ref, what, top=None):
    """test_hip_edge_weight.check_keys_and_freqs on this file's rows (float32 storage)."""
    nrows, _ = LC.rows_up_to(top)
    k = LC.kernel_inputs(1.0, False)
    rowptr, deg = k["rowptr"][:nrows + 1], k["degrees"][:nrows]
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


@pytest.mark.parametrize("S", LC.S_VALUES)
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_kernel_weight_gradients(dev, tau, tied, S):
    """(1) of the module docstring."""
    ref = LC.reference(tau, tied, OUT_SCALE, S)
    what = "tau %g %s S %d" % (tau, "tied" if tied else "distinct", S)
    res = run_kernel(dev, tau, tied, S)
    check_gw(res["gw"], ref, S, what)
    check_keys_and_freqs(res, ref, what)
    filled = run_kernel(dev, tau, tied, S, fill=FILL)
    check_gw(filled["gw"], ref, S, what + " pre-filled", fill=FILL)
    assert np.array_equal(filled["gkey"], res["gkey"]), what


@pytest.mark.parametrize("S", LC.S_VALUES)
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_no_scratch_inside_the_class(dev, tau, S):
    """(2) of the module docstring; fails on the parent commit ("need scratch")."""
    from fsw_gnn_amd import _lib
    assert _lib.lib().fsw_embed_backward_w_tuned_max_degree() >= 1024
    top = LC.NO_SCRATCH_MAX
    assert LC.DEGREES[LC.rows_up_to(top)[0] - 1] == 257 and LC.ZERO_ROW < LC.rows_up_to(top)[0]
    for tied in (False, True):
        ref = LC.reference(tau, tied, OUT_SCALE, S, top=top)
        what = "no scratch, rows <= %d, tau %g %s S %d" % (top, tau, "tied" if tied else "distinct", S)
        res = run_kernel(dev, tau, tied, S, top=top, scratch=False)
        check_gw(res["gw"], ref, S, what, top=top)
        check_keys_and_freqs(res, ref, what, top=top)


@pytest.mark.parametrize("S", LC.S_VALUES)
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_w_lo_on_long_rows(dev, tau, tied, S):
    """(3) of the module docstring; fails on the parent commit (its rows above 24 neighbours read w alone)."""
    top = LC.TUNED_MAX
    ref = LC.reference(tau, tied, OUT_SCALE, S, lo=True, top=top)
    what = "w_lo, rows <= %d, tau %g %s S %d" % (top, tau, "tied" if tied else "distinct", S)
    res = run_kernel(dev, tau, tied, S, lo=True, top=top)
    check_gw(res["gw"], ref, S, what, top=top)
    check_keys_and_freqs(res, ref, what, top=top)


# ---- (4) layer level ------------------------------------------------------------------------------------------------------------------
N_VERT, HUB_DEG, N_MID = 2100, 2048, 300


def layer_graph():
    """(edge_index [2, E] int64, weights [E] float64 exact in float32): module docstring (4); weights in [0.05, 1): rows below and
    above tau = 1."""
    rng = np.random.default_rng(5300)
    deg = np.concatenate([[HUB_DEG, 0], rng.integers(25, 601, size=N_MID), rng.integers(25, 65, size=N_VERT - 2 - N_MID)])
    dst = np.repeat(np.arange(N_VERT), deg)
    src = np.concatenate([rng.permutation(N_VERT)[:d] for d in deg])              # distinct senders per recipient
    dup = rng.integers(0, dst.size, size=200)
    dst, src = np.concatenate([dst, dst[dup]]), np.concatenate([src, src[dup]])
    order = rng.permutation(dst.size)
    w = rng.uniform(0.05, 1.0, dst.size)
    return np.stack([src[order], dst[order]]).astype(np.int64), w.astype(np.float32).astype(np.float64)


def run_long_training_case(dev, what, **kw):
    """test_hip_edge_weight.run_training_case on layer_graph()."""
    conv, twin = T.make_pair(dev, torch.float32, **kw)
    with torch.no_grad():                                 # keys exact in float32: module docstring (4)
        V = torch.round(conv.fsw_embed.projVecs * 64.0) / 64.0
        conv.fsw_embed.projVecs.copy_(V)
        twin.fsw_embed.projVecs.copy_(V.double())
    ei_h, w_h = layer_graph()
    indeg = np.bincount(ei_h[1], minlength=N_VERT)
    assert indeg[0] >= HUB_DEG and indeg[1] == 0 and (np.delete(indeg, 1) >= 25).all() and ((indeg > 64) & (indeg <= 610)).sum() >= N_MID - 30
    rng = np.random.default_rng(5400)
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
    cuts = np.concatenate([[0], np.cumsum(indeg)])
    e_w = np.array([relerr(got[order[a:b]], want[order[a:b]]) if b > a else 0.0 for a, b in zip(cuts[:-1], cuts[1:])])
    e_p = {name: relerr(p.grad.cpu().numpy().astype(np.float64), dict(twin.named_parameters())[name].grad.cpu().numpy())
           for name, p in conv.named_parameters() if p.grad is not None}
    print("%s: out per row %.2e, gx per row %.2e, g edge_weight per recipient %.2e (in-degree %d; the hub: %.2e), parameters %s" % (
        what, e_out.max(), e_x.max(), e_w.max(), indeg[e_w.argmax()], e_w[0], "  ".join("%s %.1e" % kv for kv in sorted(e_p.items()))))
    assert {"fsw_embed.projVecs", "fsw_embed.freqs", "mlp.0.weight"} <= set(e_p)
    assert e_out.max() <= T.F32_FWD, (what, int(e_out.argmax()), float(e_out.max()))
    assert e_x.max() <= T.F32_GRAD, (what, int(e_x.argmax()), float(e_x.max()))
    assert e_w.max() <= T.F32_GRAD, (what, int(e_w.argmax()), int(indeg[e_w.argmax()]), float(e_w.max()))
    assert max(e_p.values()) <= T.F32_GRAD, (what, e_p)


@pytest.mark.parametrize("embed_dim", [10, 71], ids=["S9", "S70"])
@pytest.mark.parametrize("scheme", ["unit", "gcn_loops"])
def test_layer_learnable_edge_weights_long_rows(dev, scheme, embed_dim):
    """(4) of the module docstring."""
    kw = dict(self_loop_weight=0.5, edge_weighting='gcn') if scheme == "gcn_loops" else {}
    run_long_training_case(dev, "long rows, %s S %d" % (scheme, embed_dim - 1), embed_dim=embed_dim, **kw)
