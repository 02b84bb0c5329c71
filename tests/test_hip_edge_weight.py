"""Per-edge weights of FSW_conv (forward(edge_weight=)) and their gradient on csrc/embed_w_bwd.hip, on the GPU.  The yardstick is
tests/weight_grad_ref.py (autograd of a plain float64 forward) everywhere, never the generic kernel.

(a) Kernel level: fsw_embed_backward_w_f32 through ctypes on a hand-made CSR (graph.import_csr keeps the entries in place): one
    recipient per degree 0 .. 40 (both sides of the register class of 24 and of the degree bins at 32), one row of 300 (the generic
    hand-over, an LDS line), 70 further rows of 5 (three 32-row tiles of one bin, the last partial).  Keys exact in float32 and
    distinct, or tied on the grid of 1/8 with the pad key; weights from {0, 1/4, 1/2, 1}, rows of total mass below tau, tau exactly
    and above, tau 1 and 3 (tests/edge_weight_cases.py); S = 8 (one partial chunk), 70 (two waves of a workgroup), 260 (two
    workgroups in y; the last chunk holds 4 slices); out_scale 0.7, a mass column in g; an output gradient with zero readouts
    and one zero row.
      gw per entry  <= 2 [G64_ROW (row max |gW|) + (ceil(S / 64) + 2) 2^-24 sum_s |gW_s[j]|]: the arithmetic is float64, there is
                    one float32 rounding of each chunk's sum and one per atomic add; the test applies twice the derived bound (the
                    convention of tests/test_hip_weight_grad.py).  Applied to every row: the rows above the class limit, which run
                    on the unchanged generic kernel (one add per slice, derived bound S + 2 in place of ceil(S / 64) + 2), meet it
                    as well.
      pre-filled gw the result is fill + gradient, with the fill term (S + 1) 2^-24 |fill| of test_hip_weight_grad.gw_bound;
      the zero row  adds exactly nothing (also to the fill);
      gkey / gfreq  the bounds of test_hip_weight_grad.check_keys_and_freqs: per row and gfreq F32_BOUND norm-wise, per entry
                    PER_ENTRY of the line maximum.
(b) Layer level: FSW_conv float32, 401 vertices and about 3000 edges (in-degrees 1 .. 40, a hub of 300, parallel edges, one vertex
    without in-edges), S = 9 and 70, edge_weight requiring grad.  Anchor, computed here with torch ops: the weighted coalesced
    adjacency (self loops and 'gcn' included) fed to the float64 twin's fsw_embed(x, W=adj, graph_mode=True) and _tail -- that path
    is pinned to the reference at 1e-12 by tests/test_hip_float64.py.  Per row at the module-level bounds of
    tests/test_hip_float64.py (forward 1e-5, gradients 2e-5): the output, the gradients of x, of every parameter (norm-wise) and of
    edge_weight grouped by recipient.  Variants: unit scheme; self_loop_weight 0.5 with 'gcn' (the gradient passes through the
    normalisation); a graph in which no row is below tau (the tau / 2 launch); a float64 layer with learnable weights at 1e-10;
    constant weights in Cartesian mode, with edge features and in tuple-CSR form against the anchor's forward; every refusal.

Measured on an MI355X:
    kernel level  gw per entry err / bound, largest over tau 1 and 3, distinct and tied keys (register rows | generic rows):
                  S = 8: 0.21 | 0.12 (generic rows against their own derived bound S + 2; 0.41 of the bound applied here)
                  S = 70: 0.05 | 0.22      S = 260: 0.01 | 0.12      pre-filled with 0.5: 0.19 | 0.28 (S = 8)
                  per degree, tau 1, distinct keys, S = 8:  1: 0.07  2: 0.08  3: 0.03  4: 0.03  6: 0.13  7: 0.12  8: 0.05  9: 0.07
                  10: 0.08  11: 0.11  13: 0.08  14: 0.07  15: 0.11  16: 0.08  17: 0.14  18: 0.14  19: 0.12  20: 0.13  21: 0.11  22: 0.11
                  23: 0.10  24: 0.15  | generic kernel, against S + 2:  25: 0.07  26: 0.03  27: 0.07  28: 0.10  29: 0.06  30: 0.09
                  31: 0.05  32: 0.06  33: 0.10  34: 0.07  35: 0.06  36: 0.07  37: 0.04  38: 0.06  39: 0.06  40: 0.06  300: 0.10
                  | the 70 rows of 5: 0.18   (the rows of 5 and 12 neighbours have a zero output gradient at S = 8)
                  err / row maximum 1.3e-7 (S = 8) .. 4.8e-6 (S = 260); gkey per row 9.0e-8, per entry 1.6e-7 of the line maximum,
                  gfreq 3.0e-7
    layer level   unit S 9 / S 70: out per row 7.6e-7 / 6.3e-7, gx 2.7e-7 / 5.2e-7, g edge_weight per recipient 2.8e-6 / 1.8e-6;
                  gcn_loops S 9 / S 70: out 9.9e-7 / 1.5e-6, gx 4.3e-7 / 8.7e-7, g edge_weight per recipient 2.4e-6 / 6.9e-6;
                  parameters <= 4.7e-7; no deficient row: 3.6e-7, 2.4e-7, 1.3e-6; float64 layer: 1e-15 at most;
                  constant weights: Cartesian 7.6e-7, edge features 5.7e-7, tuple CSR 4.4e-6
    float32 weights in the backward (before fsw_embed_backward_w_lo_f32 carried their float64 remainder): g edge_weight per
                  recipient 4.8e-5 / 3.2e-4 with gcn_loops (2 / 19 recipients above the bound 2e-5) and 1.2e-5 with unit S 70 --
                  both gcn_loops tests fail on that code, and on the generic float32 route (6.3e-5 / 3.0e-4): a weight rounded by
                  2^-25 moves cos(2 pi xi c) by 2 pi xi 2^-25 (xi up to 139 at S = 70), times the cancellation over the slices in a
                  recipient of one or two neighbours.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import edge_weight_cases as C
from tests.conftest import relerr
from tests.test_hip_ties import F32_BOUND, G64_ROW, PER_ENTRY, dev, line_maxima, per_row, t  # noqa: F401
from tests.weight_grad_ref import per_entry_ratio, row_maxima

pytestmark = pytest.mark.gpu
OUT_SCALE, HAS_MASS = 0.7, 1
FILL = 0.5
CLASS_LIMIT = 24                                           # csrc/embed_w_bwd.hip: kWRegMaxDeg
F32_FWD, F32_GRAD, F64_GRAD = 1e-5, 2e-5, 1e-10           # module level, per row (tests/test_hip_float64.py)


# ---- (a) kernel level -----------------------------------------------------------------------------------------------------------------
def run_kernel(dev, tau, tied, S, fill=0.0):
    """One launch of fsw_embed_backward_w_f32: {"gw" [nnz], "gkey" [nnz, S], "gfreq" [S]} as float64 numpy arrays."""
    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.graph import import_csr
    L = _lib.lib()
    k = C.kernel_inputs(tau, tied)
    Xp_h, fr_h, G_h = C.expand(k, S)
    nrows, nnz, maxdeg = len(C.KERNEL_DEGREES), k["w"].size, max(C.KERNEL_DEGREES)
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
    nbytes = int(L.fsw_embed_backward_w_scratch_bytes(maxdeg, nrows))
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    gkey = torch.full((nnz, S), float("nan"), device=dev)
    gf = torch.zeros(S, device=dev)
    gw = torch.full((nnz,), fill, device=dev)
    _lib.check(L.fsw_embed_backward_w_f32(ctypes.byref(a), maxdeg, _lib.ptr(g), g.stride(0), _lib.ptr(gkey), S, _lib.ptr(gf),
                                          _lib.ptr(gw), _lib.ptr(scratch), nbytes, stream), "fsw_embed_backward_w_f32")
    torch.cuda.synchronize()
    return {name: v.cpu().numpy().astype(np.float64) for name, v in (("gw", gw), ("gkey", gkey), ("gfreq", gf))}


def gw_bound(ref, S, adds, fill=0.0):
    """Per entry, module docstring: twice [G64_ROW of the row maximum + (adds + 2) 2^-24 sum_s |gW_s| + (S + 1) 2^-24 |fill|]."""
    rowptr = C.kernel_inputs(1.0, False)["rowptr"]
    eps = 2.0 ** -24
    return 2.0 * (G64_ROW * row_maxima(ref["gW"], rowptr) + (S + 1) * eps * abs(fill) + (adds + 2) * eps * np.abs(ref["gW_s"]).sum(axis=1))


def check_gw(got, ref, S, what, fill=0.0):
    k = C.kernel_inputs(1.0, False)
    rowptr, deg = k["rowptr"], k["degrees"]
    got = got - fill
    assert np.isfinite(got).all(), what
    rowdeg = np.repeat(deg, deg)
    chunks = -(-S // 64)
    tight = gw_bound(ref, S, chunks, fill)                                   # one add per entry and chunk
    bound = tight                                                            # every row, the generic kernel's too
    err = np.abs(got - ref["gW"])
    zero = row_maxima(ref["gW"], rowptr) == 0                 # the row whose output gradient is zero: the kernel adds nothing
    assert zero[rowptr[C.ZERO_ROW]:rowptr[C.ZERO_ROW + 1]].all() and not got[zero].any(), what
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    cls = per_row(lambda a, b: ratio[a:b].max(), rowptr)
    rel = per_entry_ratio(got, ref["gW"], rowptr)
    reg, gen = rowdeg <= CLASS_LIMIT, rowdeg > CLASS_LIMIT
    print("%s: gw per entry err / bound: register rows %.2f, generic rows %.2f; err / row maximum %.2e"
          % (what, ratio[reg].max(), ratio[gen].max(), rel.max()))
    print("   per degree err / bound:  " + "  ".join("%d: %.2f" % (d, c) for d, c in list(zip(deg, cls))[:42] if d)
          + "  5 (70 rows): %.2f" % cls[42:].max())
    worst = int(ratio.argmax())
    assert ratio.max() <= 1.0, (what, "entry %d (row of %d)" % (worst, rowdeg[worst]), float(ratio.max()), float(got[worst]),
                                float(ref["gW"][worst]))


def check_keys_and_freqs(res, ref, what):
    """test_hip_weight_grad.check_keys_and_freqs on this file's rows (float32 storage)."""
    k = C.kernel_inputs(1.0, False)
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


@pytest.mark.parametrize("S", [8, 70, 260])
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_kernel_weight_gradients(dev, tau, tied, S):
    """(a) of the module docstring: one launch into a zeroed gw, one into a pre-filled gw."""
    ref = C.reference(tau, tied, OUT_SCALE, S)
    what = "tau %g %s S %d" % (tau, "tied" if tied else "distinct", S)
    res = run_kernel(dev, tau, tied, S)
    check_gw(res["gw"], ref, S, what)
    check_keys_and_freqs(res, ref, what)
    filled = run_kernel(dev, tau, tied, S, fill=FILL)
    check_gw(filled["gw"], ref, S, what + " pre-filled", fill=FILL)
    assert np.array_equal(filled["gkey"], res["gkey"]), what


def test_kernel_entry_refuses_edge_features_and_missing_weights(dev):
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(64, device=dev)
    a = _lib.EmbedArgs()
    for name in ("rowptr", "col", "perm", "bin_start", "Xp", "freqs"):
        setattr(a, name, buf.data_ptr())
    a.S, a.ldp, a.tau, a.num_rows = 1, 1, 1.0, 0
    call = lambda: L.fsw_embed_backward_w_f32(ctypes.byref(a), 0, _lib.ptr(buf), 2, _lib.ptr(buf), 1, None, _lib.ptr(buf), None, 0, None)  # noqa: E731
    assert call() != 0 and b"weights" in L.fsw_last_error()                 # w == NULL
    a.w = a.efeat = buf.data_ptr()
    assert call() != 0 and b"edge features" in L.fsw_last_error()
    a.efeat = None
    assert call() == 0                                                       # no rows: nothing to do


# ---- (b) layer level ------------------------------------------------------------------------------------------------------------------
N_VERT, HUB, EMPTY = 401, 0, 1


def layer_graph(full):
    """(edge_index [2, E] int64, weights [E] float64): vertex 0 a hub of 300 in-edges, vertices 2 .. 41 in-degrees 1 .. 40, the rest
    1 .. 9, 40 parallel edges on top; vertex 1 has no in-edge and weights in [0.05, 1) (rows below and above tau = 1) -- or, `full`,
    vertex 1 has two and every weight lies in [1, 2): no row is below tau."""
    rng = np.random.default_rng(4300 + full)
    deg = np.concatenate([[300, 2 if full else 0], np.arange(1, 41), rng.integers(1, 10, size=N_VERT - 42)])
    dst = np.repeat(np.arange(N_VERT), deg)
    src = rng.integers(0, N_VERT, size=dst.size)
    dup = rng.integers(0, dst.size, size=40)
    dst, src = np.concatenate([dst, dst[dup]]), np.concatenate([src, src[dup]])
    order = rng.permutation(dst.size)
    w = rng.uniform(1.0, 2.0, dst.size) if full else rng.uniform(0.05, 1.0, dst.size)
    # exact in float32, like every input here: the float64 anchor and the float32 layer get the same numbers (a weight rounded by
    # 2^-25 moves cos(2 pi xi c) by 2 pi xi 2^-25, 3e-5 at the largest frequency of 70 slices)
    return np.stack([src[order], dst[order]]).astype(np.int64), w.astype(np.float32).astype(np.float64)


def make_pair(dev, dtype=torch.float32, **kw):
    """The layer under test and its float64 twin with the same parameters."""
    from fsw_gnn_amd import FSW_conv
    torch.manual_seed(11)
    conv = FSW_conv(6, 5, device=dev, dtype=dtype, **kw)
    twin = FSW_conv(6, 5, device=dev, dtype=torch.float64, **kw)
    twin.load_state_dict({name: v.double() for name, v in conv.state_dict().items()})
    return conv, twin


def anchor_forward(twin, x64, ei, w64, ef64=None):
    """The weighted coalesced adjacency by torch ops -- parallel edges summed, self loops, 'gcn' by the weighted in-degrees
    (reference fsw_conv.py:384-447) -- through the float64 twin's embedding and tail."""
    n = x64.shape[0]
    inds, vals = ei.flip(0), w64
    if twin.self_loop_weight > 0:
        loops = torch.arange(n, device=ei.device)
        inds = torch.cat([inds, torch.stack([loops, loops])], dim=1)
        vals = torch.cat([vals, torch.full((n,), float(twin.self_loop_weight), dtype=torch.float64, device=ei.device)])
    adj = torch.sparse_coo_tensor(inds, vals, (n, n)).coalesce()
    if twin.edge_weighting == 'gcn':
        ai, av = adj.indices(), adj.values()
        ds = torch.sqrt(torch.zeros(n, dtype=torch.float64, device=ei.device).index_add(0, ai[0], av))
        adj = torch.sparse_coo_tensor(ai, av / ds[ai[0]] / ds[ai[1]], (n, n), is_coalesced=True)
    x_edge = None
    if ef64 is not None:
        if twin.self_loop_weight > 0:
            ef64 = torch.cat([ef64, torch.zeros((n, ef64.shape[1]), dtype=torch.float64, device=ei.device)])
        x_edge = torch.sparse_coo_tensor(inds, ef64, (n, n, ef64.shape[1])).coalesce()
    return twin._tail(twin.fsw_embed(x64, W=adj, X_edge=x_edge, graph_mode=True), x64)


def rows_err(got, ref):
    got, ref = got.detach().cpu().numpy().astype(np.float64), ref.detach().cpu().numpy()
    return np.array([relerr(got[r], ref[r]) for r in range(ref.shape[0])])


def grouped_err(got, ref, dst, n):
    got, ref = got.detach().cpu().numpy().astype(np.float64), ref.detach().cpu().numpy()
    return np.array([relerr(got[dst == v], ref[dst == v]) if (dst == v).any() else 0.0 for v in range(n)])


def run_training_case(dev, what, full, dtype, fwd_tol, grad_tol, **kw):
    conv, twin = make_pair(dev, dtype, **kw)
    ei_h, w_h = layer_graph(full)
    rng = np.random.default_rng(4400)
    x_h, r_h = rng.standard_normal((N_VERT, 6)).astype(np.float32), rng.standard_normal((N_VERT, 5)).astype(np.float32)
    ei = torch.from_numpy(ei_h).to(dev)
    x64, w64 = t(x_h, dev, torch.float64).requires_grad_(True), t(w_h, dev, torch.float64).requires_grad_(True)
    x, w = t(x_h, dev, dtype).requires_grad_(True), t(w_h, dev, dtype).requires_grad_(True)
    ref = anchor_forward(twin, x64, ei, w64)
    (ref * t(r_h, dev, torch.float64)).sum().backward()
    out = conv(x, ei, edge_weight=w)
    (out * t(r_h, dev, dtype)).sum().backward()
    assert w.grad is not None and tuple(w.grad.shape) == tuple(w.shape) and bool(torch.isfinite(w.grad).all())
    e_out, e_x = rows_err(out, ref), rows_err(x.grad, x64.grad)
    e_w = grouped_err(w.grad, w64.grad, ei_h[1], N_VERT)
    e_p = {name: relerr(p.grad.cpu().numpy().astype(np.float64), dict(twin.named_parameters())[name].grad.cpu().numpy())
           for name, p in conv.named_parameters() if p.grad is not None}
    indeg = np.bincount(ei_h[1], minlength=N_VERT)
    print("%s: out per row %.2e, gx per row %.2e, g edge_weight per recipient %.2e (in-degree %d), parameters %s" % (
        what, e_out.max(), e_x.max(), e_w.max(), indeg[e_w.argmax()], "  ".join("%s %.1e" % kv for kv in sorted(e_p.items()))))
    assert {"fsw_embed.projVecs", "fsw_embed.freqs", "mlp.0.weight"} <= set(e_p)
    assert e_out.max() <= fwd_tol, (what, int(e_out.argmax()), float(e_out.max()))
    assert e_x.max() <= grad_tol, (what, int(e_x.argmax()), float(e_x.max()))
    assert e_w.max() <= grad_tol, (what, int(e_w.argmax()), int(indeg[e_w.argmax()]), float(e_w.max()))
    assert max(e_p.values()) <= grad_tol, (what, e_p)


@pytest.mark.parametrize("embed_dim", [10, 71], ids=["S9", "S70"])
@pytest.mark.parametrize("scheme", ["unit", "gcn_loops"])
def test_layer_learnable_edge_weights(dev, scheme, embed_dim):
    kw = dict(self_loop_weight=0.5, edge_weighting='gcn') if scheme == "gcn_loops" else {}
    run_training_case(dev, "%s S %d" % (scheme, embed_dim - 1), False, torch.float32, F32_FWD, F32_GRAD, embed_dim=embed_dim, **kw)


def test_layer_without_a_deficient_row_takes_the_half_tau_launch(dev):
    """No row below tau = 1, rows of one neighbour with m in [1, 2) and weights such that some m come close to tau: the reference pads
    nothing, and the clamp rule at tau would be wrong on a row with m == tau (tests/test_edge_weight_cpu.py)."""
    run_training_case(dev, "no deficient row S 9", True, torch.float32, F32_FWD, F32_GRAD, embed_dim=10)


def test_float64_layer_with_learnable_edge_weights(dev):
    run_training_case(dev, "float64 gcn_loops S 9", False, torch.float64, F64_GRAD, F64_GRAD, embed_dim=10, self_loop_weight=0.5,
                      edge_weighting='gcn')


@pytest.mark.parametrize("form", ["cartesian", "edge_features", "tuple_csr"])
def test_constant_edge_weights_forward(dev, form):
    """Constant weights where general weights already run, against the anchor's forward, per row at 1e-5."""
    kw = {"cartesian": dict(embed_slices=3, embed_freqs=3), "edge_features": dict(edgefeat_dim=2, embed_dim=10),
          "tuple_csr": dict(embed_dim=10, self_loop_weight=0.5, edge_weighting='gcn')}[form]
    conv, twin = make_pair(dev, **kw)
    ei_h, w_h = layer_graph(False)
    rng = np.random.default_rng(4500)
    x_h, ef_h = rng.standard_normal((N_VERT, 6)).astype(np.float32), rng.standard_normal((ei_h.shape[1], 2)).astype(np.float32)
    ei = torch.from_numpy(ei_h).to(dev)
    with torch.no_grad():
        ref = anchor_forward(twin, t(x_h, dev, torch.float64), ei, t(w_h, dev, torch.float64),
                             t(ef_h, dev, torch.float64) if form == "edge_features" else None)
        x, w = t(x_h, dev), t(w_h, dev)
        if form == "tuple_csr":
            order = np.argsort(ei_h[1], kind="stable")
            rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei_h[1], minlength=N_VERT))])
            out = conv(x, (t(rowptr, dev, torch.int64), t(ei_h[0][order], dev, torch.int64)), edge_weight=t(w_h[order], dev))
        elif form == "edge_features":
            out = conv(x, ei, edge_features=t(ef_h, dev), edge_weight=w)
        else:
            out = conv(x, ei, edge_weight=w)
        unweighted = conv(x, ei, edge_features=t(ef_h, dev)) if form == "edge_features" else conv(x, ei)
    e = rows_err(out, ref)
    print("constant weights, %s: out per row %.2e" % (form, e.max()))
    assert e.max() <= F32_FWD, (form, int(e.argmax()), float(e.max()))
    assert rows_err(unweighted, ref).max() > 1e-3                       # the weights matter


def test_refusals(dev):
    from fsw_gnn_amd import FSW_conv
    ei_h, w_h = layer_graph(False)
    ei, x = torch.from_numpy(ei_h).to(dev), torch.zeros((N_VERT, 6), device=dev)
    wg = t(w_h, dev).requires_grad_(True)
    E = ei_h.shape[1]
    for kw, extra, word in ((dict(embed_slices=3, embed_freqs=3), {}, "Cartesian"),
                            (dict(edgefeat_dim=2, embed_dim=10), dict(edge_features=torch.zeros((E, 2), device=dev)), "edge features"),
                            (dict(embed_dim=10, homog_degree_encoding=True), {}, "homog_degree_encoding")):
        conv = FSW_conv(6, 5, device=dev, **kw)
        with pytest.raises(NotImplementedError, match=word):
            conv(x, ei, edge_weight=wg, **extra)
        with torch.no_grad():                                   # the same call with grad disabled treats the weights as constants
            assert bool(torch.isfinite(conv(x, ei, edge_weight=wg, **extra)).all())
    conv = FSW_conv(6, 5, embed_dim=10, device=dev)
    order = np.argsort(ei_h[1], kind="stable")
    rowptr = t(np.concatenate([[0], np.cumsum(np.bincount(ei_h[1], minlength=N_VERT))]), dev, torch.int64)
    col = t(ei_h[0][order], dev, torch.int64)
    with pytest.raises(NotImplementedError, match="tuple form"):
        conv(x, (rowptr, col), edge_weight=wg)
    adj = torch.sparse_coo_tensor(ei.flip(0), t(w_h, dev), (N_VERT, N_VERT)).coalesce().to_sparse_csr()
    with pytest.raises(AssertionError, match="sparse_csr"):
        conv(x, adj, edge_weight=torch.ones(adj.values().numel(), device=dev))
    conv._node_parallel = True
    with pytest.raises(NotImplementedError, match="enable_slice_parallel / enable_node_parallel"):
        conv(x, ei, edge_weight=wg.detach())
    conv._node_parallel = False
    with pytest.raises(AssertionError, match="nonnegative"):
        conv(x, ei, edge_weight=-wg.detach())
