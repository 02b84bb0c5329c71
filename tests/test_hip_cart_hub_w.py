"""Cartesian mode on general-weight rows of 2048 .. 16383 neighbours (lines of 2049 .. 16384 elements with the pad element): k_cart_hub_w
(forward, no scratch) and k_cart_bwd_long_w (backward, one scratch line per wavefront) through fsw_embed_cart_f32 /
fsw_embed_cart_backward_keys_f32 and through the modules.

One graph with one recipient per degree: both edges of the three workgroup sizes (2, 4, 8 wavefronts per line), one row inside each
class and the last row of the wavefront class, next to rows of the register classes.  The keys hold 200 sender pairs with
bit-identical keys, one constant column, one control column without ties and one column of zeros, which ties with the pad element.
Three weight modes: random weights with row mass > 1, the same weights scaled to row mass 0.4 (the pad element then has positive
weight) and w = NULL with tau = 3.  Yardsticks: the float64 oracle through the diagonal identity (forward) and the generic kernel
with float64 storage on the same inputs (backward).  Bounds: the project's TOL, F32_BOUND and PER_ENTRY of tests/test_hip_ties.py;
1e-5 / 3e-5 at module level (FWD_BOUND / F32_BOUND of tests/test_hip_cartesian_conv.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests.conftest import relerr
from tests.test_hip_cart_hub import DEV, HAS_MASS, OUT_SCALE, SHAPES, cart_args, check_rows, t
from tests.test_hip_ties import F32_BOUND, FREQS, PER_ENTRY, check_key_gradients, coefficient_scale

pytestmark = pytest.mark.gpu

DEGREES = (0, 7, 2047, 2048, 3000, 4095, 4096, 8191, 8192, 12000, 16383)
BEYOND = 16384                     # one row past the classes: stays on the generic kernel
SENDERS = 17000
TIED_PAIRS = 200
COLUMN_KINDS = ("t", "a", "e", "z")        # tied pairs | constant 0.75 | control (CONTROL of test_hip_ties) | constant 0.0
MODES = {"random": 1.0, "low_mass": 1.0, "tau3": 3.0}          # weight mode -> tau
LOW_MASS = 0.4
assert SHAPES == [(3, 5), (4, 8)] and 0.0 in FREQS[:5]


@functools.lru_cache(maxsize=None)
def edges():
    """(recipients, senders, weights) of DEGREES + (BEYOND,), every row drawn without replacement, random weights in (0.05, 1)."""
    rng = np.random.default_rng(81)
    rec, snd = [], []
    for r, deg in enumerate(DEGREES + (BEYOND,)):
        rec.append(np.full(deg, r, dtype=np.int64))
        snd.append(rng.choice(SENDERS, size=deg, replace=False).astype(np.int64))
    rec, snd = np.concatenate(rec), np.concatenate(snd)
    return rec, snd, rng.uniform(0.05, 1.0, size=rec.size).astype(np.float32)


@functools.lru_cache(maxsize=None)
def graph_case(mode, beyond):
    from fsw_gnn_amd import _lib, build_csr
    degrees = DEGREES + ((BEYOND,) if beyond else ())
    rec, snd, w = edges()
    nnz = sum(degrees)
    rec, snd, w = rec[:nnz], snd[:nnz], w[:nnz].copy()
    if mode == "low_mass":
        mass = np.bincount(rec, weights=w.astype(np.float64), minlength=len(degrees))
        w = (w * (LOW_MASS / mass[rec])).astype(np.float32)
    graph = build_csr(t(rec, torch.int64), t(snd, torch.int64), None if mode == "tau3" else t(w), len(degrees), SENDERS)
    st = graph.read_stats()
    rowptr = graph.rowptr.cpu().numpy().astype(np.int64)
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_NNZ] == nnz and tuple(np.diff(rowptr)) == degrees
    assert st[_lib.STAT_MAX_DEGREE] == max(degrees)
    hub0 = _lib.BIN_MID0 + len(_lib.MID_SIZES) + _lib.NUM_LDS_BINS
    # 2047 and 2048 in the last LDS bin; 3000, 4095, 4096 | 8191, 8192 | 12000, 16383 (, 16384) in the hub bins
    assert np.diff(graph.bin_start_host[0])[hub0 - 1:].tolist() == [2, 3, 2, 3 if beyond else 2, 0, 0]
    col = graph.col[:nnz].cpu().numpy().astype(np.int64)
    assert np.array_equal(col, snd)                                # the rows keep the order of the edge list
    w64 = np.ones(nnz) if graph.w is None else graph.w[:nnz].cpu().numpy().astype(np.float64)
    mass = np.bincount(rec, weights=w64, minlength=len(degrees))
    if mode == "random":
        assert (mass[1:] > 1.0).all()
    elif mode == "low_mass":
        assert np.abs(mass[1:] - LOW_MASS).max() < 1e-4
    else:
        assert graph.w is None
    return {"graph": graph, "st": st, "rowptr": rowptr, "col": col, "nnz": nnz, "degrees": degrees, "w64": w64, "tau": MODES[mode]}


@functools.lru_cache(maxsize=None)
def inputs(S, F, freqs=FREQS):
    """Xp [SENDERS, round_up(S, 32)] float32, frequencies freqs[:F], bias, output gradient (for the graph with the row of BEYOND)."""
    rng = np.random.default_rng(82 + S)
    ldp = (S + 31) // 32 * 32
    Xp = rng.standard_normal((SENDERS, ldp)).astype(np.float32)
    pairs = rng.permutation(SENDERS)[:2 * TIED_PAIRS].reshape(2, TIED_PAIRS)
    Xp[pairs[1]] = Xp[pairs[0]]                                    # exactly tied keys in every column ...
    kinds = COLUMN_KINDS[:S]
    for c, kind in enumerate(kinds):
        if kind == "a":
            Xp[:, c] = 0.75
        elif kind == "z":                                           # ties with the pad element (key 0), which must sort last
            Xp[:, c] = 0.0
        elif kind == "e":                                           # ... but the control column: distinct, exact in float32
            Xp[:, c] = (rng.permutation(SENDERS).astype(np.float32) - 8500.0) / 4096.0
    assert np.unique(Xp[:, kinds.index("e")]).size == SENDERS and np.array_equal(Xp[pairs[0], 0], Xp[pairs[1], 0])
    fr = np.array(freqs[:F], dtype=np.float32)
    width = HAS_MASS + S * F
    bias = (0.1 * rng.standard_normal(width)).astype(np.float32)
    g = rng.standard_normal((len(DEGREES) + 1, width)).astype(np.float32)
    for a in (Xp, fr, bias, g):
        a.setflags(write=False)
    return {"Xp": Xp, "fr": fr, "bias": bias, "g": g, "kinds": kinds, "ldp": ldp}


@functools.lru_cache(maxsize=None)
def forward_reference(mode, S, F, freqs=FREQS):
    """The float64 oracle with the graph's weights and tau through the diagonal identity, on the graph with the row of BEYOND (its
    first rows are the other graph's): [rows, HAS_MASS + S F] with bias and out_scale."""
    c, x = graph_case(mode, True), inputs(S, F, freqs)
    X = x["Xp"][:, :S].astype(np.float64)
    V = np.repeat(np.eye(S), F, axis=0)
    emb, mass = O.fsw_embed_csr(X, c["rowptr"], c["col"], c["w64"], V, np.tile(x["fr"].astype(np.float64), S),
                                total_mass_pad_thresh=c["tau"], return_mass=True)
    ref = OUT_SCALE * (np.concatenate([mass[:, None], emb], axis=1) + x["bias"].astype(np.float64)[None, :])
    ref.setflags(write=False)
    return ref


def weighted_args(c, x, S, F, Xp, fr, scratch, dtype=0):
    """cart_args of tests/test_hip_cart_hub.py with the graph's weights (float64 storage: converted) and tau."""
    a = cart_args(c, x, S, F, Xp, fr, None, scratch, dtype=dtype)
    keep = None
    if c["graph"].w is not None:
        keep = c["graph"].w if dtype == 0 else c["graph"].w.double()
        a.w = keep.data_ptr()
    a.tau = c["tau"]
    return a, keep


def run_forward(c, S, F, scratch, freqs=FREQS):
    """(status, out) of fsw_embed_cart_f32; out pre-filled with NaN."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    x = inputs(S, F, freqs)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    Xp, fr, bias = t(x["Xp"]), t(x["fr"]), t(x["bias"])
    out = torch.full((len(c["degrees"]), HAS_MASS + S * F), float("nan"), device=DEV)
    a, _keep = weighted_args(c, x, S, F, Xp, fr, scratch)
    a.out, a.ldo, a.bias = out.data_ptr(), out.stride(0), bias.data_ptr()
    rc = L.fsw_embed_cart_f32(ctypes.byref(a), stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("S,F", SHAPES)
@pytest.mark.parametrize("mode", list(MODES))
def test_forward_without_scratch(mode, S, F):
    """fsw_embed_cart_f32 with scratch = NULL on general-weight rows of up to 16383 neighbours: status 0, every row (mass column
    included) within TOL of the float64 oracle.  Before these classes the call was refused (the generic kernel needs scratch)."""
    c = graph_case(mode, False)
    rc, out = run_forward(c, S, F, None)
    from fsw_gnn_amd import _lib
    assert rc == 0, _lib.lib().fsw_last_error().decode()
    check_rows(out, forward_reference(mode, S, F)[:len(DEGREES)], DEGREES, "weighted hub forward %s S %d F %d, no scratch" % (mode, S, F))


def test_boundary_row_stays_on_the_generic_kernel():
    """One row of 16384 neighbours: with a generic-sized scratch the call succeeds and the row matches; without scratch it is refused."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    S, F = SHAPES[0]
    c = graph_case("random", True)
    scratch = torch.empty(int(L.fsw_embed_cart_generic_scratch_bytes(BEYOND, 1)), dtype=torch.uint8, device=DEV)
    rc, out = run_forward(c, S, F, scratch)
    assert rc == 0, L.fsw_last_error().decode()
    check_rows(out, forward_reference("random", S, F), c["degrees"], "weighted hub forward with a row of %d" % BEYOND)
    rc, _ = run_forward(c, S, F, None)
    assert rc != 0


@pytest.mark.parametrize("S,F", SHAPES)
@pytest.mark.parametrize("mode", list(MODES))
def test_backward(mode, S, F):
    """fsw_embed_cart_backward_keys_f32 with the scratch of fsw_embed_cart_weighted_backward_scratch_bytes and with the smallest scratch
    that was valid before (fsw_embed_cart_generic_scratch_bytes(max_degree, 1)): bit-identical gkey, finite everywhere (gkey is
    pre-filled with NaN: neither the pad element nor the fill elements leave one); against the generic kernel with float64 storage per
    row <= F32_BOUND, per entry <= PER_ENTRY of the line maximum, gfreq <= F32_BOUND."""
    check_backward(mode, S, F)


def check_backward(mode, S, F, freqs=FREQS):
    """The body of test_backward at the frequencies freqs[:F]."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    c, x = graph_case(mode, False), inputs(S, F, freqs)
    nnz, nrows, rowptr = c["nnz"], len(DEGREES), c["rowptr"]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    g_host = x["g"][:nrows]

    # reference: the generic kernel, float64 storage, backward mode
    Xp64, fr64, g64 = t(x["Xp"], torch.float64), t(x["fr"], torch.float64), t(g_host, torch.float64)
    gkey_ref = torch.full((nnz, S), float("nan"), dtype=torch.float64, device=DEV)
    gf_ref = torch.zeros(F, dtype=torch.float64, device=DEV)
    gscratch = torch.empty(int(L.fsw_embed_cart_generic_scratch_bytes(max(DEGREES), nrows)), dtype=torch.uint8, device=DEV)
    a, _keep = weighted_args(c, x, S, F, Xp64, fr64, gscratch, dtype=1)
    a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g64.data_ptr(), g64.stride(0), gkey_ref.data_ptr(), S, gf_ref.data_ptr()
    _lib.check(L.fsw_embed_cart_generic(ctypes.byref(a), stream), "fsw_embed_cart_generic (backward, float64)")

    Xp, fr, g = t(x["Xp"]), t(x["fr"]), t(g_host)
    line = 12 * 16384                                               # the longest line: 16383 neighbours + the pad element
    sizes = {"new size function": int(L.fsw_embed_cart_weighted_backward_scratch_bytes(max(DEGREES), 9, S)),
             "smallest valid before": int(L.fsw_embed_cart_generic_scratch_bytes(max(DEGREES), 1))}
    assert sizes["new size function"] == 9 * S * line and sizes["smallest valid before"] >= line
    got = {}
    for name, nbytes in sizes.items():
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        gkey = torch.full((nnz, S), float("nan"), device=DEV)
        gf = torch.zeros(F, device=DEV)
        a, _keep = weighted_args(c, x, S, F, Xp, fr, scratch)
        a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g.data_ptr(), g.stride(0), gkey.data_ptr(), S, gf.data_ptr()
        _lib.check(L.fsw_embed_cart_backward_keys_f32(ctypes.byref(a), None, 0, stream), "fsw_embed_cart_backward_keys_f32")
        torch.cuda.synchronize()
        got[name] = (gkey.cpu().numpy(), gf.cpu().numpy())
    (k_new, f_new), (k_old, f_old) = got["new size function"], got["smallest valid before"]
    assert np.isfinite(k_new).all() and np.isfinite(k_old).all() and np.array_equal(k_new, k_old)

    ref = gkey_ref.cpu().numpy()
    assert np.isfinite(ref).all()
    G = OUT_SCALE * g_host[:, HAS_MASS:].astype(np.float64)
    scale = coefficient_scale(G, np.tile(x["fr"].astype(np.float64), S)).reshape(nrows, S, F).sum(axis=2)
    what = "weighted hub backward %s S %d F %d" % (mode, S, F)
    check_key_gradients(k_new.astype(np.float64), ref, rowptr, list(x["kinds"]), what, scale, row_bound=F32_BOUND, entry_bound=PER_ENTRY)
    for name, gf in (("new size function", f_new), ("smallest valid before", f_old)):
        e = relerr(gf, gf_ref.cpu().numpy())
        print("%s, %s: gfreq %.2e" % (what, name, e))
        assert np.isfinite(gf).all() and e <= F32_BOUND, (what, name, e)


# ---- module level -------------------------------------------------------------------------------------------------------------------
MODULE_FWD, MODULE_GRAD = 1e-5, 3e-5       # FWD_BOUND and F32_BOUND of tests/test_hip_cartesian_conv.py


def test_embedding_module_on_weighted_point_clouds():
    """FSW_embedding(d_in=3, nSlices=4, nFreqs=8) on two clouds of 3000 points with random positive weights: the float32 module (tuned
    kernels, _CartEmbedFn) against the float64 module (generic kernel) with the same state: output <= 1e-5, gradients of X, projVecs
    and freqs <= 3e-5; the forward allocates no scratch."""
    from fsw_gnn_amd import FSW_embedding, build_csr
    from tests.test_hip_cartesian_train import autograd_functions
    B, n, d, S, F = 2, 3000, 3, 4, 8
    torch.manual_seed(91)
    ref = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV, dtype=torch.float64)
    low = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV, dtype=torch.float32)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    rng = np.random.default_rng(92)
    X = t(rng.standard_normal((B, n, d)), torch.float64)
    W = t(rng.uniform(0.05, 1.0, size=(B, n)), torch.float64)
    G = t(rng.standard_normal((B, S, F)), torch.float64)

    graph = build_csr(torch.arange(B, device=DEV).repeat_interleave(n), torch.arange(B * n, device=DEV), W.float().reshape(-1).contiguous(),
                      B, B * n)
    from fsw_gnn_amd import _lib
    assert graph.w is not None and graph.read_stats()[_lib.STAT_MAX_DEGREE] == n
    assert low.prepare_cartesian(X.float().reshape(B * n, d).contiguous(), graph)["scratch"] is None

    def grads(E, dt):
        E.zero_grad(set_to_none=True)
        Xl = X.to(dt).clone().requires_grad_(True)
        out = E(Xl, W.to(dt))
        names = autograd_functions(out)
        (out * G.to(dt).reshape(out.shape)).sum().backward()
        return {"out": out.detach(), "gX": Xl.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad}, names

    want, _ = grads(ref, torch.float64)
    got, names = grads(low, torch.float32)
    assert "_CartEmbedFnBackward" in names
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("weighted point clouds of %d points, float32 vs float64 module:" % n, {k: "%.2e" % e for k, e in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs


def test_conv_gcn_with_self_loops_on_hub_rows():
    """FSW_conv(5, 8, embed_slices=4, embed_freqs=8, edge_weighting='gcn', self_loop_weight=1.0) on a graph with recipients of 40, 2100
    and 5000 neighbours: float32 against the float64 layer with the same state, forward <= 1e-5, gradients <= 3e-5."""
    from fsw_gnn_amd import FSW_conv
    from tests.test_hip_cartesian_conv import _loss_grads, features, make_pair
    from tests.test_hip_cartesian_conv import relerr as rel
    S, F, in_ch, out_ch = 4, 8, 5, 8
    degs = [3] * 5997 + [40, 2100, 5000]
    n = len(degs)
    rng = np.random.default_rng(93)
    src = np.concatenate([rng.choice(n, size=d, replace=False) for d in degs])     # every node receives something
    dst = np.repeat(np.arange(n), degs)
    ei = torch.from_numpy(np.stack([src, dst])).to(DEV)
    ref, low = make_pair(FSW_conv, in_ch, out_ch, S, F, mlp_layers=2, edge_weighting="gcn", self_loop_weight=1.0)
    x64, G = features(n, in_ch), features(n, out_ch, seed=37)
    want_y, want = _loss_grads(ref, x64, G, ei)
    got_y, got = _loss_grads(low, x64.float(), G, ei)
    assert set(got) == set(want) and {"fsw_embed.projVecs", "fsw_embed.freqs", "mlp.0.weight"} <= set(got)
    errs = {"out": rel(got_y, want_y), **{k: rel(got[k], want[k]) for k in want}}
    print("conv gcn + self loops with hub rows, float32 vs float64:", errs)
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs
