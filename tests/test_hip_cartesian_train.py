"""Float32 training of Cartesian mode on the tuned backward kernels (csrc/embed_cart_bwd.hip, _CartEmbedFn).

The yardsticks are the reference (float64 fixtures, tests/golden/grads_cartesian_graph.npz and grads_cartesian.npz) and the generic
Cartesian kernel, which test_float64_module_against_reference_on_the_graph pins to the reference in every degree class.  The tuned
kernels are never compared with themselves: a W that requires grad selects the generic path, a constant W the tuned one."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fsw_gnn_amd import FSW_embedding, _lib
from fsw_gnn_amd.graph import build_csr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")
F32_BOUND = 3e-5      # the project's float32-against-float64 bound for these gradients (test_hip_cartesian.py)


def load_cases(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cases = {}
    for key in z.files:
        case, field = key.split("/")
        cases.setdefault(case, {})[field] = z[key]
    return cases


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def graph_cases():
    cases = load_cases("grads_cartesian_graph")
    gr = cases.pop("graph")
    return gr, cases


def make_module(c, dt, collapse=None, method="plain", fn=None, mass=None, bias=None, learn=True, d_in=None):
    S, F = c["V"].shape[0], c["freqs"].shape[0]
    mass = bool(c["mass"]) if mass is None else mass
    E = FSW_embedding(d_in=c["V"].shape[1] if d_in is None else d_in, nSlices=S, nFreqs=F,
                      collapse_freqs=bool(c["collapse"]) if collapse is None else collapse, encode_total_mass=mass,
                      total_mass_encoding_method=method, total_mass_encoding_function=str(c["fn"]) if fn is None else fn,
                      total_mass_encoding_scale=float(c["scale"]), enable_bias=("bias" in c) if bias is None else bias,
                      learnable_slices=learn, learnable_freqs=learn, learnable_total_mass_encoding_scale=learn and mass,
                      device=DEV, dtype=dt)
    with torch.no_grad():
        E.projVecs.copy_(torch.from_numpy(c["V"]))
        E.freqs.copy_(torch.from_numpy(c["freqs"]))
        if E.enable_bias:
            if "bias" in c and c["bias"].size == E.bias.numel():
                E.bias.copy_(torch.from_numpy(c["bias"]).reshape(E.bias.shape))
            else:
                E.bias.copy_(torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(E.bias.shape)) * 0.1))
    return E


def dense_w(gr, vals, dt, nrec=12):
    W = torch.zeros((nrec, gr["X"].shape[0]), dtype=dt, device=DEV)
    W[torch.from_numpy(gr["rows"]).long().to(DEV), torch.from_numpy(gr["cols"]).long().to(DEV)] = torch.from_numpy(vals).to(dt).to(DEV)
    return W


def autograd_functions(out):
    """Names of the autograd nodes below `out`: tells which embedding Function a forward took."""
    seen, stack, names = set(), [out.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack += [nf for nf, _ in fn.next_functions]
    return names


def run_grads(E, X, W, G, graph_mode=False, w_grad=False, x_grad=True):
    """out and the gradients of sum(out * G) as float64 numpy arrays; w_grad: W is a leaf that requires grad (the generic path)."""
    E.zero_grad(set_to_none=True)
    Xl = X.detach().clone().requires_grad_(x_grad)
    Wl = W.detach().clone().requires_grad_(True) if w_grad else W
    out = E(Xl, Wl, graph_mode=graph_mode)
    names = autograd_functions(out)
    (out * G.to(out.dtype).reshape(out.shape)).sum().backward()
    g = {"out": out.detach()}
    if x_grad:
        g["gX"] = Xl.grad
    for key, p in (("gV", E.projVecs), ("gfreqs", E.freqs), ("gbias", E.bias if E.enable_bias else None),
                   ("gscale", E.total_mass_encoding_scale if E.encode_total_mass else None)):
        if p is not None and p.requires_grad:
            g[key] = p.grad
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in g.items()}, names


def assert_close(got, want, bound, what):
    assert set(got) == set(want), what
    errs = {k: relerr(got[k], want[k]) for k in want}
    print(what, {k: "%.2e" % e for k, e in errs.items()})
    for k, e in errs.items():
        assert got[k].shape == want[k].shape and e <= bound, (what, k, e)


# ---- 1. anchor: the generic kernel (float64 module) against the reference in every degree class ------------------------------
def test_float64_module_against_reference_on_the_graph():
    """Norm-wise relative error per gradient <= 1e-10, the bound of test_gradients_float64_against_reference, now on rows of
    0 .. 4500 neighbours (zero, register, wavefront and longer-line classes of the tuned kernels)."""
    gr, cases = graph_cases()
    X = torch.from_numpy(gr["X"]).to(DEV)
    for name, c in cases.items():
        E = make_module(c, torch.float64)
        W = dense_w(gr, np.ones_like(gr["vals"]) if bool(c["unit"]) else gr["vals"], torch.float64)
        g, names = run_grads(E, X, W, torch.from_numpy(c["G"]).to(DEV), graph_mode=True)
        assert "_GenericEmbedFnBackward" in names
        want = {k: c[k] for k in ("out", "gX", "gV", "gfreqs", "gbias", "gscale") if k in c}
        assert_close(g, want, 1e-10, "float64 vs reference, " + name)


# ---- 2. kernel level: fsw_embed_cart_backward_keys_f32 against fsw_embed_cart_generic (backward, float32 storage) --------------
KERNEL_DEGREES = (0, 1, 2, 31, 32, 33, 64, 65, 128, 129, 2047, 2048, 2049)
KERNEL_SENDERS = 3000


def kernel_graph(weights):
    """build_csr graph with one recipient per degree; recipient 5 (33 neighbours) holds the same sender twice (exactly tied keys)."""
    rng = np.random.default_rng(11)
    rec, snd = [], []
    for r, deg in enumerate(KERNEL_DEGREES):
        s = rng.choice(KERNEL_SENDERS, size=deg, replace=False)
        if deg == 33:
            s[20] = s[3]
        rec.append(np.full(deg, r))
        snd.append(s)
    rec, snd = np.concatenate(rec).astype(np.int64), np.concatenate(snd).astype(np.int64)
    w = None
    if weights == "random":
        w = rng.uniform(0.05, 1.0, size=rec.size).astype(np.float32)
        w[np.nonzero(rec == 6)[0][10]] = 0.0                     # one zero weight (a row of 64 neighbours)
        low = rec == 3
        w[low] *= np.float32(0.4) / w[low].sum()                 # total mass of the row of 31 neighbours below tau = 1
    graph = build_csr(torch.from_numpy(rec).to(DEV), torch.from_numpy(snd).to(DEV), torch.from_numpy(w).to(DEV) if w is not None else None,
                      len(KERNEL_DEGREES), KERNEL_SENDERS)
    graph.read_stats()
    return graph


@pytest.mark.parametrize("S,F", [(3, 5), (16, 16), (2, 70)])
@pytest.mark.parametrize("weights,tau", [("unit", 1.0), ("random", 1.0), ("unit", 3.0)])
def test_backward_kernels_against_generic_kernel(weights, tau, S, F):
    """gkey per recipient row and gfreq, norm-wise <= 3e-5, on the same Xp, g and frequencies (one of them 0)."""
    L = _lib.lib()
    graph = kernel_graph(weights)
    st = graph.stats()
    nnz, nrec = st[_lib.STAT_NNZ], len(KERNEL_DEGREES)
    rowptr = graph.rowptr.cpu().numpy()
    assert tuple(np.diff(rowptr)) == KERNEL_DEGREES
    rng = np.random.default_rng(12 + S)
    ldp = (S + 31) // 32 * 32
    Xp = torch.from_numpy(rng.standard_normal((KERNEL_SENDERS, ldp)).astype(np.float32)).to(DEV)
    fr = np.sort(rng.uniform(0.0, 4.0, size=F)).astype(np.float32)
    fr[0] = 0.0
    fr = torch.from_numpy(fr).to(DEV)
    has_mass, out_scale = 1, 0.7
    g = torch.from_numpy(rng.standard_normal((nrec, has_mass + S * F)).astype(np.float32)).to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    scratch = torch.empty(int(L.fsw_embed_cart_generic_scratch_bytes(st[_lib.STAT_MAX_DEGREE], nrec)), dtype=torch.uint8, device=DEV)

    def args(gkey, gfreq):
        a = _lib.CartArgs()
        a.value_dtype, a.S, a.F, a.has_mass = 0, S, F, has_mass
        a.rowptr, a.col, a.w = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.w.data_ptr() if graph.w is not None else None
        a.num_rows, a.max_degree = nrec, st[_lib.STAT_MAX_DEGREE]
        a.Xp, a.ldp, a.freqs, a.tau, a.out_scale = Xp.data_ptr(), ldp, fr.data_ptr(), tau, out_scale
        a.mass_fn, a.mass_scale = 0, 1.0
        a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g.data_ptr(), g.stride(0), gkey.data_ptr(), S, gfreq.data_ptr()
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        return a

    gkey_ref = torch.zeros((nnz, S), device=DEV)
    gf_ref = torch.zeros(F, device=DEV)
    _lib.check(L.fsw_embed_cart_generic(ctypes.byref(args(gkey_ref, gf_ref)), stream), "fsw_embed_cart_generic (backward)")

    gkey = torch.full((nnz, S), float("nan"), device=DEV)       # every entry must be stored
    gf = torch.zeros(F, device=DEV)
    a = args(gkey, gf)
    a.perm, a.bin_start, a.bin_start_host = graph.perm.data_ptr(), graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data
    table = dtable = None
    if weights == "unit" and tau <= 1.0:
        table = torch.empty((int(L.fsw_unit_table_rows(_lib.REG_MAX_DEG)), F), device=DEV)
        dtable = torch.empty_like(table)
        _lib.check(L.fsw_unit_coeff_table(_lib.ptr(fr), F, _lib.REG_MAX_DEG, _lib.ptr(table), F, stream), "fsw_unit_coeff_table")
        _lib.check(L.fsw_unit_dcoeff_table(_lib.ptr(fr), F, _lib.REG_MAX_DEG, _lib.ptr(dtable), F, stream), "fsw_unit_dcoeff_table")
        a.unit_table, a.ldt = table.data_ptr(), F
    _lib.check(L.fsw_embed_cart_backward_keys_f32(ctypes.byref(a), _lib.ptr(dtable), F, stream), "fsw_embed_cart_backward_keys_f32")
    torch.cuda.synchronize()

    got, ref = gkey.cpu().numpy(), gkey_ref.cpu().numpy()
    assert np.isfinite(got).all()
    errs = [relerr(got[rowptr[r]:rowptr[r + 1]], ref[rowptr[r]:rowptr[r + 1]]) for r in range(nrec) if rowptr[r + 1] > rowptr[r]]
    ef = relerr(gf.cpu().numpy(), gf_ref.cpu().numpy())
    print("weights %s tau %g S %d F %d: max gkey row error %.2e, gfreq error %.2e" % (weights, tau, S, F, max(errs), ef))
    assert max(errs) <= F32_BOUND, dict(zip([d for d in KERNEL_DEGREES if d], errs))
    assert ef <= F32_BOUND


# ---- 3. module level: the tuned path (W constant) against the generic path (the same W, requiring grad) -----------------------
def tuned_vs_generic(E, X, W, G, graph_mode, tuned_W=None, what=""):
    """tuned_W: what the tuned call passes for W when it is not the tensor itself ('unit' for a W of ones)."""
    got, names = run_grads(E, X, W if tuned_W is None else tuned_W, G, graph_mode=graph_mode)
    assert "_CartEmbedFnBackward" in names and "_GenericEmbedFnBackward" not in names, names
    want, names = run_grads(E, X, W, G, graph_mode=graph_mode, w_grad=True)
    assert "_GenericEmbedFnBackward" in names and "_CartEmbedFnBackward" not in names, names
    assert_close(got, want, F32_BOUND, what)


@pytest.mark.parametrize("case,collapse,mass", [("unit_bias", True, False), ("weighted_mass", True, True), ("weighted_mass", False, False),
                                                ("unit_bias", True, True)])
def test_module_on_the_fixture_graph(case, collapse, mass):
    gr, cases = graph_cases()
    c = cases[case]
    E = make_module(c, torch.float32, collapse=collapse, mass=mass, bias=True)
    X = torch.from_numpy(gr["X"]).float().to(DEV)
    W = dense_w(gr, np.ones_like(gr["vals"]) if bool(c["unit"]) else gr["vals"], torch.float32)
    G = torch.from_numpy(np.random.default_rng(21).standard_normal((12, E.d_out))).to(DEV)
    tuned_vs_generic(E, X, W, G, True, what="graph %s collapse %s mass %s" % (case, collapse, mass))


@pytest.mark.parametrize("case", ["unit_bias", "weighted_collapsed_bias", "weighted_mass"])
def test_module_on_the_point_clouds(case):
    c = load_cases("grads_cartesian")[case]
    E = make_module(c, torch.float32)
    X = torch.from_numpy(c["X"]).float().to(DEV)
    G = torch.from_numpy(c["G"]).to(DEV)
    if "W" in c:
        tuned_vs_generic(E, X, torch.from_numpy(c["W"]).float().to(DEV), G, False, what="point clouds " + case)
    else:       # unit weights: the tuned call takes W = 'unit' (the unit-weight kernels), the generic one a tensor of ones
        tuned_vs_generic(E, X, torch.ones(X.shape[:-1], device=DEV), G, False, tuned_W="unit", what="point clouds " + case)


@pytest.mark.parametrize("method,fn", [("homog", "sqrt"), ("homog_alt", "log")])
def test_homog_methods_against_float64_module(method, fn):
    c = load_cases("grads_cartesian")["weighted_mass"]
    X, W, G = (torch.from_numpy(c[k]).to(DEV) for k in ("X", "W", "G"))
    res = {}
    for dt in (torch.float64, torch.float32):
        E = make_module(c, dt, method=method, fn=fn, bias=True)
        res[dt], names = run_grads(E, X.to(dt), W.to(dt), G)
        assert ("_CartEmbedFnBackward" if dt == torch.float32 else "_GenericEmbedFnBackward") in names
    assert "gbias" in res[torch.float32] and "gscale" in res[torch.float32]
    assert_close(res[torch.float32], res[torch.float64], F32_BOUND, "%s / %s vs float64" % (method, fn))


def test_sparse_w_equals_dense_w_under_autograd():
    gr, cases = graph_cases()
    c = cases["weighted_mass"]
    E = make_module(c, torch.float32)
    X = torch.from_numpy(gr["X"]).float().to(DEV)
    Wd = dense_w(gr, gr["vals"], torch.float32)
    G = torch.from_numpy(c["G"]).to(DEV)
    a, names = run_grads(E, X, Wd, G, graph_mode=True)
    b, names_b = run_grads(E, X, Wd.to_sparse().coalesce(), G, graph_mode=True)
    assert "_CartEmbedFnBackward" in names and "_CartEmbedFnBackward" in names_b
    # the same CSR graph either way: identical arithmetic, except that float atomics add in arrival order into gfreqs (the
    # kernels) and into the total masses behind gscale (index_add_) -- those two within the float32 bound
    for k in a:
        if k in ("gfreqs", "gscale"):
            assert relerr(a[k], b[k]) <= F32_BOUND, k
        else:
            assert np.array_equal(a[k], b[k]), k


def test_only_x_requires_grad():
    gr, cases = graph_cases()
    c = cases["unit_bias"]
    E = make_module(c, torch.float32, learn=False)
    assert not any(p.requires_grad for p in E.parameters())
    X = torch.from_numpy(gr["X"]).float().to(DEV)
    W = dense_w(gr, gr["vals"], torch.float32)
    G = torch.from_numpy(c["G"]).to(DEV)
    got, names = run_grads(E, X, W, G, graph_mode=True)
    assert "_CartEmbedFnBackward" in names and set(got) == {"out", "gX"}
    want, names = run_grads(E, X, W, G, graph_mode=True, w_grad=True)
    assert "_GenericEmbedFnBackward" in names
    assert_close(got, want, F32_BOUND, "only X requires grad")
    # and the no_grad forward is the same tuned forward
    with torch.no_grad():
        assert np.array_equal(E(X, W, graph_mode=True).cpu().numpy().astype(np.float64), got["out"])


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------
def test_graph_without_entries_gives_zero_gradients_and_the_bias_gradient():
    E = FSW_embedding(d_in=4, nSlices=3, nFreqs=5, collapse_freqs=True, encode_total_mass=True, learnable_slices=True,
                      learnable_freqs=True, learnable_total_mass_encoding_scale=True, device=DEV)
    with torch.no_grad():
        E.bias.normal_()
    X = torch.randn(6, 4, device=DEV)
    W = torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.int64, device=DEV), torch.zeros(0, device=DEV), (7, 6)).coalesce()
    G = torch.randn(7, 16, device=DEV)
    g, names = run_grads(E, X, W, G, graph_mode=True)
    assert "_CartEmbedFnBackward" in names
    assert np.array_equal(g["out"], np.broadcast_to(E.bias.detach().cpu().numpy().astype(np.float64), (7, 16)))
    assert not g["gX"].any() and not g["gV"].any() and not g["gfreqs"].any() and g["gscale"] == 0.0
    np.testing.assert_allclose(g["gbias"], G.sum(0).cpu().numpy(), rtol=1e-6, atol=1e-6)


def test_no_recipients():
    E = FSW_embedding(d_in=4, nSlices=3, nFreqs=5, learnable_slices=True, learnable_freqs=True, device=DEV)
    X = torch.randn(0, 9, 4, device=DEV, requires_grad=True)
    out = E(X)
    assert tuple(out.shape) == (0, 3, 5)
    W = torch.zeros((0, 6), device=DEV)
    out = E(torch.randn(6, 4, device=DEV, requires_grad=True), W, graph_mode=True)
    assert tuple(out.shape) == (0, 3, 5)


def test_two_backward_passes_are_bit_identical():
    """Store-and-sum: senders of at most 256 out-edges (one segment of fsw_segment_sum_rows_f32, or two partial sums that commute)
    get bitwise reproducible key-gradient sums, hence gX and gV."""
    rng = np.random.default_rng(31)
    m, d, S, F = 20000, 7, 8, 6
    rec = torch.from_numpy(rng.integers(0, m, size=200000)).to(DEV)
    snd = torch.from_numpy(rng.integers(0, m, size=200000)).to(DEV)
    assert int(torch.bincount(snd, minlength=m).max()) <= 256
    order = torch.argsort(rec * m + snd)
    idx = torch.stack([rec[order], snd[order]])
    W = torch.sparse_coo_tensor(idx, torch.from_numpy(rng.uniform(0.1, 1.0, size=200000).astype(np.float32)).to(DEV), (m, m)).coalesce()
    X = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(DEV)
    G = torch.from_numpy(rng.standard_normal((m, S * F)).astype(np.float32)).to(DEV)
    E = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, collapse_freqs=True, learnable_slices=True, learnable_freqs=True, device=DEV)
    runs = []
    for _ in range(2):
        g, names = run_grads(E, X, W, G, graph_mode=True)
        assert "_CartEmbedFnBackward" in names
        runs.append(g)
    assert np.array_equal(runs[0]["gX"], runs[1]["gX"]) and np.array_equal(runs[0]["gV"], runs[1]["gV"])
    assert runs[0]["gX"].any() and runs[0]["gV"].any()
