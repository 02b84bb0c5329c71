"""The public layers on strided, offset, expanded and sliced arguments (tests/layout_cases.py), one argument at a time and all at once.

Per call: the contiguous control lies within the project's bounds of the float64 oracle (oracle/fsw_oracle.py: forward TOL = 1e-5
norm-wise and 2e-5 * max|ref| per entry, float32 gradients F32_BOUND = 3e-5, float64 1e-10); it is run twice; a layout the layer has
to copy must then reproduce every result that was bit-identical between the two control runs BIT FOR BIT, and meet the control's
oracle bound for the others.  The results that are not reproducible run to run are gradients accumulated by float atomics: dL/dfreqs
of every call, dL/dX and dL/dprojVecs of the calls that take the atomic backward (general weights, Cartesian mode, the generic
kernels, store_sum_backward_max_bytes = 0) and what GEMMs make of them; and dL/d(total-mass scale) with general weights, whose row
masses torch's index_add_ sums by float atomics.  The last is a scalar and dL/dfreqs a handful of numbers, which two runs can round
alike by chance: both are ALWAYS held to the oracle bound (ATOMIC_BY_DESIGN), never to the two-run check.  The forward is always
reproducible and must be.  'offset1' / 'oddslice' (contiguous, no
copy, pointer off 16-byte alignment: the kernels' scalar paths) meet the oracle bounds; their largest difference from the aligned
call is printed (DESIGN.md "Call conditions").  In every case: results finite, nothing outside the view written (the poisoned base
is bit-identical afterwards), and with base.requires_grad the gradient lands on the view's elements of base.grad and is exactly 0
elsewhere ('expanded': the sum over the batch of the control's gradient)."""
import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests import cases, layout_cases as LC
from tests.conftest import relerr

pytestmark = pytest.mark.gpu
TOL, ENTRY, F32_BOUND, F64_BOUND = 1e-5, 2e-5, 3e-5, 1e-10
N, DE = LC.N_VERT, LC.D_EDGE
S_DIAG, S_CART, F_CART = 24, 4, 8
ATOMIC_BY_DESIGN = ("g_scale", "g_freqs")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


# ---- modules with fixed parameters ---------------------------------------------------------------------------------------------
def embedding(dev, d, cart=False, dtype=torch.float32, d_edge=0, learn=True):
    from fsw_gnn_amd import FSW_embedding
    size = dict(nSlices=S_CART, nFreqs=F_CART, collapse_freqs=True) if cart else dict(d_out=S_DIAG + 1)
    E = FSW_embedding(d_in=d, d_edge=d_edge, encode_total_mass=True, total_mass_encoding_scale=0.7, learnable_slices=learn,
                      learnable_freqs=learn, learnable_total_mass_encoding_scale=learn, cartesian_edge_features=cart and d_edge > 0,
                      device=dev, dtype=dtype, **size)
    S = E.nSlices
    with torch.no_grad():
        E.projVecs.copy_(t(cases.synth.unit_slices(S, d + d_edge, seed=81 + d), dev))
        E.freqs.copy_(t(cases.random_freqs(E.nFreqs, seed=82), dev))
        E.bias.copy_(t(0.1 * cases.synth.normal(83, 1, tuple(E.bias.shape)), dev))
    return E


def conv_layer(dev, d, cls=None, **kw):
    from fsw_gnn_amd import FSW_conv
    cart = "embed_slices" in kw
    C = (cls or FSW_conv)(d, 16, embed_dim=None if cart else S_DIAG + 1, device=dev, **kw)
    E = C.fsw_embed
    with torch.no_grad():
        E.projVecs.copy_(t(cases.synth.unit_slices(E.nSlices, d + E.d_edge, seed=84 + d), dev))
        E.freqs.copy_(t(cases.random_freqs(E.nFreqs, seed=85), dev))
    return C


def params_of(E):
    return {"projVecs": E.projVecs, "freqs": E.freqs, "bias": E.bias, "scale": E.total_mass_encoding_scale}


def f64(p):
    return p.detach().cpu().numpy().astype(np.float64)


def weights_for(shape, seed=7):
    return np.random.default_rng(seed).standard_normal(shape)


def hip_projection(E, X):
    """float32 X . projVecs[:, :d_in]^T of the path under test: decides the sort order in the oracle's backward."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    Xc = X.detach().contiguous()
    n, S, V = Xc.shape[0], E.nSlices, E.projVecs.detach()
    Xp = torch.empty((n, (S + 63) // 64 * 64), dtype=torch.float32, device=Xc.device)
    _lib.check(L.fsw_project_f32(Xc.data_ptr(), n, E.d_in, Xc.stride(0), V.data_ptr(), S, V.stride(0), Xp.data_ptr(), Xp.stride(0), None,
                                 0, None, torch.cuda.current_stream(Xc.device).cuda_stream), "project")
    return Xp[:, :S].cpu().numpy().astype(np.float64)


def float32_keys(xp, ef, Ve):
    """The edge-feature kernels' float32 chain key = Xp[col]; key += ef[q] * Ve[k, q], q ascending (tests/edge_feature_cases.py)."""
    key = xp.astype(np.float32).copy()
    for q in range(ef.shape[1]):
        key = (key + (ef[:, q].astype(np.float32)[:, None] * Ve[:, q].astype(np.float32)[None, :]).astype(np.float32)).astype(np.float32)
    return key


def embedding_refs(E, X, rowptr, col, w, R=None, ef=None, dev=None, gX_shape=None):
    """Oracle output (and with R the gradients of sum(out * R)) of an FSW_embedding with the total-mass column, 'plain' / 'identity'.
    Cartesian mode is the diagonal oracle on every slice repeated nFreqs times against the frequencies tiled nSlices times."""
    V, fr, bias, scale = f64(E.projVecs), f64(E.freqs), f64(E.bias).reshape(-1), float(f64(E.total_mass_encoding_scale))
    S, F, cart = E.nSlices, E.nFreqs, E.cartesian_mode
    Vr, frr = (np.repeat(V, F, axis=0), np.tile(fr, S)) if cart else (V, fr)
    X = np.asarray(X, dtype=np.float64)
    w = np.ones(col.size) if w is None else np.asarray(w, dtype=np.float64)
    ef64 = None if ef is None else np.asarray(ef, dtype=np.float64)
    refs = {"out": O.fsw_embedding_forward(X, rowptr, col, w, Vr, frr, bias=bias, encode_total_mass=True, total_mass_encoding_scale=scale,
                                           edge_feat=ef64)}
    if R is None:
        return refs
    over = {}
    if E.get_dtype() == torch.float32:
        xp = hip_projection(E, t(X, dev, torch.float32))
        xp = np.repeat(xp, F, axis=1) if cart else xp
        if ef is None:
            over["Xp_override"] = xp
        else:
            over["keys_override"] = float32_keys(xp[col], np.asarray(ef), Vr[:, E.d_in:])
    res = O.fsw_embed_csr_backward(X, rowptr, col, w, Vr, frr, R[:, 1:], edge_feat=ef64, **over)
    gX, gV, gxi = res[:3]
    if cart:
        gV, gxi = gV.reshape(S, F, -1).sum(1), gxi.reshape(S, F).sum(0)
    mass = np.zeros(rowptr.size - 1)
    np.add.at(mass, np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr)), w)
    refs.update({"g_X": gX.reshape(gX_shape or gX.shape), "g_projVecs": gV, "g_freqs": gxi, "g_bias": R.sum(0).reshape(tuple(E.bias.shape)),
                 "g_scale": np.asarray((R[:, 0] * mass).sum())})
    if ef is not None:
        refs["g_ef"] = res[3]
    return refs


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def check_ref(name, got, ref, dtype, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
    assert bool(np.isfinite(got).all()), (what, name, "not finite")
    e = relerr(got, ref)
    if dtype == torch.float64:
        assert e <= F64_BOUND, (what, name, e)
    elif name == "out":
        worst = float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-30)
        assert e <= TOL and worst <= ENTRY, (what, name, e, worst)
    else:
        assert e <= F32_BOUND, (what, name, e)
    return e


class Sweep:
    """One call of a layer: `call(tensors)` -> output tensor, on arguments `args` {name: key of layout_cases.arguments()};
    params {name: Parameter} and grad_args (argument names) are differentiated when R (the weights of the loss sum(out * R)) is given.
    refs(control) -> the oracle's {"out", "g_<param>", "g_<arg>"} (the control's results decide what float32 rounding may decide: the
    side of a LeakyReLU kink); a result without a reference is compared with the control only."""

    def __init__(self, dev, what, call, args, refs, params=None, grad_args=(), R=None, dtype=torch.float32, fixed=None):
        self.dev, self.what, self.call, self.args, self.refs = dev, what, call, args, refs
        self.params, self.grad_args, self.R, self.dtype = params or {}, tuple(grad_args), R, dtype
        self.fixed = fixed or {}                   # argument -> layouts it takes in this call (default: all of its table entry)
        self.Rd = None if R is None else t(R, dev, dtype)

    def layouts(self, arg):
        return self.fixed.get(arg, LC.layouts(self.args[arg]))

    def run(self, choice):
        """Results of the call with argument a in layout choice.get(a, 'contig'); checks of the bases."""
        train = self.R is not None
        bases, views, host = {}, {}, {}
        for a, key in self.args.items():
            if choice.get(a) == "expanded":
                key = self.expanded_key(a)
            hb, hv = LC.case(key, choice.get(a, "contig"))
            bases[a], views[a] = LC.on_device(hb, hv, self.dev, requires_grad=train and a in self.grad_args)
            host[a] = (hb, hv)
            if choice.get(a) == "offset1":
                assert views[a].data_ptr() % 16 == hb.element_size() and views[a].is_contiguous()
            if choice.get(a) == "oddslice":
                assert views[a].data_ptr() % 16 == (LC.ODD_OFFSET * hb.element_size()) % 16 and views[a].is_contiguous()
        before = {a: LC.bits(b) for a, b in bases.items()}
        for p in self.params.values():
            p.grad = None
        with torch.set_grad_enabled(train):
            y = self.call(views)
            res = {"out": y.detach()}
            if train:
                (y * self.Rd.reshape(y.shape)).sum().backward()
                for name, p in self.params.items():
                    if p.requires_grad:
                        res["g_" + name] = p.grad.detach().clone()
        for a, b in bases.items():
            assert np.array_equal(LC.bits(b), before[a]), (self.what, choice, a, "the layer wrote outside or inside its input")
        if train:
            for a in self.grad_args:
                g = bases[a].grad
                assert g is not None and g.shape == bases[a].shape, (self.what, choice, a)
                hv = host[a][1]
                if choice.get(a) == "expanded":
                    res["gsum_" + a] = g.detach()
                    continue
                outside = LC.outside_mask(bases[a], views[a])
                assert bool((g[outside] == 0).all()), (self.what, choice, a, "gradient outside the view")
                res["g_" + a] = torch.as_strided(g.detach(), hv.shape, hv.stride(), hv.storage_offset()).contiguous()
        for k, v in res.items():
            assert bool(torch.isfinite(v).all()), (self.what, choice, k, "not finite")
        return res

    def expanded_key(self, arg):
        return {"Xb12": "x1_12", "Xb7": "x1_7", "Wb": "w1"}[self.args[arg]]

    def go(self):
        control, again = self.run({}), self.run({})
        repro = {k: torch.equal(control[k], again[k]) and k not in ATOMIC_BY_DESIGN for k in control}
        assert repro["out"], (self.what, "the forward is not reproducible run to run")
        refs = self.refs(control)
        errs = {k: check_ref(k, control[k].cpu().numpy(), refs[k], self.dtype, self.what + " control") for k in control if k in refs}
        assert "out" in errs
        print("%s: control vs oracle %s; not reproducible: %s" % (self.what, {k: "%.1e" % e for k, e in errs.items()},
                                                                  sorted(k for k, same in repro.items() if not same)))
        singles = [{a: lay} for a in self.args for lay in self.layouts(a) if lay != "contig"]
        every = {a: [lay for lay in self.layouts(a) if lay in LC.COPIED][:1] for a in self.args}
        singles.append({a: lays[0] for a, lays in every.items() if lays})
        for choice in singles:
            if "expanded" in choice.values():
                self.expanded(choice, repro, refs)
                continue
            res = self.run(choice)
            copied = all(lay in LC.COPIED for lay in choice.values())
            assert set(res) == set(control), (self.what, choice)
            for k in res:
                if copied and repro[k]:
                    assert torch.equal(res[k], control[k]), (self.what, choice, k, "differs from the contiguous call")
                elif k in refs:
                    check_ref(k, res[k].cpu().numpy(), refs[k], self.dtype, "%s %s" % (self.what, choice))
                else:
                    assert relerr(res[k].cpu().numpy(), control[k].cpu().numpy()) <= (F64_BOUND if self.dtype == torch.float64 else F32_BOUND)
            if not copied:
                d = float((res["out"].double() - control["out"].double()).abs().max())
                key = "%s %s" % (self.what, sorted(choice.items()))
                print("UNALIGNED %s: max |out - aligned out| = %.3e (max |out| = %.3e)" % (key, d, float(control["out"].abs().max())))

    def expanded(self, choice, repro, refs):
        """stride 0 on the batch axis: its own control (the element repeated, contiguous); the gradient of the one element is the sum
        over the batch of the control's gradient."""
        saved = dict(self.args)
        try:      # control on the repeated array, contiguous (layout_cases: "<key>_rep")
            self.args = {a: self.expanded_key(a) + "_rep" if choice.get(a) == "expanded" else key for a, key in saved.items()}
            control = self.run({})
        finally:
            self.args = saved
        res = self.run(choice)
        assert torch.equal(res["out"], control["out"]), (self.what, choice, "differs from the call on the repeated array")
        for k in res:
            if k.startswith("gsum_"):
                want = control["g_" + k[5:]].double().sum(0).cpu().numpy()
                assert relerr(res[k].cpu().numpy(), want) <= F32_BOUND, (self.what, choice, k)
            elif k != "out":
                assert relerr(res[k].cpu().numpy(), control[k].cpu().numpy()) <= F32_BOUND, (self.what, choice, k)


# ---- 1-4: FSW_embedding --------------------------------------------------------------------------------------------------------
def cloud_weights(kind, Wb):
    if kind == "unit":
        return None
    if kind == "uniform":
        return np.full(Wb.shape, 1.0 / Wb.shape[1])
    return Wb


@pytest.mark.parametrize("train", [False, True], ids=["no_grad", "autograd"])
@pytest.mark.parametrize("cart", [False, True], ids=["diagonal", "cartesian"])
@pytest.mark.parametrize("d", LC.D_INS)
@pytest.mark.parametrize("W", ["unit", "uniform", "dense"])
def test_embedding_point_clouds(dev, d, W, cart, train):
    """FSW_embedding.forward on B = 3 clouds of 300 points: X [3, 300, d] in every layout incl. 'batchslice' (reshape(B n, d) stays a
    view: the float32 diagonal no_grad path used to die here with a bare AssertionError) and 'expanded'; W 'unit', 'uniform', dense."""
    E = embedding(dev, d, cart)
    B, n = LC.CLOUDS, LC.CLOUD_POINTS
    args = {"X": "Xb%d" % d}
    if W == "dense":
        args["W"] = "Wb"
    rowptr, col = np.arange(B + 1, dtype=np.int64) * n, np.arange(B * n, dtype=np.int64)
    R = weights_for((B, E.d_out)) if train else None

    def refs(control):
        w = cloud_weights(W, LC.array("Wb"))
        return embedding_refs(E, LC.array(args["X"]).reshape(B * n, d), rowptr, col, None if w is None else w.reshape(-1), R, dev=dev,
                              gX_shape=(B, n, d))

    fixed = {"X": LC.layouts(args["X"]) + ("expanded",), "W": LC.layouts("Wb") + ("expanded",)}
    Sweep(dev, "clouds d=%d W=%s %s" % (d, W, "cart" if cart else "diag"), lambda v: E(v["X"], v["W"] if W == "dense" else W), args, refs,
          params_of(E), ("X",), R, fixed={a: fixed[a] for a in args}).go()


def sparse_W(kind, v, dev, dtype=torch.float32, ef=False):
    """The graph of layout_cases.graph() as a sparse W [N, N] (and X_edge [N, N, DE]) whose values / index tensors are the views."""
    g = LC.graph()
    if kind == "coo":
        idx = t(np.stack([g["rec"], g["col"]]), dev)
        W = torch.sparse_coo_tensor(idx, v["w"], (N, N), is_coalesced=True)
        Xe = torch.sparse_coo_tensor(idx, v["ef"], (N, N, DE), is_coalesced=True) if ef else None
    else:
        W = torch.sparse_csr_tensor(v["crow"], v["col"], v["w"], size=(N, N))
        Xe = torch.sparse_csr_tensor(v["crow"], v["col"], v["ef"], size=(N, N, DE)) if ef else None
    return W, Xe


@pytest.mark.parametrize("train", [False, True], ids=["no_grad", "autograd"])
@pytest.mark.parametrize("cart", [False, True], ids=["diagonal", "cartesian"])
@pytest.mark.parametrize("form", ["dense", "coo", "csr_i32", "csr_i64"])
@pytest.mark.parametrize("d", LC.D_INS)
def test_embedding_graph_mode(dev, d, form, cart, train):
    """graph_mode: X [2200, d] shared by the recipients; W dense [64, 2200] (the cut rows 0, 1, 2, 31, 32, 33, 256, 257, 2048, 2049 and
    54 short ones), coalesced COO [2200, 2200] whose values are a view, torch.sparse_csr with views as its three tensors."""
    E = embedding(dev, d, cart)
    g = LC.graph()
    args = {"X": "X%d" % d}
    if form == "dense":
        args["W"] = "Wdense"
        rows = LC.DENSE_ROWS
        nd = int(g["rowptr"][rows])
        rowptr, col, w = g["rowptr"][:rows + 1], g["col"][:nd], LC.array("wvals")[:nd]
        call = lambda v: E(v["X"], v["W"], graph_mode=True)
    else:
        rows, rowptr, col, w = N, g["rowptr"], g["col"], LC.array("wvals")
        args["w"] = "wvals"
        if form != "coo":
            args["crow"], args["col"] = "rowptr_" + form[4:], "col_" + form[4:]
        call = lambda v: E(v["X"], sparse_W("coo" if form == "coo" else "csr", v, dev)[0], graph_mode=True)
    R = weights_for((rows, E.d_out)) if train else None
    Sweep(dev, "graph d=%d W=%s %s" % (d, form, "cart" if cart else "diag"), call, args,
          lambda control: embedding_refs(E, LC.array(args["X"]), rowptr, col, w, R, dev=dev), params_of(E), ("X",), R).go()


def test_float64_module_on_the_generic_kernels(dev):
    """A float64 module (generic kernels): X [2200, 12] float64, dense W [64, 2200] float64 and a COO W with a view as its values."""
    E = embedding(dev, 12, dtype=torch.float64)
    g = LC.graph()
    rows = LC.DENSE_ROWS
    nd = int(g["rowptr"][rows])
    R = weights_for((rows, E.d_out))
    Sweep(dev, "float64 dense", lambda v: E(v["X"], v["W"], graph_mode=True), {"X": "X12_f64", "W": "Wdense_f64"},
          lambda control: embedding_refs(E, LC.array("X12_f64"), g["rowptr"][:rows + 1], g["col"][:nd], LC.array("wvals")[:nd], R, dev=dev),
          params_of(E), ("X",), R, dtype=torch.float64).go()
    R2 = weights_for((N, E.d_out))
    Sweep(dev, "float64 coo", lambda v: E(v["X"], sparse_W("coo", v, dev)[0], graph_mode=True), {"X": "X12_f64", "w": "wvals_f64"},
          lambda control: embedding_refs(E, LC.array("X12_f64"), g["rowptr"], g["col"], LC.array("wvals"), R2, dev=dev),
          params_of(E), ("X",), R2, dtype=torch.float64, fixed={"X": ("contig", "colslice")}).go()


def test_float32_weight_gradient_on_the_generic_kernels(dev):
    """float32 with W.requires_grad (generic kernels, dL/dW): W dense [64, 2200] a view of a leaf; dL/dW lands on the view's elements,
    the reference of dL/dW is tests/weight_grad_ref.py on the float32 projections of the path under test."""
    from tests import weight_grad_ref as WR
    E = embedding(dev, 12)
    g = LC.graph()
    rows = LC.DENSE_ROWS
    nd = int(g["rowptr"][rows])
    rowptr, col, w = g["rowptr"][:rows + 1], g["col"][:nd], LC.array("wvals")[:nd]
    R = weights_for((rows, E.d_out))

    def refs(control):
        refs = embedding_refs(E, LC.array("X12"), rowptr, col, w, R, dev=dev)
        keys = hip_projection(E, t(LC.array("X12"), dev))
        res = WR.weight_grad_reference(rowptr, col, w, keys, f64(E.freqs), 1.0, R, mass_fn="identity",
                                       mass_scale=float(f64(E.total_mass_encoding_scale)), per_slice=False)
        gW = np.zeros((rows, N))
        gW[g["rec"][:nd], col] = res["gW"]
        refs["g_W"] = gW
        return refs

    Sweep(dev, "float32 dL/dW", lambda v: E(v["X"], v["W"], graph_mode=True), {"X": "X12", "W": "Wdense"}, refs, params_of(E), ("X", "W"),
          R, fixed={"X": ("contig", "colslice")}).go()


# ---- 5: edge features ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True], ids=["no_grad", "autograd"])
@pytest.mark.parametrize("cart", [False, True], ids=["diagonal", "cartesian_edge_features"])
@pytest.mark.parametrize("form", ["dense", "coo", "csr_i32"])
def test_embedding_edge_features(dev, form, cart, train):
    """d_edge = 3: X_edge dense [64, 2200, 3] (views incl. 'batchslice'), sparse COO / CSR whose value tensors [nnz, 3] are views."""
    E = embedding(dev, 12, cart, d_edge=DE)
    g = LC.graph()
    ef_all = LC.array("efvals")
    if form == "dense":
        rows = LC.DENSE_ROWS
        nd = int(g["rowptr"][rows])
        rowptr, col, w, ef = g["rowptr"][:rows + 1], g["col"][:nd], LC.array("wvals")[:nd], ef_all[:nd]
        args = {"X": "X12", "W": "Wdense", "Xe": "Xedge_dense"}
        call = lambda v: E(v["X"], v["W"], v["Xe"], graph_mode=True)
        fixed = {"X": ("contig", "rowstep"), "W": ("contig", "colslice")}
    else:
        rows, rowptr, col, w, ef = N, g["rowptr"], g["col"], LC.array("wvals"), ef_all
        args = {"X": "X12", "w": "wvals", "ef": "efvals"}
        fixed = {"X": ("contig", "transposed"), "w": ("contig", "rowstep")}
        if form != "coo":
            args["crow"], args["col"] = "rowptr_i32", "col_i32"
            fixed.update({"crow": ("contig", "oddslice"), "col": ("contig", "rowstep")})
        call = lambda v: E(v["X"], *sparse_W("coo" if form == "coo" else "csr", v, dev, ef=True), graph_mode=True)
    R = weights_for((rows, E.d_out)) if train else None

    def refs(control):
        r = embedding_refs(E, LC.array("X12"), rowptr, col, w, R, ef=ef, dev=dev)
        r.pop("g_ef", None)
        return r

    Sweep(dev, "edge features %s %s" % (form, "cart" if cart else "diag"), call, args, refs, params_of(E), ("X",), R, fixed=fixed).go()


# ---- 6: FSW_conv ---------------------------------------------------------------------------------------------------------------
def conv_refs(C, X, ei, R=None, ef=None, dev=None, control=None):
    """Oracle of a float32 FSW_conv with one Linear + LeakyReLU(0.2) layer on cat(emb, x), and with R the gradients of sum(y * R)."""
    E = C.fsw_embed
    V, fr = f64(E.projVecs), f64(E.freqs)
    S, F, cart = E.nSlices, E.nFreqs, E.cartesian_mode
    Vr, frr = (np.repeat(V, F, axis=0), np.tile(fr, S)) if cart else (V, fr)
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    co = O.coalesce_edge_index(ei, n, float(C.self_loop_weight), C.edge_weighting, edge_features=ef)
    rowptr, col, w = co[:3]
    efc = co[4] if ef is not None else None
    emb = O.fsw_embedding_forward(X, rowptr, col, w, Vr, frr, encode_total_mass=True, edge_feat=efc)
    Wl, bl = f64(C.mlp[0].weight), f64(C.mlp[0].bias)
    h = np.concatenate([emb, X], axis=1)
    pre = h @ Wl.T + bl
    refs = {"out": np.where(pre >= 0, pre, 0.2 * pre)}
    if R is None:
        return refs
    gpre = R * np.where(control["out"].cpu().numpy() >= 0, 1.0, 0.2)       # the side of the kink the layer under test took
    gh = gpre @ Wl
    over = {}
    xp = hip_projection(E, t(X, dev, torch.float32))
    xp = np.repeat(xp, F, axis=1) if cart else xp
    if ef is None:
        over["Xp_override"] = xp
    else:
        over["keys_override"] = float32_keys(xp[col], efc, Vr[:, E.d_in:])
    res = O.fsw_embed_csr_backward(X, rowptr, col, w, Vr, frr, gh[:, 1:E.d_out], edge_feat=efc, **over)
    gX, gV, gxi = res[:3]
    if cart:
        gV, gxi = gV.reshape(S, F, -1).sum(1), gxi.reshape(S, F).sum(0)
    refs.update({"g_X": gX + gh[:, E.d_out:], "g_projVecs": gV, "g_freqs": gxi, "g_lin_w": gpre.T @ h, "g_lin_b": gpre.sum(0)})
    if ef is not None:
        refs["g_ef"] = res[3][co[5]]
    return refs


def conv_params(C):
    return {"projVecs": C.fsw_embed.projVecs, "freqs": C.fsw_embed.freqs, "lin_w": C.mlp[0].weight, "lin_b": C.mlp[0].bias}


CONV_CASES = {
    # name: (graph, layer keywords, fuse_linear, train, adjacency form)
    "fused_short_rows": ("_short", {}, True, False, "edges"),
    "fused_long_rows_finished": ("", {}, True, False, "edges"),
    "unfused": ("", {}, False, False, "edges"),
    "training": ("", {}, True, True, "edges"),
    "cartesian_fused": ("_short", dict(embed_slices=S_CART, embed_freqs=F_CART), True, False, "edges"),
    "cartesian": ("", dict(embed_slices=S_CART, embed_freqs=F_CART), True, False, "edges"),
    "cartesian_training": ("", dict(embed_slices=S_CART, embed_freqs=F_CART), True, True, "edges"),
    "gcn_self_loops": ("", dict(edge_weighting="gcn", self_loop_weight=0.5), True, False, "edges"),
    "gcn_self_loops_training": ("", dict(edge_weighting="gcn", self_loop_weight=0.5), True, True, "edges"),
    "csr_tuple_i32": ("", {}, True, False, "i32"),
    "csr_tuple_i64": ("", {}, True, False, "i64"),
    "csr_tuple_i32_training": ("", {}, True, True, "i32"),
}


@pytest.mark.parametrize("d", LC.D_INS)
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv(dev, name, d):
    """FSW_conv.forward on views of vertex_features, edge_index (incl. ei_T.t() of an [E, 2] tensor and rows 8- but not 16-byte
    aligned) and the (rowptr, col) tuple: the fused kernel on short rows, with the long rows finished, unfused, training, Cartesian
    (embed_slices / embed_freqs), 'gcn' weighting with self loops."""
    tag, kw, fuse, train, form = CONV_CASES[name]
    C = conv_layer(dev, d, **kw)
    C.fuse_linear = fuse
    if name in ("fused_short_rows", "fused_long_rows_finished", "cartesian_fused", "unfused"):
        assert C._fusable() == (name != "unfused")
    gr = LC.graph(short=bool(tag))
    ei = LC.array("edge_index" + tag)
    args = {"X": "X%d" % d}
    if form == "edges":
        args["ei"] = "edge_index" + tag
        call = lambda v: C(v["X"], v["ei"])
    else:
        args["rowptr"], args["col"] = "rowptr_" + form, "col_" + form
        call = lambda v: C(v["X"], (v["rowptr"], v["col"]))
    R = weights_for((N, 16)) if train else None
    Sweep(dev, "conv %s d=%d" % (name, d), call, args, lambda control: conv_refs(C, LC.array(args["X"]), ei, R, dev=dev, control=control), conv_params(C), ("X",),
          R).go()
    if name == "fused_long_rows_finished":
        assert int(gr["deg"].max()) > 32
    if name == "fused_short_rows":
        assert int(gr["deg"].max()) == 32


@pytest.mark.parametrize("train", [False, True], ids=["no_grad", "training"])
@pytest.mark.parametrize("cart", [False, True], ids=["diagonal", "cartesian_edge_features"])
def test_conv_edge_features(dev, cart, train):
    """edgefeat_dim = 3: edge_features [E, 3] in every layout; with training dL/d edge_features lands in the caller's layout."""
    kw = dict(embed_slices=S_CART, embed_freqs=F_CART, cartesian_edge_features=True) if cart else {}
    C = conv_layer(dev, 12, edgefeat_dim=DE, **kw)
    ei = LC.array("edge_index")
    R = weights_for((N, 16)) if train else None
    Sweep(dev, "conv edge features %s" % ("cart" if cart else "diag"), lambda v: C(v["X"], v["ei"], v["ef"]),
          {"X": "X12", "ei": "edge_index", "ef": "edge_features"},
          lambda control: conv_refs(C, LC.array("X12"), ei, R, ef=LC.array("edge_features"), dev=dev, control=control), conv_params(C), ("X", "ef"), R,
          fixed={"X": ("contig", "colslice"), "ei": ("contig", "transposed", "widerows")}).go()


# ---- 7: FSW_readout ------------------------------------------------------------------------------------------------------------
def readout_refs(C, R, dev, control):
    """Oracle of an FSW_readout (one Linear + LeakyReLU(0.2) layer on the embedding) on the graphs of READOUT_SIZES over X12."""
    E = C.fsw_embed
    ptr = np.concatenate([[0], np.cumsum(LC.READOUT_SIZES)]).astype(np.int64)
    X = LC.array("X12").astype(np.float64)
    V, fr = f64(E.projVecs), f64(E.freqs)
    col = np.arange(N, dtype=np.int64)
    emb = O.fsw_embedding_forward(X, ptr, col, np.ones(N), V, fr, encode_total_mass=True)
    Wl, bl = f64(C.mlp[0].weight), f64(C.mlp[0].bias)
    pre = emb @ Wl.T + bl
    refs = {"out": np.where(pre >= 0, pre, 0.2 * pre)}
    if R is not None:
        gpre = R * np.where(control["out"].cpu().numpy() >= 0, 1.0, 0.2)
        gh = gpre @ Wl
        gX, gV, gxi = O.fsw_embed_csr_backward(X, ptr, col, np.ones(N), V, fr, gh[:, 1:], Xp_override=hip_projection(E, t(X, dev, torch.float32)))
        refs.update({"g_X": gX, "g_projVecs": gV, "g_freqs": gxi, "g_lin_w": gpre.T @ emb, "g_lin_b": gpre.sum(0)})
    return refs


@pytest.mark.parametrize("train", [False, True], ids=["no_grad", "training"])
@pytest.mark.parametrize("form", ["graph_index", "ptr_i32", "ptr_i64"])
def test_readout(dev, form, train):
    """FSW_readout.forward on views of graph_index (int64) and of ptr (int32 and int64), and of vertex_features."""
    from fsw_gnn_amd import FSW_readout
    sizes = LC.READOUT_SIZES
    C = conv_layer(dev, 12, cls=FSW_readout, concat_self=False)
    E = C.fsw_embed
    args = {"X": "X12", "seg": form}
    call = (lambda v: C(v["X"], v["seg"], len(sizes))) if form == "graph_index" else (lambda v: C(v["X"], ptr=v["seg"]))
    R = weights_for((len(sizes), 16)) if train else None
    Sweep(dev, "readout %s" % form, call, args, lambda control: readout_refs(C, R, dev, control), conv_params(C), ("X",), R).go()


# ---- argument errors stay loud and specific ------------------------------------------------------------------------------------
def test_argument_errors_keep_their_messages(dev):
    from fsw_gnn_amd import FSW_conv, segcumsum
    E = embedding(dev, 12, learn=False)
    g = LC.graph()
    base, view = LC.on_device(*LC.case("X12", "colslice"), dev)
    idx = t(np.stack([g["rec"], g["col"]]), dev)
    W = torch.sparse_coo_tensor(idx, t(LC.array("wvals"), dev), (N, N))                    # not coalesced
    with torch.no_grad():
        with pytest.raises(AssertionError, match="Sparse W must be coalesced"):
            E(view, W, graph_mode=True)
        with pytest.raises(AssertionError, match="The last dimension of X must equal d_in"):
            E(base, W.coalesce(), graph_mode=True)                                         # the 17-column base instead of the view
        with pytest.raises(AssertionError, match="NaNs or infs"):
            E(base[:, :12], W.coalesce(), graph_mode=True)                                 # a view that does contain the poison
        vals = torch.ones(2 * N, device=dev)
        ids = torch.arange(2 * N, device=dev)
        with pytest.raises(AssertionError, match="segment_ids must be in contiguous format"):
            segcumsum(vals[::2], ids[::2])
        C = FSW_conv(12, 16, device=dev)
        bi, vi = LC.on_device(*LC.case("edge_index", "transposed"), dev)
        with pytest.raises(AssertionError, match="rowptr and col of a CSR adjacency must both be int32 or both be int64"):
            C(view, (vi[0].to(torch.int32), vi[1]))
