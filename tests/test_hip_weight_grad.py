"""d loss / d W of the generic kernel (csrc/embed_generic.hip) and of the host layer on top of it, per entry, against the float64
restatement tests/weight_grad_ref.py (pinned to the reference's autograd by tests/test_weight_grad_ref_cpu.py) and against the
reference's own gW in tests/golden/grads_w_long.npz.

(a) Kernel level: fsw_embed_generic / fsw_embed_cart_generic with gw set, on a plain CSR with one recipient per degree of
weight_grad_ref.KERNEL_DEGREES (both sides of every 256-element scan chunk up to 512, of the LDS line at 2048 and of the next
power of two at 4096) and hand-made keys that are exact in float32, so both storages sort bit-identical keys.  Rows of total mass
0.3 / 0.4 / 0.9 / 2.0, one of m == 1 exactly, exact zero weights, tau 1 and 3, has_mass 1 with out_scale 0.7, an output gradient with
zero readouts, zero slices and one zero row (the gk == 0 skip), one case with the edge term Ke, one Cartesian case on per-entry
keys with the identity as col.
    float64 storage: per entry |gw - ref| <= G64_ROW = 1e-10 of the row's largest |ref|.
    float32 storage: every input is exact in float32 and the arithmetic is float64; per slice the kernel casts its contribution
        to float32 and adds it with one float32 atomic, so |err_j| <= (S + 2) 2^-24 sum_s |gW_s[j]| plus the float64 term; the
        test applies twice that.
    one-line scratch: the same launch with scratch for a single workgroup, which then walks every row through one LDS / scratch
        line: float64 gw and gkey equal the full launch bit for bit; both meet the bounds.
    pre-filled gw: the result is the fill plus the gradient (the entry point accumulates).
    gkey / gfreq of the same launches: the bounds of test_hip_ties.py::test_generic_kernel_on_tied_keys.
(b) Module level: FSW_embedding, float64 and float32, W requiring grad, per row norm-wise at the bounds of tests/test_hip_float64.py
(gW 1e-10 / 2e-5, forward 1e-12 / 1e-5): every case of grads_w_long.npz against the fixture (sparse COO W; the Cartesian cases
also with the dense W they were made with), the other (function, method) pairs of the mass column against the restatement on the
HIP projection (no mass column among them: the fixture had no room for the diagonal cases without one, see
tools/make_weight_grad_goldens.py), and a dense [2, 2100] batch of two clouds of 300 and 2100 points.  The nopad case must take
the tau / 2 launch of _GenericEmbedFn.key_grads: its rows of m == 1 match the fixture, where the clamp rule is off by 210 % (test_weight_grad_ref_cpu.py).

Not covered, because the layers refuse it: a torch.sparse_csr W that requires grad raises NotImplementedError
(tests/test_csr_import_cpu.py) -- here a sparse_csr W only runs the forward of every fixture case; FSW_readout takes no weight
tensor at all (graph_index / ptr only), so there is no dL/dW through it.  A dense graph-mode W keeps only its nonzero entries
(FSW_embedding.forward: W.nonzero()), so a zero entry gets gradient 0 where the reference, which treats every sender as an element
of weight 0, gives a nonzero one: the dense comparison is made on the nonzero entries.

Measured on an MI355X, largest figure over the six kernel-level cases (one-line scratch: the same figures):
    float64 storage   gw per entry 8.8e-13 of the row maximum (D = 4500; 0.009 of the bound), forward per row 4.1e-13,
                      gkey per row 6.2e-13, per entry 2.5e-12 of the line maximum, gfreq 4.4e-14; one line == full launch bit for bit
    float32 storage   gw per entry err / bound, per degree: 1: 0.07  2: 0.07  3: 0.09  254: 0.14  255: 0.15  256: 0.19  257: 0.17
                      511: 0.19  1023: 0.15  2046: 0.17  2047: 0.18  2048: 0.17  2049: 0.16  4095: 0.16  4096: 0.20  4500: 0.20
                      (largest 0.20; 1.5e-7 of the row maximum); pre-filled with 0.5: 0.36; forward 3.9e-8, gkey per entry 5.9e-8,
                      gfreq 3.3e-7
    module level      float64: gW per row 6.6e-15 against the sparse-path fixture cases, 4.9e-14 against the restatement; forward
                      2.1e-15 / 4.5e-14.  float32: gW per row 7.2e-7, forward 1.4e-6 (sparse_csr W, the tuned kernels), 1.5e-7
                      otherwise.  Cartesian cases with weights of arbitrary long-row mass (an earlier fixture): gW 3.6e-13, forward
                      1.33e-12, the reference's dense-path rounding (now within the bounds with the 'cart' weights; the fixture's
                      own error is 1.4e-13 at most, tests/test_weight_grad_ref_cpu.py).
    mutations         (not kept) a reverse scan that drops the carry of all but the last chunk, and one that hands rank 255 the
                      reverse sum of rank 256, each fail all 40 tests of this file; the seven older tests that compare a gW
                      (test_hip_float64, test_hip_signed_freqs, test_hip_cartesian) pass under both.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import weight_grad_ref as R
from tests.conftest import relerr
from tests.test_hip_ties import F32_BOUND, G64_ROW, PER_ENTRY, TOL, coefficient_scale, dev, line_maxima, per_row, t  # noqa: F401
from tests.test_weight_grad_ref_cpu import LONG_CASES, long_case

pytestmark = pytest.mark.gpu
OUT_SCALE, HAS_MASS = 0.7, 1
F64_FWD, F64_GRAD, F32_FWD, F32_GRAD = 1e-12, 1e-10, 1e-5, 2e-5      # module level, per row (tests/test_hip_float64.py)
FILL = 0.5

# name: (cartesian, tau, edge term, per-entry keys with the identity as col)
KERNEL_CASES = {
    "diag_tau1": (False, 1.0, False, False),
    "diag_tau3": (False, 3.0, False, False),
    "diag_tau1_ke": (False, 1.0, True, False),
    "cart_tau1": (True, 1.0, False, False),
    "cart_tau3": (True, 3.0, False, False),
    "cart_tau3_entry_keys": (True, 3.0, True, True),
}


def case_shape(name):
    cart = KERNEL_CASES[name][0]
    S, F = (R.S_CART, len(R.CART_FREQS)) if cart else (R.S_DIAG, 1)
    return S, F, np.array(R.CART_FREQS if cart else R.DIAG_FREQS, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def kernel_reference(name):
    """The restatement on the case's keys: out [rows, 1 + S F] as the kernel scales it, gW, gW_s, gkey, gfreq, the key scale."""
    cart, tau, ke, _ = KERNEL_CASES[name]
    k = R.kernel_inputs()
    S, F, fr = case_shape(name)
    K = k["K"][:, :S].astype(np.float64) + (k["Ke"][:, :S].astype(np.float64) if ke else 0.0)
    G = OUT_SCALE * k["G"][:, HAS_MASS:HAS_MASS + S * F].astype(np.float64)
    res = R.weight_grad_reference(k["rowptr"], None, k["w"], K, fr, tau, G, cartesian=cart)
    res["out"] = OUT_SCALE * np.concatenate([res["mass"][:, None], res["out"]], axis=1)
    res["scale"] = coefficient_scale(G, np.tile(fr.astype(np.float64), S) if cart else fr.astype(np.float64)).reshape(-1, S, F).sum(axis=2)
    for a in res.values():
        a.setflags(write=False)
    return res


def run_kernel(dev, name, storage, one_line=False, fill=None, backward=True):
    """One forward (backward=False) or backward launch of the case's entry point.  Returns arrays in the storage type:
    {"out"} or {"gw", "gkey", "gfreq"}."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    cart, tau, ke, entry_keys = KERNEL_CASES[name]
    k = R.kernel_inputs()
    S, F, fr_host = case_shape(name)
    dt = torch.float64 if storage == "float64" else torch.float32
    nrows, nnz, maxdeg = len(R.KERNEL_DEGREES), k["w"].size, max(R.KERNEL_DEGREES)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rowptr, w = t(k["rowptr"], dev, torch.int32), t(k["w"], dev, dt)
    if entry_keys:
        Xp = t((k["K"][:, :S].astype(np.float64) + k["Ke"][:, :S]).astype(np.float32), dev, dt)
        col = torch.arange(nnz, dtype=torch.int32, device=dev)
    else:
        Xp, col = t(k["Xp"], dev, dt), t(k["col"], dev, torch.int32)
    Ke = t(k["Ke"], dev, dt) if (ke and not entry_keys) else None
    fr, g = t(fr_host, dev, dt), t(k["G"][:, :HAS_MASS + S * F], dev, dt)
    entry = "fsw_embed_cart_generic" if cart else "fsw_embed_generic"
    line_elems = 1
    while line_elems < maxdeg + 1:
        line_elems <<= 1
    nbytes = line_elems * 36 if one_line else int(getattr(L, entry + "_scratch_bytes")(maxdeg, nrows))      # kGenScratchBytesPerElem
    assert nbytes >= line_elems * 36
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = _lib.CartArgs() if cart else _lib.GenericArgs()
    a.value_dtype, a.S = (1 if dt == torch.float64 else 0), S
    a.rowptr, a.col, a.w, a.num_rows, a.max_degree = rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), nrows, maxdeg
    a.Xp, a.ldp, a.freqs, a.tau = Xp.data_ptr(), Xp.stride(0), fr.data_ptr(), tau
    a.out_scale, a.has_mass, a.mass_fn, a.mass_scale = OUT_SCALE, HAS_MASS, 0, 1.0
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    if cart:
        a.F = F
    elif Ke is not None:
        a.Ke, a.ldke = Ke.data_ptr(), Ke.stride(0)
    if not backward:
        out = torch.full((nrows, HAS_MASS + S * F), float("nan"), dtype=dt, device=dev)
        a.out, a.ldo = out.data_ptr(), out.stride(0)
        _lib.check(getattr(L, entry)(ctypes.byref(a), stream), entry)
        torch.cuda.synchronize()
        return {"out": out.cpu().numpy()}
    gkey = torch.full((nnz, S), float("nan"), dtype=dt, device=dev)
    gf = torch.zeros(F if cart else S, dtype=dt, device=dev)
    gw = torch.full((nnz,), 0.0 if fill is None else fill, dtype=dt, device=dev)
    a.g, a.ldg, a.gkey, a.ldk, a.gfreq, a.gw = g.data_ptr(), g.stride(0), gkey.data_ptr(), S, gf.data_ptr(), gw.data_ptr()
    _lib.check(getattr(L, entry)(ctypes.byref(a), stream), entry + " (backward)")
    torch.cuda.synchronize()
    return {"gw": gw.cpu().numpy(), "gkey": gkey.cpu().numpy(), "gfreq": gf.cpu().numpy()}


def gw_bound(ref, storage, S, fill=0.0):
    """Per entry: the float64 term G64_ROW of the row maximum; float32 storage adds 2 (S + 2) 2^-24 sum_s |gW_s| (module docstring).
    With a pre-filled buffer every one of the S atomic adds also rounds the fill: S + 1 roundings of |fill| (the last: the
    subtraction in the test)."""
    rowptr = R.kernel_inputs()["rowptr"]
    eps = 2.0 ** -53 if storage == "float64" else 2.0 ** -24
    b = G64_ROW * R.row_maxima(ref["gW"], rowptr) + (S + 1) * eps * abs(fill)
    if storage == "float32":
        b = 2.0 * (b + (S + 2) * eps * np.abs(ref["gW_s"]).sum(axis=1))
    return b


def check_gw(got, ref, storage, S, what, fill=0.0):
    rowptr, deg = R.kernel_inputs()["rowptr"], R.kernel_inputs()["degrees"]
    got = got.astype(np.float64) - fill
    assert np.isfinite(got).all(), what
    bound = gw_bound(ref, storage, S, fill)
    err = np.abs(got - ref["gW"])
    zero = R.row_maxima(ref["gW"], rowptr) == 0           # the row whose output gradient is zero: the kernel adds nothing
    assert zero.sum() == 512 and not got[zero].any(), what
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    rel = R.per_entry_ratio(got, ref["gW"], rowptr)
    cls = per_row(lambda a, b: ratio[a:b].max(), rowptr)
    print("%s: gw per entry err / bound max %.2e (D = %d), err / row maximum max %.2e (D = %d)" % (
        what, cls.max(), deg[cls.argmax()], rel.max(), deg[rel.argmax()]))
    print("   per degree err / bound:  " + "  ".join("%d: %.1e" % (d, c) for d, c in zip(deg, cls) if d))
    worst = int(ratio.argmax())
    assert ratio.max() <= 1.0, (what, "entry %d (row of %d)" % (worst, deg[np.searchsorted(rowptr, worst, side="right") - 1]),
                                float(ratio.max()), float(got[worst]), float(ref["gW"][worst]))


def check_keys_and_freqs(res, ref, storage, what):
    """gkey and gfreq at the bounds of test_generic_kernel_on_tied_keys: per row norm-wise, per entry against the line maximum
    (floored at 2e-4, float32 1e-6, of the line's scale), gfreq norm-wise.  A line whose output gradient is zero must be exactly 0."""
    rowptr, deg = R.kernel_inputs()["rowptr"], R.kernel_inputs()["degrees"]
    row_bound, entry_bound, floor = (G64_ROW, G64_ROW, 2e-4) if storage == "float64" else (F32_BOUND, PER_ENTRY, 1e-6)
    got = res["gkey"].astype(np.float64)
    assert got.shape == ref["gkey"].shape and np.isfinite(got).all(), what
    rows = per_row(lambda a, b: relerr(got[a:b], ref["gkey"][a:b]), rowptr)
    lm = np.maximum(line_maxima(ref["gkey"], rowptr), floor * np.repeat(ref["scale"], deg, axis=0))
    assert not got[lm == 0].any(), what
    ratio = np.abs(got - ref["gkey"]) / np.where(lm > 0, lm, 1.0)
    egf = relerr(res["gfreq"], ref["gfreq"])
    print("%s: gkey per row %.2e, per entry / line maximum %.2e, gfreq %.2e" % (what, rows.max(), ratio.max(), egf))
    assert rows.max() <= row_bound, (what, dict(zip(deg.tolist(), rows.tolist())))
    assert ratio.max() <= entry_bound, (what, float(ratio.max()))
    assert egf <= row_bound, (what, egf)


@pytest.mark.parametrize("storage", ["float64", "float32"])
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_weight_gradients(dev, name, storage):
    """(a) of the module docstring: forward, backward, backward with scratch for one workgroup, backward into a pre-filled gw."""
    ref = kernel_reference(name)
    S = case_shape(name)[0]
    what = "%s %s" % (name, storage)
    out = run_kernel(dev, name, storage, backward=False)["out"].astype(np.float64)
    errs = np.array([relerr(out[r], ref["out"][r]) for r in range(out.shape[0])])
    print("%s: forward per row max %.2e (D = %d)" % (what, errs.max(), R.KERNEL_DEGREES[errs.argmax()]))
    assert np.isfinite(out).all() and errs.max() <= (G64_ROW if storage == "float64" else TOL), (what, errs)
    full = run_kernel(dev, name, storage)
    check_gw(full["gw"], ref, storage, S, what)
    check_keys_and_freqs(full, ref, storage, what)
    one = run_kernel(dev, name, storage, one_line=True)
    check_gw(one["gw"], ref, storage, S, what + " one line")
    check_keys_and_freqs(one, ref, storage, what + " one line")
    if storage == "float64":
        assert np.array_equal(one["gw"], full["gw"]) and np.array_equal(one["gkey"], full["gkey"]), what
    filled = run_kernel(dev, name, storage, fill=FILL)
    check_gw(filled["gw"], ref, storage, S, what + " pre-filled", fill=FILL)
    assert np.array_equal(filled["gkey"], full["gkey"]), what


# ---- (b) module level -------------------------------------------------------------------------------------------------------------------
def make_module(dev, dtype, V, fr, tau, cartesian, fn, method, scale):
    from fsw_gnn_amd import FSW_embedding
    kw = dict(total_mass_pad_thresh=tau, enable_bias=False, learnable_slices=True, learnable_freqs=True, device=dev, dtype=dtype)
    if fn is not None:
        kw.update(encode_total_mass=True, total_mass_encoding_function=fn, total_mass_encoding_method=method, total_mass_encoding_scale=scale)
    if cartesian:
        E = FSW_embedding(d_in=V.shape[1], nSlices=V.shape[0], nFreqs=len(fr), collapse_freqs=True, **kw)
    else:
        E = FSW_embedding(d_in=V.shape[1], d_out=V.shape[0] + (fn is not None), **kw)
    with torch.no_grad():
        E.projVecs.copy_(t(V, dev, dtype))
        E.freqs.copy_(t(fr, dev, dtype))
        if fn is not None:
            E.total_mass_encoding_scale.fill_(scale)
    return E


def check_forward_rows(what, out, ref_out, rowptr, dtype):
    deg = np.diff(rowptr)
    fwd = np.array([relerr(out[r], ref_out[r]) for r in range(ref_out.shape[0])])
    print("%s: forward per row max %.2e (D = %d)" % (what, fwd.max(), deg[fwd.argmax()]))
    assert np.isfinite(out).all(), what
    assert fwd.max() <= (F64_FWD if dtype == torch.float64 else F32_FWD), (what, dict(zip(deg.tolist(), fwd.tolist())))


def check_gw_rows(what, gW, ref_gW, rowptr, dtype, sel=None):
    """gW per row, norm-wise, over the entries in `sel` (all by default)."""
    deg = np.diff(rowptr)
    sel = np.ones(ref_gW.shape[0], dtype=bool) if sel is None else sel
    assert np.isfinite(gW).all(), what
    grd = per_row(lambda a, b: relerr(gW[a:b][sel[a:b]], ref_gW[a:b][sel[a:b]]), rowptr)
    print("%s: gW per row max %.2e (D = %d)" % (what, grd.max(), deg[grd.argmax()]))
    assert grd.max() <= (F64_GRAD if dtype == torch.float64 else F32_GRAD), (what, dict(zip(deg.tolist(), grd.tolist())))
    return grd


def check_rows(what, out, ref_out, gW, ref_gW, rowptr, dtype):
    check_gw_rows(what, gW, ref_gW, rowptr, dtype)
    check_forward_rows(what, out, ref_out, rowptr, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", LONG_CASES)
def test_module_on_the_long_row_fixture(dev, name, dtype):
    """Every case of grads_w_long.npz: sparse COO W requiring grad; the Cartesian cases also with their dense W; and the forward
    alone with a torch.sparse_csr W (module docstring).  nopad_tau1: the rows of m == 1 (1 and 256 neighbours) within the bound.
    The Cartesian cases carry weights whose long rows have a power-of-two mass, so that the reference's dense-W path is exact where
    it would otherwise be off by more than the forward bound (tests/test_weight_grad_ref_cpu.py::
    test_the_fixture_forward_against_long_double)."""
    c = long_case(name)
    rowptr, deg = c["rowptr"], c["degrees"]
    nrows, n = deg.size, c["X"].shape[0]
    idx = torch.from_numpy(np.stack([np.repeat(np.arange(nrows), deg), c["cols"]])).to(dev)
    E = make_module(dev, dtype, c["V"], c["freqs"], c["tau"], c["cartesian"], c["fn"], c["method"], c["scale"])
    X, G = t(c["X"], dev, dtype), t(c["G"], dev, dtype)
    outs = {}
    for layout in ("coo", "dense") if c["cartesian"] else ("coo",):
        vals = t(c["w"], dev, dtype).requires_grad_(True)
        if layout == "coo":
            W = torch.sparse_coo_tensor(idx, vals, (nrows, n), is_coalesced=True)
        else:
            W = torch.zeros((nrows, n), dtype=dtype, device=dev).index_put((idx[0], idx[1]), vals)
        out = E(X, W, graph_mode=True)
        (out * G).sum().backward()
        outs[layout] = out.detach().cpu().numpy().astype(np.float64)
        grd = check_gw_rows("%s %s %s" % (name, layout, dtype), vals.grad.cpu().numpy().astype(np.float64), c["gW"], rowptr, dtype,
                            sel=None if layout == "coo" else c["w"] != 0)
        if layout == "dense":
            assert not vals.grad.cpu().numpy()[c["w"] == 0].any()
        if name == "nopad_tau1":
            on_tau = [grd[list(deg).index(d)] for d in (1, 256)]
            assert max(on_tau) <= (F64_GRAD if dtype == torch.float64 else F32_GRAD), ("m == tau rows: the tau / 2 launch", on_tau)
    with torch.no_grad():
        Wc = torch.sparse_coo_tensor(idx, t(c["w"], dev, dtype), (nrows, n), is_coalesced=True).to_sparse_csr()
        outs["sparse_csr"] = E(X, Wc, graph_mode=True).cpu().numpy().astype(np.float64)
    for layout, out in outs.items():
        check_forward_rows("%s %s %s" % (name, layout, dtype), out, c["out"], rowptr, dtype)


def hip_projection(E, X):
    """X . projVecs^T as the path under test computes it, in its dtype: the restatement sorts these keys."""
    from fsw_gnn_amd.fsw_embedding import _project
    S = E.nSlices
    return _project(X.detach().contiguous(), E.projVecs.detach(), E.d_in, S, (S + 63) // 64 * 64)[:, :S].cpu().numpy().astype(np.float64)


SUB_ROWS = (0, 1, 2, 3, 4, 5, 8)      # of the fixture's graph: 0, 1, 2, 255, 256, 257 and 2049 neighbours
OTHER_MASS = [(None, "plain"), ("identity", "plain"), ("sqrt", "plain"), ("log", "plain"), ("identity", "homog"), ("log", "homog"),
              ("identity", "homog_alt"), ("sqrt", "homog_alt")]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("fn,method", OTHER_MASS)
def test_module_other_mass_encodings(dev, fn, method, dtype):
    """The (function, method) pairs of the mass column the fixture does not hold, and no mass column, diagonal mode, sparse COO W, on
    seven rows of the fixture's graph at tau 1 (identity, none) or 3, against the restatement on the HIP projection: the mass
    column's f'(m) term of _GenericEmbedFn.backward and autograd through _homog_epilogue."""
    c = long_case("diag_tau1_sqrt_homog")
    tau = 1.0 if fn in (None, "identity") else 3.0
    ent = np.concatenate([np.arange(c["rowptr"][r], c["rowptr"][r + 1]) for r in SUB_ROWS])
    deg = c["degrees"][list(SUB_ROWS)]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    cols, w = c["cols"][ent], c["w"][ent]
    E = make_module(dev, dtype, c["V"], c["freqs"], tau, False, fn, method, 0.7)
    X = t(c["X"], dev, dtype)
    vals = t(w, dev, dtype).requires_grad_(True)
    idx = torch.from_numpy(np.stack([np.repeat(np.arange(deg.size), deg), cols])).to(dev)
    out = E(X, torch.sparse_coo_tensor(idx, vals, (deg.size, X.shape[0]), is_coalesced=True), graph_mode=True)
    G = R.kernel_inputs()["G"][:deg.size, :out.shape[1]].copy()
    G[G == 0] = 0.5
    (out * t(G, dev, dtype)).sum().backward()
    scale = float(E.total_mass_encoding_scale.detach()) if fn is not None else 1.0
    ref = R.weight_grad_reference(rowptr, cols, w, hip_projection(E, X), E.freqs.detach().cpu().numpy().astype(np.float64), tau,
                                  G.astype(np.float64), mass_fn=fn, mass_scale=scale, method=method, per_slice=False)
    check_rows("mass %s / %s tau %g %s" % (fn, method, tau, dtype), out.detach().cpu().numpy().astype(np.float64), ref["out"],
               vals.grad.cpu().numpy().astype(np.float64), ref["gW"], rowptr, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_module_dense_batch_of_two_clouds(dev, dtype):
    """Point-cloud mode, W a dense [2, 2100] tensor requiring grad: a cloud of 300 points padded with 1800 zero weights (total mass
    0.9, below tau) and one of 2100 points with a few zeros; mass column identity / plain.  Every entry of a dense W is an element,
    so the zero weights have gradients too; against the restatement on the HIP projection."""
    from fsw_gnn_amd import synth
    B, n, d, S = 2, 2100, 3, 8
    X = synth.features(B * n, d, seed=801)
    w = R.long_row_weights((n, n), {}, seed=802, zeros=12).reshape(B, n)
    w[0, 300:] = 0.0
    w[0, :300] *= np.float32(0.9) / w[0, :300].sum(dtype=np.float32)
    V = synth.unit_slices(S, d, seed=803)
    fr = np.array(R.DIAG_FREQS, dtype=np.float32)
    E = make_module(dev, dtype, V, fr, 1.0, False, "identity", "plain", 0.7)
    Xd = t(X, dev, dtype)
    W = t(w, dev, dtype).requires_grad_(True)
    out = E(Xd.reshape(B, n, d), W)
    G = synth.normal(804, 1, tuple(out.shape)).astype(np.float32)
    (out * t(G, dev, dtype)).sum().backward()
    rowptr = np.arange(B + 1) * n
    ref = R.weight_grad_reference(rowptr, None, w.reshape(-1), hip_projection(E, Xd), fr.astype(np.float64), 1.0, G.astype(np.float64),
                                  mass_fn="identity", mass_scale=float(E.total_mass_encoding_scale.detach()), per_slice=False)
    got = W.grad.cpu().numpy().astype(np.float64).reshape(-1)
    assert np.abs(got[300:n]).min() > 0                                     # zero weights, nonzero gradients
    check_rows("dense batch %s" % dtype, out.detach().cpu().numpy().astype(np.float64), ref["out"], got, ref["gW"], rowptr, dtype)
