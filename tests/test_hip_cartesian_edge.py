"""Cartesian mode (nSlices x nFreqs) with edge features (d_edge > 0): fsw_edge_keys_f32 + the tuned Cartesian kernels on the keys of the
CSR entries with the identity as their column array, from the C ABI up to FSW_conv.

(a) C ABI.  A coalesced graph from EC.edge_list with one recipient per degree of CLASS_DEGREES -- both sides of every class boundary of
the general-weight Cartesian table kCartLong[1] (csrc/embed_cart.h), whose lines hold D + 1 elements: 32/33 (registers), 64/65,
128/129 (one lane per slice / wavefront lines), 2046/2047/2048 (line 2048 | 2049: the first long class), 4095/4096 (8 | 16 wavefronts),
8191/8192, 16383/16384 (line 16384 | 16385: the giant class, its split form with FSW_CART_SPLIT_W_LINES / _BWD_LINES), 24576 (a giant
line of more than one block) -- about 95 k entries.  S = 3 slices x F = 5 frequencies, d_edge = 2; key columns of EC.xp_columns of kind
'e' (distinct keys, the control), 'cancel' (the edge term cancels the difference of two Xp: ties exist only on the sum) and 'zero_ve'
(an all-zero Ve row), frequencies 0, 0.37, 1.5, -0.37, -2.5 of EC.FREQ_CYCLE; general weights with exact zeros and the row of 31
neighbours at total mass 0.4.  fsw_edge_keys_f32 (bit for bit against EC.keys_float32), then fsw_embed_cart_f32 and
fsw_embed_cart_backward_keys_f32 on (K, identity) at tau = 1 and tau = 3, without flags and with the split flags and scratch the host
layer chooses, against the oracle with edge_feat= in the repeated-slice form.  Bounds: the project's, imported from
tests/test_hip_ties.py -- forward per row <= TOL, stored gkey per row <= F32_BOUND and per entry <= PER_ENTRY of the line maximum,
gfreq <= F32_BOUND.

(b) Module against tests/golden/cartesian_edge.npz (the reference's dense-W path): float32 modules norm-wise <= TOL, float64 modules
(generic kernel) <= G64_ROW; dense W + dense X_edge and sparse COO W + sparse X_edge give the same output; serialize_num_slices = 2
equals the unchunked result bit for bit; gradients of the float32 tuned path <= F32_BOUND, of the generic path with
X_edge.requires_grad <= G64_ROW (float64) and <= F32_BOUND (float32), gX_edge included.

(c) FSW_conv(8, 16, edgefeat_dim=2, embed_slices=4, embed_freqs=4, cartesian_edge_features=True) against its diagonal twin FSW_conv(8, 16, edgefeat_dim=2,
embed_dim=17) with the slices repeated and the frequencies tiled (existing, separately pinned code): 300 vertices, degrees up to 70,
10 % duplicate edges with features of their own, no self loops; forward (inference and training) <= 2 TOL, gX and g edge_features
<= 2 F32_BOUND -- two float32 evaluations of one float64 function, each within its own bound of it; a float64 layer <= TOL of the
float32 one.

Measured on an MI355X (every test prints its figures):
    (a) forward per row <= 1.2e-7 at tau = 1 (D = 128), 1.6e-7 at tau = 3 (the row of 31 neighbours and total mass 0.4); stored gkey per
        row <= 1.3e-7, per entry / line maximum <= 3.4e-7 in the control column and <= 2.1e-7 in the tied columns of every class with
        two neighbours and more (D = 1: 1.3e-6, a single key at tau = 1), the long classes 2046 .. 24576 at 1.0e-7 .. 1.8e-7; gfreq
        <= 1.6e-7.  The split form gives the same figures (gfreq 1.6e-7 against 5.9e-8 .. 1.0e-7).  No class has a bound of its own.
    (b) float32 modules 4.8e-8 .. 2.0e-7 (the reference's own float32 modules: 5.9e-8 .. 8.9e-7), float64 modules <= 6.8e-15; gradients
        of the tuned path gX 3.2e-7, gV 5.5e-7, gfreqs 7.7e-8, gbias 6.5e-8; of the generic path in float64 <= 2.2e-14 (gX_edge
        1.9e-14), in float32 <= 5.3e-7 (gX_edge 3.3e-7).
    (c) against the diagonal twin: inference 4.6e-8, training 4.6e-8, gX 1.4e-7, g edge_features 8.2e-8; float32 against float64 1.1e-7.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests import cartesian_edge_cases as CE
from tests import edge_feature_cases as EC
from tests.conftest import relerr
from tests.test_hip_ties import F32_BOUND, G64_ROW, OUT_SCALE, PER_ENTRY, TOL, check_key_gradients, coefficient_scale

pytestmark = pytest.mark.gpu

CLASS_DEGREES = (0, 1, 2, 31, 32, 33, 64, 65, 128, 129, 2046, 2047, 2048, 4095, 4096, 8191, 8192, 16383, 16384, 24576)
S_A, F_A, D_EDGE_A, D_IN_A = 3, 5, 2, 4
KEY_COLUMNS = (0, 6, 7)                       # of EC.kinds(13): 'e', 'cancel', 'zero_ve'
FREQ_INDEX = (0, 1, 3, 10, 11)                # of EC.FREQ_CYCLE: 0, 0.37, 1.5, -0.37, -2.5
HAS_MASS = 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- (a) C ABI -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def abi_case():
    """The coalesced graph on the device, read back for the oracle, and the key columns."""
    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.graph import build_csr_coalesced
    dev = torch.device("cuda:0")
    degrees = CLASS_DEGREES
    rows, nnz = len(degrees), int(sum(degrees))
    rec, snd, w, ef = EC.edge_list(degrees, D_EDGE_A)
    graph = build_csr_coalesced(t(rec, dev, torch.int64), t(snd, dev, torch.int64), t(w, dev), t(ef, dev), rows, nnz)
    st = graph.read_stats()
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_NNZ] == nnz and st[_lib.STAT_MAX_DEGREE] == max(degrees)
    rowptr = graph.rowptr.cpu().numpy().astype(np.int64)
    assert tuple(np.diff(rowptr)) == degrees
    order = EC.csr_order(rec, snd)
    col = graph.col[:nnz].cpu().numpy().astype(np.int64)
    assert np.array_equal(col, snd[order]) and np.array_equal(np.sort(col), np.arange(nnz))      # every sender exactly once
    wv, efv = graph.w[:nnz].cpu().numpy(), graph.ef[:nnz].cpu().numpy()
    assert np.array_equal(wv, w[order]) and np.array_equal(efv, ef[order]) and (wv == 0).sum() >= 30
    low = degrees.index(31)
    assert abs(wv[rowptr[low]:rowptr[low + 1]].astype(np.float64).sum() - 0.4) < 1e-5
    kinds = [EC.kinds(13)[c] for c in KEY_COLUMNS]
    assert kinds == ["e", "cancel", "zero_ve"]
    Ve13 = EC.slice_vectors(13, D_EDGE_A)
    xp = EC.xp_columns(rowptr, EC.edge_term(efv, Ve13))[:, list(KEY_COLUMNS)]
    Ve = Ve13[list(KEY_COLUMNS)]
    keys32 = EC.keys_float32(xp, efv, Ve)
    assert np.array_equal(keys32.astype(np.float64), xp.astype(np.float64) + EC.edge_term(efv, Ve))   # exact: the oracle ranks the same keys
    assert np.array_equal(bits(keys32), bits(EC.keys_float32(xp, efv, Ve, reverse=True)))
    fr = np.array([EC.FREQ_CYCLE[i] for i in FREQ_INDEX], dtype=np.float32)
    g = np.random.default_rng(43).standard_normal((rows, HAS_MASS + S_A * F_A)).astype(np.float32)
    return {"graph": graph, "st": st, "rowptr": rowptr, "col": col, "w": wv.astype(np.float64), "ef": efv, "xp": xp, "Ve": Ve,
            "keys32": keys32, "kinds": kinds, "freqs": fr, "g": g, "nnz": nnz}


@functools.lru_cache(maxsize=None)
def abi_reference(tau):
    """The oracle in the repeated-slice form: column s F + f carries the Xp of slice s, the unit vector of that column next to Ve[s], and
    frequency f; gkey and the coefficient scale summed over f, gfreq over s."""
    c = abi_case()
    S, F, nnz = S_A, F_A, c["nnz"]
    X = np.repeat(c["xp"].astype(np.float64), F, axis=1)
    V = np.concatenate([np.eye(S * F), np.repeat(c["Ve"].astype(np.float64), F, axis=0)], axis=1)
    fr = np.tile(c["freqs"].astype(np.float64), S)
    ident = np.arange(nnz)
    emb, mass = O.fsw_embed_csr(X, c["rowptr"], ident, c["w"], V, fr, total_mass_pad_thresh=tau, return_mass=True, edge_feat=c["ef"])
    G = OUT_SCALE * c["g"][:, HAS_MASS:].astype(np.float64)
    _, _, gxi, _, gkey = O.fsw_embed_csr_backward(X, c["rowptr"], ident, c["w"], V, fr, G, total_mass_pad_thresh=tau, edge_feat=c["ef"],
                                                  return_gkey=True)
    ref = {"out": OUT_SCALE * np.concatenate([mass[:, None], emb], axis=1), "gkey": gkey.reshape(nnz, S, F).sum(axis=2),
           "gfreq": gxi.reshape(S, F).sum(axis=0), "scale": coefficient_scale(G, fr).reshape(-1, S, F).sum(axis=2)}
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def abi_keys():
    """fsw_edge_keys_f32 on the graph: (K [nnz, 4] on the device with NaN in the pad column, identity int32 [nnz])."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    c = abi_case()
    nnz, graph = c["nnz"], c["graph"]
    Xp = np.full((nnz, S_A + 5), np.nan, dtype=np.float32)
    Xp[c["col"], :S_A] = c["xp"]                                      # sender col[e] carries the Xp of entry e
    Vfull = np.full((S_A, D_IN_A + D_EDGE_A), np.nan, dtype=np.float32)
    Vfull[:, D_IN_A:] = c["Ve"]
    Xp_d, V_d = t(Xp, dev), t(Vfull, dev)
    K = torch.full((nnz, 4), float("nan"), device=dev)
    _lib.check(L.fsw_edge_keys_f32(_lib.ptr(graph.col), nnz, _lib.ptr(Xp_d), Xp_d.stride(0), _lib.ptr(graph.ef), D_EDGE_A,
                                   V_d.data_ptr() + 4 * D_IN_A, V_d.stride(0), S_A, _lib.ptr(K), 4,
                                   torch.cuda.current_stream(dev).cuda_stream), "fsw_edge_keys_f32")
    torch.cuda.synchronize()
    return K, torch.arange(nnz, dtype=torch.int32, device=dev)


def test_abi_keys_bit_for_bit(dev):
    c = abi_case()
    K = abi_keys()[0].cpu().numpy()
    assert np.array_equal(bits(K[:, :S_A]), bits(c["keys32"])) and np.isnan(K[:, S_A:]).all()


def run_cart_on_keys(dev, tau, split):
    """fsw_embed_cart_f32 and fsw_embed_cart_backward_keys_f32 on (K, identity): (out [rows, 1 + S F], gkey [nnz, S], gfreq [F]).
    split: the flags and the scratch the host layer chooses for this graph (FSW_embedding._cart_split_w / _cart_split_w_backward)."""
    from fsw_gnn_amd import FSW_embedding, _lib
    L = _lib.lib()
    c = abi_case()
    graph, st, nnz, rows = c["graph"], c["st"], c["nnz"], len(CLASS_DEGREES)
    K, ident = abi_keys()
    S, F = S_A, F_A
    E = FSW_embedding(d_in=D_IN_A, d_edge=D_EDGE_A, nSlices=S, nFreqs=F, cartesian_edge_features=True, collapse_freqs=True, encode_total_mass=True,
                      total_mass_pad_thresh=tau, device=dev)
    fwd_split, bwd_split = (E._cart_split_w(graph, st), E._cart_split_w_backward(graph, st)) if split else (0, 0)
    if split:
        assert fwd_split > 0 and bwd_split > 0, "the host chooses the split form for the 6 lines of 16385 and more elements"
    stream = torch.cuda.current_stream(dev).cuda_stream
    fr, g = t(c["freqs"], dev), t(c["g"], dev)

    def args(scratch, flags):
        a = _lib.CartArgs()
        a.value_dtype, a.S, a.F, a.has_mass, a.flags = 0, S, F, HAS_MASS, flags
        a.rowptr, a.col, a.w = graph.rowptr.data_ptr(), ident.data_ptr(), graph.w.data_ptr()
        a.perm, a.bin_start, a.bin_start_host = graph.perm.data_ptr(), graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data
        a.num_rows, a.max_degree = rows, st[_lib.STAT_MAX_DEGREE]
        a.Xp, a.ldp, a.freqs, a.tau, a.out_scale = K.data_ptr(), K.stride(0), fr.data_ptr(), tau, OUT_SCALE
        a.mass_fn, a.mass_scale = 0, 1.0
        if scratch is not None:
            a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        return a

    out = torch.full((rows, HAS_MASS + S * F), float("nan"), device=dev)
    scratch = E._cart_scratch(graph, st, split_bytes=fwd_split)
    a = args(scratch, _lib.CART_SPLIT_W_LINES if split else 0)
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    _lib.check(L.fsw_embed_cart_f32(ctypes.byref(a), stream), "fsw_embed_cart_f32")
    gkey = torch.full((nnz, S), float("nan"), device=dev)
    gf = torch.zeros(F, device=dev)
    scratch = E._cart_scratch(graph, st, backward=True, split_bytes=bwd_split)
    a = args(scratch, _lib.CART_SPLIT_W_BWD_LINES if split else 0)
    a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g.data_ptr(), g.stride(0), gkey.data_ptr(), S, gf.data_ptr()
    _lib.check(L.fsw_embed_cart_backward_keys_f32(ctypes.byref(a), None, F, stream), "fsw_embed_cart_backward_keys_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), gkey.cpu().numpy().astype(np.float64), gf.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_abi_cartesian_kernels_on_edge_keys(dev, tau, split):
    """Measured on an MI355X, largest over tau and both forms: forward per row 1.6e-7, gkey per row 1.3e-7, per entry 1.3e-6 of the line
    maximum (D = 1; 3.4e-7 from two neighbours on), gfreq 1.6e-7 (module docstring)."""
    c, ref = abi_case(), abi_reference(tau)
    what = "cartesian edge keys tau %g%s" % (tau, " split" if split else "")
    out, gkey, gf = run_cart_on_keys(dev, tau, split)
    assert np.isfinite(out).all() and np.abs(out[0, HAS_MASS:]).max() == 0.0          # the empty row
    errs = np.array([relerr(out[r], ref["out"][r]) for r in range(len(CLASS_DEGREES))])
    print("%s: forward per row max %.2e (D = %d)   %s" % (what, errs.max(), CLASS_DEGREES[errs.argmax()],
                                                          "  ".join("%d: %.1e" % de for de in zip(CLASS_DEGREES, errs))))
    assert errs.max() <= TOL, (what, dict(zip(CLASS_DEGREES, errs.tolist())))
    check_key_gradients(gkey, ref["gkey"], c["rowptr"], c["kinds"], what, ref["scale"], row_bound=F32_BOUND, entry_bound=PER_ENTRY)
    e = relerr(gf, ref["gfreq"])
    print("%s: gfreq %.2e" % (what, e))
    assert np.isfinite(gf).all() and e <= F32_BOUND, (what, e)


# ---- (b) module against the golden file ----------------------------------------------------------------------------------------------
FORWARD_CASES = ("collapsed_bias", "matrix_bias", "mass_plain", "mass_homog_sqrt", "d_edge1_squeezed")


@functools.lru_cache(maxsize=None)
def golden_cases():
    return CE.load_cases()


def module_for(c, dev, dtype, learn=False):
    from fsw_gnn_amd import FSW_embedding
    S, F, d_in, d_edge = CE.dims(c)
    E = FSW_embedding(d_in=d_in, d_edge=d_edge, nSlices=S, nFreqs=F, cartesian_edge_features=True, collapse_freqs=bool(c["collapse"]),
                      encode_total_mass=bool(c["mass"]),
                      total_mass_encoding_method=str(c["method"]), total_mass_encoding_function=str(c["fn"]),
                      total_mass_encoding_scale=float(c["scale"]), enable_bias="bias" in c, learnable_slices=learn, learnable_freqs=learn,
                      device=dev, dtype=dtype)
    with torch.no_grad():
        E.projVecs.copy_(t(c["V"], dev, dtype))
        E.freqs.copy_(t(c["freqs"], dev, dtype))
        if "bias" in c:
            E.bias.copy_(t(c["bias"], dev, dtype).reshape(E.bias.shape))
    return E


def inputs_for(c, dev, dtype, sparse=False):
    """(X, W, X_edge): dense W [nR, n] and X_edge [nR, n, d_edge] ([nR, n] for the squeezed d_edge = 1 case), or both sparse COO."""
    nR, n, d_edge = c["num_rows"], c["X"].shape[0], int(c["d_edge"])
    idx = torch.from_numpy(np.stack([c["rows"], c["cols"]]).astype(np.int64)).to(dev)
    vals, ef = t(c["vals"], dev, dtype), t(c["ef"], dev, dtype)
    squeeze = bool(c["squeeze"])
    if sparse:
        W = torch.sparse_coo_tensor(idx, vals, (nR, n)).coalesce()
        Xe = torch.sparse_coo_tensor(idx, ef[:, 0] if squeeze else ef, (nR, n) if squeeze else (nR, n, d_edge)).coalesce()
    else:
        W = torch.zeros((nR, n), dtype=dtype, device=dev)
        W[idx[0], idx[1]] = vals
        Xe = torch.zeros((nR, n, d_edge), dtype=dtype, device=dev)
        Xe[idx[0], idx[1]] = ef
        Xe = Xe[..., 0].contiguous() if squeeze else Xe
    return t(c["X"], dev, dtype), W, Xe


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_module_forward_against_the_reference(dev, name):
    """float32 modules (tuned kernels) <= TOL, float64 modules (generic kernel) <= G64_ROW, norm-wise against the reference's float64
    output; sparse inputs give the dense inputs' output; serialize_num_slices = 2 the unchunked one, bit for bit."""
    c = golden_cases()[name]
    with torch.no_grad():
        E32 = module_for(c, dev, torch.float32)
        X, W, Xe = inputs_for(c, dev, torch.float32)
        y = E32(X, W, X_edge=Xe, graph_mode=True)
        assert tuple(y.shape) == c["out"].shape
        e32 = relerr(y.cpu().numpy(), c["out"])
        Xs, Ws, Xes = inputs_for(c, dev, torch.float32, sparse=True)
        assert torch.equal(E32(Xs, Ws, X_edge=Xes, graph_mode=True), y), "sparse W / X_edge differ from dense"
        assert torch.equal(E32(X, W, X_edge=Xe, graph_mode=True, serialize_num_slices=2), y), "serialize_num_slices=2 differs"
        E64 = module_for(c, dev, torch.float64)
        X, W, Xe = inputs_for(c, dev, torch.float64)
        y64 = E64(X, W, X_edge=Xe, graph_mode=True)
        e64 = relerr(y64.cpu().numpy(), c["out"])
        Xs, Ws, Xes = inputs_for(c, dev, torch.float64, sparse=True)
        assert torch.equal(E64(Xs, Ws, X_edge=Xes, graph_mode=True), y64)
    print("%s: float32 module %.2e (the reference's own float32 module: %.2e), float64 module %.2e" % (
        name, e32, relerr(c["out_f32"], c["out"]), e64))
    assert e32 <= TOL and e64 <= G64_ROW, (name, e32, e64)


def run_gradients(c, dev, dtype, edge_grad):
    E = module_for(c, dev, dtype, learn=True)
    X, W, Xe = inputs_for(c, dev, dtype)
    X.requires_grad_(True)
    Xe.requires_grad_(edge_grad)
    out = E(X, W, X_edge=Xe, graph_mode=True)
    (out * t(c["G"], dev, dtype)).sum().backward()
    got = {"out": out.detach(), "gX": X.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad, "gbias": E.bias.grad.reshape(-1)}
    if edge_grad:
        got["gX_edge"] = Xe.grad[torch.from_numpy(c["rows"].astype(np.int64)).to(dev), torch.from_numpy(c["cols"].astype(np.int64)).to(dev)]
    return {k: relerr(v.cpu().numpy(), c[k]) for k, v in got.items()}


def test_module_gradients_float32_tuned_path(dev):
    """X and the parameters require grad, X_edge does not: _CartEdgeEmbedFn on the tuned backward kernels."""
    errs = run_gradients(golden_cases()["grad_collapsed_bias"], dev, torch.float32, edge_grad=False)
    print("float32 tuned path against the reference's float64 gradients: " + "  ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs.pop("out") <= TOL and max(errs.values()) <= F32_BOUND, errs


@pytest.mark.parametrize("dtype,bound", [(torch.float64, G64_ROW), (torch.float32, F32_BOUND)])
def test_module_gradients_generic_path_with_edge_gradient(dev, dtype, bound):
    """X_edge.requires_grad takes the generic kernel on (K, identity) in either precision; gX_edge at the entries."""
    errs = run_gradients(golden_cases()["grad_collapsed_bias"], dev, dtype, edge_grad=True)
    print("generic path %s against the reference's float64 gradients: %s" % (dtype, "  ".join("%s %.2e" % kv for kv in errs.items())))
    assert "gX_edge" in errs and max(errs.values()) <= bound, errs


# ---- (c) FSW_conv --------------------------------------------------------------------------------------------------------------------
def conv_graph(seed=91):
    """300 vertices, in-degrees 0 .. 70 (distinct senders, no self loops), 10 % of the edges repeated with features of their own."""
    rng = np.random.default_rng(seed)
    n = 300
    deg = rng.integers(0, 71, size=n)
    deg[:3] = (70, 0, 33)
    src, dst = [], []
    for v in range(n):
        cand = np.delete(np.arange(n), v)                            # self loops dropped
        src.append(rng.choice(cand, size=deg[v], replace=False))
        dst.append(np.full(deg[v], v))
    src, dst = np.concatenate(src), np.concatenate(dst)
    dup = rng.choice(src.size, size=src.size // 10, replace=False)
    src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
    order = rng.permutation(src.size)
    ei = np.stack([src[order], dst[order]]).astype(np.int64)
    ef = rng.standard_normal((ei.shape[1], 2)).astype(np.float32)
    x = rng.standard_normal((n, 8)).astype(np.float32)
    return n, ei, ef, x


def conv_pair(dev):
    from fsw_gnn_amd import FSW_conv
    torch.manual_seed(7)
    cart = FSW_conv(8, 16, edgefeat_dim=2, embed_slices=4, embed_freqs=4, cartesian_edge_features=True, device=dev)
    twin = FSW_conv(8, 16, edgefeat_dim=2, embed_dim=17, device=dev)
    sd = cart.state_dict()
    sd["fsw_embed.projVecs"] = sd["fsw_embed.projVecs"].repeat_interleave(4, dim=0)       # column s F + f: slice s ...
    sd["fsw_embed.freqs"] = sd["fsw_embed.freqs"].repeat(4)                               # ... at frequency f
    twin.load_state_dict(sd)                                                              # MLP weights, total-mass scale, bias if any
    assert cart.fsw_embed.cartesian_mode and not twin.fsw_embed.cartesian_mode and cart.embed_dim == twin.embed_dim == 17
    return cart, twin


def test_conv_layer_against_its_diagonal_twin(dev):
    n, ei, ef, x = conv_graph()
    cart, twin = conv_pair(dev)
    ei_d = t(ei, dev, torch.int64)
    res = {}
    for name, layer in (("cart", cart), ("twin", twin)):
        layer.eval()
        with torch.no_grad():
            y_inf = layer(t(x, dev), ei_d, t(ef, dev))
        layer.train()
        xd, efd = t(x, dev).requires_grad_(True), t(ef, dev).requires_grad_(True)
        y = layer(xd, ei_d, efd)
        (y * torch.linspace(-1, 1, y.numel(), device=dev).reshape(y.shape)).sum().backward()
        res[name] = {"inference": y_inf, "training": y.detach(), "gX": xd.grad, "g_edge_features": efd.grad}
    errs = {k: relerr(res["cart"][k].cpu().numpy(), res["twin"][k].cpu().numpy()) for k in res["cart"]}
    print("FSW_conv 4 x 4 with edge features against its diagonal twin: " + "  ".join("%s %.2e" % kv for kv in errs.items()))
    assert tuple(res["cart"]["inference"].shape) == (n, 16) and float(res["cart"]["g_edge_features"].abs().sum()) > 0
    assert errs["inference"] <= 2 * TOL and errs["training"] <= 2 * TOL, errs
    assert errs["gX"] <= 2 * F32_BOUND and errs["g_edge_features"] <= 2 * F32_BOUND, errs
    # merged parallel edges each receive their slot's gradient
    key = ei[0] * n + ei[1]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    gef = res["cart"]["g_edge_features"].cpu().numpy()
    first = {}
    for i in np.nonzero(cnt[inv] > 1)[0]:
        j = first.setdefault(inv[i], i)
        assert np.array_equal(gef[i], gef[j])
    assert len(first) == ei.shape[1] // 11


def test_conv_layer_float64_matches_float32(dev):
    from fsw_gnn_amd import FSW_conv
    n, ei, ef, x = conv_graph()
    cart, _ = conv_pair(dev)
    c64 = FSW_conv(8, 16, edgefeat_dim=2, embed_slices=4, embed_freqs=4, cartesian_edge_features=True, device=dev, dtype=torch.float64)
    c64.load_state_dict(cart.state_dict())
    cart.eval(), c64.eval()
    with torch.no_grad():
        y32 = cart(t(x, dev), t(ei, dev, torch.int64), t(ef, dev))
        y64 = c64(t(x, dev, torch.float64), t(ei, dev, torch.int64), t(ef, dev, torch.float64))
    e = relerr(y32.cpu().numpy(), y64.cpu().numpy())
    print("FSW_conv 4 x 4 with edge features, float32 against float64: %.2e" % e)
    assert y64.dtype == torch.float64 and e <= TOL, e


def test_documented_shapes_run_forward_and_backward(dev):
    """FSW_embedding(d_in=8, nSlices=16, nFreqs=16, d_edge=4) and FSW_conv(128, 128, edgefeat_dim=4, embed_slices=16, embed_freqs=16), each with
    cartesian_edge_features=True."""
    from fsw_gnn_amd import FSW_conv, FSW_embedding
    rng = np.random.default_rng(3)
    n, E = 500, 6000
    ei = np.stack([rng.integers(0, n, E), rng.integers(0, n, E)]).astype(np.int64)
    emb = FSW_embedding(d_in=8, nSlices=16, nFreqs=16, d_edge=4, cartesian_edge_features=True, device="cuda", learnable_slices=True,
                        learnable_freqs=True)
    idx = torch.from_numpy(np.unique(ei[::-1], axis=1)).to(dev)
    W = torch.sparse_coo_tensor(idx, torch.rand(idx.shape[1], device=dev) + 0.1, (n, n)).coalesce()
    Xe = torch.sparse_coo_tensor(idx, torch.randn(idx.shape[1], 4, device=dev), (n, n, 4)).coalesce()
    X = torch.randn(n, 8, device=dev, requires_grad=True)
    out = emb(X, W, X_edge=Xe, graph_mode=True)
    out.square().sum().backward()
    assert tuple(out.shape) == (n, 16, 16) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(X.grad).all())
    assert tuple(emb.projVecs.grad.shape) == (16, 12) and float(emb.projVecs.grad[:, 8:].abs().sum()) > 0
    conv = FSW_conv(128, 128, edgefeat_dim=4, embed_slices=16, embed_freqs=16, cartesian_edge_features=True, device=dev)
    x = torch.randn(n, 128, device=dev, requires_grad=True)
    ef = torch.randn(E, 4, device=dev, requires_grad=True)
    y = conv(x, t(ei, dev, torch.int64), ef)
    y.square().sum().backward()
    assert tuple(y.shape) == (n, 128) and bool(torch.isfinite(y).all())
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(ef.grad).all()) and float(ef.grad.abs().sum()) > 0


def test_without_the_keyword_the_constructors_refuse_as_before(dev):
    """cartesian_edge_features is an opt-in: without it the combination raises what it always raised."""
    from fsw_gnn_amd import FSW_conv, FSW_embedding
    with pytest.raises(NotImplementedError, match="edge features"):
        FSW_embedding(d_in=4, d_edge=2, nSlices=2, nFreqs=3, device=dev)
    with pytest.raises(NotImplementedError, match="edge features"):
        FSW_conv(6, 8, edgefeat_dim=2, embed_slices=4, embed_freqs=8, device=dev)
    assert FSW_embedding(d_in=4, d_edge=2, nSlices=2, nFreqs=3, cartesian_edge_features=True, device=dev).d_edge == 2
    assert FSW_embedding(d_in=4, d_edge=2, d_out=5, cartesian_edge_features=True, device=dev).d_edge == 2     # no effect in diagonal mode
