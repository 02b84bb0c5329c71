"""Equal keys: every backward kernel class against the oracle, checked per entry.

Under equal keys the output of a row does not depend on their order, the gradient of a single key does: the element that ends
up at rank r receives the coefficient C(r).  The project's rule (DESIGN.md "equal keys"): equal keys rank in entry order, -0.0 and
+0.0 are equal, the pad element of a mass-deficient row (key 0) is the row's last entry.  The reference leaves that order to an
unstable sort (tests/test_oracle_vs_golden.py::test_tied_keys_contract), so the yardstick here is the oracle, which states the rule
in float64 (oracle/fsw_oracle.py), on bit-identical keys: the kernel-level tests hand the C entry points a hand-made float32 Xp, the
module-level tests hand the oracle the projection the HIP path computed.

Bounds.  TOL (1e-5) on the forward and F32_BOUND (3e-5) on gradients are the project's float32 bounds, here applied per recipient
row.  PER_ENTRY: |got - ref| <= 1e-5 * max|ref| over the entry's (row, slice) line.  The kernels evaluate the coefficients in float64
and round to float32 about three times (2e-7 of the entry); one swap of two adjacent ranks at xi >= 0.37 in a row of D <= 9000
neighbours moves an entry by 2 pi xi / D >= 2.6e-4 of the line's largest coefficient, so the bound sits a factor 26 below the
smallest error a wrong order can make and a factor 50 above rounding.

Measured on an MI355X, largest per-entry error / line maximum over all degree classes, tied columns | control column:
    fsw_embed_backward_f32 / _keys_f32   unit, tau 1 and 3: 1.5e-7 (D = 1023) | 1.3e-7 (D = 513);  general weights: 2.1e-6 (D = 2049) | 7.8e-7 (D = 31)
    fsw_embed_cart_backward_keys_f32     unit, tau 1 and 3: 1.8e-7 (D = 2047) | 1.5e-7 (D = 256);  general weights: 5.0e-7 (D = 31) | 3.6e-7 (D = 31)
    fsw_embed_generic, float32 storage   6.2e-8 (D = 2049) | 5.7e-8 (D = 513);  float64 storage: per row 3.3e-12, forward 5.4e-14
    stored key gradients against the atomic form: identical in every entry, every mode
    per row: forward <= 7.1e-7, gkey <= 8.5e-7, gfreq <= 2.2e-7 (Cartesian 7.1e-7); module level: gX per entry <= 0.05 of its bound
The control column stays below the bound in every class, so no class has a bound of its own.  The largest figures belong to the rows
of total mass 0.4: when this was measured the kernels rounded the pad element's weight to float32 (6e-8), which shifts the phase
2 pi xi c of every element behind the pad by 2 pi xi * 4e-8 -- rounding, the same for tied and distinct keys, not an order effect
(since then the pad weight enters the cumulative weight in float64: tests/test_hip_large_freqs.py).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests import cases
from tests.conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5            # forward, norm-wise (tests/test_hip_parity.py)
F32_BOUND = 3e-5      # float32 gradients, norm-wise (tests/test_hip_parity.py, tests/test_hip_cartesian_train.py)
PER_ENTRY = 1e-5      # per entry, relative to the largest reference entry of the (row, slice) line
G64_ROW = 1e-10       # generic kernel with float64 storage, per row (tests/test_hip_float64.py)

# one recipient per degree: both ends of every unit-weight and weighted class of launch_embed_long_bwd (embed_wsort_bwd.hip), both
# register launches of embed_bwd.hip, the padded networks of embed_mid_bwd.hip, hub bins 0 .. 2
DEGREES = (0, 1, 2, 3, 16, 17, 31, 32, 33, 40, 41, 64, 65, 128, 129, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047,
           2048, 2049, 4096, 4097, 9000)
NNZ = sum(DEGREES)
FREQS = (0.0, 0.37, 1.0, 1.5, 2.5, 4.0, 7.25, 13.0)
# key columns: (a) one constant, (b) +0.0 / -0.0, (c) four values, (d) ascending / descending runs of three, (e) distinct (control)
COLUMNS = ("a", "b", "c", "d_up", "d_down", "e", "b", "c")
CONTROL = "e"
MODES = [("unit", 1.0), ("unit", 3.0), ("random", 1.0)]
OUT_SCALE, HAS_MASS = 0.7, 1
LOW_MASS_ROWS = (31, 193, 2049)     # degrees of the rows scaled to total mass 0.4 in the 'random' weights


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


# ---- inputs (numpy only) ------------------------------------------------------------------------------------------------------
def edge_list(weights):
    """(recipients, senders, weights or None) in shuffled order; sender j occurs exactly once."""
    rng = np.random.default_rng(41)
    rec = np.repeat(np.arange(len(DEGREES)), DEGREES).astype(np.int64)
    snd = rng.permutation(NNZ).astype(np.int64)
    w = None
    if weights == "random":
        w = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), size=NNZ)
        w[rng.choice(NNZ, size=40, replace=False)] = 0.0
        for deg in LOW_MASS_ROWS:
            low = rec == DEGREES.index(deg)
            w[low] *= np.float32(0.4) / w[low].sum(dtype=np.float32)
    order = rng.permutation(NNZ)
    return rec[order], snd[order], None if w is None else w[order]


def key_columns(rowptr, kinds=COLUMNS):
    """float32 keys [NNZ, len(kinds)] per CSR entry, column c of kind kinds[c]."""
    rng = np.random.default_rng(42)
    deg = np.diff(rowptr)
    pos = np.arange(NNZ) - np.repeat(rowptr[:-1], deg)              # position of the entry in its row
    last = np.repeat(deg, deg) - 1 - pos
    K = np.empty((NNZ, len(kinds)), dtype=np.float32)
    for c, kind in enumerate(kinds):
        if kind == "a":
            K[:, c] = 0.75
        elif kind == "b":
            K[:, c] = np.where(rng.random(NNZ) < 0.5, np.float32(0.0), np.float32(-0.0))
        elif kind == "c":
            K[:, c] = rng.choice(np.array([-1.0, -0.0, 0.0, 0.5], dtype=np.float32), size=NNZ)
        elif kind == "d_up":
            K[:, c] = (pos // 3) * 0.125 - 100.0                    # exact in float32
        elif kind == "d_down":
            K[:, c] = (last // 3) * 0.125 - 100.0
        else:
            v = rng.standard_normal(NNZ).astype(np.float32)
            for a, b in zip(rowptr[:-1], rowptr[1:]):               # distinct inside every row
                while np.unique(v[a:b]).size < b - a:
                    _, first = np.unique(v[a:b], return_index=True)
                    dup = np.setdiff1d(np.arange(b - a), first)
                    v[a + dup] = rng.standard_normal(dup.size).astype(np.float32)
            K[:, c] = v
    if kinds[1] == "b":
        assert np.signbit(K[:, 1]).any() and not np.signbit(K[:, 1]).all()
    return K


def expected_bin_rows(degrees=DEGREES):
    """Rows per degree bin of include/fsw_hip.h for `degrees`."""
    from fsw_gnn_amd import _lib
    uppers = list(range(_lib.REG_MAX_DEG + 1)) + list(_lib.MID_SIZES) + [512, 1024, 2048, 4096, 8192, 16384, 32768, 1 << 62]
    rows = [0] * len(uppers)
    for d in degrees:
        rows[next(i for i, u in enumerate(uppers) if d <= u)] += 1
    return rows


def line_maxima(ref, rowptr):
    """max |ref| over every (row, slice) line, repeated per entry: [nnz, S]."""
    out = np.zeros_like(ref)
    for a, b in zip(rowptr[:-1], rowptr[1:]):
        if b > a:
            out[a:b] = np.abs(ref[a:b]).max(axis=0, keepdims=True)
    return out


def per_row(fn, rowptr):
    return np.array([fn(a, b) if b > a else 0.0 for a, b in zip(rowptr[:-1], rowptr[1:])])


def coefficient_scale(G, freqs):
    """[rows, len(freqs)]: |G| times the size of the two values F(xi; c) = (1 + xi) sin(2 pi xi c) / (pi xi) whose difference a
    coefficient is, min(2, 1 / (pi |xi|)) |1 + xi| (frequencies of either sign)."""
    xi = np.asarray(freqs, dtype=np.float64)
    return np.abs(G) * (np.abs(1 + xi) * np.minimum(2.0, 1.0 / (np.pi * np.maximum(np.abs(xi), 1e-300))))[None, :]


def check_key_gradients(got, ref, rowptr, columns, what, scale, row_bound=F32_BOUND, entry_bound=PER_ENTRY, floor=1e-6):
    """Finite; per row norm-wise <= row_bound; per entry <= entry_bound * line maximum.  Prints the largest per-entry ratio of the
    tied columns and of the control column per degree class; a tied column never gets a looser bound than the control.
    scale [rows, S] (coefficient_scale): a line whose coefficients all vanish -- unit weights, xi / D a multiple of 1/2, e.g.
    D = 1 at every integer xi, D = 3 at xi = 1.5 -- has a reference of pure float64 rounding (1e-17) and no order to get wrong; the
    line maximum is floored at `floor` = 1e-6 of the line's scale (the smallest non-vanishing line here, D = 9000 at xi = 0.37, is
    1e-4 of it)."""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    deg = np.diff(rowptr)
    rows = per_row(lambda a, b: relerr(got[a:b], ref[a:b]), rowptr)
    lm = np.maximum(line_maxima(ref, rowptr), floor * np.repeat(scale, deg, axis=0))
    assert (lm > 0).all(), what
    ratio = np.abs(got - ref) / lm
    ctrl = np.array([c == CONTROL for c in columns])
    tied_cls = per_row(lambda a, b: ratio[a:b][:, ~ctrl].max(), rowptr) if not ctrl.all() else np.zeros(deg.size)
    ctrl_cls = per_row(lambda a, b: ratio[a:b][:, ctrl].max(), rowptr) if ctrl.any() else np.zeros(deg.size)
    print("%s: row norm-wise max %.2e | per entry tied max %.2e (D = %d), control max %.2e (D = %d)" % (
        what, rows.max(), tied_cls.max(), deg[tied_cls.argmax()], ctrl_cls.max(), deg[ctrl_cls.argmax()]))
    print("   per class D: tied / control  " + "  ".join("%d: %.1e/%.1e" % (d, a, b) for d, a, b in zip(deg, tied_cls, ctrl_cls) if d))
    assert rows.max() <= row_bound, (what, dict(zip(deg.tolist(), rows.tolist())))
    worst = np.unravel_index(ratio.argmax(), ratio.shape)
    assert ratio.max() <= entry_bound, (what, "entry %d (row of %d), column %s" % (
        worst[0], deg[np.searchsorted(rowptr, worst[0], side="right") - 1], columns[worst[1]]), float(ratio.max()))


# ---- the graph on the device and the oracle's answers, computed once per weight mode ----------------------------------------------
@functools.lru_cache(maxsize=None)
def tied_case(weights, kinds=COLUMNS, ladder=None, tau=None):
    """ladder (tests/large_freq_cases.py: Ladder): another graph of one recipient per degree, with the ladder's own edge list for the
    weight mode `weights` and its own len(kinds) key columns for (weights, tau); None: the graph of DEGREES and the columns `kinds`."""
    from fsw_gnn_amd import _lib, build_csr
    dev = torch.device("cuda:0")
    degrees = DEGREES if ladder is None else ladder.degrees
    nnz = sum(degrees)
    rec, snd, w = edge_list(weights) if ladder is None else ladder.edge_list(weights)
    graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None if w is None else t(w, dev), len(degrees), nnz)
    st = graph.read_stats()
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_NNZ] == nnz and st[_lib.STAT_MAX_DEGREE] == max(degrees)
    rowptr = graph.rowptr.cpu().numpy().astype(np.int64)
    assert tuple(np.diff(rowptr)) == degrees
    bins = np.diff(graph.bin_start_host[0]).tolist()
    assert bins == expected_bin_rows(degrees)
    if ladder is None:
        assert bins[_lib.BIN_MID0:] == [2, 1, 1, 1, 0, 1, 1, 1, 3, 3, 3, 3, 2, 1, 1, 0, 0]   # mid, LDS, hub bins, global
    col = graph.col[:nnz].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(col), np.arange(nnz))            # every sender exactly once
    for r in (5, 20, 31) if ladder is None else range(len(degrees)):   # the rows keep the order of the (shuffled) edge list
        assert np.array_equal(col[rowptr[r]:rowptr[r + 1]], snd[rec == r])
    wv = np.ones(nnz) if w is None else graph.w[:nnz].cpu().numpy().astype(np.float64)
    if w is not None and ladder is None:
        assert (wv == 0).sum() >= 30
        for deg in LOW_MASS_ROWS:
            r = DEGREES.index(deg)
            assert abs(wv[rowptr[r]:rowptr[r + 1]].sum() - 0.4) < 1e-5
    if w is not None and ladder is not None:
        assert np.array_equal(graph.w[:nnz].cpu().numpy(), w[np.argsort(rec, kind="stable")])      # the float32 weights, untouched
    K = key_columns(rowptr, kinds) if ladder is None else ladder.key_columns(weights, tau, len(kinds))
    Xp = np.zeros((nnz, 64), dtype=np.float32)
    Xp[col, :K.shape[1]] = K                                       # sender col[e] carries the keys of entry e
    g = np.random.default_rng(43).standard_normal((len(degrees), HAS_MASS + 20)).astype(np.float32)
    more = np.random.default_rng(44).standard_normal((len(degrees), 12)).astype(np.float32)     # columns 21 .. 32: Cartesian 4 x 8
    g = np.concatenate([g, more], axis=1)
    return {"graph": graph, "st": st, "rowptr": rowptr, "col": col, "w": wv, "K": K, "Xp": Xp, "g": g, "degrees": degrees, "nnz": nnz}


@functools.lru_cache(maxsize=None)
def diagonal_reference(weights, tau, S, freqs=FREQS, kinds=COLUMNS, ladder=None):
    """Oracle (float64, entry order among equal keys) on the first S key columns (of kind kinds[:S], at freqs[:S]): out [rows, 1 + S],
    gkey [nnz, S], gfreq [S]."""
    c = tied_case(weights, kinds) if ladder is None else tied_case(weights, kinds, ladder, tau)
    K, fr, rowptr = c["K"][:, :S].astype(np.float64), np.array(freqs[:S]), c["rowptr"]
    ident = np.arange(c["nnz"])                                       # the oracle's "features" are the keys of every entry
    emb, mass = O.fsw_embed_csr(K, rowptr, ident, c["w"], np.eye(S), fr, total_mass_pad_thresh=tau, return_mass=True)
    G = OUT_SCALE * c["g"][:, HAS_MASS:HAS_MASS + S].astype(np.float64)
    _, _, gxi, gkey = O.fsw_embed_csr_backward(K, rowptr, ident, c["w"], np.eye(S), fr, G, total_mass_pad_thresh=tau, return_gkey=True)
    for a in (emb, gkey, gxi):
        a.setflags(write=False)
    return {"out": OUT_SCALE * np.concatenate([mass[:, None], emb], axis=1), "gkey": gkey, "gfreq": gxi, "scale": coefficient_scale(G, fr)}


@functools.lru_cache(maxsize=None)
def cartesian_reference(weights, tau, cols, F, freqs=FREQS, kinds=COLUMNS, ladder=None):
    """The oracle through the diagonal identity of tests/test_cartesian_cpu.py: key column s repeated F times, freqs[:F] tiled;
    gkey[e, s] is the sum over f, gkey_sf [nnz, S, F] its terms."""
    c = tied_case(weights, kinds) if ladder is None else tied_case(weights, kinds, ladder, tau)
    S, rowptr, NNZ = len(cols), c["rowptr"], c["nnz"]
    K = np.repeat(c["K"][:, list(cols)].astype(np.float64), F, axis=1)        # column s F + f = key column s
    fr = np.tile(np.array(freqs[:F]), S)
    ident = np.arange(NNZ)
    emb, mass = O.fsw_embed_csr(K, rowptr, ident, c["w"], np.eye(S * F), fr, total_mass_pad_thresh=tau, return_mass=True)
    G = OUT_SCALE * c["g"][:, HAS_MASS:HAS_MASS + S * F].astype(np.float64)
    _, _, gxi, gkey = O.fsw_embed_csr_backward(K, rowptr, ident, c["w"], np.eye(S * F), fr, G, total_mass_pad_thresh=tau, return_gkey=True)
    return {"out": OUT_SCALE * np.concatenate([mass[:, None], emb], axis=1), "gkey": gkey.reshape(NNZ, S, F).sum(axis=2),
            "gfreq": gxi.reshape(S, F).sum(axis=0), "scale": coefficient_scale(G, fr).reshape(-1, S, F).sum(axis=2),
            "gkey_sf": gkey.reshape(NNZ, S, F)}


def check_forward(got, ref, what, degrees=DEGREES):
    assert np.isfinite(got).all()
    errs = np.array([relerr(got[r], ref[r]) for r in range(len(degrees))])
    print("%s: forward per row max %.2e (D = %d)" % (what, errs.max(), degrees[errs.argmax()]))
    assert degrees[0] == 0 and np.abs(got[0, HAS_MASS:]).max() == 0.0      # the empty row
    assert errs.max() <= TOL, (what, dict(zip(degrees, errs.tolist())))


# ---- 2. kernel level ----------------------------------------------------------------------------------------------------------------
def embed_args(c, S, tau, fr, table, scratch):
    from fsw_gnn_amd import _lib
    graph, st = c["graph"], c["st"]
    a = _lib.EmbedArgs()
    a.rowptr, a.col, a.perm, a.bin_start = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.perm.data_ptr(), graph.bin_start.data_ptr()
    a.w = graph.w.data_ptr() if graph.w is not None else None
    a.num_rows, a.bin_start_host = len(c["degrees"]), graph.bin_start_host[0].ctypes.data
    a.Xp, a.ldp, a.freqs, a.S, a.tau = c["Xp_dev"].data_ptr(), c["Xp_dev"].stride(0), fr.data_ptr(), S, tau
    a.unit_table, a.ldt = (table.data_ptr(), table.stride(0)) if table is not None else (None, 0)
    a.out_scale, a.has_mass, a.mass_fn, a.mass_scale = OUT_SCALE, HAS_MASS, 0, 1.0
    a.num_reg_rows, a.num_lds_rows = st[_lib.STAT_NUM_REG], st[_lib.STAT_NUM_LDS]
    a.num_global_rows, a.num_zero_rows, a.max_degree = st[_lib.STAT_NUM_GLOBAL], st[_lib.STAT_NUM_ZERO], st[_lib.STAT_MAX_DEGREE]
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    return a


def run_tuned_kernels(dev, weights, tau, S, freqs=FREQS, kinds=COLUMNS, ladder=None):
    """fsw_embed_f32, fsw_embed_backward_f32 and fsw_embed_backward_keys_f32 on the graph of DEGREES (or of `ladder`), key columns
    kinds[:S], frequencies freqs[:S]: (out [rows, 1 + S], gkey read back from the atomic form [nnz, S], stored gkey [nnz, S],
    {name: gfreq [S]}), float64."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    c = dict(tied_case(weights, kinds) if ladder is None else tied_case(weights, kinds, ladder, tau))
    col, DEGREES, NNZ = c["col"], c["degrees"], c["nnz"]
    stream = torch.cuda.current_stream(dev).cuda_stream
    c["Xp_dev"] = t(c["Xp"], dev)
    fr = t(np.array(freqs[:S]), dev)
    g = t(c["g"][:, :HAS_MASS + S], dev)
    unit_fast = weights == "unit" and tau <= 1.0
    table = dtable = None
    if unit_fast:
        table = torch.empty((int(L.fsw_unit_table_rows(_lib.REG_MAX_DEG)), 64), device=dev)
        dtable = torch.empty_like(table)
        _lib.check(L.fsw_unit_coeff_table(_lib.ptr(fr), S, _lib.REG_MAX_DEG, _lib.ptr(table), 64, stream), "fsw_unit_coeff_table")
        _lib.check(L.fsw_unit_dcoeff_table(_lib.ptr(fr), S, _lib.REG_MAX_DEG, _lib.ptr(dtable), 64, stream), "fsw_unit_dcoeff_table")
    scratch = torch.empty(int(L.fsw_embed_scratch_bytes(max(DEGREES))), dtype=torch.uint8, device=dev)

    out = torch.full((len(DEGREES), HAS_MASS + S), float("nan"), device=dev)
    a = embed_args(c, S, tau, fr, table, scratch)
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    _lib.check(L.fsw_embed_f32(ctypes.byref(a), stream), "fsw_embed_f32")
    torch.cuda.synchronize()

    a = embed_args(c, S, tau, fr, table, scratch)
    gXp = torch.zeros((NNZ, 64), device=dev)
    gf_atomic = torch.zeros(S, device=dev)
    _lib.check(L.fsw_embed_backward_f32(ctypes.byref(a), _lib.ptr(dtable), _lib.ptr(g), g.stride(0), _lib.ptr(gXp), gXp.stride(0),
                                        _lib.ptr(gf_atomic), stream), "fsw_embed_backward_f32")
    gkey = torch.full((NNZ, S), float("nan"), device=dev)
    gf_keys = torch.zeros(S, device=dev)
    _lib.check(L.fsw_embed_backward_keys_f32(ctypes.byref(a), _lib.ptr(dtable), _lib.ptr(g), g.stride(0), _lib.ptr(gkey), S,
                                             _lib.ptr(gf_keys), stream), "fsw_embed_backward_keys_f32")
    torch.cuda.synchronize()
    atomic = gXp.cpu().numpy().astype(np.float64)
    assert np.abs(atomic[:, S:]).max() == 0.0
    atomic = atomic[col, :S]                                       # every sender has one entry: its gXp row is that entry's key gradient
    return (out.cpu().numpy().astype(np.float64), atomic, gkey.cpu().numpy().astype(np.float64),
            {"atomics": gf_atomic.cpu().numpy(), "stored": gf_keys.cpu().numpy()})


@pytest.mark.parametrize("S", [8, 6])
@pytest.mark.parametrize("weights,tau", MODES)
def test_tuned_kernels_on_tied_keys(dev, weights, tau, S):
    """fsw_embed_f32, fsw_embed_backward_f32 (atomics) and fsw_embed_backward_keys_f32 (stored key gradients: unit weights with the
    coefficient tables = the store-and-sum form, the other modes without) on the graph of DEGREES and the key columns COLUMNS[:S].
    S = 8: rows of 129 .. 2048 neighbours take k_embed_quad_bwd in the store form; S = 6: k_embed_wsort_bwd.  unit / tau = 3 runs the
    general kernels with w == NULL; 'random' weights hold exact zeros and three rows of total mass 0.4, whose pad element ties with
    every zero key (all keys of column b).
    Forward per row <= TOL; gkey of both forms against the oracle and against each other: finite (gkey is pre-filled with NaN), per
    row <= F32_BOUND, per entry <= PER_ENTRY of the line maximum; gfreq <= F32_BOUND."""
    ref = diagonal_reference(weights, tau, S)
    rowptr = tied_case(weights)["rowptr"]
    what = "%s tau %g S %d" % (weights, tau, S)
    out, atomic, keys, gfreq = run_tuned_kernels(dev, weights, tau, S)
    check_forward(out, ref["out"], what)
    check_key_gradients(atomic, ref["gkey"], rowptr, COLUMNS[:S], what + " atomics", ref["scale"])
    check_key_gradients(keys, ref["gkey"], rowptr, COLUMNS[:S], what + " stored", ref["scale"])
    check_key_gradients(keys, atomic, rowptr, COLUMNS[:S], what + " stored vs atomics", ref["scale"])
    for name, gf in gfreq.items():
        e = relerr(gf, ref["gfreq"])
        print("%s %s: gfreq %.2e" % (what, name, e))
        assert e <= F32_BOUND, (what, name, e)


def run_generic_kernel(dev, weights, tau, storage, freqs=FREQS, kinds=COLUMNS, ladder=None, S=8):
    """fsw_embed_generic, forward and backward, on the plain CSR of the graph of DEGREES (or of `ladder`), the S key columns `kinds`
    and frequencies `freqs`: (out [rows, 1 + S], gkey [nnz, S], gfreq [S]) in the storage type."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    c = tied_case(weights, kinds) if ladder is None else tied_case(weights, kinds, ladder, tau)
    graph, DEGREES, NNZ = c["graph"], c["degrees"], c["nnz"]
    dt = torch.float64 if storage == "float64" else torch.float32
    stream = torch.cuda.current_stream(dev).cuda_stream
    Xp = t(c["Xp"], dev, dt)
    fr = t(np.array(freqs[:S]), dev, dt)
    g = t(c["g"][:, :HAS_MASS + S], dev, dt)
    w = graph.w[:NNZ].to(dt).contiguous() if graph.w is not None else None
    scratch = torch.empty(int(L.fsw_embed_generic_scratch_bytes(max(DEGREES), len(DEGREES))), dtype=torch.uint8, device=dev)
    out = torch.full((len(DEGREES), HAS_MASS + S), float("nan"), dtype=dt, device=dev)
    gkey = torch.full((NNZ, S), float("nan"), dtype=dt, device=dev)
    gf = torch.zeros(S, dtype=dt, device=dev)

    def args(**fields):
        a = _lib.GenericArgs()
        a.value_dtype, a.S = (1 if dt == torch.float64 else 0), S
        a.rowptr, a.col, a.w = graph.rowptr.data_ptr(), graph.col.data_ptr(), w.data_ptr() if w is not None else None
        a.num_rows, a.max_degree = len(DEGREES), max(DEGREES)
        a.Xp, a.ldp, a.freqs, a.tau = Xp.data_ptr(), Xp.stride(0), fr.data_ptr(), tau
        a.out_scale, a.has_mass, a.mass_fn, a.mass_scale = OUT_SCALE, HAS_MASS, 0, 1.0
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        for k, v in fields.items():
            setattr(a, k, v)
        return a

    _lib.check(L.fsw_embed_generic(ctypes.byref(args(out=out.data_ptr(), ldo=out.stride(0))), stream), "fsw_embed_generic")
    _lib.check(L.fsw_embed_generic(ctypes.byref(args(g=g.data_ptr(), ldg=g.stride(0), gkey=gkey.data_ptr(), ldk=S, gfreq=gf.data_ptr())),
                                   stream), "fsw_embed_generic (backward)")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), gkey.cpu().numpy().astype(np.float64), gf.cpu().numpy()


@pytest.mark.parametrize("storage", ["float64", "float32"])
@pytest.mark.parametrize("weights,tau", MODES)
def test_generic_kernel_on_tied_keys(dev, weights, tau, storage):
    """fsw_embed_generic (the yardstick of the Cartesian and weight-gradient tests) on the same plain CSR and the 8 key columns,
    forward and backward: float64 storage per row <= G64_ROW (forward and gkey) and per entry 1e-10 of the line maximum; float32 storage at
    the bounds of the tuned kernels.
    The float64 per-entry check floors the line maximum at 2e-4 of the line's scale: the oracle itself evaluates sin(pi xi w) with
    an argument rounded to float64, an absolute error of 2 pi xi 2^-53 <= 1e-14 of the scale at xi = 13, i.e. 1e-10 of a line of
    1e-4 of the scale (measured on the vanishing lines, where the kernel's sinpi returns an exact 0: 5.9e-15 of the scale)."""
    S = 8
    ref = diagonal_reference(weights, tau, S)
    rowptr = tied_case(weights)["rowptr"]
    got, gkey, gf = run_generic_kernel(dev, weights, tau, storage)
    what = "generic %s %s tau %g" % (storage, weights, tau)
    if storage == "float64":
        errs = np.array([relerr(got[r], ref["out"][r]) for r in range(len(DEGREES))])
        print("%s: forward per row max %.2e" % (what, errs.max()))
        assert np.isfinite(got).all() and errs.max() <= G64_ROW, (what, errs)
        check_key_gradients(gkey, ref["gkey"], rowptr, COLUMNS[:S], what, ref["scale"], row_bound=G64_ROW, entry_bound=G64_ROW,
                            floor=2e-4)
        assert relerr(gf, ref["gfreq"]) <= G64_ROW
    else:
        check_forward(got, ref["out"], what)
        check_key_gradients(gkey, ref["gkey"], rowptr, COLUMNS[:S], what, ref["scale"])
        e = relerr(gf, ref["gfreq"])
        print("%s: gfreq %.2e" % (what, e))
        assert e <= F32_BOUND, (what, e)


CART_COLUMNS = [(0, 1, 2, 5), (3, 4, 6, 5)]      # indices into COLUMNS: (a, b, c, e) and (d_up, d_down, b, e)


def run_cartesian_kernels(dev, weights, tau, cols, F, freqs=FREQS, kinds=COLUMNS, ladder=None, flags=0):
    """fsw_embed_cart_f32 and fsw_embed_cart_backward_keys_f32, S = len(cols) slices (key columns cols of `kinds`) x F frequencies
    freqs[:F], on the graph of DEGREES (or of `ladder`): (out [rows, 1 + S F], gkey [nnz, S], gfreq [F]).  flags: fsw_cart_args.flags
    of both calls (the split forms of the longest rows); the scratch then also holds what every split query asks for."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    S = len(cols)
    c = tied_case(weights, kinds) if ladder is None else tied_case(weights, kinds, ladder, tau)
    graph, st, DEGREES, NNZ = c["graph"], c["st"], c["degrees"], c["nnz"]
    stream = torch.cuda.current_stream(dev).cuda_stream
    Xp_host = np.zeros((NNZ, 32), dtype=np.float32)
    Xp_host[:, :S] = c["Xp"][:, list(cols)]
    Xp = t(Xp_host, dev)
    fr = t(np.array(freqs[:F]), dev)
    g = t(c["g"][:, :HAS_MASS + S * F], dev)
    unit_fast = weights == "unit" and tau <= 1.0
    table = dtable = None
    if unit_fast:
        table = torch.empty((int(L.fsw_unit_table_rows(_lib.REG_MAX_DEG)), F), device=dev)
        dtable = torch.empty_like(table)
        _lib.check(L.fsw_unit_coeff_table(_lib.ptr(fr), F, _lib.REG_MAX_DEG, _lib.ptr(table), F, stream), "fsw_unit_coeff_table")
        _lib.check(L.fsw_unit_dcoeff_table(_lib.ptr(fr), F, _lib.REG_MAX_DEG, _lib.ptr(dtable), F, stream), "fsw_unit_dcoeff_table")
    scratch = None

    def args():
        a = _lib.CartArgs()
        a.value_dtype, a.S, a.F, a.has_mass, a.flags = 0, S, F, HAS_MASS, flags
        a.rowptr, a.col, a.w = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.w.data_ptr() if graph.w is not None else None
        a.perm, a.bin_start, a.bin_start_host = graph.perm.data_ptr(), graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data
        a.num_rows, a.max_degree = len(DEGREES), st[_lib.STAT_MAX_DEGREE]
        a.Xp, a.ldp, a.freqs, a.tau, a.out_scale = Xp.data_ptr(), Xp.stride(0), fr.data_ptr(), tau, OUT_SCALE
        a.mass_fn, a.mass_scale = 0, 1.0
        if table is not None:
            a.unit_table, a.ldt = table.data_ptr(), F
        if scratch is not None:
            a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        return a

    nbytes = int(L.fsw_embed_cart_generic_scratch_bytes(max(DEGREES), len(DEGREES)))
    if flags:
        queries = (L.fsw_embed_cart_split_scratch_bytes, L.fsw_embed_cart_split_backward_scratch_bytes,
                   L.fsw_embed_cart_split_w_scratch_bytes, L.fsw_embed_cart_split_w_backward_scratch_bytes)
        nbytes = max([nbytes] + [int(q(ctypes.byref(args()))) for q in queries])
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.full((len(DEGREES), HAS_MASS + S * F), float("nan"), device=dev)
    a = args()
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    _lib.check(L.fsw_embed_cart_f32(ctypes.byref(a), stream), "fsw_embed_cart_f32")
    gkey = torch.full((NNZ, S), float("nan"), device=dev)
    gf = torch.zeros(F, device=dev)
    a = args()
    a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g.data_ptr(), g.stride(0), gkey.data_ptr(), S, gf.data_ptr()
    _lib.check(L.fsw_embed_cart_backward_keys_f32(ctypes.byref(a), _lib.ptr(dtable), F, stream), "fsw_embed_cart_backward_keys_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), gkey.cpu().numpy().astype(np.float64), gf.cpu().numpy()


@pytest.mark.parametrize("cols", CART_COLUMNS)
@pytest.mark.parametrize("weights,tau", MODES)
def test_cartesian_kernels_on_tied_keys(dev, weights, tau, cols):
    """fsw_embed_cart_f32 and fsw_embed_cart_backward_keys_f32, S = 4 slices x F = 5 frequencies, on the same graph and key columns
    (two sets of four, each with the control column); the rows above 2048 neighbours run the generic kernel inside these entries.
    Same per-row, per-entry and gfreq assertions as the diagonal kernels."""
    F = 5
    ref = cartesian_reference(weights, tau, cols, F)
    rowptr = tied_case(weights)["rowptr"]
    names = [COLUMNS[i] for i in cols]
    what = "cartesian %s tau %g columns %s" % (weights, tau, ",".join(names))
    out, gkey, gf = run_cartesian_kernels(dev, weights, tau, cols, F)
    check_forward(out, ref["out"], what)
    check_key_gradients(gkey, ref["gkey"], rowptr, names, what, ref["scale"])
    e = relerr(gf, ref["gfreq"])
    print("%s: gfreq %.2e" % (what, e))
    assert e <= F32_BOUND, (what, e)


# ---- 3. module level: duplicate nodes -----------------------------------------------------------------------------------------------
MODULE_DEGREES = (20, 130, 700, 3000)


def duplicate_nodes(weighted):
    """Readout-shaped graph, one sender per entry; the senders' feature rows are drawn from 40 vectors, one of them zero."""
    rng = np.random.default_rng(51)
    n, d = sum(MODULE_DEGREES), 5
    proto = rng.standard_normal((40, d)).astype(np.float32)
    proto[0] = 0.0
    which = rng.integers(0, 40, size=n)
    which[:6] = [0, 3, 0, 3, 0, 7]                                # the row of 20 holds the zero vector more than once
    rec = np.repeat(np.arange(len(MODULE_DEGREES)), MODULE_DEGREES).astype(np.int64)
    w = None
    if weighted:
        w = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), size=n)
        w[rec == 0] *= np.float32(0.4) / w[rec == 0].sum(dtype=np.float32)     # mass-deficient: the pad element ties with the zero vectors
    return proto[which], which, rec, w, np.concatenate([[0], np.cumsum(MODULE_DEGREES)])


def make_module(dev, V, fr, **kw):
    from fsw_gnn_amd import FSW_embedding
    E = FSW_embedding(d_in=V.shape[1] - kw.get("d_edge", 0), d_out=V.shape[0], device=dev, enable_bias=False, learnable_slices=True,
                      learnable_freqs=True, **kw)
    with torch.no_grad():
        E.projVecs.copy_(t(V, dev))
        E.freqs.copy_(t(fr, dev))
    return E


def hip_projection(E, X, d):
    """float32 X . projVecs[:, :d]^T of the path under test: decides the oracle's order."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    Xc, V = X.detach().contiguous(), E.projVecs.detach()
    n, S = Xc.shape[0], E.nSlices
    Xp = torch.empty((n, (S + 63) // 64 * 64), dtype=torch.float32, device=Xc.device)
    _lib.check(L.fsw_project_f32(Xc.data_ptr(), n, d, Xc.stride(0), V.data_ptr(), S, V.stride(0), Xp.data_ptr(), Xp.stride(0), None, 0, None,
                                 torch.cuda.current_stream(Xc.device).cuda_stream), "fsw_project_f32")
    return Xp[:, :S].cpu().numpy()


def check_module_rows(got, ref, bound, rowptr, what):
    """got, ref [n, q] per sender = per entry; bound [n, q] per entry; and per row norm-wise <= F32_BOUND."""
    assert np.isfinite(got).all()
    rows = per_row(lambda a, b: relerr(got[a:b], ref[a:b]), rowptr)
    ratio = (np.abs(got - ref) / bound).max()
    print("%s: per row max %.2e, per entry max %.2f of the bound" % (what, rows.max(), ratio))
    assert rows.max() <= F32_BOUND, (what, rows)
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("weighted", [False, True])
def test_module_duplicate_nodes(dev, weighted):
    """FSW_embedding.embed_autograd on rows of 20 / 130 / 700 / 3000 neighbours whose feature rows repeat (40 distinct vectors, one all
    zero): identical feature rows project to bit-identical keys, so every row holds large tie groups; weighted, the row of 20 has
    total mass 0.4 and its pad element ties with the zero vectors.  The oracle ranks by the HIP projection.  out per row <= TOL;
    gX row by row -- rows of one tie group differ only through their rank -- per row <= F32_BOUND and per entry within PER_ENTRY of
    the line maxima carried through projVecs, sum_s PER_ENTRY * linemax[row, s] * |V[s, j]| (the float32 GEMM's own rounding, below
    5e-7 of the same sum, is inside it); gV and gfreqs <= F32_BOUND."""
    from fsw_gnn_amd import build_csr
    X, which, rec, w, rowptr = duplicate_nodes(weighted)
    n, S = X.shape[0], 8
    V = cases.synth.unit_slices(S, X.shape[1], seed=52)
    fr = np.array(FREQS[:S], dtype=np.float32)
    E = make_module(dev, V, fr)
    Xd = t(X, dev).requires_grad_(True)
    snd = np.arange(n)
    graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None if w is None else t(w, dev), len(MODULE_DEGREES), n)
    R = np.random.default_rng(53).standard_normal((len(MODULE_DEGREES), S))
    out = E.embed_autograd(Xd, graph)
    (out * t(R, dev)).sum().backward()
    xp = hip_projection(E, Xd, X.shape[1])
    for v in range(40):
        assert np.unique(xp[which == v], axis=0).shape[0] == 1, v     # identical feature rows: bit-identical keys
    assert not xp[which == 0].any()
    wv = np.ones(n) if w is None else w.astype(np.float64)
    ref_out = O.fsw_embed_csr(X, rowptr, snd, wv, V, fr)
    gX, gV, gxi, gkey = O.fsw_embed_csr_backward(X, rowptr, snd, wv, V, fr, R, Xp_override=xp, return_gkey=True)
    what = "module duplicate nodes, %s" % ("weighted" if weighted else "unit")
    got_out = out.detach().cpu().numpy()
    errs = np.array([relerr(got_out[r], ref_out[r]) for r in range(len(MODULE_DEGREES))])
    print("%s: forward per row max %.2e" % (what, errs.max()))
    assert errs.max() <= TOL, errs
    bound = PER_ENTRY * line_maxima(gkey, rowptr) @ np.abs(V.astype(np.float64))
    check_module_rows(Xd.grad.cpu().numpy().astype(np.float64), gX, bound, rowptr, what + " gX")
    egV, egf = relerr(E.projVecs.grad.cpu().numpy(), gV), relerr(E.freqs.grad.cpu().numpy(), gxi)
    print("%s: gV %.2e gfreqs %.2e" % (what, egV, egf))
    assert egV <= F32_BOUND and egf <= F32_BOUND


def test_module_duplicate_nodes_with_edge_features(dev):
    """The same duplicate nodes with one edge feature in {0, 1} whose slice weight is 0.5 in every slice, coalesced graph with general
    weights: the key of an entry is its sender's projection plus 0 or exactly 0.5, so the tie groups split in two and stay exact.  The
    gradient of the edge features, 0.5 * sum_s gkey[e, s], is the per-entry check (against the oracle's g_edge_feat, bound
    sum_s PER_ENTRY * linemax[row, s] * 0.5), next to gX as above, gV (both parts) and gfreqs."""
    from fsw_gnn_amd.graph import build_csr_coalesced
    X, which, rec, w, rowptr = duplicate_nodes(True)
    n, d, S = X.shape[0], X.shape[1], 8
    rng = np.random.default_rng(54)
    ef = rng.integers(0, 2, size=(n, 1)).astype(np.float32)
    V = np.concatenate([cases.synth.unit_slices(S, d, seed=52), np.full((S, 1), 0.5, dtype=np.float32)], axis=1)
    fr = np.array(FREQS[:S], dtype=np.float32)
    E = make_module(dev, V, fr, d_edge=1)
    Xd = t(X, dev).requires_grad_(True)
    efd = t(ef, dev).requires_grad_(True)
    snd = np.arange(n)
    graph = build_csr_coalesced(t(rec, dev, torch.int64), t(snd, dev, torch.int64), t(w, dev), efd.detach(), len(MODULE_DEGREES), n,
                                want_slots=True)
    assert np.array_equal(graph.slot_of_edge.cpu().numpy()[:n], np.arange(n))      # (recipient, sender) order = the input order
    R = np.random.default_rng(55).standard_normal((len(MODULE_DEGREES), S))
    out = E.embed_autograd(Xd, graph, edge_feat=efd)
    (out * t(R, dev)).sum().backward()
    xp = hip_projection(E, Xd, d).astype(np.float64)
    keys = (xp + 0.5 * ef.astype(np.float64)).astype(np.float32)    # one rounding, like the kernels' fma
    for v in range(40):
        for bit in (0.0, 1.0):
            sel = (which == v) & (ef[:, 0] == bit)
            assert np.unique(keys[sel], axis=0).shape[0] <= 1
    wv = w.astype(np.float64)
    ref_out = O.fsw_embed_csr(X, rowptr, snd, wv, V, fr, edge_feat=ef)
    gX, gV, gxi, gef, gkey = O.fsw_embed_csr_backward(X, rowptr, snd, wv, V, fr, R, edge_feat=ef, keys_override=keys, return_gkey=True)
    what = "module duplicate nodes, edge features"
    got_out = out.detach().cpu().numpy()
    errs = np.array([relerr(got_out[r], ref_out[r]) for r in range(len(MODULE_DEGREES))])
    print("%s: forward per row max %.2e" % (what, errs.max()))
    assert errs.max() <= TOL, errs
    lm = line_maxima(gkey, rowptr)
    check_module_rows(efd.grad.cpu().numpy().astype(np.float64), gef, PER_ENTRY * lm @ np.full((S, 1), 0.5), rowptr, what + " g_edge_feat")
    check_module_rows(Xd.grad.cpu().numpy().astype(np.float64), gX, PER_ENTRY * lm @ np.abs(V[:, :d].astype(np.float64)), rowptr, what + " gX")
    egV, egf = relerr(E.projVecs.grad.cpu().numpy(), gV), relerr(E.freqs.grad.cpu().numpy(), gxi)
    print("%s: gV %.2e gfreqs %.2e" % (what, egV, egf))
    assert egV <= F32_BOUND and egf <= F32_BOUND
