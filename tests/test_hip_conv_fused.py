"""The C entry points behind the fused layer, called directly and checked per entry against float64 numpy (tests/conv_fused_ref.py):
fsw_unit_coeff_table, fsw_pack_linear_f32, fsw_add_bias_act_f32, fsw_conv_fused_f32, fsw_project_linear_f32 and
fsw_conv_fused_cart_f32, and the layer itself on a graph that holds every in-degree 0 .. 32.

The graphs are degree ladders: recipients of EVERY in-degree 0 .. 32, so that each of the 33 sorting networks and every row of the
coefficient table is used, in counts of 1, 31, 32, 33, 127, 128, 129 and 257 rows per degree, so that the 32-row and the 128-row
tile are met empty but for one row, one short, full and one over.  Ladders A and B shift the counts by four degrees: every degree
meets a small count and a count >= 127.  Senders are drawn with replacement (tied keys), a few sender rows are scaled by 1e3 and
1e-3, duplicated or all +-0.0, and the frequencies hold 0, -0.0, -1, 1, 2 and 0.5.

Every entry of a row of degree <= 32 must lie within the derived bound of the float64 value (conv_fused_ref: (D + K + 8) 2^-24 of the
sum of absolute values of the terms; tests/test_conv_fused_ref_cpu.py shows that plain float32 arithmetic uses less than half of
it and that one wrong coefficient, column, bias, row or weight interleave leaves it).  The outputs are pre-filled with NaN: rows
above 32 neighbours and the padding columns must still be NaN afterwards, every other entry must be finite."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests import conv_fused_ref as R
from tests.conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5            # forward, norm-wise (tests/test_hip_parity.py)
LADDERS = {"A": dict(offset=0), "B": dict(offset=4), "A_long": dict(offset=0, long_rows=True), "B_long": dict(offset=4, long_rows=True),
           "small": dict(offset=0, counts=(1, 33)), "small_long": dict(offset=0, counts=(1, 33), long_rows=True)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def f32(x):
    """A Python float as the float32 the C ABI receives."""
    return float(np.float32(x))


def stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def last_error():
    from fsw_gnn_amd import _lib
    return _lib.lib().fsw_last_error().decode()


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder_graph(name):
    """The ladder `name` of LADDERS as a CSRGraph on the device, with host copies; its CSR must be the plain numpy one."""
    from fsw_gnn_amd import _lib, build_csr
    dev = torch.device("cuda:0")
    rec, snd, nr, nc = R.ladder(**LADDERS[name])
    graph = build_csr(t(rec, dev, torch.int64), t(snd, dev, torch.int64), None, nr, nc, want_invperm=True)
    st = graph.read_stats()
    rowptr = graph.rowptr.cpu().numpy().astype(np.int64)
    col = graph.col[:rec.size].cpu().numpy().astype(np.int64)
    want_rp, want_col = R.csr_of(rec, snd, nr)
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_NNZ] == rec.size
    assert np.array_equal(rowptr, want_rp)
    rows = np.repeat(np.arange(nr), np.diff(rowptr))
    assert np.array_equal(np.sort(rows * nc + col), np.sort(rows * nc + want_col))
    deg = np.diff(rowptr)
    perm = graph.perm.cpu().numpy().astype(np.int64)
    invperm = graph.invperm.cpu().numpy().astype(np.int64)
    assert np.array_equal(perm[invperm], np.arange(nr)) and not np.array_equal(perm, np.arange(nr))
    bins = graph.bin_start_host[0].astype(np.int64)
    counts = LADDERS[name].get("counts", R.DEFAULT_COUNTS)
    off = LADDERS[name]["offset"]
    assert np.diff(bins)[:33].tolist() == [counts[(D + off) % len(counts)] for D in range(33)]
    assert st[_lib.STAT_MAX_DEGREE] == (2049 if LADDERS[name].get("long_rows") else 32)
    dup = sum(np.unique(col[rowptr[r]:rowptr[r + 1]]).size < deg[r] for r in np.nonzero((deg >= 16) & (deg <= 32))[0])
    assert dup >= 10                                              # duplicates inside a row: tied keys
    return dict(graph=graph, st=st, rowptr=rowptr, col=col, deg=deg, perm=perm, invperm=invperm, bins=bins, nr=nr, nc=nc)


def unit_table(dev, fr_dev, S, ldt):
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    rows = int(L.fsw_unit_table_rows(_lib.REG_MAX_DEG))
    table = torch.full((rows, ldt), float("nan"), device=dev)
    _lib.check(L.fsw_unit_coeff_table(_lib.ptr(fr_dev), S, _lib.REG_MAX_DEG, _lib.ptr(table), ldt, stream_of(dev)), "fsw_unit_coeff_table")
    return table


def pack(dev, W1, Hout, K):
    """fsw_pack_linear_f32 of a float32 W1 [Hout, K]."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    Wd = t(W1, dev)
    Wq = torch.full((int(L.fsw_packed_linear_floats(K, Hout)),), float("nan"), device=dev)
    _lib.check(L.fsw_pack_linear_f32(_lib.ptr(Wd), K, Hout, 0, K, _lib.ptr(Wq), None, 0, None, 0, stream_of(dev)), "fsw_pack_linear_f32")
    return Wq


def check_entries(Y, Y_ref, bound, g, Hout, tile_rows, what, act=0):
    """Assertions (ii) - (v) of a fused call: rows of degree <= 32 finite and within the bound entry by entry (the worst entry is
    named), norm-wise below TOL without activation, rows above 32 neighbours and the padding columns still NaN.  Returns the
    largest |err| / bound."""
    deg = g["deg"]
    short = deg <= 32
    assert np.isnan(Y[~short]).all(), what + ": rows above 32 neighbours were written"
    assert np.isnan(Y[:, Hout:]).all(), what + ": padding columns were written"
    got = Y[short, :Hout].astype(np.float64)
    ref, bnd = Y_ref[short], bound[short]
    assert np.isfinite(got).all(), (what, "rows never written (degrees)", sorted(set(deg[short][~np.isfinite(got).all(axis=1)].tolist())))
    err = np.abs(got - ref)
    ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))
    i, j = np.unravel_index(ratio.argmax(), ratio.shape)
    node = np.nonzero(short)[0][i]
    D = int(deg[node])
    pos = int(g["invperm"][node] - g["bins"][D])
    worst = "degree %d, row %d of its bin (%d in its %d-row tile), column %d: got %.9g, want %.9g, bound %.3g" % (
        D, pos, pos % tile_rows, tile_rows, j, got[i, j], ref[i, j], bnd[i, j])
    print("%s: largest |err| / bound %.3f (%s)" % (what, ratio.max(), worst))
    assert (err <= bnd).all(), (what, worst, "%d entries outside the bound" % int((err > bnd).sum()))
    if act == 0:
        assert relerr(got, ref) < TOL, what
    return float(ratio.max())


# ---- 3. fsw_unit_coeff_table ------------------------------------------------------------------------------------------------------
def test_unit_coeff_table_against_float64(dev):
    """Every entry within one float32 rounding of the float64 formula (+ 1e-13 for the library's own float64 evaluation at |xi| <= 3);
    the columns S .. ldt - 1 keep the sentinel."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    for S in (1, 6, 64):
        fr = R.freqs(S)
        ldt = S + 3
        rows = int(L.fsw_unit_table_rows(_lib.REG_MAX_DEG))
        assert rows == 32 * 33 // 2
        table = torch.full((rows, ldt), -777.0, device=dev)
        assert L.fsw_unit_coeff_table(_lib.ptr(t(fr, dev)), S, _lib.REG_MAX_DEG, _lib.ptr(table), ldt, stream_of(dev)) == 0
        tab = table.cpu().numpy()
        T = R.unit_coeffs_flat(fr)
        assert (tab[:, S:] == -777.0).all()
        err = np.abs(tab[:, :S].astype(np.float64) - T)
        lim = R.U * np.abs(T) + 1e-13
        r, k = np.unravel_index((err - lim).argmax(), err.shape)
        print("S = %d: largest |tab - T| / (2^-24 |T| + 1e-13) = %.3f" % (S, (err / lim).max()))
        assert (err <= lim).all(), (S, "row %d, column %d (xi = %g)" % (r, k, fr[k]), tab[r, k], T[r, k])


# ---- 4. fsw_pack_linear_f32, fsw_add_bias_act_f32 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Hout,K", [(1, 1), (31, 7), (32, 8), (33, 9), (128, 64), (129, 65), (300, 257)])
def test_pack_linear_bitwise(dev, Hout, K):
    """Bitwise equal to the header's formula for col0 in {0, 5}, with and without the W2 block (whose padding keeps a sentinel)."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    d2 = 5
    for col0 in (0, 5):
        ldw_in = col0 + K + d2 + 3
        W = np.random.default_rng(10 * Hout + K + col0).standard_normal((Hout, ldw_in)).astype(np.float32)
        Wd = t(W, dev)
        want = R.pack_reference(W, ldw_in, Hout, col0, K)
        nq = int(L.fsw_packed_linear_floats(K, Hout))
        assert nq == want.size == ((K + 7) // 8 + 16) * (32 * ((Hout + 31) // 32)) * 8
        for with_w2 in (False, True):
            Wq = torch.full((nq,), float("nan"), device=dev)
            W2out = torch.full((Hout, d2 + 2), -777.0, device=dev)
            w2 = ctypes.c_void_p(Wd.data_ptr() + 4 * (col0 + K)) if with_w2 else None
            rc = L.fsw_pack_linear_f32(_lib.ptr(Wd), ldw_in, Hout, col0, K, _lib.ptr(Wq), w2, d2 if with_w2 else 0,
                                       _lib.ptr(W2out) if with_w2 else None, d2 + 2 if with_w2 else 0, stream_of(dev))
            assert rc == 0, last_error()
            assert np.array_equal(Wq.cpu().numpy().view(np.uint32), want.view(np.uint32)), (Hout, K, col0, with_w2)
            out2 = W2out.cpu().numpy()
            if with_w2:
                assert np.array_equal(out2[:, :d2].view(np.uint32), np.ascontiguousarray(W[:, col0 + K:col0 + K + d2]).view(np.uint32))
                assert (out2[:, d2:] == -777.0).all()
            else:
                assert (out2 == -777.0).all()
            assert np.array_equal(Wd.cpu().numpy().view(np.uint32), W.view(np.uint32))
    buf = torch.full((nq + 4,), float("nan"), device=dev)
    rc = L.fsw_pack_linear_f32(_lib.ptr(Wd), ldw_in, Hout, col0, K, ctypes.c_void_p(buf.data_ptr() + 4), None, 0, None, 0, stream_of(dev))
    assert rc != 0 and "aligned" in last_error()
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


def bias_act_reference(Rm, Yin, bias, act, slope):
    """np.float32 in the kernel's order: R + Yin, then + bias, then the activation."""
    y = Rm.copy()
    if Yin is not None:
        y = y + Yin
    if bias is not None:
        y = y + bias[None, :]
    if act == 1:
        y = np.maximum(y, np.float32(0))
    elif act == 2:
        y = np.where(y >= 0, y, np.float32(slope) * y)
    assert y.dtype == np.float32
    return y


def run_bias_act(dev, rows, H, with_yin, with_bias, act, seed):
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(seed)
    ldr, ldyin = H + 1, H + 2
    Rm = rng.standard_normal((rows, ldr)).astype(np.float32)
    Rm[:, H:] = -777.0
    Yin = rng.standard_normal((rows, ldyin)).astype(np.float32) if with_yin else None
    bias = rng.standard_normal(H).astype(np.float32) if with_bias else None
    Rd, Yd, bd = t(Rm, dev), (t(Yin, dev) if with_yin else None), (t(bias, dev) if with_bias else None)
    rc = L.fsw_add_bias_act_f32(_lib.ptr(Rd), ldr, _lib.ptr(Yd), ldyin if with_yin else 0, _lib.ptr(bd), rows, H, act, 0.2, stream_of(dev))
    assert rc == 0, last_error()
    got = Rd.cpu().numpy()
    want = bias_act_reference(Rm[:, :H], None if Yin is None else Yin[:, :H], bias, act, 0.2)
    what = (rows, H, with_yin, with_bias, act)
    assert np.array_equal(got[:, :H].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), what
    assert (got[:, H:] == -777.0).all(), what
    if with_yin:
        assert np.array_equal(Yd.cpu().numpy().view(np.uint32), Yin.view(np.uint32)), what


@pytest.mark.parametrize("H", [1, 3, 4, 5, 12, 128, 129])
def test_add_bias_act_bitwise(dev, H):
    """R = act(R + Yin + bias) bitwise, ldr = H + 1 (misaligned rows), Yin and bias present and absent, every activation, 1 and
    4097 rows; the padding column keeps its sentinel."""
    seed = 0
    for rows in (1, 4097):
        for with_yin in (False, True):
            for with_bias in (False, True):
                for act in (0, 1, 2):
                    seed += 1
                    run_bias_act(dev, rows, H, with_yin, with_bias, act, 100 * H + seed)


def test_add_bias_act_grid_stride_and_no_rows(dev):
    """40000 x 128: more float4 items than the 4096 x 256 threads of the largest grid, so the grid-stride loop wraps; rows = 0
    returns 0 and writes nothing."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    assert 40000 * (128 // 4) > 4096 * 256
    run_bias_act(dev, 40000, 128, True, True, 2, 5)
    Rd = torch.full((4, 9), -777.0, device=dev)
    assert L.fsw_add_bias_act_f32(_lib.ptr(Rd), 9, None, 0, None, 0, 8, 1, 0.2, stream_of(dev)) == 0
    torch.cuda.synchronize()
    assert (Rd == -777.0).all()


# ---- 5. fsw_conv_fused_f32 --------------------------------------------------------------------------------------------------------
def run_fused(dev, g, S, hm, Hout, bias=False, mass_fn=0, mass_scale=1.0, out_scale=1.0, yin=None, ldyin_pad=0, lin_bias=False, act=0,
              slope=0.0, W1=None, yin_node=None, seed=0, mutate=None, reference=True, fr=None):
    """One call of fsw_conv_fused_f32 on the ladder graph g (ladder_graph).  yin: None, 'perm' (row p belongs to node perm[p]) or
    'node'.  mutate(args, call): edits the arguments before the call (refusal tests).  Returns a dict: rc, Y [rows, Hout + 3] as
    float32 numpy, and with reference=True E, A, Y_ref, bound.  Checks (vi): Yin, Wq and Xp are bitwise unchanged."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    graph, st, nr, nc = g["graph"], g["st"], g["nr"], g["nc"]
    K = hm + S
    rng = np.random.default_rng(1000 * S + 10 * Hout + seed)
    ldp, ldt, ldy = S + 3, S + 1, Hout + 3
    Xp = R.keys(nc, ldp, seed=11 + S)
    fr = R.freqs(S, seed=13 + S) if fr is None else np.asarray(fr, dtype=np.float32)     # fr: the S frequencies, instead of the drawn ones
    bias_h = rng.standard_normal(K).astype(np.float32) if bias else None
    if W1 is None:
        W1 = (rng.standard_normal((Hout, K)) / np.sqrt(K)).astype(np.float32)
    lb_h = rng.standard_normal(Hout).astype(np.float32) if lin_bias else None
    if yin is not None and yin_node is None:
        yin_node = rng.standard_normal((nr, Hout)).astype(np.float32)
    ldyin = Hout + ldyin_pad
    Yin_h = None
    if yin is not None:
        Yin_h = np.full((nr, ldyin), 555.0, dtype=np.float32)
        Yin_h[:, :Hout] = yin_node[g["perm"]] if yin == "perm" else yin_node
    out_scale, mass_scale, slope = f32(out_scale), f32(mass_scale), f32(slope)

    Xp_d, fr_d = t(Xp, dev), t(fr, dev)
    table = unit_table(dev, fr_d, S, ldt)
    Wq = pack(dev, W1, Hout, K)
    Wq_before = Wq.clone()
    bias_d = t(bias_h, dev) if bias else None
    lb_d = t(lb_h, dev) if lin_bias else None
    Yin_d = t(Yin_h, dev) if yin is not None else None
    Y = torch.full((nr, ldy), float("nan"), device=dev)
    a = _lib.EmbedArgs()
    a.rowptr, a.col, a.perm, a.bin_start = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.perm.data_ptr(), graph.bin_start.data_ptr()
    a.w, a.num_rows, a.bin_start_host = None, nr, graph.bin_start_host[0].ctypes.data
    a.Xp, a.ldp, a.freqs, a.S, a.tau = Xp_d.data_ptr(), ldp, fr_d.data_ptr(), S, 1.0
    a.unit_table, a.ldt = table.data_ptr(), ldt
    a.bias, a.out_scale, a.has_mass, a.mass_fn, a.mass_scale = _lib.ptr(bias_d), out_scale, hm, mass_fn, mass_scale
    a.num_reg_rows, a.num_lds_rows = st[_lib.STAT_NUM_REG], st[_lib.STAT_NUM_LDS]
    a.num_global_rows, a.num_zero_rows, a.max_degree = st[_lib.STAT_NUM_GLOBAL], st[_lib.STAT_NUM_ZERO], st[_lib.STAT_MAX_DEGREE]
    call = dict(ldw=32 * ((Hout + 31) // 32), Hout=Hout, ldyin=ldyin if yin is not None else 0, act=act, ldy=ldy)
    keep = []
    if mutate is not None:
        keep = mutate(a, call)
    rc = L.fsw_conv_fused_f32(ctypes.byref(a), _lib.ptr(Wq), call["ldw"], _lib.ptr(lb_d), call["Hout"], _lib.ptr(Yin_d), call["ldyin"],
                              1 if yin == "node" else 0, call["act"], slope, _lib.ptr(Y), call["ldy"], stream_of(dev))
    torch.cuda.synchronize()
    del keep
    out = dict(rc=rc, Y=Y.cpu().numpy(), K=K, tile_rows=128 if (S <= 32 and Hout <= 128) else 32)
    assert torch.equal(Wq.view(torch.int32), Wq_before.view(torch.int32))
    assert np.array_equal(Xp_d.cpu().numpy().view(np.uint32), Xp.view(np.uint32))
    if yin is not None:
        assert np.array_equal(Yin_d.cpu().numpy().view(np.uint32), Yin_h.view(np.uint32))
    if reference:
        E, A = R.embed_rows(g["rowptr"], g["col"], Xp, R.unit_coeffs(fr), bias_h, out_scale, hm, mass_fn, mass_scale)
        y0 = yin_node if yin is not None else lb_h
        Y_ref, bound = R.layer_reference(np.nan_to_num(E), np.nan_to_num(A), W1, g["deg"], yin=y0, act=act, slope=slope)
        out.update(E=E, A=A, Y_ref=Y_ref, bound=bound, W1=W1)
    return out


def largest_S(fn):
    """Largest S with fn(S) <= 64 KiB (fn is non-decreasing)."""
    S = 1
    while fn(S + 1) <= 65536:
        S += 1
    return S


def fused_S_max():
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    return largest_S(lambda S: int(L.fsw_conv_fused_lds_bytes(S, 1)))


FUSED_CASES = {
    # id: (ladder, S or None = largest accepted, has_mass, Hout, arguments): what it is there for
    "smallest_wide_tile": ("A", 1, 0, 1, dict()),
    "wide_tile_upper_corner": ("A", 32, 1, 128, dict(bias=True, mass_fn=1, mass_scale=0.7, out_scale=0.5, yin="perm", ldyin_pad=5, act=2, slope=0.2)),
    "wide_tile_two_slabs_long_rows": ("B_long", 7, 1, 33, dict(bias=True, mass_fn=2, yin="node", act=1)),
    "narrow_block_wide_layer": ("A", 32, 1, 129, dict(bias=True, yin="perm", act=2, slope=0.2)),
    "narrow_block_ten_slabs": ("B", 5, 0, 300, dict(lin_bias=True, act=1)),
    "one_chunk_four_row_groups": ("A", 33, 0, 31, dict()),
    "one_prefetch_round": ("A", 63, 1, 32, dict(bias=True, mass_fn=0, out_scale=-1.5)),
    "k_padding_7_lipschitz": ("A", 64, 1, 128, dict(yin="node", act=2, slope=-0.5)),
    "two_chunks_wide_epilogue": ("B_long", 65, 0, 160, dict(yin="perm", act=1)),
    "three_chunks_one_row_group": ("A", 129, 1, 64, dict(bias=True, lin_bias=True)),
    "five_chunks_second_wave_pass": ("A", 257, 0, 96, dict(act=2, slope=0.2)),
    "lds_limit_accepted": ("small", None, 1, 40, dict(bias=True, yin="perm", act=1)),
}


@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_conv_fused_per_entry(dev, case):
    """fsw_conv_fused_f32, one call per case: rc == 0, every entry of every row of degree <= 32 finite and within the bound, norm-wise
    < TOL without activation, rows above 32 neighbours and the padding columns of Y still NaN, inputs unchanged."""
    name, S, hm, Hout, kw = FUSED_CASES[case]
    if S is None:
        S = fused_S_max()
        assert S == 503
    g = ladder_graph(name)
    r = run_fused(dev, g, S, hm, Hout, **kw)
    assert r["rc"] == 0, last_error()
    if "long" in name:
        assert (g["deg"] > 32).sum() == 4
    check_entries(r["Y"], r["Y_ref"], r["bound"], g, Hout, r["tile_rows"], "%s (S %d, mass %d, Hout %d)" % (case, S, hm, Hout), kw.get("act", 0))


def test_conv_fused_lds_limit_refused(dev):
    """One slice more than the largest accepted S: non-zero, the message names LDS, Y untouched."""
    S = fused_S_max() + 1
    r = run_fused(dev, ladder_graph("small"), S, 1, 40, bias=True, yin="perm", act=1, reference=False)
    assert r["rc"] != 0 and "LDS" in last_error()
    assert np.isnan(r["Y"]).all()


def test_conv_fused_yin_row_order(dev):
    """Yin in perm order (row p belongs to node perm[p]) and Yin by node, built from the same by-node array: bitwise equal outputs."""
    g = ladder_graph("A")
    yin_node = np.random.default_rng(77).standard_normal((g["nr"], 128)).astype(np.float32)
    kw = dict(act=2, slope=-0.5, yin_node=yin_node)
    a = run_fused(dev, g, 64, 1, 128, yin="node", reference=False, **kw)
    b = run_fused(dev, g, 64, 1, 128, yin="perm", ldyin_pad=4, reference=False, **kw)
    assert a["rc"] == 0 and b["rc"] == 0
    assert np.isfinite(a["Y"][:, :128]).all()
    assert np.array_equal(a["Y"].view(np.uint32), b["Y"].view(np.uint32))


@pytest.mark.parametrize("K", [33, 65, 161])
def test_conv_fused_selector_weights(dev, K):
    """W1[j, :] = 2^(j % 5 - 2) e_pi(j), Hout = K (33: the 128-row tile; 65: the 32-row tile, three slabs staged through LDS; 161: the
    wide epilogue, Hout > 128, every wave storing its own slabs): every product but one per output is an exact zero and the
    scale a power of two, so Y[i, j] is the embedding entry itself, |Y - 2^m E[i, pi(j)]| <= (D + 4) 2^-24 2^m A[i, pi(j)] -- the bound
    without its K term.  Pins the k-interleave of the packed operand and the row / column map of the matrix instruction."""
    g = ladder_graph("A")
    pi = np.random.default_rng(K).permutation(K)
    scale = 2.0 ** (np.arange(K) % 5 - 2)
    W1 = np.zeros((K, K), dtype=np.float32)
    W1[np.arange(K), pi] = scale
    r = run_fused(dev, g, K - 1, 1, K, bias=True, mass_fn=1, W1=W1)
    assert r["rc"] == 0, last_error()
    Y_ref = r["E"][:, pi] * scale[None, :]
    bound = (g["deg"][:, None] + 4.0) * R.U * scale[None, :] * r["A"][:, pi]
    check_entries(r["Y"], Y_ref, bound, g, K, r["tile_rows"], "selector K = %d" % K)


def test_conv_fused_argument_checks(dev):
    """Refusals: each returns non-zero and leaves Y untouched."""
    g = ladder_graph("small")
    S, Hout = 8, 40
    wdummy = torch.ones(g["col"].size, device=dev)

    def set_w(a, call):
        a.w = wdummy.data_ptr()

    def set_tau(a, call):
        a.tau = 2.0

    def set_ldw(a, call):
        call["ldw"] = 64 + 8

    def set_ldy(a, call):
        call["ldy"] = Hout - 1

    def set_act(a, call):
        call["act"] = 3

    for name, mutate in [("w != NULL", set_w), ("tau = 2", set_tau), ("ldw % 32", set_ldw), ("ldy < Hout", set_ldy), ("act = 3", set_act)]:
        r = run_fused(dev, g, S, 1, Hout, mutate=mutate, reference=False)
        assert r["rc"] != 0 and last_error(), name
        assert np.isnan(r["Y"]).all(), name
    r = run_fused(dev, g, S, 1, Hout, reference=False)          # the same call without an edit is accepted
    assert r["rc"] == 0 and np.isfinite(r["Y"][:, :Hout]).all()


# ---- 6. fsw_project_linear_f32 ------------------------------------------------------------------------------------------------------
def run_project_linear(dev, X, V, S, W2, b2, row_map, ldp, ldy2, pads=(4, 4, 4)):
    """fsw_project_linear_f32 on host arrays X [n, d], V [S, d], W2 [H2, d]: (Xp [n, ldp], Y2 [n, ldy2], flags), outputs pre-filled
    with NaN.  pads: extra columns of the rows of X, V and W2 on the device."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    n, d = X.shape
    H2 = W2.shape[0]

    def padded(a, pad):
        out = np.full((a.shape[0], a.shape[1] + pad), 333.0, dtype=np.float32)
        out[:, :a.shape[1]] = a
        return t(out, dev)

    Xd, Vd, Wd = padded(X, pads[0]), padded(V, pads[1]), padded(W2, pads[2])
    bd = t(b2, dev) if b2 is not None else None
    md = t(row_map, dev, torch.int32) if row_map is not None else None
    Xp = torch.full((n, ldp), float("nan"), device=dev)
    Y2 = torch.full((n, ldy2), float("nan"), device=dev)
    stats = torch.zeros(_lib.NUM_STATS, dtype=torch.int32, device=dev)
    rc = L.fsw_project_linear_f32(_lib.ptr(Xd), n, d, Xd.stride(0), _lib.ptr(Vd), S, Vd.stride(0), _lib.ptr(Xp), ldp, _lib.ptr(Wd), H2,
                                  Wd.stride(0), _lib.ptr(bd), _lib.ptr(Y2), ldy2, _lib.ptr(md), _lib.ptr(stats), stream_of(dev))
    assert rc == 0, last_error()
    return Xp.cpu().numpy(), Y2.cpu().numpy(), int(stats.cpu()[_lib.STAT_FLAGS])


def full_significands(rng, shape):
    """float32 standard normal with the last significand bit set: all 24 bits in use."""
    a = rng.standard_normal(shape).astype(np.float32)
    return (a.view(np.uint32) | np.uint32(1)).view(np.float32)


@pytest.mark.parametrize("d", [4, 32, 64, 128, 256])
def test_project_linear_exact_cases(dev, d):
    """Inputs on which every partial sum of the bf16x3 product is representable (the accumulation argument of csrc/project.hip:
    x = x1 + x2 + x3, six products, each exact in the float32 accumulator), so the result must be bit-exact:
    (a) V rows one-hot times a power of two, X with full 24-bit significands: Xp[i, j] == X[i, k_j] 2^m;
    (b) the roles exchanged for the W2 block, b2 = None: Y2[row_map[i], j] == W2[j, k_i] 2^m;
    (c) both operands 1 + 2^-9 in one position: 1 + 2^-8 + 2^-18, which needs the x2 v2 term.
    Together: every one of the six planes, and the k mapping for every k < d."""
    rng = np.random.default_rng(d)
    ldp = 32 * ((d + 31) // 32) + 4
    pow2 = (2.0 ** (np.arange(d) % 5 - 2)).astype(np.float32)
    pi = rng.permutation(d)
    # (a)
    n = 33
    X = full_significands(rng, (n, d))
    V = np.zeros((d, d), dtype=np.float32)
    V[np.arange(d), pi] = pow2
    W2 = full_significands(rng, (5, d))
    Xp, _, flags = run_project_linear(dev, X, V, d, W2, None, None, ldp, 8)
    assert flags == 0
    assert np.array_equal(Xp[:, :d].view(np.uint32), np.ascontiguousarray(X[:, pi] * pow2[None, :]).view(np.uint32)), "(a)"
    # (b)
    n = d
    X = np.zeros((n, d), dtype=np.float32)
    X[np.arange(n), pi] = pow2
    W2 = full_significands(rng, (33, d))
    row_map = rng.permutation(n).astype(np.int32)
    _, Y2, _ = run_project_linear(dev, X, V, d, W2, None, row_map, ldp, 33 + 3)
    want = np.empty((n, 33), dtype=np.float32)
    want[row_map] = (W2[:, pi] * pow2[None, :]).T
    assert np.array_equal(Y2[:, :33].view(np.uint32), want.view(np.uint32)), "(b)"
    assert np.isnan(Y2[:, 33:]).all()
    # (c)
    one = np.float32(1.0 + 2.0 ** -9)
    X = np.zeros((d, d), dtype=np.float32)
    X[np.arange(d), pi] = one
    V = np.zeros((d, d), dtype=np.float32)
    V[np.arange(d), np.arange(d)] = one
    Xp, Y2, _ = run_project_linear(dev, X, V, d, V[:3], None, None, ldp, 4)
    want = np.zeros((d, d), dtype=np.float32)
    want[np.arange(d), pi] = np.float32(1.0 + 2.0 ** -8 + 2.0 ** -18)
    assert float(want.max()) == 1.0 + 2.0 ** -8 + 2.0 ** -18
    assert np.array_equal(Xp[:, :d], want), "(c)"
    assert np.array_equal(Y2[:, :3], want[:, :3]), "(c), second block"


# n, d, S, H2, row_map, b2, aligned Y2 (ldy2 a multiple of 4: 16-byte stores) -- every value of the issue's table occurs at least once
PROJECT_CASES = [
    (1, 4, 19, 1, False, True, False),
    (31, 36, 64, 31, True, False, False),
    (33, 128, 257, 32, False, True, True),
    (1000, 132, 19, 33, True, True, False),
    (1000, 256, 64, 160, True, False, True),
    (33, 13, 19, 33, True, True, False),           # d % 4 != 0: the generic kernel
    (1000, 128, 257, 160, False, True, False),
    (31, 256, 257, 1, True, True, True),
    (1, 13, 64, 31, False, False, False),
    (1000, 4, 257, 32, True, False, True),
    (33, 36, 19, 160, False, False, False),
    (31, 132, 64, 33, False, True, True),
]


@pytest.mark.parametrize("n,d,S,H2,mapped,with_b2,aligned", PROJECT_CASES)
def test_project_linear_random_cases(dev, n, d, S, H2, mapped, with_b2, aligned):
    """Xp = X V^T and Y2[row_map] = X W2^T + b2 per entry within (6 d + 8) 2^-24 sum |x| |v| (+ |b2|) of float64; every Y2 row is
    written exactly once (pre-filled with NaN, all finite afterwards, rows where row_map says), the padding of Y2 and of Xp keeps
    its NaN.  The matrix-core kernels store whole 32-column slabs of Xp (the caller pads its rows to 32 ceil(S / 32), the
    zero weights of the columns past S give exact zeros there): these columns may hold 0.0, nothing else; from the slab boundary on,
    and from S on in the generic kernel, the rows are untouched."""
    from fsw_gnn_amd import _lib
    rng = np.random.default_rng(n + 7 * d + 11 * S + 13 * H2)
    generic = d % 4 != 0
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = (rng.standard_normal((S, d)) / np.sqrt(d)).astype(np.float32)
    W2 = (rng.standard_normal((H2, d)) / np.sqrt(d)).astype(np.float32)
    b2 = rng.standard_normal(H2).astype(np.float32) if with_b2 else None
    row_map = rng.permutation(n).astype(np.int32) if mapped else None
    slab_end = S if generic else 32 * ((S + 31) // 32)
    ldp = slab_end + (3 if generic else 4)
    ldy2 = 4 * ((H2 + 3) // 4) if aligned else H2 + 3
    pads = (1, 2, 2) if generic else (4, 4, 4)
    Xp, Y2, flags = run_project_linear(dev, X, V, S, W2, b2, row_map, ldp, ldy2, pads)
    assert flags == 0
    X64 = X.astype(np.float64)
    ref1, bound1 = X64 @ V.astype(np.float64).T, R.project_bound(X, V)
    ref2 = X64 @ W2.astype(np.float64).T + (b2.astype(np.float64) if with_b2 else 0.0)
    bound2 = R.project_bound(X, W2, b2)
    assert np.isfinite(Xp[:, :S]).all() and np.isfinite(Y2[:, :H2]).all()
    pad = Xp[:, S:slab_end]
    assert (np.isnan(pad) | (pad == 0.0)).all()
    assert np.isnan(Xp[:, slab_end:]).all() and np.isnan(Y2[:, H2:]).all()
    got2 = Y2[row_map, :H2] if mapped else Y2[:, :H2]
    e1, e2 = np.abs(Xp[:, :S] - ref1), np.abs(got2 - ref2)
    print("n %d d %d S %d H2 %d: largest |err| / bound: Xp %.3f, Y2 %.3f" % (n, d, S, H2, (e1 / bound1).max(), (e2 / bound2).max()))
    assert (e1 <= bound1).all(), ("Xp", np.unravel_index((e1 / bound1).argmax(), e1.shape))
    assert (e2 <= bound2).all(), ("Y2", np.unravel_index((e2 / bound2).argmax(), e2.shape))
    assert relerr(Xp[:, :S], ref1) < TOL and relerr(got2, ref2) < TOL
    if (n, d) == (33, 128):                        # a non-finite X sets the flag
        X[5, 7] = np.inf
        _, _, flags = run_project_linear(dev, X, V, S, W2, b2, row_map, ldp, ldy2, pads)
        assert flags & _lib.FLAG_X_NONFINITE


# ---- 7. fsw_conv_fused_cart_f32 -------------------------------------------------------------------------------------------------------
def run_fused_cart(dev, g, S, F, hm, Hout, bias=False, mass_fn=0, mass_scale=1.0, out_scale=1.0, yin=None, lin_bias=False, act=0,
                   slope=0.0, reference=True):
    """One call of fsw_conv_fused_cart_f32 on the ladder graph g: the arguments of run_fused with K = hm + S F."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    graph, st, nr, nc = g["graph"], g["st"], g["nr"], g["nc"]
    K = hm + S * F
    rng = np.random.default_rng(1000 * S + 10 * Hout + F)
    ldp, ldt, ldy = S + 3, F + 1, Hout + 3
    Xp = R.keys(nc, ldp, seed=21 + S)
    fr = R.freqs(F, seed=23 + F)
    bias_h = rng.standard_normal(K).astype(np.float32) if bias else None
    W1 = (rng.standard_normal((Hout, K)) / np.sqrt(K)).astype(np.float32)
    lb_h = rng.standard_normal(Hout).astype(np.float32) if lin_bias else None
    yin_node = rng.standard_normal((nr, Hout)).astype(np.float32) if yin is not None else None
    ldyin = Hout + 1
    Yin_h = None
    if yin is not None:
        Yin_h = np.full((nr, ldyin), 555.0, dtype=np.float32)
        Yin_h[:, :Hout] = yin_node[g["perm"]] if yin == "perm" else yin_node
    out_scale, mass_scale, slope = f32(out_scale), f32(mass_scale), f32(slope)
    Xp_d, fr_d = t(Xp, dev), t(fr, dev)
    table = unit_table(dev, fr_d, F, ldt)
    Wq = pack(dev, W1, Hout, K)
    bias_d = t(bias_h, dev) if bias else None
    lb_d = t(lb_h, dev) if lin_bias else None
    Yin_d = t(Yin_h, dev) if yin is not None else None
    Y = torch.full((nr, ldy), float("nan"), device=dev)
    a = _lib.CartArgs()
    a.value_dtype, a.S, a.F, a.has_mass = 0, S, F, hm
    a.rowptr, a.col, a.w = graph.rowptr.data_ptr(), graph.col.data_ptr(), None
    a.perm, a.bin_start, a.bin_start_host = graph.perm.data_ptr(), graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data
    a.num_rows, a.max_degree = nr, st[_lib.STAT_MAX_DEGREE]
    a.Xp, a.ldp, a.freqs, a.tau, a.out_scale = Xp_d.data_ptr(), ldp, fr_d.data_ptr(), 1.0, out_scale
    a.unit_table, a.ldt = table.data_ptr(), ldt
    a.bias, a.mass_fn, a.mass_scale = _lib.ptr(bias_d), mass_fn, mass_scale
    rc = L.fsw_conv_fused_cart_f32(ctypes.byref(a), _lib.ptr(Wq), 32 * ((Hout + 31) // 32), _lib.ptr(lb_d), Hout, _lib.ptr(Yin_d),
                                   ldyin if yin is not None else 0, 1 if yin == "node" else 0, act, slope, _lib.ptr(Y), ldy, stream_of(dev))
    torch.cuda.synchronize()
    out = dict(rc=rc, Y=Y.cpu().numpy(), K=K)
    if reference:
        keys, frx = R.cartesian_expand(Xp, fr, S)
        E, A = R.embed_rows(g["rowptr"], g["col"], keys, R.unit_coeffs(frx), bias_h, out_scale, hm, mass_fn, mass_scale)
        y0 = yin_node if yin is not None else lb_h
        Y_ref, bound = R.layer_reference(E, A, W1, g["deg"], yin=y0, act=act, slope=slope)
        out.update(Y_ref=Y_ref, bound=bound)
    return out


def cart_F_max():
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    return largest_S(lambda F: int(L.fsw_conv_fused_cart_lds_bytes(1, F, 1)))


CART_CASES = {
    "smallest": ("A", 1, 1, 0, 1, dict()),
    "bias_branches_benchmark_shape": ("A", 16, 16, 1, 128, dict(bias=True, mass_fn=1, yin="perm", act=2, slope=0.2)),
    "bias_odd_F_wide_epilogue": ("A", 3, 5, 0, 160, dict(bias=True, lin_bias=True, act=1)),
    "degree0_bias_fill": ("B", 2, 70, 1, 33, dict(bias=True, yin="node")),
    "lds_limit_accepted": ("small", 1, None, 1, 40, dict(bias=True, yin="perm", act=1)),
}


@pytest.mark.parametrize("case", list(CART_CASES))
def test_conv_fused_cart_per_entry(dev, case):
    """fsw_conv_fused_cart_f32 where the layer cannot reach it (the embedding-bias branches: the degree-0 fill, the bias term of the
    readout, the bias inside the mass column; the S F limit), per entry against the Cartesian expansion, K = has_mass + S F."""
    name, S, F, hm, Hout, kw = CART_CASES[case]
    if F is None:
        F = cart_F_max()
        assert F == 503
    g = ladder_graph(name)
    r = run_fused_cart(dev, g, S, F, hm, Hout, **kw)
    assert r["rc"] == 0, last_error()
    check_entries(r["Y"], r["Y_ref"], r["bound"], g, Hout, 32, "cartesian %s (S %d, F %d, mass %d, Hout %d)" % (case, S, F, hm, Hout),
                  kw.get("act", 0))


def test_conv_fused_cart_refusals(dev):
    """One frequency past the S F limit, and a graph with rows above 32 neighbours: non-zero, Y all NaN."""
    r = run_fused_cart(dev, ladder_graph("small"), 1, cart_F_max() + 1, 1, 40, bias=True, reference=False)
    assert r["rc"] != 0 and "LDS" in last_error()
    assert np.isnan(r["Y"]).all()
    r = run_fused_cart(dev, ladder_graph("small_long"), 3, 5, 1, 40, bias=True, reference=False)
    assert r["rc"] != 0 and "rows of at most 32" in last_error()
    assert np.isnan(r["Y"]).all()


# ---- 8. the layer on the ladder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_ch,embed_dim", [(24, 65), (160, 33)])
def test_layer_on_degree_ladder(dev, out_ch, embed_dim):
    """FSW_conv on ladder B with long rows as a square graph (senders drawn from all nodes): every row within 1e-5 of the largest
    entry of its float64 reference row (oracle embedding, then the layer's own MLP in float64).  Degrees 31 / 32 and, at
    embed_dim = 33 and 160 outputs, the narrow-block / wide-layer kernel under the Python layer."""
    from fsw_gnn_amd import FSW_conv
    rec, snd, n, nc = R.ladder(offset=4, long_rows=True, square=True)
    assert nc == n
    ei = np.stack([snd, rec])
    X = np.random.default_rng(8).standard_normal((n, 12)).astype(np.float32)
    torch.manual_seed(out_ch)
    conv = FSW_conv(12, out_ch, embed_dim=embed_dim, device=dev)
    with torch.no_grad():
        assert conv._fusable()
        y = conv(t(X, dev), t(ei, dev, torch.int64)).cpu().numpy().astype(np.float64)
    em = conv.fsw_embed
    rowptr, col, w, _ = O.coalesce_edge_index(ei, n)
    emb = O.fsw_embedding_forward(X, rowptr, col, w, em.projVecs.detach().cpu().numpy(), em.freqs.detach().cpu().numpy(),
                                  encode_total_mass=em.encode_total_mass, total_mass_encoding_function=em.total_mass_encoding_function)
    h = torch.from_numpy(np.concatenate([conv.message_weight_vs_self * emb, X.astype(np.float64)], axis=1) if conv.concat_self else emb)
    with torch.no_grad():
        ref = conv.mlp.double().cpu()(h).numpy()
    deg = np.bincount(rec, minlength=n)
    assert set(range(33)) | set(R.LONG_DEGREES) == set(deg.tolist())
    assert np.isfinite(y).all()
    rowerr = np.abs(y - ref).max(axis=1) / np.abs(ref).max(axis=1)
    per_deg = {int(D): float(rowerr[deg == D].max()) for D in np.unique(deg)}
    print("layer %d -> %d, embed_dim %d: largest row error per degree: %s" % (12, out_ch, embed_dim,
          "  ".join("%d: %.1e" % kv for kv in per_deg.items())))
    worst = int(rowerr.argmax())
    assert (rowerr <= 1e-5).all(), ("node %d of degree %d" % (worst, deg[worst]), float(rowerr.max()), per_deg)
