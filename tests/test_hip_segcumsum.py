"""GPU tests of the segmented cumulative sum, entry by entry and to the bit.

The cases come from tests/segcumsum_cases.py: dyadic values whose sums are exact in any order, so the single-pass kernel
(k_segscan_chained: in-register scan, DPP scan, halo shortcut, descriptor look-back, persistent grid) and the legacy kernels must
reproduce an integer-arithmetic reference exactly -- every comparison here is equality.  Boundaries are placed from the geometry
that the library itself reports (fsw_segcumsum_geometry).  A reverse scan is given the flipped arrays, so that a boundary sits
at the same LOGICAL position in both directions; its expected result is the flipped forward reference.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import segcumsum_cases as S

pytestmark = pytest.mark.gpu

VALUE_DTYPE = {"float32": 0, "float64": 1}     # the C ABI's value_dtype
IDT_NP = {"int32": np.int32, "int64": np.int64}
VARIANTS = [(v, i, r) for v in ("float32", "float64") for i in ("int32", "int64") for r in (False, True)]
variants = pytest.mark.parametrize("vdt,idt,rev", VARIANTS, ids=["%s-%s-%s" % (v, i, "reverse" if r else "forward") for v, i, r in VARIANTS])
PAD = 16            # elements: packed cases start on multiples of 16 elements and are at least 16 elements apart
SENTINEL = 12345.0  # fills the gaps of packed buffers: a store outside a case's range shows


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(dev):
    from fsw_gnn_amd import _lib
    return _lib.lib()


def query(L, vdt, idt, rev):
    out = (ctypes.c_int32 * 4)()
    rc = L.fsw_segcumsum_geometry(VALUE_DTYPE[vdt], np.dtype(IDT_NP[idt]).itemsize, 1 if rev else 0, out)
    assert rc == 0, L.fsw_last_error().decode()
    return S.geometry(out[0], out[1], out[2]), int(out[3])


def scan_abi(L, vbuf, voff, ibuf, ioff, obuf, ooff, n, rev, ws):
    """fsw_segcumsum on element ranges [off, off + n) of three device buffers (checked here: the kernel is given raw pointers)"""
    from fsw_gnn_amd import _lib
    for buf, off in ((vbuf, voff), (ibuf, ioff), (obuf, ooff)):
        assert buf.is_contiguous() and buf.dim() == 1 and 0 <= off and off + n <= buf.numel()
    assert vbuf.dtype == obuf.dtype and ws.dtype == torch.uint8 and ws.numel() >= L.fsw_segcumsum_workspace_bytes(n)
    dnum = 0 if vbuf.dtype == torch.float32 else 1
    rc = L.fsw_segcumsum(dnum, vbuf.data_ptr() + voff * vbuf.element_size(), obuf.data_ptr() + ooff * obuf.element_size(),
                         ibuf.data_ptr() + ioff * ibuf.element_size(), ibuf.element_size(), n, 1 if rev else 0,
                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "fsw_segcumsum")


def directed(case, ref, rev):
    """(values, ids, expected) as the kernel gets them: flipped for a reverse scan"""
    if rev:
        return case.values[::-1].copy(), case.ids[::-1].copy(), ref[::-1].copy()
    return case.values, case.ids, ref


def as_ids(ids, idt):
    out = ids.astype(idt)
    assert np.array_equal(out.astype(np.int64), ids)
    return out


class Packed:
    """Many small cases in a few device buffers: values, ids and expected results once with every case on a 64-byte boundary
    and once with every case one element past it."""

    def __init__(self, cases, refs, vdt, idt, rev, dev):
        self.names, self.spans = [], []
        o = 0
        for c in cases:
            self.names.append(c.name)
            self.spans.append((o, len(c.ids)))
            o += -(-len(c.ids) // PAD) * PAD + PAD
        self.total = o
        hv = np.full(o, SENTINEL, dtype=vdt)
        hi = np.zeros(o, dtype=idt)
        hr = np.full(o, SENTINEL, dtype=vdt)
        for c, ref, (a, n) in zip(cases, refs, self.spans):
            v, ids, want = directed(c, ref, rev)
            hv[a:a + n], hi[a:a + n], hr[a:a + n] = v, as_ids(ids, idt), want
        self.host_ref = hr
        self.v, self.i, self.ref = (torch.from_numpy(x).to(dev) for x in (hv, hi, hr))
        self.v1, self.i1 = self.shifted(self.v, SENTINEL), self.shifted(self.i, 0)

    @staticmethod
    def shifted(buf, fill):
        out = torch.full((buf.numel() + PAD,), fill, dtype=buf.dtype, device=buf.device)
        out[1:1 + buf.numel()] = buf
        return out

    def expect(self, got, shift, what):
        """got[shift : shift + total] is the packed expectation and the rest of got still holds the sentinel"""
        body = got[shift:shift + self.total]
        if torch.equal(body, self.ref) and bool((got[:shift] == SENTINEL).all()) and bool((got[shift + self.total:] == SENTINEL).all()):
            return
        h = got.cpu().numpy()
        assert (h[:shift] == SENTINEL).all() and (h[shift + self.total:] == SENTINEL).all(), "%s: store outside the buffers" % what
        h = h[shift:shift + self.total]
        bad = np.nonzero(h != self.host_ref)[0]
        k = max(j for j, (a, n) in enumerate(self.spans) if a <= bad[0])
        a, n = self.spans[k]
        raise AssertionError("%s: %s: %d wrong entries in the packed buffer, the first at %d of this case's %d: got %r, expected %r" %
                             (what, self.names[k], bad.size, bad[0] - a, n, h[bad[0]], self.host_ref[bad[0]]))


def check_packed(L, P, rev, what):
    """Every packed case out of place and in place through the Python wrapper, and with only the values, only the ids or only
    the output one element off alignment (the scalar kernel, for each reason separately) through the C ABI."""
    from fsw_gnn_amd import segcumsum
    outs = [segcumsum(P.v[a:a + n], P.i[a:a + n], reverse=rev) for a, n in P.spans]
    packed = torch.full_like(P.v, SENTINEL)
    for (a, n), o in zip(P.spans, outs):
        assert o.shape == (n,) and o.dtype == P.v.dtype
        packed[a:a + n] = o
    P.expect(packed, 0, what + ", out of place")
    w = P.v.clone()
    for a, n in P.spans:
        r = segcumsum(w[a:a + n], P.i[a:a + n], in_place=True, reverse=rev)
        assert r.data_ptr() == w.data_ptr() + a * w.element_size()
    P.expect(w, 0, what + ", in place")
    ws = torch.empty(int(L.fsw_segcumsum_workspace_bytes(max(n for _, n in P.spans))), dtype=torch.uint8, device=P.v.device)
    for off in ("values", "ids", "output"):
        dv, di, do = int(off == "values"), int(off == "ids"), int(off == "output")
        out = torch.full((P.total + PAD,), SENTINEL, dtype=P.v.dtype, device=P.v.device)
        for a, n in P.spans:
            scan_abi(L, P.v1 if dv else P.v, a + dv, P.i1 if di else P.i, a + di, out, a + do, n, rev, ws)
        P.expect(out, do, "%s, %s off alignment" % (what, off))


@functools.lru_cache(maxsize=8)
def family(name, g, vdt, wide=False):
    """(cases, forward references) of one family for one geometry, built once for both directions"""
    if name == "single_head":
        cases = [S.single_head(p, g, vdt) for p in S.single_head_positions(g)]
        # ... and with a length that is a multiple of EPL: the only lengths at which a reverse scan takes the vector kernel
        cases += [S.single_head(p, g, vdt, n=3 * g.TILE + 8) for p in S.single_head_positions(g)]
    elif name == "runs":
        cases = [S.runs(Lr, sh, g, vdt) for Lr in S.run_lengths(g) for sh in S.run_shifts(g)]
        cases += [S.runs(Lr, 0, g, vdt, align_n=g.EPL, seed=1) for Lr in (g.GRP + 1, g.TILE, 2 * g.TILE, 64 * g.TILE + 1)]
    elif name == "sizes":
        cases = S.sizes(g, vdt) + S.sizes(g, vdt, kind="int", seed=1)
    else:
        cases = S.id_patterns(g, vdt, wide)
    return cases, [S.exact_segcumsum(c.values, c.ids) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------------
@variants
def test_geometry_matches_the_cases(dev, L, vdt, idt, rev):
    g, grid = query(L, vdt, idt, rev)
    assert (g.EPL, g.GRP, g.TILE) == S.GEOMETRIES[(vdt, idt)] and g.WCH * 4 == g.TILE
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert grid > 0 and grid % cus == 0 and grid <= 6 * cus, (grid, cus)
    print("resident workgroups %s %s %s: %d on %d CUs" % (vdt, idt, "reverse" if rev else "forward", grid, cus))
    bad = (ctypes.c_int32 * 4)()
    assert L.fsw_segcumsum_geometry(2, 8, 0, bad) == 1 and L.fsw_segcumsum_geometry(0, 2, 0, bad) == 1
    assert L.fsw_segcumsum_geometry(0, 8, 0, None) == 1


@variants
def test_single_head_positions(dev, L, vdt, idt, rev):
    g, _ = query(L, vdt, idt, rev)
    cases, refs = family("single_head", g, vdt)
    check_packed(L, Packed(cases, refs, vdt, idt, rev, dev), rev, "single_head")


@variants
def test_runs_of_every_boundary_length(dev, L, vdt, idt, rev):
    g, _ = query(L, vdt, idt, rev)
    cases, refs = family("runs", g, vdt)
    assert max(S.longest_segment(c.ids) for c in cases) == 65 * g.TILE
    check_packed(L, Packed(cases, refs, vdt, idt, rev, dev), rev, "runs")


@variants
def test_sizes(dev, L, vdt, idt, rev):
    g, _ = query(L, vdt, idt, rev)
    cases, refs = family("sizes", g, vdt)
    check_packed(L, Packed(cases, refs, vdt, idt, rev, dev), rev, "sizes")


@variants
def test_id_patterns(dev, L, vdt, idt, rev):
    g, _ = query(L, vdt, idt, rev)
    cases, refs = family("ids", g, vdt, idt == "int64")
    assert len(cases) == (8 if idt == "int64" else 6)
    check_packed(L, Packed(cases, refs, vdt, idt, rev, dev), rev, "id patterns")


@variants
def test_nonfinite_segments_do_not_leak(dev, L, vdt, idt, rev):
    """An inf or a NaN stays inside its own segment, wherever the segment lies relative to tiles, the halo and the look-back."""
    from fsw_gnn_amd import segcumsum
    g, _ = query(L, vdt, idt, rev)
    for kind in S.NONFINITE_KINDS:
        case, want = S.nonfinite(kind, g, vdt)
        v, ids, want = directed(case, want, rev)
        marked = case.marked[::-1] if rev else case.marked
        assert np.isfinite(want[~marked]).all() and not np.isfinite(want[marked]).all()
        vd, idd = torch.from_numpy(v).to(dev), torch.from_numpy(as_ids(ids, IDT_NP[idt])).to(dev)
        got = segcumsum(vd, idd, reverse=rev).cpu().numpy()
        work = vd.clone()
        segcumsum(work, idd, in_place=True, reverse=rev)
        for how, h in (("out of place", got), ("in place", work.cpu().numpy())):
            outside = np.nonzero(~marked & (h != want))[0]          # want is finite there, so a NaN in h counts too
            assert outside.size == 0, (kind, how, "%d entries outside the marked segments differ, the first at %d: got %r, expected %r" %
                                       (outside.size, outside[0], h[outside[0]], want[outside[0]]))
            assert np.array_equal(h[~marked], want[~marked])
            assert np.array_equal(h[marked], want[marked], equal_nan=True), (kind, how)


@variants
def test_three_rounds_of_the_persistent_grid(dev, L, vdt, idt, rev):
    """Every workgroup of the resident grid walks at least three tiles: the reload of the next tile, the reuse of the LDS carry
    behind the closing barrier, and look-back onto tiles that the same workgroup published a round earlier."""
    from fsw_gnn_amd import segcumsum
    g, grid = query(L, vdt, idt, rev)
    for layout in S.ROUND_LAYOUTS:
        case, ref = rounds_case(grid, g, vdt, layout)
        n = len(case.ids)
        assert -(-n // g.TILE) >= 2 * grid + 3
        v, ids, want = directed(case, ref, rev)
        vd, idd, wd = torch.from_numpy(v).to(dev), torch.from_numpy(as_ids(ids, IDT_NP[idt])).to(dev), torch.from_numpy(want).to(dev)
        got = segcumsum(vd, idd, reverse=rev)
        assert torch.equal(got, wd), (layout, "out of place", first_difference(got, wd, g))
        r = segcumsum(vd, idd, in_place=True, reverse=rev)
        assert r.data_ptr() == vd.data_ptr()
        assert torch.equal(vd, wd), (layout, "in place", first_difference(vd, wd, g))


@functools.lru_cache(maxsize=3)
def rounds_case(grid, g, vdt, layout):
    case = S.rounds(grid, g, vdt, layout)
    return case, S.exact_segcumsum(case.values, case.ids)


def first_difference(got, want, g):
    bad = torch.nonzero(got != want).flatten()
    if bad.numel() == 0:
        return None
    i = int(bad[0])
    return "%d wrong entries, the first at memory index %d (tile %d, offset %d): got %r, expected %r" % (
        bad.numel(), i, i // g.TILE, i % g.TILE, float(got[i]), float(want[i]))


def test_dirty_and_reused_workspace(dev, L):
    """One workspace, first filled with 0xFF, serves a float64 call, a float32 call, a longer call and a shorter call: stale
    descriptor tags of an earlier call (other word count per tile, other tile count) must never be taken for published ones."""
    rng = np.random.default_rng(21)
    calls = []      # (value type, id type, reverse, n): long segments, so that the look-back reads many descriptors
    for vdt, idt, rev, tiles, extra in (("float64", "int64", False, 37, 11), ("float32", "int32", True, 30, 1),
                                        ("float32", "int64", False, 90, 5), ("float64", "int32", True, 9, 3)):
        g, _ = query(L, vdt, idt, rev)
        n = tiles * g.TILE + extra
        ids = np.cumsum(S.random_heads(rng, n, 6.0 * g.TILE), dtype=np.int64)
        calls.append((vdt, idt, rev, S.Case("workspace(%s,%s,n=%d)" % (vdt, idt, n), S.dyadic_values(rng, ids, vdt), ids, None)))
    assert calls[2][3].ids.size > calls[1][3].ids.size and calls[3][3].ids.size < calls[2][3].ids.size
    ws = torch.empty(int(max(L.fsw_segcumsum_workspace_bytes(c.ids.size) for *_, c in calls)), dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)
    for in_place in (False, True):
        for vdt, idt, rev, case in calls:
            assert S.longest_segment(case.ids) > 2 * S.geometry(*S.GEOMETRIES[(vdt, idt)]).TILE
            v, ids, want = directed(case, S.exact_segcumsum(case.values, case.ids), rev)
            vd, idd = torch.from_numpy(v).to(dev), torch.from_numpy(as_ids(ids, IDT_NP[idt])).to(dev)
            out = vd if in_place else torch.full_like(vd, SENTINEL)
            scan_abi(L, vd, 0, idd, 0, out, 0, v.size, rev, ws)
            assert np.array_equal(out.cpu().numpy(), want), (case.name, "in place" if in_place else "out of place")


def test_python_wrapper_surface(dev):
    from fsw_gnn_amd import segcumsum
    g = S.geometry(*S.GEOMETRIES[("float32", "int64")])
    case = S.runs(g.GRP + 1, 1, g, "float32")
    want = S.exact_segcumsum(case.values, case.ids)
    n = case.ids.size
    ids = torch.from_numpy(case.ids).to(dev)
    # non-contiguous values, out of place
    wide = torch.full((2 * n,), SENTINEL, dtype=torch.float32, device=dev)
    wide[::2] = torch.from_numpy(case.values).to(dev)
    before = wide.clone()
    got = segcumsum(wide[::2], ids)
    assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), want) and torch.equal(wide, before)
    with pytest.raises(AssertionError, match="contiguous"):
        segcumsum(wide[::2], ids, in_place=True)
    # in place: the same storage; max_seg_size is accepted and changes nothing
    vals = torch.from_numpy(case.values).to(dev)
    same = segcumsum(vals, ids, max_seg_size=3, in_place=True)
    assert same.data_ptr() == vals.data_ptr() and np.array_equal(vals.cpu().numpy(), want)
    assert np.array_equal(segcumsum(torch.from_numpy(case.values).to(dev), ids.to(torch.int32), max_seg_size=10 ** 6).cpu().numpy(), want)
    # n = 0
    empty = segcumsum(torch.empty(0, device=dev), torch.empty(0, dtype=torch.int64, device=dev))
    assert empty.shape == (0,) and empty.dtype == torch.float32
    # thorough_verify_input
    vals = torch.from_numpy(case.values).to(dev)
    assert np.array_equal(segcumsum(vals, ids, thorough_verify_input=True).cpu().numpy(), want)
    with pytest.raises(AssertionError, match="repeated segment IDs"):
        segcumsum(vals, ids % 2, thorough_verify_input=True)
    poisoned = vals.clone()
    poisoned[5] = float("nan")
    with pytest.raises(AssertionError, match="nans"):
        segcumsum(poisoned, ids, thorough_verify_input=True)
    poisoned[5] = float("inf")
    with pytest.raises(AssertionError, match="infs"):
        segcumsum(poisoned, ids, thorough_verify_input=True)
    # unsupported types
    with pytest.raises(RuntimeError, match="Unsupported input_tensor dtype"):
        segcumsum(vals.to(torch.float16), ids)
    with pytest.raises(AssertionError, match="int32 or int64"):
        segcumsum(vals, ids.to(torch.int16))
    with pytest.raises(RuntimeError, match="pure-PyTorch"):
        segcumsum(vals, ids, always_use_pure_torch=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        segcumsum(vals.cpu(), ids.cpu())
    # values produced on a side stream and scanned there, no synchronisation by the caller
    side = torch.cuda.Stream(device=dev)
    src = torch.from_numpy(case.values).to(dev)
    big = torch.randn((2048, 2048), device=dev)
    late = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        acc = big
        for _ in range(20):
            acc = acc @ big * 1e-2                    # queued producer work
        late.copy_(src)
        host = segcumsum(late, ids).cpu().numpy()     # the copy is ordered on the side stream too
    assert np.array_equal(host, want)
    torch.cuda.synchronize()


def legacy_hierarchy(L, vals, ids, tpb, launch_exports):
    """The reference's driver loop over segcumsum_wrapper / add_block_sums_wrapper (as test_legacy_abi_drives_reference_hierarchy),
    or the same through the launch_* exports, which do not synchronise."""
    dev, dt = vals.device, vals.dtype
    tag = "float" if dt == torch.float32 else "double"
    dnum = 0 if dt == torch.float32 else 1
    sizes, max_seg = [vals.numel()], [1300]
    while sizes[-1] > tpb:
        sizes.append((sizes[-1] + tpb - 1) // tpb)
        max_seg.append((max_seg[-1] + tpb - 1) // tpb)
    nblocks = sizes[1:] + [1]
    outs = [vals.clone()] + [torch.zeros(s, device=dev, dtype=dt) for s in sizes[1:]]
    idts = [ids] + [torch.zeros(s, device=dev, dtype=torch.int64) for s in sizes[1:]]
    torch.cuda.synchronize()
    for i, s in enumerate(sizes):
        nxt = i < len(sizes) - 1
        assert nblocks[i] * tpb >= s and outs[i].numel() == s and (not nxt or outs[i + 1].numel() >= nblocks[i])
        so, io = (outs[i + 1].data_ptr(), idts[i + 1].data_ptr()) if nxt else (None, None)
        if launch_exports:
            getattr(L, "launch_segcumsum_kernel_" + tag)(outs[i].data_ptr(), idts[i].data_ptr(), s, max_seg[i], so, io, nxt, nblocks[i],
                                                         tpb, tpb * vals.element_size())
        else:
            L.segcumsum_wrapper(dnum, outs[i].data_ptr(), idts[i].data_ptr(), s, max_seg[i], so, io, nxt, nblocks[i], tpb,
                                tpb * vals.element_size())
    for i in reversed(range(len(sizes) - 1)):
        if launch_exports:
            getattr(L, "launch_add_block_sums_kernel_" + tag)(outs[i].data_ptr(), outs[i + 1].data_ptr(), idts[i].data_ptr(),
                                                              idts[i + 1].data_ptr(), sizes[i], nblocks[i], tpb)
        else:
            L.add_block_sums_wrapper(dnum, outs[i].data_ptr(), outs[i + 1].data_ptr(), idts[i].data_ptr(), idts[i + 1].data_ptr(),
                                     sizes[i], nblocks[i], tpb)
    torch.cuda.synchronize()
    return outs[0], len(sizes)


@pytest.mark.parametrize("tpb", [64, 96, 100, 256, 1000, 1024])
def test_legacy_kernels_every_block_width(dev, L, tpb):
    """Block widths that are and are not multiples of the wavefront, a partial last block on every level, segments of mean
    length 40 and one that crosses the first boundary of the second level (element tpb * tpb)."""
    n = tpb * (tpb + 3) + 37
    rng = np.random.default_rng([22, tpb])
    heads = S.random_heads(rng, n, 40.0)
    long = min(70_000, n // 2)
    heads[n - long + 1:] = False
    assert n % tpb and -(-n // tpb) % tpb and n - long < tpb * tpb < n
    ids_np = np.cumsum(heads, dtype=np.int64)
    ids = torch.from_numpy(ids_np).to(dev)
    for vdt in ("float32", "float64"):
        vals = S.dyadic_values(rng, ids_np, vdt)
        want = S.exact_segcumsum(vals, ids_np)
        for launch_exports in (False, True):
            got, levels = legacy_hierarchy(L, torch.from_numpy(vals).to(dev), ids, tpb, launch_exports)
            assert levels >= 3
            assert np.array_equal(got.cpu().numpy(), want), (tpb, vdt, "launch_* exports" if launch_exports else "wrappers")
