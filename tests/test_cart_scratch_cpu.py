"""Cartesian mode, one scratch query: fsw_embed_cart_scratch_bytes against the rules the host layer applied before it existed, the
host method that wraps it, the class table as the only place the cuts are written, and the unchanged ABI.  No GPU is needed."""
import ctypes
import glob
import itertools
import os
import re
import types

import numpy as np
import pytest

from tests.conftest import ROOT

LIB = os.path.join(ROOT, "fsw_gnn_amd", "libfsw_hip.so")
CSRC = os.path.join(ROOT, "fsw_gnn_amd", "csrc")
REG_MAX_DEG, LDS_MAX_DEG, HUB_MAX_DEG, CART_W_MAX_LINE = 32, 2048, 32768, 16384
MID_SIZES = (40, 48, 64, 80, 96, 128, 160, 192, 256)
BIN_MID0 = REG_MAX_DEG + 1
BIN_LDS0 = BIN_MID0 + len(MID_SIZES)
BIN_HUB0 = BIN_LDS0 + 3
BIN_GLOBAL = BIN_HUB0 + 4
NUM_BINS = BIN_GLOBAL + 1
STAT_MAX_DEGREE = 1

LONGEST = (32, 2047, 2048, 2049, 4095, 4096, 8192, 16383, 16384, 16385, 32768, 32769, 150000)
LONG_ROWS = (1, 3, 1000)
SLICES = (1, 4, 64)
MODES = (("unit", False, 1.0), ("weights", True, 1.0), ("tau", False, 3.0))    # (name, w != NULL, tau)


def degree_bin(deg):
    """csrc/fsw_common.h: degree_bin"""
    if deg <= REG_MAX_DEG:
        return deg
    if deg > HUB_MAX_DEG:
        return BIN_GLOBAL
    if deg > LDS_MAX_DEG:
        return BIN_HUB0 + (deg > 4096) + (deg > 8192) + (deg > 16384)
    if deg > MID_SIZES[-1]:
        return BIN_LDS0 + (deg > 512) + (deg > 1024)
    return BIN_MID0 + sum(deg > s for s in MID_SIZES[:-1])


def bin_table(longest, long_rows, lower):
    """Host copy of bin_start for a graph with some short rows, long_rows rows in the bin of `longest` neighbours and, with lower,
    five more rows one bin below (where that is still a bin of the long classes: the last LDS bin or above)."""
    counts = np.zeros(NUM_BINS, dtype=np.int64)
    counts[0], counts[3], counts[REG_MAX_DEG] = 2, 7, 1
    b = degree_bin(longest)
    counts[b] += long_rows
    if lower and b - 1 >= BIN_HUB0 - 1:
        counts[b - 1] += 5
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def parent_rules(L, unit, bs, md, S, backward):
    """What FSW_embedding._cart_scratch and ._cart_backward_scratch allocated before fsw_embed_cart_scratch_bytes, in bytes (0: None),
    on the three size functions whose values this library keeps."""
    def forward():
        if md < (HUB_MAX_DEG + 1 if unit else CART_W_MAX_LINE):
            return 0
        first = NUM_BINS - 1 if unit else BIN_HUB0 + 2
        return L.fsw_embed_cart_generic_scratch_bytes(md, max(int(bs[NUM_BINS]) - int(bs[first]), 1))

    if not backward:
        return forward()
    if not unit:
        if md < LDS_MAX_DEG:
            return forward()
        return L.fsw_embed_cart_weighted_backward_scratch_bytes(md, int(bs[NUM_BINS]) - int(bs[BIN_HUB0 - 1]), S)   # 2048: last LDS bin
    if int(bs[NUM_BINS - 1]) == int(bs[BIN_HUB0]):
        return forward()                     # no hub rows: the backward reused the forward's buffer
    return L.fsw_embed_cart_backward_scratch_bytes(md, int(bs[NUM_BINS]) - int(bs[BIN_HUB0]), S)


def pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    return _lib.lib()                       # loads without a device


def query(L, bs, md, has_w, tau, S, backward):
    from fsw_gnn_amd import _lib
    a = _lib.CartArgs()
    a.bin_start_host, a.max_degree, a.tau, a.S = bs.ctypes.data, md, tau, S
    a.w = 16 if has_w else None             # never dereferenced: only compared with NULL
    return int(L.fsw_embed_cart_scratch_bytes(ctypes.byref(a), backward))


def test_parity_with_the_rules_of_the_host_layer_before(L):
    cells = nonzero = 0
    for (name, has_w, tau), S, longest, rows, lower in itertools.product(MODES, SLICES, LONGEST, LONG_ROWS, (False, True)):
        bs = bin_table(longest, rows, lower)
        unit = not has_w and tau <= 1.0
        for backward in (0, 1):
            want = parent_rules(L, unit, bs, longest, S, backward)
            got = query(L, bs, longest, has_w, tau, S, backward)
            assert got == want, (name, S, longest, rows, lower, backward, got, want)
            cells += 1
            nonzero += got > 0
    assert cells == 3 * 3 * 13 * 3 * 2 * 2 and 0 < nonzero < cells


def test_unit_rows_above_the_hub_bins_only_reuse_the_forward_size(L):
    """Unit weights, rows above 32768 neighbours and none in the hub bins: the backward ran out of the forward's buffer."""
    for longest, rows, S in ((32769, 1, 4), (150000, 3, 64), (150000, 1000, 1)):
        bs = bin_table(longest, rows, False)
        assert int(bs[BIN_GLOBAL]) == int(bs[BIN_HUB0]) and int(bs[NUM_BINS]) - int(bs[BIN_GLOBAL]) == rows
        fwd = query(L, bs, longest, False, 1.0, S, 0)
        assert fwd == L.fsw_embed_cart_generic_scratch_bytes(longest, rows) > 0
        assert query(L, bs, longest, False, 1.0, S, 1) == fwd


def test_old_size_functions_keep_their_values(L):
    """Below the rows of the generic kernel the two older exports are whole lines of 12 bytes per element of the padded longest line,
    min(2048, rows * S) of them, at most 2 GiB, at least one."""
    for f, pad, first, last in ((L.fsw_embed_cart_backward_scratch_bytes, 0, LDS_MAX_DEG + 1, HUB_MAX_DEG),
                                (L.fsw_embed_cart_weighted_backward_scratch_bytes, 1, LDS_MAX_DEG, CART_W_MAX_LINE - 1)):
        assert f(first - 1, 5, 4) == 0
        for md, rows, S in itertools.product((first, 3000, 4096, 8192, 16383, last), (0, 1, 3, 1000, 1 << 20), (1, 4, 64, 1024)):
            if not first <= md <= last:
                continue
            line = 12 * pow2ceil(md + pad)
            lines = max(min(max(rows, 1) * S, 2048, (2 << 30) // line), 1)
            assert f(md, rows, S) == lines * line, (pad, md, rows, S)
        for md in (last + 1, 150000):
            assert f(md, 3, 4) == max(f(last, 3, 4), L.fsw_embed_cart_generic_scratch_bytes(md, 3))


def test_host_method(L):
    """FSW_embedding._cart_scratch_bytes on a stand-in graph.  The module itself needs a device to be constructed, so the method runs
    as a plain function on an object that carries the two attributes it reads (nSlices, total_mass_pad_thresh)."""
    import torch

    from fsw_gnn_amd.fsw_embedding import FSW_embedding
    cells = ((2049, 3, True), (4096, 1, False), (16383, 1000, True), (16384, 3, False), (32769, 1, False), (150000, 3, True), (32, 1, False))
    for (name, has_w, tau), S, (longest, rows, lower) in itertools.product(MODES, (1, 64), cells):
        bs = bin_table(longest, rows, lower)
        graph = types.SimpleNamespace(bin_start_host=bs.reshape(1, -1), w=torch.zeros(1) if has_w else None)
        module = types.SimpleNamespace(nSlices=S, total_mass_pad_thresh=tau)
        st = [0] * 8
        st[STAT_MAX_DEGREE] = longest
        for backward in (False, True):
            got = FSW_embedding._cart_scratch_bytes(module, graph, st, backward)
            assert got == parent_rules(L, not has_w and tau <= 1.0, bs, longest, S, backward), (name, S, longest, rows, lower, backward)


def test_the_cuts_are_written_once():
    cuts = re.compile(r"\b(2047|4095|8191|16383)\b|FSW_BIN_HUB0 \+ 2")
    files = sorted(glob.glob(os.path.join(CSRC, "embed_cart*.hip")))
    assert len(files) == 6
    for path in files:
        hits = [ln for ln in open(path).read().split("\n") if cuts.search(ln)]
        assert not hits, (os.path.basename(path), hits)
    header = open(os.path.join(CSRC, "embed_cart.h")).read()
    m = re.search(r"constexpr CartLongMode kCartLong\[2\] = \{.*?\n\};\n", header, re.S)
    assert m and len(cuts.findall(m.group(0))) >= 4
    rest = header[:m.start()] + header[m.end():]
    assert not re.search(r"\b(2047|4095|4096|8191|8192|16383|16384|32768|32769)\b|FSW_BIN_HUB0 \+ [123]", rest)
    host = open(os.path.join(ROOT, "fsw_gnn_amd", "fsw_embedding.py")).read()
    cart = host[host.index("    def _cart_unit_table"):host.index("    def _homog_epilogue")]
    assert not re.search(r"HUB_MAX_DEG|CART_W_MAX_LINE|LDS_MAX_DEG|NUM_BINS|NUM_LDS_BINS|MID_SIZES", cart)


def test_symbol_and_abi(L):
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert "fsw_embed_cart_scratch_bytes" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(LIB), "fsw_embed_cart_scratch_bytes")
    assert "size_t fsw_embed_cart_scratch_bytes(const fsw_cart_args* args, int backward);" in header
    for old in ("fsw_embed_cart_generic_scratch_bytes", "fsw_embed_cart_backward_scratch_bytes", "fsw_embed_cart_weighted_backward_scratch_bytes"):
        assert old in _lib.EXPORTED_SYMBOLS and re.search(r"size_t %s\(" % old, header)
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33
    assert (_lib.LDS_MAX_DEG, _lib.HUB_MAX_DEG, _lib.CART_W_MAX_LINE, _lib.NUM_BINS) == (LDS_MAX_DEG, HUB_MAX_DEG, CART_W_MAX_LINE, NUM_BINS)
