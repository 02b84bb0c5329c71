"""Cartesian mode, the split form of the longest general-weight rows (csrc/embed_split_cart_w.hip): the three host-only exports
fsw_embed_cart_split_w_scratch_bytes, fsw_embed_cart_split_w_lines and fsw_embed_cart_split_w_max_lines, the flag FSW_CART_SPLIT_W_LINES,
the formula of include/fsw_hip.h on hand-made bin tables, the ABI and the older queries left as they were, and the host layer's policy.
No GPU is needed."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_cart_scratch_cpu import LIB, NUM_BINS
from tests.test_cart_split_cpu import args

BLOCK, TILE = 8192, 4096                    # (key, weight) elements of a block / ranks of a tile
CAP = 2 << 30
FIRST = 16384                               # FSW_CART_W_MAX_LINE: the shortest row of the class
MAX_DEGREES, SLICES, FREQS, ROWS = (16384, 24575, 24576, 40000, 150000), (1, 3, 16), (1, 5, 70), (1, 2, 5)
MODES = ((True, 1.0), (False, 3.0), (True, 0.5))     # (has_w, tau): a weight tensor; w == NULL with tau > 1; both


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    return _lib.lib()                       # loads without a device


def class_bin_table(rows, below=4, last=0):
    """Host copy of bin_start: `below` rows spread over shorter bins, `rows` rows in the class's first degree bin (8193 .. 16384
    neighbours, the third hub bin) and `last` rows in the bins above it."""
    counts = np.zeros(NUM_BINS, dtype=np.int64)
    counts[0], counts[5], counts[NUM_BINS - 4] = 1, below - 2, 1
    counts[NUM_BINS - 3] = rows
    counts[NUM_BINS - 1] = last
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def up16(v):
    return (v + 15) // 16 * 16


def formula(rows, md, S, F):
    """include/fsw_hip.h: four block-rounded float lines per line, a float64 sum per line and tile, a partial sum per line, tile and
    frequency, a float64 mass piece per row and block; every part rounded up to a multiple of 16."""
    lines = rows * S
    cap = -(-(md + 1) // BLOCK) * BLOCK
    nbmax, tiles = cap // BLOCK, cap // TILE
    return lines * cap * 16 + up16(lines * tiles * 8) + up16(lines * tiles * F * 4) + up16(rows * nbmax * 8)


def test_exports_prototypes_flag_and_abi(L):
    """Fails on a library without the split form of general weights: the symbols do not exist."""
    from fsw_gnn_amd import _lib
    handle = ctypes.CDLL(LIB)
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    for name, proto, restype, argtypes in (
            ("fsw_embed_cart_split_w_scratch_bytes", "size_t fsw_embed_cart_split_w_scratch_bytes(const fsw_cart_args* args);",
             ctypes.c_size_t, [ctypes.POINTER(_lib.CartArgs)]),
            ("fsw_embed_cart_split_w_lines", "int64_t fsw_embed_cart_split_w_lines(const fsw_cart_args* args);", ctypes.c_int64,
             [ctypes.POINTER(_lib.CartArgs)]),
            ("fsw_embed_cart_split_w_max_lines", "int64_t fsw_embed_cart_split_w_max_lines(void);", ctypes.c_int64, [])):
        assert hasattr(handle, name), name
        assert name in _lib.EXPORTED_SYMBOLS and proto in header, name
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name
    assert re.search(r"#define FSW_CART_SPLIT_W_LINES 4\b", header) and _lib.CART_SPLIT_W_LINES == 4
    assert re.search(r"#define FSW_CART_SPLIT_LINES 1\b", header) and re.search(r"#define FSW_CART_SPLIT_BWD_LINES 2\b", header)
    # the formula is documented next to the query
    doc = header[header.index("Split form of the longest GENERAL-WEIGHT rows"):header.index("#define FSW_CART_SPLIT_W_LINES")]
    for piece in ("lines * cap * 16", "lines * tiles * 8", "lines * tiles * F * 4", "rows * nbmax * 8", "blocks of 8192", "cap / 4096",
                  "2 GiB", "16-byte aligned"):
        assert piece in doc, piece
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33
    assert int(re.search(r"#define FSW_CART_W_MAX_LINE (\d+)", header).group(1)) == FIRST


def test_query_follows_the_documented_formula(L):
    for rows, md, S, F, (has_w, tau) in itertools.product(ROWS, MAX_DEGREES, SLICES, FREQS, MODES):
        bs = class_bin_table(rows)
        a = args(bs, md, S, F, has_w=has_w, tau=tau)
        want = formula(rows, md, S, F)
        assert want <= CAP and want % 16 == 0
        assert int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))) == want, (rows, md, S, F, has_w, tau)
        assert int(L.fsw_embed_cart_split_w_lines(ctypes.byref(a))) == rows * S, (rows, md, S, F)
    # rows of the bins above the class's first one count too
    a = args(class_bin_table(1, last=2), 40000, 3, 5, has_w=True)
    assert int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))) == formula(3, 40000, 3, 5)
    assert int(L.fsw_embed_cart_split_w_lines(ctypes.byref(a))) == 9
    # hand-checked: one row of 150000 neighbours (19 blocks = 155648 elements, 38 tiles), S = 16, F = 16
    a = args(class_bin_table(0, last=1), 150000, 16, 16, has_w=True)
    assert int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))) == 16 * 155648 * 16 + 16 * 38 * 8 + 16 * 38 * 16 * 4 + 160
    assert 16 * 155648 * 16 + 16 * 38 * 8 + 16 * 38 * 16 * 4 + 160 == 39889824


def test_nothing_to_split(L):
    """0 bytes and 0 lines: unit weights with tau <= 1, an empty class, max_degree below the class, NULL."""
    for md, S, F in itertools.product(MAX_DEGREES, SLICES, FREQS):
        for a in (args(class_bin_table(2), md, S, F), args(class_bin_table(2), md, S, F, tau=0.5),
                  args(class_bin_table(0), md, S, F, has_w=True), args(class_bin_table(0), md, S, F, tau=3.0),
                  args(class_bin_table(2), FIRST - 1, S, F, has_w=True), args(class_bin_table(2), 0, S, F, tau=3.0)):
            assert int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))) == 0
            assert int(L.fsw_embed_cart_split_w_lines(ctypes.byref(a))) == 0
    assert int(L.fsw_embed_cart_split_w_scratch_bytes(None)) == 0 and int(L.fsw_embed_cart_split_w_lines(None)) == 0


def test_nothing_above_two_gib(L):
    """The largest size up to 2 GiB follows the formula, the first above it returns 0 (and no lines: there is no split form then)."""
    S, F, md = 16, 16, 150000
    fit = 1
    while formula(fit + 1, md, S, F) <= CAP:
        fit += 1
    a = args(class_bin_table(fit), md, S, F, has_w=True)
    assert int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))) == formula(fit, md, S, F) <= CAP
    a = args(class_bin_table(fit + 1), md, S, F, has_w=True)
    assert formula(fit + 1, md, S, F) > CAP
    assert int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))) == 0 and int(L.fsw_embed_cart_split_w_lines(ctypes.byref(a))) == 0
    for rows, big in ((1, 100000000), (1, 600000000), (1 << 20, 150000)):
        a = args(class_bin_table(rows), big, 64, F, tau=2.0)
        assert int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))) == 0


def test_max_lines(L):
    top = int(L.fsw_embed_cart_split_w_max_lines())
    assert top in (16, 32, 64, 128, 256, 512)              # a measured line count; one cloud at S = 16 qualifies


def test_older_queries_ignore_the_flag(L):
    from fsw_gnn_amd import _lib
    queries = ("fsw_embed_cart_forward_scratch_bytes", "fsw_embed_cart_backward_keys_scratch_bytes", "fsw_embed_cart_split_scratch_bytes",
               "fsw_embed_cart_split_lines", "fsw_embed_cart_split_backward_scratch_bytes", "fsw_embed_cart_split_backward_lines")
    bit = _lib.CART_SPLIT_W_LINES
    some = 0
    for rows, md, S, (has_w, tau) in itertools.product(ROWS, MAX_DEGREES + (16383, 32769, 70000), SLICES,
                                                       ((False, 1.0), (True, 1.0), (False, 3.0))):
        bs = class_bin_table(rows, last=1)
        for name, flags in itertools.product(queries, (0, 1, 2, 3)):
            off = int(getattr(L, name)(ctypes.byref(args(bs, md, S, 8, has_w, tau, flags=flags))))
            on = int(getattr(L, name)(ctypes.byref(args(bs, md, S, 8, has_w, tau, flags=flags | bit))))
            assert on == off, (name, rows, md, S, has_w, tau, flags)
            some += off > 0
        for backward in (0, 1):
            off = int(L.fsw_embed_cart_scratch_bytes(ctypes.byref(args(bs, md, S, 8, has_w, tau)), backward))
            on = int(L.fsw_embed_cart_scratch_bytes(ctypes.byref(args(bs, md, S, 8, has_w, tau, flags=bit)), backward))
            assert on == off
    assert some > 0
    # and the new query does not read the flags
    for flags in (0, 1, 2, 4, 7):
        a = args(class_bin_table(1), 40000, 3, 5, has_w=True, flags=flags)
        assert int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))) == formula(1, 40000, 3, 5)


def test_host_policy():
    """FSW_embedding._cart_split_w on stand-in graphs: the query's bytes for 0 < rows x nSlices <= fsw_embed_cart_split_w_max_lines(), 0
    above it, for unit weights and without a row of the class; _cart_split keeps returning 0 for general weights; _cart_tuned_args sets the
    bit only when asked."""
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    import types

    import torch

    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.fsw_embedding import FSW_embedding
    lib = _lib.lib()
    top = int(lib.fsw_embed_cart_split_w_max_lines())

    def stand_ins(rows, S, F, has_w, tau, md):
        graph = types.SimpleNamespace(bin_start_host=class_bin_table(rows).reshape(1, -1), w=torch.zeros(1) if has_w else None)
        module = types.SimpleNamespace(nSlices=S, nFreqs=F, total_mass_pad_thresh=tau)
        st = [0] * 8
        st[_lib.STAT_MAX_DEGREE] = md
        return module, graph, st

    def split_w(rows, S, F=8, has_w=True, tau=1.0, md=40000):
        return FSW_embedding._cart_split_w(*stand_ins(rows, S, F, has_w, tau, md))

    def split(rows, S, F=8, has_w=True, tau=1.0, md=40000):
        return FSW_embedding._cart_split(*stand_ins(rows, S, F, has_w, tau, md))

    assert _lib.STAT_MAX_DEGREE == 1
    assert split_w(1, 4) == formula(1, 40000, 4, 8) and split_w(1, 4, has_w=False, tau=3.0) == formula(1, 40000, 4, 8)
    assert split_w(1, top) == formula(1, 40000, top, 8) and split_w(1, top + 1) == 0
    assert split_w(2, top // 2) == formula(2, 40000, top // 2, 8) and split_w(2, top // 2 + 1, F=1) == 0
    assert split_w(1, 4, has_w=False) == 0 and split_w(0, 4) == 0 and split_w(1, 4, md=FIRST - 1) == 0
    # the unit-weight policy keeps leaving general weights alone, also on rows of its own class
    assert split(1, 4) == 0 and split(1, 4, has_w=False, tau=3.0) == 0 and split(1, 4, md=70000) == 0
    assert split(1, 4, has_w=False, tau=3.0, md=70000) == 0
