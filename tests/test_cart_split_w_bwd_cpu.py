"""Cartesian mode, the split form of the longest general-weight rows' backward (csrc/embed_split_cart_w_bwd.hip): the three host-only
exports fsw_embed_cart_split_w_backward_scratch_bytes, fsw_embed_cart_split_w_backward_lines and
fsw_embed_cart_split_w_backward_max_lines, the flag FSW_CART_SPLIT_W_BWD_LINES as a fourth bit of `flags`, the formula of
include/fsw_hip.h on hand-made bin tables, the rows of the classes below, which run out of the same buffer, the older queries and the ABI
left as they were, and the host policy.  The merge levels use the span helpers of the unit form untouched
(tests/native/test_split_bwd_levels.cpp, run by tests/test_cart_split_bwd_cpu.py).  No GPU is needed."""
import ctypes
import itertools
import os
import re
import types

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_cart_scratch_cpu import LIB, NUM_BINS
from tests.test_cart_split_cpu import args

RUN = 2048                                  # words of a sorted run = ranks of a walk tile: a line is rounded up to whole runs
WORD_BYTES = 16                             # per word of a line: ping and pong, 8 bytes each
FIRST = 16384                               # FSW_CART_W_MAX_LINE: the shortest row of the class
BELOW_LINE_BYTES, BELOW_MAX_LINES = 12 * 16384, 2048   # the classes below: one scratch line of 16384 elements x 12 bytes per wavefront
CAP = 2 << 30
MAX_DEGREES, SLICES, FREQS, ROWS = (16384, 24575, 24576, 32768, 70000), (1, 3, 16), (1, 5, 70), (1, 2, 5)
MODES = ((True, 1.0), (False, 3.0), (True, 0.5))     # (has_w, tau): a weight tensor; w == NULL with tau > 1; both
NAMES = ("fsw_embed_cart_split_w_backward_scratch_bytes", "fsw_embed_cart_split_w_backward_lines",
         "fsw_embed_cart_split_w_backward_max_lines")


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    return _lib.lib()                       # loads without a device


def bin_table(rows, below=0, last=0):
    """Host copy of bin_start: three short rows, `below` rows of 2049 .. 4096 neighbours (the classes below), `rows` rows in the class's
    first degree bin (8193 .. 16384 neighbours) and `last` rows in the last bin."""
    counts = np.zeros(NUM_BINS, dtype=np.int64)
    counts[0], counts[5] = 1, 2
    counts[NUM_BINS - 5], counts[NUM_BINS - 3], counts[NUM_BINS - 1] = below, rows, last
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def up16(v):
    return (v + 15) // 16 * 16


def own(rows, md, S, F):
    """include/fsw_hip.h: two regions of run-rounded max_degree + 1 words of 8 bytes per line, a float64 mass piece per row and run, a
    float64 sum per line and walk tile, a partial sum per line, walk tile and frequency; every part rounded up to a multiple of 16."""
    lines, words = rows * S, -(-(md + 1) // RUN) * RUN
    tiles = words // RUN
    return lines * words * WORD_BYTES + up16(rows * tiles * 8) + up16(lines * tiles * 8) + up16(lines * tiles * F * 4)


def below_part(rows_from_2049, S):
    """Part 1 of fsw_embed_cart_backward_keys_scratch_bytes for general weights and a longest row of at least 16383 neighbours: one line
    of 16384 elements x 12 bytes per wavefront, for the rows from the first degree bin of these classes on."""
    return min(max(rows_from_2049, 1) * S, BELOW_MAX_LINES) * BELOW_LINE_BYTES


def query(L, a):
    return (int(L.fsw_embed_cart_split_w_backward_scratch_bytes(ctypes.byref(a))),
            int(L.fsw_embed_cart_split_w_backward_lines(ctypes.byref(a))))


def test_exports_prototypes_flag_and_abi(L):
    """Fails on a library without the split backward of general weights: the symbols do not exist."""
    from fsw_gnn_amd import _lib
    handle = ctypes.CDLL(LIB)
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    for name, proto, restype, argtypes in (
            (NAMES[0], "size_t fsw_embed_cart_split_w_backward_scratch_bytes(const fsw_cart_args* args);", ctypes.c_size_t,
             [ctypes.POINTER(_lib.CartArgs)]),
            (NAMES[1], "int64_t fsw_embed_cart_split_w_backward_lines(const fsw_cart_args* args);", ctypes.c_int64,
             [ctypes.POINTER(_lib.CartArgs)]),
            (NAMES[2], "int64_t fsw_embed_cart_split_w_backward_max_lines(void);", ctypes.c_int64, [])):
        assert hasattr(handle, name), name
        assert name in _lib.EXPORTED_SYMBOLS and proto in header, name
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name
    assert re.search(r"#define FSW_CART_SPLIT_W_BWD_LINES 8\b", header) and _lib.CART_SPLIT_W_BWD_LINES == 8
    assert re.search(r"#define FSW_CART_SPLIT_LINES 1\b", header) and _lib.CART_SPLIT_LINES == 1
    assert re.search(r"#define FSW_CART_SPLIT_BWD_LINES 2\b", header) and _lib.CART_SPLIT_BWD_LINES == 2
    assert re.search(r"#define FSW_CART_SPLIT_W_LINES 4\b", header) and _lib.CART_SPLIT_W_LINES == 4
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6
    # the layout of the parent: 240 bytes, 33 fields, flags at byte 164 between mass_fn and mass_scale
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33
    assert _lib.CartArgs.flags.offset == 164 and _lib.CartArgs.flags.size == 4
    assert int(re.search(r"#define FSW_CART_W_MAX_LINE (\d+)", header).group(1)) == FIRST
    # the formula is documented next to the query
    doc = header[header.index("Split form of the longest GENERAL-WEIGHT rows' BACKWARD"):header.index("#define FSW_CART_SPLIT_W_BWD_LINES")]
    for piece in ("lines * words * 16", "rows * tiles * 8", "lines * tiles * 8", "lines * tiles * F * 4", "max_degree + 1 rounded up",
                  "whole runs of 2048", "words / 2048", "2 GiB", "16-byte aligned", "where that is larger"):
        assert piece in doc, piece


def test_query_follows_the_documented_formula(L):
    for rows, md, S, F, (has_w, tau) in itertools.product(ROWS, MAX_DEGREES, SLICES, FREQS, MODES):
        want = own(rows, md, S, F)
        assert below_part(rows, S) < want <= CAP and want % 16 == 0
        assert query(L, args(bin_table(rows), md, S, F, has_w=has_w, tau=tau)) == (want, rows * S), (rows, md, S, F, has_w, tau)
    # rows of the bins above the class's first one count too
    assert query(L, args(bin_table(1, last=2), 40000, 3, 5, has_w=True)) == (own(3, 40000, 3, 5), 9)
    # hand-checked: one row of 150000 neighbours (150001 elements: 74 runs = 151552 words, 74 walk tiles), S = 16, F = 16
    want = 16 * 151552 * 16 + 1 * 74 * 8 + 16 * 74 * 8 + 16 * 74 * 16 * 4
    assert want == 38883152
    assert query(L, args(bin_table(0, last=1), 150000, 16, 16, has_w=True)) == (want, 16)
    # parts that are no multiple of 16 bytes are rounded up: 9 runs, one line, one frequency -- 72 -> 80, 72 -> 80, 36 -> 48 bytes
    assert query(L, args(bin_table(1), 16384, 1, 1, tau=3.0)) == (18432 * 16 + 80 + 80 + 48, 1)
    # the query does not read the flags
    for flags in (0, 1, 2, 4, 8, 15):
        assert query(L, args(bin_table(1), 40000, 3, 5, has_w=True, flags=flags)) == (own(1, 40000, 3, 5), 3)


def test_query_covers_the_rows_of_the_classes_below(L):
    """Rows of 8193 .. 16383 neighbours share the class's first degree bin: the host cannot tell them apart, so they count as lines (the
    kernels skip them), and they -- and the rows of 2049 neighbours and more -- run their own kernels out of the same buffer: the query is
    the larger of the two needs."""
    larger = {"own": 0, "below": 0}
    for rows, below, md, S in itertools.product(ROWS, (0, 1, 300), MAX_DEGREES, SLICES):
        a, b = own(rows, md, S, 8), below_part(rows + below, S)
        assert query(L, args(bin_table(rows, below), md, S, 8, has_w=True)) == (max(a, b), rows * S), (rows, below, md, S)
        larger["own" if a >= b else "below"] += 1
    assert min(larger.values()) > 0, larger
    # five rows in the shared bin of which the longest has 16384 neighbours: all five count, whatever the other four hold
    assert query(L, args(bin_table(5), 16384, 3, 8, has_w=True))[1] == 15


def test_nothing_to_split(L):
    """0 bytes and 0 lines: unit weights with tau <= 1, no row in the bin, max_degree below the class, NULL."""
    for md, S, F in itertools.product(MAX_DEGREES, SLICES, FREQS):
        for a in (args(bin_table(2), md, S, F), args(bin_table(2), md, S, F, tau=0.5), args(bin_table(2, last=1), md, S, F, tau=1.0),
                  args(bin_table(0, below=4), md, S, F, has_w=True), args(bin_table(0, below=4), md, S, F, tau=3.0),
                  args(bin_table(2), FIRST - 1, S, F, has_w=True), args(bin_table(2), 0, S, F, tau=3.0)):
            assert query(L, a) == (0, 0)
    assert int(L.fsw_embed_cart_split_w_backward_scratch_bytes(None)) == 0 and int(L.fsw_embed_cart_split_w_backward_lines(None)) == 0


def test_nothing_above_two_gib(L):
    """The largest size up to 2 GiB follows the formula, the first above it returns 0 (and no lines: there is no split form then)."""
    S, F, md = 16, 16, 150000
    fit = 1
    while own(fit + 1, md, S, F) <= CAP:
        fit += 1
    assert own(fit, md, S, F) <= CAP < own(fit + 1, md, S, F)
    assert query(L, args(bin_table(fit), md, S, F, has_w=True)) == (own(fit, md, S, F), fit * S)
    assert query(L, args(bin_table(fit + 1), md, S, F, has_w=True)) == (0, 0)
    for rows, big in ((1, 200000000), (1, 600000000), (1 << 20, 150000)):
        assert query(L, args(bin_table(rows), big, 64, F, tau=2.0)) == (0, 0)


def test_max_lines(L):
    assert int(L.fsw_embed_cart_split_w_backward_max_lines()) >= 16      # one cloud at S = 16 always qualifies


def test_other_queries(L):
    """The older queries ignore bit 8; fsw_embed_cart_split_backward_* keep returning (0, 0) for general weights, with or without it."""
    from fsw_gnn_amd import _lib
    queries = ("fsw_embed_cart_forward_scratch_bytes", "fsw_embed_cart_backward_keys_scratch_bytes", "fsw_embed_cart_split_scratch_bytes",
               "fsw_embed_cart_split_lines", "fsw_embed_cart_split_backward_scratch_bytes", "fsw_embed_cart_split_backward_lines",
               "fsw_embed_cart_split_w_scratch_bytes", "fsw_embed_cart_split_w_lines")
    bit = _lib.CART_SPLIT_W_BWD_LINES
    some = 0
    for rows, md, S, (has_w, tau) in itertools.product(ROWS, MAX_DEGREES + (16383, 32769), SLICES, ((False, 1.0), (True, 1.0), (False, 3.0))):
        bs = bin_table(rows, 1, last=1)
        for name, flags in itertools.product(queries, (0, 2, 7)):
            off = int(getattr(L, name)(ctypes.byref(args(bs, md, S, 8, has_w, tau, flags=flags))))
            on = int(getattr(L, name)(ctypes.byref(args(bs, md, S, 8, has_w, tau, flags=flags | bit))))
            assert on == off, (name, rows, md, S, has_w, tau, flags)
            some += off > 0
            if "split_backward" in name and (has_w or tau > 1):
                assert on == 0, (name, rows, md, S, has_w, tau, flags)
        for backward in (0, 1):
            off = int(L.fsw_embed_cart_scratch_bytes(ctypes.byref(args(bs, md, S, 8, has_w, tau)), backward))
            on = int(L.fsw_embed_cart_scratch_bytes(ctypes.byref(args(bs, md, S, 8, has_w, tau, flags=bit)), backward))
            assert on == off
    assert some > 0


def test_host_policy():
    """FSW_embedding._cart_split_w_backward on stand-in graphs: the query's bytes for 0 < rows x nSlices <=
    fsw_embed_cart_split_w_backward_max_lines(), 0 above it, for unit weights with tau <= 1 and without a row of the class; positive
    for a weight tensor and for tau = 3 with w = None; _cart_split_backward keeps leaving general weights alone; _cart_tuned_args sets
    each of the four bits only when asked."""
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    import struct

    import torch

    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.fsw_embedding import FSW_embedding
    top = int(_lib.lib().fsw_embed_cart_split_w_backward_max_lines())

    def stand_ins(rows, S, F, has_w, tau, md):
        graph = types.SimpleNamespace(bin_start_host=bin_table(rows).reshape(1, -1), w=torch.zeros(1) if has_w else None)
        module = types.SimpleNamespace(nSlices=S, nFreqs=F, total_mass_pad_thresh=tau)
        module._unit_fast = types.MethodType(FSW_embedding._unit_fast, module)
        st = [0] * 8
        st[_lib.STAT_MAX_DEGREE] = md
        return module, graph, st

    def split_w_bwd(rows, S, F=8, has_w=True, tau=1.0, md=40000):
        return FSW_embedding._cart_split_w_backward(*stand_ins(rows, S, F, has_w, tau, md))

    def split_bwd(rows, S, F=8, has_w=True, tau=1.0, md=40000):
        return FSW_embedding._cart_split_backward(*stand_ins(rows, S, F, has_w, tau, md))

    assert split_w_bwd(1, 4) == own(1, 40000, 4, 8) > 0 and split_w_bwd(1, 4, has_w=False, tau=3.0) == own(1, 40000, 4, 8)
    assert split_w_bwd(1, top) == own(1, 40000, top, 8) and split_w_bwd(1, top + 1) == 0
    assert split_w_bwd(2, top // 2) == own(2, 40000, top // 2, 8) and split_w_bwd(2, top // 2 + 1, F=1) == 0
    assert split_w_bwd(1, 4, has_w=False) == 0 and split_w_bwd(1, 4, has_w=False, tau=0.5) == 0
    assert split_w_bwd(0, 4) == 0 and split_w_bwd(1, 4, md=FIRST - 1) == 0
    # the unit-weight policy keeps leaving general weights alone
    assert split_bwd(1, 4) == 0 and split_bwd(1, 4, has_w=False, tau=3.0) == 0 and split_bwd(1, 4, md=70000) == 0

    # _cart_tuned_args on stand-ins whose tensors live on the host: only the addresses are taken
    words = torch.zeros(NUM_BINS + 1, dtype=torch.int32)
    graph = types.SimpleNamespace(rowptr=words, col=words, w=None, perm=words, bin_start=words, bin_start_host=bin_table(1).reshape(1, -1),
                                  num_rows=1)
    module = types.SimpleNamespace(nFreqs=8, total_mass_pad_thresh=3.0, total_mass_encoding_function="identity", encode_total_mass=False)
    module._mass_scale_read = types.MethodType(FSW_embedding._mass_scale_read, module)
    st = [0] * 8
    st[_lib.STAT_MAX_DEGREE], st[_lib.STAT_USER] = 40000, struct.unpack("i", struct.pack("f", 1.0))[0]
    Xp, fr = torch.zeros((4, 32)), torch.zeros(8)
    bits = {"split": _lib.CART_SPLIT_LINES, "split_backward": _lib.CART_SPLIT_BWD_LINES, "split_w": _lib.CART_SPLIT_W_LINES,
            "split_w_backward": _lib.CART_SPLIT_W_BWD_LINES}
    assert sorted(bits.values()) == [1, 2, 4, 8]
    assert FSW_embedding._cart_tuned_args(module, graph, st, Xp, 32, fr, 4, None, None, 1.0, 0).flags == 0
    for name, bit in bits.items():
        assert FSW_embedding._cart_tuned_args(module, graph, st, Xp, 32, fr, 4, None, None, 1.0, 0, **{name: True}).flags == bit, name
        assert FSW_embedding._cart_tuned_args(module, graph, st, Xp, 32, fr, 4, None, None, 1.0, 0, **{name: False}).flags == 0, name
    everything = FSW_embedding._cart_tuned_args(module, graph, st, Xp, 32, fr, 4, None, None, 1.0, 0, **{name: True for name in bits})
    assert everything.flags == 15
    # the backward asks both policies and hands each its own bit
    src = open(os.path.join(ROOT, "fsw_gnn_amd", "fsw_embedding.py")).read()
    assert "module._cart_split_w_backward(graph, st)" in src and "split_w_backward=split_w_bytes > 0" in src
