"""Cartesian mode, the split form of the longest unit-weight rows' backward (csrc/embed_split_cart_bwd.hip): the three host-only exports
fsw_embed_cart_split_backward_scratch_bytes, fsw_embed_cart_split_backward_lines and fsw_embed_cart_split_backward_max_lines, the flag
FSW_CART_SPLIT_BWD_LINES as a second bit of `flags`, the formula of include/fsw_hip.h on hand-made bin tables, the older queries and the
ABI left as they were, the host policy, and the merge levels run on the CPU with the kernel's own span helpers.  No GPU is needed."""
import ctypes
import itertools
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_cart_scratch_cpu import LIB, NUM_BINS
from tests.test_cart_split_cpu import args

RUN = 2048                                  # words of a sorted run: a line is rounded up to whole runs
WORD_BYTES = 16                             # per word of a line: ping and pong, 8 bytes each
WALK = 4096                                 # ranks of a tile of the walk: 256 threads x 16
HUB_LINE_BYTES, HUB_MAX_LINES, HUB_MAX_DEG = 12, 2048, 32768   # the classes below: one scratch line per wavefront
CAP = 2 << 30
MAX_DEGREES, SLICES, FREQS, ROWS = (32769, 65536, 65537, 140000), (1, 3, 16), (1, 5, 70), (1, 2, 5)
NAMES = ("fsw_embed_cart_split_backward_scratch_bytes", "fsw_embed_cart_split_backward_lines", "fsw_embed_cart_split_backward_max_lines")


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    return _lib.lib()                       # loads without a device


def bin_table(rows, hub_rows=0):
    """Host copy of bin_start: three short rows, hub_rows rows of 16385 .. 32768 neighbours and `rows` rows in the last bin."""
    counts = np.zeros(NUM_BINS, dtype=np.int64)
    counts[0], counts[5] = 1, 2
    counts[NUM_BINS - 2], counts[NUM_BINS - 1] = hub_rows, rows
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def own(rows, md, S, F):
    """include/fsw_hip.h: every line owns two regions of run-rounded max_degree words of 8 bytes, then one partial sum per line, walk
    tile and frequency, rounded up to 16 bytes."""
    lines, words, tiles = rows * S, -(-md // RUN) * RUN, -(-md // WALK)
    return lines * words * WORD_BYTES + -(-(lines * tiles * F * 4) // 16) * 16


def hub_part(rows, hub_rows, S):
    """Part 1 of fsw_embed_cart_backward_keys_scratch_bytes for a longest row above 32768 neighbours: lines of 12 x 32768 bytes."""
    if hub_rows == 0:
        return 0
    return min((rows + hub_rows) * S, HUB_MAX_LINES) * HUB_LINE_BYTES * HUB_MAX_DEG


def query(L, a):
    return int(L.fsw_embed_cart_split_backward_scratch_bytes(ctypes.byref(a))), int(L.fsw_embed_cart_split_backward_lines(ctypes.byref(a)))


def test_exports_prototypes_flag_and_abi(L):
    """Fails on a library without the split backward: the symbols do not exist."""
    from fsw_gnn_amd import _lib
    handle = ctypes.CDLL(LIB)
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    for name, proto, restype, argtypes in (
            (NAMES[0], "size_t fsw_embed_cart_split_backward_scratch_bytes(const fsw_cart_args* args);", ctypes.c_size_t, [ctypes.POINTER(_lib.CartArgs)]),
            (NAMES[1], "int64_t fsw_embed_cart_split_backward_lines(const fsw_cart_args* args);", ctypes.c_int64, [ctypes.POINTER(_lib.CartArgs)]),
            (NAMES[2], "int64_t fsw_embed_cart_split_backward_max_lines(void);", ctypes.c_int64, [])):
        assert hasattr(handle, name), name
        assert name in _lib.EXPORTED_SYMBOLS and proto in header, name
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name
    assert re.search(r"#define FSW_CART_SPLIT_BWD_LINES 2\b", header) and _lib.CART_SPLIT_BWD_LINES == 2
    assert re.search(r"#define FSW_CART_SPLIT_LINES 1\b", header) and _lib.CART_SPLIT_LINES == 1
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6
    # the layout of the parent: 240 bytes, 33 fields, flags at byte 164 between mass_fn and mass_scale
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33
    assert _lib.CartArgs.flags.offset == 164 and _lib.CartArgs.flags.size == 4
    assert _lib.CartArgs.mass_fn.offset == 160 and _lib.CartArgs.mass_scale.offset == 168
    # the formula is documented next to the query
    doc = header[header.index("Split form of the longest unit-weight rows' BACKWARD"):header.index("#define FSW_CART_SPLIT_BWD_LINES")]
    for piece in ("lines * words * 16", "lines * tiles * F * 4", "whole runs of 2048", "ceil(max_degree / 4096)", "2 GiB", "16-byte aligned"):
        assert piece in doc, piece


def test_query_follows_the_documented_formula(L):
    for rows, md, S, F in itertools.product(ROWS, MAX_DEGREES, SLICES, FREQS):
        want = own(rows, md, S, F)
        assert want <= CAP and want % 16 == 0
        assert query(L, args(bin_table(rows), md, S, F)) == (want, rows * S), (rows, md, S, F)
    # hand-checked: one row of 140000 neighbours (69 runs, 35 walk tiles), S = 16, F = 16
    assert query(L, args(bin_table(1), 140000, 16, 16)) == (16 * 141312 * 16 + 16 * 35 * 16 * 4, 16)
    # a partial-sum part that is no multiple of 16 bytes is rounded up: 1 line x 9 tiles x 1 frequency = 36 -> 48 bytes
    assert query(L, args(bin_table(1), 32769, 1, 1)) == (34816 * 16 + 48, 1)


def test_query_covers_the_rows_of_the_other_classes(L):
    """Rows of 16385 .. 32768 neighbours run their kernels out of the same buffer: the query is the larger of the two needs."""
    larger = {"own": 0, "hub": 0}
    for rows, hub_rows, md, S in itertools.product(ROWS, (1, 300), MAX_DEGREES, SLICES):
        a, b = own(rows, md, S, 8), hub_part(rows, hub_rows, S)
        assert query(L, args(bin_table(rows, hub_rows), md, S, 8)) == (max(a, b), rows * S), (rows, hub_rows, md, S)
        larger["own" if a >= b else "hub"] += 1
    assert min(larger.values()) > 0, larger


def test_nothing_to_split(L):
    """0 bytes and 0 lines: general weights, tau = 3, no row in the last bin, max_degree <= 32768."""
    for md, S, F in itertools.product(MAX_DEGREES, SLICES, FREQS):
        for a in (args(bin_table(2), md, S, F, has_w=True), args(bin_table(2), md, S, F, tau=3.0), args(bin_table(0, 4), md, S, F),
                  args(bin_table(2), 32768, S, F), args(bin_table(2), 0, S, F)):
            assert query(L, a) == (0, 0)
    assert int(L.fsw_embed_cart_split_backward_scratch_bytes(None)) == 0 and int(L.fsw_embed_cart_split_backward_lines(None)) == 0


def test_nothing_above_two_gib(L):
    """The largest size up to 2 GiB follows the formula, the first above it returns 0 (and no lines: there is no split form then)."""
    S, F, md = 16, 16, 140000
    per_row = own(1, md, S, F)
    fit = CAP // per_row
    assert query(L, args(bin_table(fit), md, S, F)) == (fit * per_row, fit * S) and fit * per_row <= CAP < (fit + 1) * per_row
    assert query(L, args(bin_table(fit + 1), md, S, F)) == (0, 0)
    for rows, big in ((1, 400000000), (1, 600000000), (1 << 20, 150000)):
        assert query(L, args(bin_table(rows), big, 64, F)) == (0, 0)


def test_max_lines(L):
    assert int(L.fsw_embed_cart_split_backward_max_lines()) >= 16      # one cloud at S = 16 always qualifies


def test_older_queries_ignore_the_flag(L):
    from fsw_gnn_amd import _lib
    bit = _lib.CART_SPLIT_BWD_LINES
    for rows, md, S, (has_w, tau) in itertools.product(ROWS, MAX_DEGREES + (32768, 16384), SLICES, ((False, 1.0), (True, 1.0), (False, 3.0))):
        bs = bin_table(rows, 1)
        for name in ("fsw_embed_cart_backward_keys_scratch_bytes", "fsw_embed_cart_forward_scratch_bytes", "fsw_embed_cart_split_scratch_bytes"):
            off = int(getattr(L, name)(ctypes.byref(args(bs, md, S, 8, has_w, tau))))
            on = int(getattr(L, name)(ctypes.byref(args(bs, md, S, 8, has_w, tau, flags=bit))))
            assert on == off, (name, rows, md, S, has_w, tau)


def test_host_policy():
    """FSW_embedding._cart_split_backward on stand-in graphs: the query's bytes for 0 < rows x nSlices <=
    fsw_embed_cart_split_backward_max_lines(), 0 above it, for general weights, for tau > 1 and without a row of the class;
    _cart_tuned_args sets each flag only when asked."""
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    import torch

    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.fsw_embedding import FSW_embedding
    top = int(_lib.lib().fsw_embed_cart_split_backward_max_lines())

    def split(rows, S, F=8, has_w=False, tau=1.0, md=70000):
        graph = types.SimpleNamespace(bin_start_host=bin_table(rows).reshape(1, -1), w=torch.zeros(1) if has_w else None)
        module = types.SimpleNamespace(nSlices=S, nFreqs=F, total_mass_pad_thresh=tau)
        module._unit_fast = types.MethodType(FSW_embedding._unit_fast, module)
        st = [0] * 8
        st[1] = md                           # STAT_MAX_DEGREE
        return FSW_embedding._cart_split_backward(module, graph, st)

    assert split(1, 4) == own(1, 70000, 4, 8)
    assert split(1, top) == own(1, 70000, top, 8) and split(1, top + 1) == 0
    assert split(2, top // 2) == own(2, 70000, top // 2, 8) and split(2, top // 2 + 1, F=1) == 0
    assert split(1, 4, has_w=True) == 0 and split(1, 4, tau=3.0) == 0 and split(0, 4) == 0 and split(1, 4, md=32768) == 0
    src = open(os.path.join(ROOT, "fsw_gnn_amd", "fsw_embedding.py")).read()
    assert "split_backward=split_bytes > 0" in src and "reuse=prepared[\"scratch\"], split_bytes=split_bytes" in src


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-g")], ids=["plain", "sanitized"])
def test_split_bwd_levels_native(tmp_path, flags):
    """tests/native/test_split_bwd_levels.cpp: the levels of the split backward on the CPU with the kernel's own span helpers, the spans
    of every level in reversed and in shuffled order, as a plain executable and once more under the address and undefined-behaviour
    sanitizers (a stand-alone program: no sanitizer enters this process)."""
    exe = str(tmp_path / "fsw_test_split_bwd_levels")
    src = os.path.join(ROOT, "tests", "native", "test_split_bwd_levels.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", *flags, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
