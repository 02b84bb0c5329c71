"""Cartesian mode, the forward's scratch query fsw_embed_cart_forward_scratch_bytes: one scratch line per workgroup of the kernels of
the longest rows (csrc/embed_giant_cart.hip, csrc/embed_giant_cart_w.hip).  Its export, its values against the rules of
include/fsw_hip.h, the host method that wraps it, and the older queries and the ABI left as they were.  No GPU is needed."""
import ctypes
import itertools
import os
import types

import pytest

from tests.conftest import ROOT
from tests.test_cart_scratch_cpu import LIB, LONGEST, MODES, STAT_MAX_DEGREE, bin_table, parent_rules, query

UNIT_BLOCK, W_BLOCK = 32768, 8192          # keys of a block of k_cart_giant, (key, weight) elements of one of k_cart_mergepath_w
UNIT_MIN, W_MIN = 32769, 16384             # the shortest rows of the longest class of each mode
MAX_WORKGROUPS = {True: 256, False: 512}   # unit weights / general weights: resident workgroups of the launch
CAP = 2 << 30


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    return _lib.lib()                       # loads without a device


def forward_query(L, bs, md, has_w, tau, S):
    from fsw_gnn_amd import _lib
    a = _lib.CartArgs()
    a.bin_start_host, a.max_degree, a.tau, a.S = bs.ctypes.data, md, tau, S
    a.w = 16 if has_w else None             # never dereferenced: only compared with NULL
    return int(L.fsw_embed_cart_forward_scratch_bytes(ctypes.byref(a)))


def line_bytes(unit, longest):
    """include/fsw_hip.h: what one workgroup needs for the longest row."""
    if unit:
        return 4 * -(-longest // UNIT_BLOCK) * UNIT_BLOCK
    return 16 * -(-(longest + 1) // W_BLOCK) * W_BLOCK


def test_symbol_prototype_binding_and_abi(L):
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert "fsw_embed_cart_forward_scratch_bytes" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(LIB), "fsw_embed_cart_forward_scratch_bytes")
    assert "size_t fsw_embed_cart_forward_scratch_bytes(const fsw_cart_args* args);" in header
    assert L.fsw_embed_cart_forward_scratch_bytes.restype is ctypes.c_size_t
    assert L.fsw_embed_cart_forward_scratch_bytes.argtypes == [ctypes.POINTER(_lib.CartArgs)]
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33


def test_zero_below_the_longest_class_and_positive_from_it(L):
    for (name, has_w, tau), longest, rows, S in itertools.product(MODES, LONGEST, (1, 3), (1, 4)):
        unit = not has_w and tau <= 1.0
        got = forward_query(L, bin_table(longest, rows, True), longest, has_w, tau, S)
        if longest < (UNIT_MIN if unit else W_MIN):
            assert got == 0, (name, longest, rows, S, got)
        else:
            assert got > 0, (name, longest, rows, S)
    assert forward_query(L, bin_table(32768, 1, False), 32768, False, 1.0, 4) == 0
    assert forward_query(L, bin_table(32769, 1, False), 32769, False, 1.0, 4) > 0
    for has_w, tau in ((True, 1.0), (False, 3.0)):
        assert forward_query(L, bin_table(16383, 1, False), 16383, has_w, tau, 4) == 0
        assert forward_query(L, bin_table(16384, 1, False), 16384, has_w, tau, 4) > 0


def test_whole_lines_monotone_and_capped(L):
    """lines x line_bytes with lines = min(rows x S, the launch's workgroups: at most the resident ones, a multiple of 8 from 8 on), at
    most 2 GiB, at least one line; a multiple of 16 bytes; monotone in rows and in S."""
    row_counts, slices = (1, 2, 3, 7, 8, 9, 100, 1000, 1 << 20), (1, 2, 4, 9, 64, 1024)
    for (name, has_w, tau), longest in itertools.product(MODES, (16384, 24576, 32769, 65536, 65537, 150000, 2200000, 400000000)):
        unit = not has_w and tau <= 1.0
        if longest < (UNIT_MIN if unit else W_MIN):
            continue
        line = line_bytes(unit, longest)
        table = {}
        for rows, S in itertools.product(row_counts, slices):
            got = forward_query(L, bin_table(longest, rows, False), longest, has_w, tau, S)
            n = min(rows * S, MAX_WORKGROUPS[unit])
            if n >= 8:
                n -= n % 8
            want = max(min(n, CAP // line), 1) * line
            assert got == want, (name, longest, rows, S, got, want)
            assert got % line == 0 and got % 16 == 0 and got >= line and (got <= CAP or got == line)
            table[rows, S] = got
        for S in slices:
            assert all(table[a, S] <= table[b, S] for a, b in zip(row_counts, row_counts[1:])), (name, longest, S)
        for rows in row_counts:
            assert all(table[rows, a] <= table[rows, b] for a, b in zip(slices, slices[1:])), (name, longest, rows)
        assert table[1, 1] == line


def test_one_line_is_smaller_than_the_generic_buffer(L):
    """A buffer of fsw_embed_cart_generic_scratch_bytes(longest, 1) bytes -- the smallest that worked before -- holds a line."""
    for longest in (16384, 32769, 150000, 2200000):
        generic = int(L.fsw_embed_cart_generic_scratch_bytes(longest, 1))
        for name, has_w, tau in MODES:
            unit = not has_w and tau <= 1.0
            if longest < (UNIT_MIN if unit else W_MIN):
                continue
            one = forward_query(L, bin_table(longest, 1, False), longest, has_w, tau, 1)
            assert one == line_bytes(unit, longest) and 0 < one < generic, (name, longest, one, generic)


def test_host_methods(L):
    """FSW_embedding._cart_forward_scratch_bytes returns the new query's value on the stand-in graph of
    tests/test_cart_scratch_cpu.py::test_host_method, and _cart_scratch_bytes still returns the old values."""
    import torch

    from fsw_gnn_amd.fsw_embedding import FSW_embedding
    cells = ((2049, 3, True), (4096, 1, False), (16383, 1000, True), (16384, 3, False), (32769, 1, False), (150000, 3, True), (32, 1, False))
    positive = 0
    for (name, has_w, tau), S, (longest, rows, lower) in itertools.product(MODES, (1, 64), cells):
        bs = bin_table(longest, rows, lower)
        graph = types.SimpleNamespace(bin_start_host=bs.reshape(1, -1), w=torch.zeros(1) if has_w else None)
        module = types.SimpleNamespace(nSlices=S, total_mass_pad_thresh=tau)
        st = [0] * 8
        st[STAT_MAX_DEGREE] = longest
        got = FSW_embedding._cart_forward_scratch_bytes(module, graph, st)
        assert got == forward_query(L, bs, longest, has_w, tau, S), (name, S, longest, rows, lower)
        positive += got > 0
        for backward in (False, True):
            old = FSW_embedding._cart_scratch_bytes(module, graph, st, backward)
            assert old == parent_rules(L, not has_w and tau <= 1.0, bs, longest, S, backward) == query(L, bs, longest, has_w, tau, S, int(backward))
    assert 0 < positive < 3 * 2 * len(cells)
