"""Cartesian mode, the backward's scratch query fsw_embed_cart_backward_keys_scratch_bytes -- one scratch line per wavefront of the hub
classes, one per workgroup of the kernel of the longest rows (csrc/embed_giant_cart_bwd.hip) -- and the merge path of that kernel
(csrc/merge_path64.h) run on the CPU.  The export, its values against the rule of include/fsw_hip.h recomputed here, the host method
that wraps it, and the older queries and the ABI left as they were.  No GPU is needed."""
import ctypes
import itertools
import os
import subprocess
import types

import pytest

from tests.conftest import ROOT
from tests.test_cart_scratch_cpu import (BIN_GLOBAL, BIN_HUB0, CART_W_MAX_LINE, HUB_MAX_DEG, LDS_MAX_DEG, LIB, MODES, NUM_BINS,
                                         STAT_MAX_DEGREE, bin_table, parent_rules, pow2ceil, query)

LONGEST = (16383, 16384, 24576, 32768, 32769, 65536, 65537, 150000, 2200000)
ROWS = (1, 3, 8, 1000)
SLICES = (1, 4, 64, 1024)
RUN = LDS_MAX_DEG                          # words of a sorted run: a line is rounded up to whole runs
LINE_BYTES = 16                            # per word of a workgroup's line: ping and pong
HUB_LINE_BYTES, HUB_MAX_LINES = 12, 2048   # the classes with one scratch line per wavefront
MAX_WORKGROUPS = 512                       # resident workgroups of the launch, both modes
CAP = 2 << 30
NEW = "fsw_embed_cart_backward_keys_scratch_bytes"


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    return _lib.lib()                       # loads without a device


def backward_query(L, bs, md, has_w, tau, S):
    from fsw_gnn_amd import _lib
    a = _lib.CartArgs()
    a.bin_start_host, a.max_degree, a.tau, a.S = bs.ctypes.data, md, tau, S
    a.w = 16 if has_w else None             # never dereferenced: only compared with NULL
    return int(getattr(L, NEW)(ctypes.byref(a)))


def giant_line_bytes(unit, longest):
    """include/fsw_hip.h: what one workgroup needs for the longest row."""
    return LINE_BYTES * -(-(longest + (0 if unit else 1)) // RUN) * RUN


def rule(unit, bs, md, S):
    """include/fsw_hip.h, recomputed: the maximum of the hub classes' part and of the longest class's part."""
    pad = 0 if unit else 1
    hub = 0
    first_bin, last = (BIN_HUB0, HUB_MAX_DEG) if unit else (BIN_HUB0 - 1, CART_W_MAX_LINE - 1)
    if md > LDS_MAX_DEG - pad and not (unit and int(bs[BIN_GLOBAL]) == int(bs[BIN_HUB0])):
        line = HUB_LINE_BYTES * pow2ceil(min(md, last) + pad)
        rows = max(int(bs[NUM_BINS]) - int(bs[first_bin]), 1)
        hub = max(min(rows * S, HUB_MAX_LINES, CAP // line), 1) * line
    giant = 0
    giant_bin, giant_min = (BIN_GLOBAL, HUB_MAX_DEG + 1) if unit else (BIN_HUB0 + 2, CART_W_MAX_LINE)
    rows = int(bs[NUM_BINS]) - int(bs[giant_bin])
    if md >= giant_min and rows > 0:
        line = giant_line_bytes(unit, md)
        n = min(rows * S, MAX_WORKGROUPS)
        if n >= 8:
            n -= n % 8
        giant = max(min(n, CAP // line), 1) * line
    return max(hub, giant), hub, giant


def test_symbol_prototype_binding_and_abi(L):
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert NEW in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(LIB), NEW)
    assert "size_t fsw_embed_cart_backward_keys_scratch_bytes(const fsw_cart_args* args);" in header
    assert getattr(L, NEW).restype is ctypes.c_size_t
    assert getattr(L, NEW).argtypes == [ctypes.POINTER(_lib.CartArgs)]
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33


def test_the_rule_of_the_header(L):
    cells = with_giant = 0
    for (name, has_w, tau), longest, rows, S, lower in itertools.product(MODES, LONGEST, ROWS, SLICES, (False, True)):
        unit = not has_w and tau <= 1.0
        bs = bin_table(longest, rows, lower)
        want, hub, giant = rule(unit, bs, longest, S)
        got = backward_query(L, bs, longest, has_w, tau, S)
        assert got == want, (name, longest, rows, S, lower, got, want, hub, giant)
        assert got % 16 == 0 and got > 0
        if hub:     # the part of the hub classes is what the two older size functions say for the longest row of those classes
            f = L.fsw_embed_cart_backward_scratch_bytes if unit else L.fsw_embed_cart_weighted_backward_scratch_bytes
            first_bin, last = (BIN_HUB0, HUB_MAX_DEG) if unit else (BIN_HUB0 - 1, CART_W_MAX_LINE - 1)
            assert hub == f(min(longest, last), int(bs[NUM_BINS]) - int(bs[first_bin]), S)
        assert (giant > 0) == (longest >= (HUB_MAX_DEG + 1 if unit else CART_W_MAX_LINE))
        if giant:
            line = giant_line_bytes(unit, longest)
            assert giant % line == 0 and (giant <= CAP or giant == line)
        cells += 1
        with_giant += giant > 0
    assert cells == 3 * 9 * 4 * 4 * 2 and 0 < with_giant < cells


def test_zero_below_the_classes(L):
    for (name, has_w, tau), rows, S in itertools.product(MODES, ROWS, SLICES):
        pad = 1 if has_w or tau > 1.0 else 0
        for longest in (0, 32, 1024, LDS_MAX_DEG - pad):
            assert backward_query(L, bin_table(longest, rows, True), longest, has_w, tau, S) == 0, (name, longest, rows, S)
        assert backward_query(L, bin_table(LDS_MAX_DEG - pad + 1, rows, False), LDS_MAX_DEG - pad + 1, has_w, tau, S) > 0
    assert getattr(L, NEW)(None) == 0


def test_monotone_in_rows_and_slices(L):
    for (name, has_w, tau), longest, lower in itertools.product(MODES, LONGEST, (False, True)):
        table = {(rows, S): backward_query(L, bin_table(longest, rows, lower), longest, has_w, tau, S) for rows in ROWS for S in SLICES}
        for S in SLICES:
            assert all(table[a, S] <= table[b, S] for a, b in zip(ROWS, ROWS[1:])), (name, longest, S)
        for rows in ROWS:
            assert all(table[rows, a] <= table[rows, b] for a, b in zip(SLICES, SLICES[1:])), (name, longest, rows)


def test_one_line_fits_the_buffers_that_worked_before(L):
    """One line < fsw_embed_cart_generic_scratch_bytes(longest, 1), the smallest buffer that worked before, <= the old backward query:
    both still hold a line of the new kernel."""
    seen = 0
    for (name, has_w, tau), longest in itertools.product(MODES, LONGEST):
        unit = not has_w and tau <= 1.0
        if longest < (HUB_MAX_DEG + 1 if unit else CART_W_MAX_LINE):
            continue
        bs = bin_table(longest, 1, False)
        one = backward_query(L, bs, longest, has_w, tau, 1)
        generic = int(L.fsw_embed_cart_generic_scratch_bytes(longest, 1))
        assert one == giant_line_bytes(unit, longest) and 0 < one < generic, (name, longest, one, generic)
        for rows, S in itertools.product(ROWS, SLICES):
            old = query(L, bin_table(longest, rows, False), longest, has_w, tau, S, 1)
            assert generic <= old, (name, longest, rows, S, generic, old)
        seen += 1
    assert seen == 5 + 2 * 8


def test_host_methods(L):
    """FSW_embedding._cart_backward_scratch_bytes returns the new query's value on the stand-in graph of
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
        got = FSW_embedding._cart_backward_scratch_bytes(module, graph, st)
        assert got == backward_query(L, bs, longest, has_w, tau, S), (name, S, longest, rows, lower)
        positive += got > 0
        for backward in (False, True):
            old = FSW_embedding._cart_scratch_bytes(module, graph, st, backward)
            assert old == parent_rules(L, not has_w and tau <= 1.0, bs, longest, S, backward) == query(L, bs, longest, has_w, tau, S, int(backward))
    assert 0 < positive < 3 * 2 * len(cells)


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-g")], ids=["plain", "sanitized"])
def test_merge_path64_native(tmp_path, flags):
    """tests/native/test_merge_path64.cpp: the merge levels of csrc/merge_path64.h on the CPU with the kernel's own helpers, as a plain
    executable and once more under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "fsw_test_merge_path64")
    src = os.path.join(ROOT, "tests", "native", "test_merge_path64.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", *flags, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
