"""Cartesian mode, the split form of the longest unit-weight rows (csrc/embed_split_cart.hip): the three host-only exports
fsw_embed_cart_split_scratch_bytes, fsw_embed_cart_split_lines and fsw_embed_cart_split_max_lines, the flag FSW_CART_SPLIT_LINES in the
field that was `reserved`, the formula of include/fsw_hip.h on hand-made bin tables, and the ABI and the older query left as they were.
No GPU is needed."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_cart_scratch_cpu import LIB, NUM_BINS

BLOCK = 32768                               # keys of a block (k_cart_giant, the split kernels)
CAP = 2 << 30
MAX_DEGREES, SLICES, FREQS, ROWS = (32769, 65536, 65537, 140000), (1, 3, 16), (1, 5, 70), (1, 2, 5)


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    return _lib.lib()                       # loads without a device


def last_bin_table(rows, below=4):
    """Host copy of bin_start: `below` rows spread over shorter bins and `rows` rows in the last bin (above 32768 neighbours)."""
    counts = np.zeros(NUM_BINS, dtype=np.int64)
    counts[0], counts[5], counts[NUM_BINS - 2] = 1, below - 2, 1
    counts[NUM_BINS - 1] = rows
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def args(bs, md, S, F, has_w=False, tau=1.0, flags=0):
    from fsw_gnn_amd import _lib
    a = _lib.CartArgs()
    a.keep = bs                             # the struct holds only the address
    a.bin_start_host, a.max_degree, a.tau, a.S, a.F, a.flags = bs.ctypes.data, md, tau, S, F, flags
    a.w = 16 if has_w else None             # never dereferenced: only compared with NULL
    return a


def formula(rows, md, S, F):
    """include/fsw_hip.h: every line owns block-rounded max_degree keys of 4 bytes, then one partial sum per line, block and frequency."""
    lines, nbmax = rows * S, -(-md // BLOCK)
    regions = lines * nbmax * BLOCK * 4
    assert regions % 16 == 0                # so the partial sums start 16-byte aligned right behind the regions
    return regions + lines * nbmax * F * 4


def test_exports_prototypes_flag_and_abi(L):
    """Fails on a library without the split form: the symbols do not exist."""
    from fsw_gnn_amd import _lib
    handle = ctypes.CDLL(LIB)
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    for name, proto, restype, argtypes in (
            ("fsw_embed_cart_split_scratch_bytes", "size_t fsw_embed_cart_split_scratch_bytes(const fsw_cart_args* args);", ctypes.c_size_t,
             [ctypes.POINTER(_lib.CartArgs)]),
            ("fsw_embed_cart_split_lines", "int64_t fsw_embed_cart_split_lines(const fsw_cart_args* args);", ctypes.c_int64,
             [ctypes.POINTER(_lib.CartArgs)]),
            ("fsw_embed_cart_split_max_lines", "int64_t fsw_embed_cart_split_max_lines(void);", ctypes.c_int64, [])):
        assert hasattr(handle, name), name
        assert name in _lib.EXPORTED_SYMBOLS and proto in header, name
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name
    assert re.search(r"#define FSW_CART_SPLIT_LINES 1\b", header) and _lib.CART_SPLIT_LINES == 1
    # the formula is documented next to the query
    doc = header[header.index("Split form of the longest unit-weight rows"):header.index("#define FSW_CART_SPLIT_LINES")]
    for piece in ("lines * nbmax * 32768 * 4", "lines * nbmax * F * 4", "ceil(max_degree / 32768)", "2 GiB", "16-byte aligned"):
        assert piece in doc, piece
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6


def test_struct_layout_is_unchanged():
    """`reserved` became `flags`: same offset (between mass_fn and mass_scale), same size, same struct size, no field more."""
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    body = header[header.index("int32_t value_dtype;"):header.index("} fsw_cart_args;")]
    assert re.search(r"int32_t mass_fn;\s*int32_t flags;[^\n]*\n\s*double mass_scale;", body) and "reserved" not in body
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33
    names = [f[0] for f in _lib.CartArgs._fields_]
    assert "reserved" not in names and names.index("flags") == names.index("mass_fn") + 1 == names.index("mass_scale") - 1
    assert _lib.CartArgs.flags.offset == _lib.CartArgs.mass_fn.offset + 4 == _lib.CartArgs.mass_scale.offset - 4
    assert _lib.CartArgs.flags.size == 4
    assert _lib.CartArgs().flags == 0       # a caller that never sets it keeps flags == 0


def test_query_follows_the_documented_formula(L):
    for rows, md, S, F in itertools.product(ROWS, MAX_DEGREES, SLICES, FREQS):
        bs = last_bin_table(rows)
        a = args(bs, md, S, F)
        want = formula(rows, md, S, F)
        assert want <= CAP
        assert int(L.fsw_embed_cart_split_scratch_bytes(ctypes.byref(a))) == want, (rows, md, S, F)
        assert int(L.fsw_embed_cart_split_lines(ctypes.byref(a))) == rows * S, (rows, md, S, F)
    # hand-checked: one row of 140000 neighbours (5 blocks), S = 16, F = 16
    a = args(last_bin_table(1), 140000, 16, 16)
    assert int(L.fsw_embed_cart_split_scratch_bytes(ctypes.byref(a))) == 16 * 5 * 131072 + 16 * 5 * 16 * 4


def test_nothing_to_split(L):
    """0 bytes and 0 lines: general weights, tau > 1, no row in the class's bin, max_degree below the class."""
    for md, S, F in itertools.product(MAX_DEGREES, SLICES, FREQS):
        for a in (args(last_bin_table(2), md, S, F, has_w=True), args(last_bin_table(2), md, S, F, tau=3.0),
                  args(last_bin_table(0), md, S, F), args(last_bin_table(2), 32768, S, F), args(last_bin_table(2), 0, S, F)):
            assert int(L.fsw_embed_cart_split_scratch_bytes(ctypes.byref(a))) == 0
            assert int(L.fsw_embed_cart_split_lines(ctypes.byref(a))) == 0
    assert int(L.fsw_embed_cart_split_scratch_bytes(None)) == 0 and int(L.fsw_embed_cart_split_lines(None)) == 0


def test_nothing_above_two_gib(L):
    """The largest sizes up to 2 GiB follow the formula, the first above it returns 0 (and no lines: there is no split form then)."""
    S, F, md = 16, 16, 140000
    per_row = formula(1, md, S, F)
    fit = CAP // per_row
    a = args(last_bin_table(fit), md, S, F)
    assert int(L.fsw_embed_cart_split_scratch_bytes(ctypes.byref(a))) == fit * per_row <= CAP
    a = args(last_bin_table(fit + 1), md, S, F)
    assert (fit + 1) * per_row > CAP
    assert int(L.fsw_embed_cart_split_scratch_bytes(ctypes.byref(a))) == 0 and int(L.fsw_embed_cart_split_lines(ctypes.byref(a))) == 0
    for rows, big in ((1, 400000000), (1, 600000000), (1 << 20, 150000)):
        a = args(last_bin_table(rows), big, 64, F)
        assert int(L.fsw_embed_cart_split_scratch_bytes(ctypes.byref(a))) == 0


def test_max_lines(L):
    assert int(L.fsw_embed_cart_split_max_lines()) >= 16      # one cloud at S = 16 always qualifies


def test_forward_query_ignores_the_flag(L):
    from fsw_gnn_amd import _lib
    for rows, md, S, (has_w, tau) in itertools.product(ROWS, MAX_DEGREES + (32768, 16384), SLICES, ((False, 1.0), (True, 1.0), (False, 3.0))):
        bs = last_bin_table(rows)
        off = int(L.fsw_embed_cart_forward_scratch_bytes(ctypes.byref(args(bs, md, S, 8, has_w, tau))))
        on = int(L.fsw_embed_cart_forward_scratch_bytes(ctypes.byref(args(bs, md, S, 8, has_w, tau, flags=_lib.CART_SPLIT_LINES))))
        assert on == off, (rows, md, S, has_w, tau)


def test_host_policy():
    """FSW_embedding._cart_split on stand-in graphs: the split query's bytes for 0 < rows x nSlices <= fsw_embed_cart_split_max_lines(),
    0 above it, for general weights, for tau > 1 and without a row of the class; _cart_tuned_args sets the flag only when asked."""
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    import types

    import torch

    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.fsw_embedding import FSW_embedding
    lib = _lib.lib()
    top = int(lib.fsw_embed_cart_split_max_lines())
    st = [0] * 8
    st[1] = 70000                            # STAT_MAX_DEGREE

    def split(rows, S, F=8, has_w=False, tau=1.0, md=70000):
        graph = types.SimpleNamespace(bin_start_host=last_bin_table(rows).reshape(1, -1), w=torch.zeros(1) if has_w else None)
        module = types.SimpleNamespace(nSlices=S, nFreqs=F, total_mass_pad_thresh=tau)
        s = list(st)
        s[1] = md
        return FSW_embedding._cart_split(module, graph, s)

    assert split(1, 4) == formula(1, 70000, 4, 8)
    assert split(1, top) == formula(1, 70000, top, 8) and split(1, top + 1) == 0
    assert split(2, top // 2) == formula(2, 70000, top // 2, 8) and split(2, top // 2 + 1, F=1) == 0
    assert split(1, 4, has_w=True) == 0 and split(1, 4, tau=3.0) == 0 and split(0, 4) == 0 and split(1, 4, md=32768) == 0
