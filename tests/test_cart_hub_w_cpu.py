"""Cartesian mode, general weights, lines of 2049 .. 16384 elements (2048 .. 16383 neighbours plus the pad element): what can be checked
without a GPU -- the scratch-size export of the weighted backward, that a scratch buffer sized the old way still holds a line, the
new constant of the header and the unchanged ABI."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT

LIB = os.path.join(ROOT, "fsw_gnn_amd", "libfsw_hip.so")
LDS_MAX_DEG, CART_W_MAX_LINE = 2048, 16384
CLASS_DEGREES = (2048, 4095, 4096, 16383)       # neighbours: both ends of the tuned classes and one edge between two
BEYOND_DEGREES = (16384, 40000)                 # these rows stay on the generic kernel
SHAPES = ((1, 1), (1, 4), (3, 16), (1000, 64))  # (rows, S)


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


def test_weighted_backward_scratch_export(L):
    """fsw_embed_cart_weighted_backward_scratch_bytes is bound and exported; 0 below 2048 neighbours; for the tuned classes whole lines
    of 12 bytes per element of the padded line (D + 1), at most min(2048, rows * S) of them; with rows that stay on the generic kernel
    at least what that kernel needs."""
    from fsw_gnn_amd import _lib
    assert "fsw_embed_cart_weighted_backward_scratch_bytes" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(LIB), "fsw_embed_cart_weighted_backward_scratch_bytes")
    f = L.fsw_embed_cart_weighted_backward_scratch_bytes
    for d in (0, 32, 2047):
        assert f(d, 1, 4) == 0 and f(d, 0, 1) == 0, d
    for d in CLASS_DEGREES:
        line = 12 * pow2ceil(d + 1)
        for rows, S in SHAPES:
            n = f(d, rows, S)
            assert n >= line and n % line == 0 and n // line <= min(2048, rows * S), (d, rows, S, n)
    for d in BEYOND_DEGREES:
        for rows, S in SHAPES:
            assert f(d, rows, S) >= L.fsw_embed_cart_generic_scratch_bytes(d, rows) > 0, (d, rows, S)
            assert f(d, rows, S) >= 12 * CART_W_MAX_LINE, (d, rows, S)
    # capped at 2 GiB, never below one line
    assert 12 * CART_W_MAX_LINE <= f(CART_W_MAX_LINE - 1, 1 << 20, 1024) <= 2 << 30


def test_generic_sized_scratch_still_holds_a_line(L):
    """Callers that size the backward scratch with fsw_embed_cart_generic_scratch_bytes(max_degree, 1) -- what was required before these
    classes -- still pass a buffer that holds one 12-byte-per-element line of the longest row."""
    for d in CLASS_DEGREES + BEYOND_DEGREES:
        assert L.fsw_embed_cart_generic_scratch_bytes(d, 1) >= 12 * pow2ceil(d + 1), d


def test_unit_backward_scratch_sizes_are_unchanged(L):
    """The new export sits next to fsw_embed_cart_backward_scratch_bytes and does not replace it."""
    f = L.fsw_embed_cart_backward_scratch_bytes
    assert f(2048, 1, 4) == 0 and f(2049, 1, 4) == 4 * 12 * 4096 and f(32768, 3, 16) == 48 * 12 * 32768


def test_header_constant_and_abi(L):
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert re.search(r"^#define FSW_CART_W_MAX_LINE 16384\b", header, re.M)
    assert "size_t fsw_embed_cart_weighted_backward_scratch_bytes(int64_t max_degree, int64_t long_rows, int32_t S);" in header
    assert _lib.CART_W_MAX_LINE == CART_W_MAX_LINE
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33
