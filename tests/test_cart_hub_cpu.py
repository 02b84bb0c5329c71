"""Cartesian mode, hub rows (2049 .. 32768 unit-weight neighbours): what can be checked without a GPU -- the scratch-size export of
the backward, that a scratch buffer sized the old way still holds a line, and the unchanged ABI."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT

LIB = os.path.join(ROOT, "fsw_gnn_amd", "libfsw_hip.so")
LDS_MAX_DEG, HUB_MAX_DEG = 2048, 32768


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


def boundaries():
    """Every power-of-two boundary of 2049 .. 32768 and the degrees next to it."""
    out = set()
    for p in (2048, 4096, 8192, 16384, 32768):
        out |= {p - 1, p, p + 1}
    return sorted(d for d in out if d >= LDS_MAX_DEG - 1)


def test_backward_scratch_export(L):
    """fsw_embed_cart_backward_scratch_bytes exists, is 0 up to 2048 neighbours and holds at least one line of 12 bytes per element of
    the padded row above."""
    from fsw_gnn_amd import _lib
    assert "fsw_embed_cart_backward_scratch_bytes" in _lib.EXPORTED_SYMBOLS
    f = L.fsw_embed_cart_backward_scratch_bytes
    for d in (0, 1, 32, 2047, 2048):
        assert f(d, 1, 4) == 0 and f(d, 0, 1) == 0, d
    for d in boundaries() + [2049, 3000, 5000, 20000]:
        if LDS_MAX_DEG < d <= HUB_MAX_DEG:
            for rows, S in ((1, 1), (1, 4), (3, 16), (1000, 64)):
                n = f(d, rows, S)
                assert n >= 12 * pow2ceil(d), (d, rows, S, n)
                assert n % (12 * pow2ceil(d)) == 0 and n // (12 * pow2ceil(d)) <= min(2048, rows * S), (d, rows, S, n)
    # rows above 32768 neighbours run on the generic kernel out of the same buffer
    assert f(40000, 2, 4) >= L.fsw_embed_cart_generic_scratch_bytes(40000, 2) >= 12 * pow2ceil(HUB_MAX_DEG)
    # capped at 2 GiB, never below one line
    assert 12 * pow2ceil(HUB_MAX_DEG) <= f(HUB_MAX_DEG, 1 << 20, 1024) <= 2 << 30


def test_generic_sized_scratch_still_holds_a_line(L):
    """Callers that size the scratch with fsw_embed_cart_generic_scratch_bytes(max_degree, 1) -- what was required before the hub
    kernels -- still pass a buffer that holds one 12-byte-per-element line of the longest hub row."""
    for d in boundaries():
        if d > LDS_MAX_DEG:
            assert L.fsw_embed_cart_generic_scratch_bytes(d, 1) >= 12 * pow2ceil(min(d, HUB_MAX_DEG)), d


def test_abi_is_unchanged(L):
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert ctypes.sizeof(_lib.CartArgs) == 240
