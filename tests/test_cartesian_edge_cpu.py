"""Cartesian mode with edge features (d_edge > 0): what can be checked without a GPU -- the new entry point fsw_edge_keys_f32 is declared,
bound and checks its arguments on the host; the ABI version and struct fsw_cart_args are what they were (the feature adds a symbol and
nothing else); the golden file of the reference's dense-W path loads; and the oracle in the repeated-slice form (every slice repeated F
times, the frequencies tiled S times, edge_feat=) reproduces it -- the restatement tests/test_hip_cartesian_edge.py leans on."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import cartesian_edge_cases as CE
from tests.conftest import ROOT, relerr

LIB = os.path.join(ROOT, "fsw_gnn_amd", "libfsw_hip.so")
TOL64 = 1e-12
FORWARD_CASES = ("collapsed_bias", "matrix_bias", "mass_plain", "mass_homog_sqrt", "d_edge1_squeezed")


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(LIB):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    return _lib.lib()                       # loads without a device


@pytest.fixture(scope="module")
def cases():
    return CE.load_cases()


def test_entry_point_is_declared_and_bound(L):
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert re.search(r"int fsw_edge_keys_f32\(const int32_t\* col, int64_t nnz, const float\* Xp, int64_t ldp, const float\* efeat, "
                     r"int d_edge, const float\* Ve,\s+int64_t ldve, int S, float\* K, int64_t ldk, fsw_stream_t stream\);", header)
    assert "fmaf(efeat[e*d_edge + q], Ve[s*ldve + q], key)" in header            # the rounding rule is part of the contract
    assert "fsw_edge_keys_f32" in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(LIB), "fsw_edge_keys_f32")
    assert len(_lib._SIGNATURES["fsw_edge_keys_f32"][1]) == 12


def test_abi_version_and_cart_args_are_unchanged(L):
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _lib.FSW_ABI_VERSION == 6 and L.fsw_abi_version() == 6
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33


def test_argument_checks_on_the_host(L):
    """nnz == 0 returns 0 without a launch (null pointers allowed); bad strides and sizes return the error code before any launch."""
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int32 * 4)()
    p, ip = ctypes.addressof(buf), ctypes.addressof(idx)
    assert L.fsw_edge_keys_f32(None, 0, None, 4, None, 2, None, 2, 4, None, 4, None) == 0
    assert L.fsw_edge_keys_f32(ip, 0, p, 3, p, 2, p, 7, 3, p, 4, None) == 0
    bad = [dict(ldp=2), dict(ldk=2), dict(ldve=1), dict(S=0), dict(d_edge=0), dict(nnz=-1), dict(nnz=1 << 31)]
    for kw in bad:
        a = dict(nnz=4, ldp=3, d_edge=2, ldve=2, S=3, ldk=3)
        a.update(kw)
        rc = L.fsw_edge_keys_f32(ip, a["nnz"], p, a["ldp"], p, a["d_edge"], p, a["ldve"], a["S"], p, a["ldk"], None)
        assert rc == 1 and b"fsw_edge_keys_f32" in L.fsw_last_error(), kw
    for null in range(5):                   # col, Xp, efeat, Ve, K
        ptrs = [ip, p, p, p, p]
        ptrs[null] = None
        assert L.fsw_edge_keys_f32(ptrs[0], 4, ptrs[1], 3, ptrs[2], 2, ptrs[3], 2, 3, ptrs[4], 3, None) == 1, null


def test_golden_file_loads(cases):
    assert set(cases) == set(FORWARD_CASES) | {"grad_collapsed_bias"}
    for name, c in cases.items():
        S, F, d_in, d_edge = CE.dims(c)
        assert (S, F, d_in) == (3, 4, 5) and d_edge == (1 if name == "d_edge1_squeezed" else 2) and c["V"].shape == (S, d_in + d_edge)
        assert c["ef"].shape == (c["rows"].size, d_edge) and c["X"].shape == (2200, d_in)
        deg = np.bincount(c["rows"], minlength=c["num_rows"])
        assert tuple(deg) == (0, 1, 32, 33, 300, 2047, 2048, 2100)
        order = np.lexsort((c["cols"], c["rows"]))
        assert np.array_equal(order, np.arange(order.size))                       # coalesced COO order
        assert abs(c["vals"][c["rows"] == 4].sum() - 0.4) < 1e-6                  # one row of total mass 0.4
        assert (c["freqs"] == 0).any() or name.startswith("grad")
        assert (c["freqs"] < 0).any()
        assert c["out"].shape == ((8, S * F + int(c["mass"])) if bool(c["collapse"]) else (8, S, F))
        if not name.startswith("grad"):
            assert c["out_f32"].shape == c["out"].shape and relerr(c["out_f32"], c["out"]) < 1e-5
    g = cases["grad_collapsed_bias"]
    assert g["gX"].shape == (2200, 5) and g["gV"].shape == (3, 7) and g["gfreqs"].shape == (4,) and g["gbias"].shape == (12,)
    assert g["gX_edge"].shape == (g["rows"].size, 2)


@pytest.mark.parametrize("name", FORWARD_CASES + ("grad_collapsed_bias",))
def test_oracle_in_repeated_slice_form_reproduces_the_reference(cases, name):
    c = cases[name]
    e = relerr(CE.oracle_forward(c), c["out"])
    print("%s: oracle (repeated slices, edge_feat) against the reference's dense-W path %.2e" % (name, e))
    assert e <= TOL64, (name, e)


def test_oracle_gradients_reproduce_the_reference(cases):
    c = cases["grad_collapsed_bias"]
    gX, gV, gfreqs, gef = CE.oracle_gradients(c)
    errs = {"gX": relerr(gX, c["gX"]), "gV": relerr(gV, c["gV"]), "gfreqs": relerr(gfreqs, c["gfreqs"]),
            "gX_edge": relerr(gef, c["gX_edge"]), "gbias": relerr(c["G"].sum(axis=0), c["gbias"])}
    print("gradients, oracle against the reference: " + "  ".join("%s %.2e" % kv for kv in errs.items()))
    assert max(errs.values()) <= TOL64, errs
