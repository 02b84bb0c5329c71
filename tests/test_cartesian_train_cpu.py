"""Float32 training path of Cartesian mode without a GPU: the new entry point in the header and the binding, the unchanged
fsw_cart_args ABI, and the graph-mode gradient fixture (tests/golden/grads_cartesian_graph.npz)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GRAPH_DEGREES = (0, 1, 32, 33, 256, 257, 2047, 2048, 2049, 4500, 10, 3)


def load_cases(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cases = {}
    for key in z.files:
        case, field = key.split("/")
        cases.setdefault(case, {})[field] = z[key]
    return cases


def test_backward_entry_point_is_declared_and_bound():
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    m = re.search(r"int\s+fsw_embed_cart_backward_keys_f32\s*\(([^)]*)\)\s*;", header)
    assert m, "fsw_embed_cart_backward_keys_f32 is not declared in include/fsw_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["args", "unit_dtable", "lddt", "stream"]
    assert "fsw_embed_cart_backward_keys_f32" in _lib.EXPORTED_SYMBOLS
    restype, argtypes = _lib._SIGNATURES["fsw_embed_cart_backward_keys_f32"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.POINTER(_lib.CartArgs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]


def test_cart_args_abi_is_unchanged():
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33
    assert _lib.FSW_ABI_VERSION == 6 and re.search(r"#define\s+FSW_ABI_VERSION\s+6\b", header)


def test_graph_gradient_fixture_is_consistent():
    cases = load_cases("grads_cartesian_graph")
    assert set(cases) == {"graph", "unit_bias", "weighted_mass"}
    gr = cases["graph"]
    n, d_in = gr["X"].shape
    nnz = gr["rows"].shape[0]
    assert (n, d_in) == (5000, 5) and gr["cols"].shape == (nnz,) and gr["vals"].shape == (nnz,)
    assert tuple(np.bincount(gr["rows"], minlength=len(GRAPH_DEGREES))) == GRAPH_DEGREES
    assert gr["cols"].min() >= 0 and gr["cols"].max() < n and (gr["vals"] > 0).all()
    assert (np.diff(gr["rows"]) >= 0).all()                                   # coalesced COO order
    for name in ("unit_bias", "weighted_mass"):
        c = cases[name]
        S, F = c["V"].shape[0], c["freqs"].shape[0]
        mass = int(bool(c["mass"]))
        assert (S, F) == (6, 4) and c["V"].shape == (S, d_in) and bool(c["collapse"]), name
        assert (c["freqs"] >= 0.25).all(), name                               # shifted away from xi = 0
        width = S * F + mass
        assert c["out"].shape == (len(GRAPH_DEGREES), width) and c["G"].shape == c["out"].shape, name
        assert c["gX"].shape == (n, d_in) and c["gV"].shape == (S, d_in) and c["gfreqs"].shape == (F,), name
        assert all(np.isfinite(c[k]).all() for k in ("out", "gX", "gV", "gfreqs")), name
        # senders without an edge receive no gradient
        unused = np.setdiff1d(np.arange(n), gr["cols"])
        assert unused.size > 0 and not c["gX"][unused].any(), name
    u, w = cases["unit_bias"], cases["weighted_mass"]
    assert bool(u["unit"]) and not bool(w["unit"])
    assert u["bias"].shape == (24,) and u["gbias"].shape == (24,) and "gscale" not in u and not bool(u["mass"])
    # the empty recipient's output is the bias alone, and the bias gradient is the column sum of G
    np.testing.assert_allclose(u["out"][0], u["bias"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(u["gbias"], u["G"].sum(0), rtol=1e-13, atol=1e-13)
    assert bool(w["mass"]) and str(w["fn"]) == "sqrt" and float(w["scale"]) == 0.8 and w["gscale"].shape == () and "bias" not in w
    # total-mass column: f(m) * scale with f = 2 (sqrt(1 + m) - 1) of the summed weights
    m = np.bincount(gr["rows"], weights=gr["vals"], minlength=len(GRAPH_DEGREES))
    np.testing.assert_allclose(w["out"][:, 0], 0.8 * 2 * (np.sqrt(1 + m) - 1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(float(w["gscale"]), (w["G"][:, 0] * 2 * (np.sqrt(1 + m) - 1)).sum(), rtol=1e-12)
    assert os.path.getsize(os.path.join(GOLD, "grads_cartesian_graph.npz")) < (1 << 20)
