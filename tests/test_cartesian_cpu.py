"""Cartesian mode (nSlices x nFreqs) without a GPU: the golden fixtures against the diagonal identity, the fsw_cart_args layout,
and the constructor's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import fsw_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def load_cases(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cases = {}
    for key in z.files:
        case, field = key.split("/")
        cases.setdefault(case, {})[field] = z[key]
    return cases


def case_csr(c):
    """CSR (rowptr, col, w) of a fixture case, rows in output order."""
    X = c["X"]
    if bool(c["graph_mode"]):
        rows, cols, vals = c["rows"].astype(np.int64), c["cols"].astype(np.int64), c["vals"]
        nr = int(c["out"].shape[0])
        rowptr = np.zeros(nr + 1, dtype=np.int64)
        np.add.at(rowptr, rows + 1, 1)
        return X, np.cumsum(rowptr), cols, vals
    Xb = X.reshape(-1, X.shape[-2], X.shape[-1])
    b, n = Xb.shape[0], Xb.shape[1]
    if "W" in c:
        w = c["W"].reshape(-1)
    elif str(c["Wmode"]) == "uniform":
        w = np.full(b * n, 1.0 / n)
    else:
        w = np.ones(b * n)
    return Xb.reshape(b * n, -1), np.arange(b + 1, dtype=np.int64) * n, np.arange(b * n, dtype=np.int64), w


def diagonal_expansion(c):
    """out of the diagonal embedding whose slice s F + f has projVecs[s] and freqs[f] (the reference's own identity)."""
    V, fr = c["V"], c["freqs"]
    S, F = V.shape[0], fr.shape[0]
    X, rowptr, col, w = case_csr(c)
    emb, mass = O.fsw_embed_csr(X, rowptr, col, w, np.repeat(V, F, axis=0), np.tile(fr, S), return_mass=True)
    if bool(c["mass"]):
        emb = O.total_mass_encode(emb, mass, str(c["fn"]), str(c["method"]), float(c["scale"]))
    if "bias" in c:
        emb = emb + c["bias"].reshape(-1)
    return emb


def test_cartesian_goldens_match_diagonal_identity():
    cases = load_cases("cartesian")
    assert {"pc_unit", "pc_batch_weighted", "mass_homog_alt", "graph_weighted", "graph_unit_collapsed"} <= set(cases)
    for name, c in cases.items():
        ref = diagonal_expansion(c)
        out = c["out"].reshape(ref.shape[0], -1)
        assert out.shape == ref.shape, name
        np.testing.assert_allclose(out, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()), err_msg=name)
        # the float32 reference agrees to float32 accuracy
        np.testing.assert_allclose(c["out_f32"].reshape(ref.shape), ref, rtol=0, atol=2e-4 * max(1.0, np.abs(ref).max()), err_msg=name)


def test_cartesian_goldens_shapes():
    cases = load_cases("cartesian")
    for name, c in cases.items():
        S, F = c["V"].shape[0], c["freqs"].shape[0]
        tail = (S * F + int(bool(c["mass"])),) if bool(c["collapse"]) else (S, F)
        assert c["out"].shape[-len(tail):] == tail, name
    degs = np.bincount(cases["graph_weighted"]["rows"], minlength=12)
    assert {0, 1, 32, 33, 2048, 2049} <= set(degs.tolist()) and degs.max() > 4096


def test_cartesian_gradient_fixtures_are_consistent():
    g = load_cases("grads_cartesian")
    for name, c in g.items():
        S, F = c["V"].shape[0], c["freqs"].shape[0]
        assert c["gV"].shape == (S, c["X"].shape[-1]) and c["gfreqs"].shape == (F,) and c["gX"].shape == c["X"].shape, name
    assert "gW" in g["weighted_mass_w"] and "gscale" in g["weighted_mass"] and g["unit_bias"]["gbias"].shape == (6, 4)


def test_cart_args_struct_matches_header_layout():
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    end = header.index("} fsw_cart_args;")
    body = header[header.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.replace("typedef struct {", "").strip()
        if stmt:
            names += [re.findall(r"[A-Za-z_0-9]+", part)[-1] for part in stmt.split(",")]
    assert names == [f[0] for f in _lib.CartArgs._fields_]
    assert ctypes.sizeof(_lib.CartArgs) == 16 + 8 * 6 + 8 * 2 + 8 * 4 + 8 * 2 + 8 * 2 + 8 * 2 + 8 + 8 + 8 * 2 + 8 * 2 + 8 * 2 + 8 * 2
    assert _lib.FSW_ABI_VERSION == 6


def test_cartesian_constructor_on_cpu():
    from fsw_gnn_amd import FSW_embedding
    with pytest.raises(NotImplementedError, match="Cartesian mode needs a HIP device"):
        FSW_embedding(d_in=5, nSlices=3, nFreqs=4, device="cpu")
    with pytest.raises(NotImplementedError, match="Cartesian mode needs a HIP device"):
        FSW_embedding(d_in=5, nSlices=3, nFreqs=4, collapse_freqs=True, encode_total_mass=True, device="cpu")
    # the reference's own assertion for the unsupported combination comes first, on any device
    with pytest.raises(AssertionError, match="collapse_freqs=False is not supported when encode_total_mass=True"):
        FSW_embedding(d_in=5, nSlices=3, nFreqs=4, collapse_freqs=False, encode_total_mass=True, device="cpu")


def test_cartesian_parameter_shapes_match_reference_generator():
    from fsw_gnn_amd import FSW_embedding
    gen = FSW_embedding.generate_embedding_parameters
    for cart, collapse, mass, shape in ((True, False, 0, (3, 4)), (True, True, 0, (12,)), (True, True, 1, (13,)), (False, False, 1, (4,))):
        V, fr, b, _ = gen(d_in=5, nSlices=3, nFreqs=4 if cart else 3, total_mass_encoding_dim=mass, total_mass_encoding_scale_init=1.0,
                          freqs_init='spread', device='cpu', cartesian_mode=cart, collapse_freqs=collapse)
        assert tuple(b.shape) == shape and tuple(V.shape) == (3, 5) and fr.numel() == (4 if cart else 3)
