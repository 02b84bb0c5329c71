"""Cartesian mode with edge features: the golden cases of tests/golden/cartesian_edge.npz (tools/make_cartesian_edge_goldens.py) and the
oracle's restatement of them (tests/test_cartesian_edge_cpu.py, tests/test_hip_cartesian_edge.py).  numpy only.

The restatement: an S x F Cartesian embedding is the diagonal embedding with every slice repeated F times and the frequencies tiled S
times (np.repeat(V, F, 0), np.tile(freqs, S)); column s F + f is (slice s, frequency f).  The gradients of the repeated form are summed
back over the copies: gV over the F copies of a slice, gfreqs over the S copies of a frequency."""
import numpy as np

from oracle import fsw_oracle as O
from tests.conftest import golden


def load_cases():
    """{case: {name: array}} with '<case>/graph' replaced by the graph's arrays (X, rows, cols, vals, ef in float64, num_rows)."""
    data = golden("cartesian_edge")
    groups = {}
    for key in data.files:
        cn, name = key.split("/", 1)
        groups.setdefault(cn, {})[name] = data[key]
    cases = {}
    for cn, c in groups.items():
        if "graph" not in c:
            continue
        g = groups[str(c["graph"])]
        c = dict(c)
        c.update({k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in g.items()})
        c["num_rows"] = int(c["num_rows"])
        cases[cn] = c
    return cases


def dims(c):
    """(S, F, d_in, d_edge)"""
    return c["V"].shape[0], c["freqs"].shape[0], c["X"].shape[1], int(c["d_edge"])


def csr(c):
    rowptr, col, vals = O.csr_from_coo(c["rows"].astype(np.int64), c["cols"].astype(np.int64), c["vals"], c["num_rows"])
    return rowptr, col, vals


def oracle_forward(c):
    """The golden 'out' from the oracle in the repeated-slice form, in the golden's shape."""
    S, F, _, _ = dims(c)
    rowptr, col, vals = csr(c)
    mass = bool(c["mass"])
    bias = c["bias"].reshape(-1) if "bias" in c else None
    out = O.fsw_embedding_forward(c["X"], rowptr, col, vals, np.repeat(c["V"], F, axis=0), np.tile(c["freqs"], S), bias=bias,
                                  encode_total_mass=mass, total_mass_encoding_function=str(c["fn"]),
                                  total_mass_encoding_method=str(c["method"]), total_mass_encoding_scale=float(c["scale"]),
                                  edge_feat=c["ef"])
    return out if bool(c["collapse"]) else out.reshape(c["num_rows"], S, F)


def oracle_gradients(c):
    """(gX, gV [S, d_in + d_edge], gfreqs [F], gX_edge [nnz, d_edge]) of sum(out * G), summed back over the copies."""
    S, F, _, _ = dims(c)
    rowptr, col, vals = csr(c)
    G = c["G"].reshape(c["num_rows"], -1)[:, -S * F:]
    gX, gV, gxi, gef = O.fsw_embed_csr_backward(c["X"], rowptr, col, vals, np.repeat(c["V"], F, axis=0), np.tile(c["freqs"], S), G,
                                                edge_feat=c["ef"])
    return gX, gV.reshape(S, F, -1).sum(axis=1), gxi.reshape(S, F).sum(axis=0), gef
