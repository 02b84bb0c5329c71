"""Generates tests/golden/cartesian_edge.npz: Cartesian mode (nSlices x nFreqs) WITH edge features (d_edge > 0) of the UNMODIFIED
reference, run on CPU through oracle/ref_harness.py (only where the reference exists).

    python tools/make_cartesian_edge_goldens.py

The reference runs this combination only through its dense-W graph path (graph_mode=True, dense W [nR, n], dense X_edge
[nR, n, d_edge] or [nR, n] for d_edge = 1); its sparse-W path fails for it, and its constructor cannot build a Cartesian module with
both the total mass and a bias, so the mass cases have enable_bias=False (as in tools/make_cartesian_goldens.py).

Every case is stored as flat arrays '<case>/<name>' in float64 (parameters, outputs) plus the float32 module's output
'<case>/out_f32'.  The two graphs (d_edge = 2 and d_edge = 1) are stored once, '<graph>/<name>' with '<case>/graph' naming the one a
case uses: X and the nonzero entries (rows, cols, vals, ef [nnz, d_edge]) sorted by (row, col), all exactly representable in the
float32 they are stored in; the tests rebuild W and X_edge densely.
One gradient case (float64): gX, gV (all d_in + d_edge columns), gfreqs, gbias and gX_edge at the entries.
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fsw_gnn_amd import synth  # noqa: E402
from oracle import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
S, F, D_IN, D_EDGE = 3, 4, 5, 2
DEGREES = (0, 1, 32, 33, 300, 2047, 2048, 2100)     # in-degrees of the recipients: both sides of the kernels' class boundaries
SENDERS = 2200
LOW_MASS_ROW, LOW_MASS = 4, 0.4                     # the row of 300 neighbours carries total mass 0.4 (< tau = 1: the pad element)
FREQS = np.array([0.0, -0.6, 0.8, 2.5])             # xi = 0 (the readout's limit) and a negative frequency
FREQS_GRAD = np.array([-0.6, 0.3, 1.1, 2.4])        # gradients away from xi = 0
warnings.filterwarnings("ignore")


def graph(d_edge, seed=504):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r, deg in enumerate(DEGREES):
        rows.append(np.full(deg, r))
        cols.append(np.sort(rng.choice(SENDERS, size=deg, replace=False)))
    rows = np.concatenate(rows).astype(np.int32)
    cols = np.concatenate(cols).astype(np.int32)
    vals = rng.uniform(0.05, 1.0, size=rows.shape[0])
    low = rows == LOW_MASS_ROW
    vals[low] *= LOW_MASS / vals[low].sum()
    vals = vals.astype(np.float32).astype(np.float64)
    ef = rng.normal(size=(rows.shape[0], d_edge)).astype(np.float32).astype(np.float64)
    X = synth.features(SENDERS, D_IN, seed=seed + 1).astype(np.float64)
    return X, rows, cols, vals, ef


def dense(rows, cols, vals, ef, dt, squeeze):
    r, c = torch.from_numpy(rows).long(), torch.from_numpy(cols).long()
    W = torch.zeros((len(DEGREES), SENDERS), dtype=dt)
    W[r, c] = torch.from_numpy(vals).to(dt)
    Xe = torch.zeros((len(DEGREES), SENDERS, ef.shape[1]), dtype=dt)
    Xe[r, c] = torch.from_numpy(ef).to(dt)
    return W, (Xe[..., 0] if squeeze else Xe)         # d_edge = 1: X_edge of shape W.shape


def params(seed, d_edge, bias_shape, freqs):
    V = synth.unit_slices(S, D_IN + d_edge, seed=seed).astype(np.float64)
    bias = None if bias_shape is None else (0.1 * synth.normal(seed + 2, 1, bias_shape, dtype=np.float64)).astype(np.float32).astype(np.float64)
    return V, freqs.astype(np.float64), bias


def make_module(emb, dt, d_edge, collapse, mass=False, method="plain", fn="identity", bias=True, scale=1.0, learn=False):
    return emb.FSW_embedding(d_in=D_IN, d_edge=d_edge, nSlices=S, nFreqs=F, collapse_freqs=collapse, encode_total_mass=mass,
                             total_mass_encoding_method=method, total_mass_encoding_function=fn, total_mass_encoding_scale=scale,
                             enable_bias=bias, learnable_slices=learn, learnable_freqs=learn, device="cpu", dtype=dt,
                             load_custom_cuda_lib=False)


def set_params(E, V, fr, bias):
    with torch.no_grad():
        E.projVecs.copy_(torch.from_numpy(V).to(E.projVecs.dtype))
        E.freqs.copy_(torch.from_numpy(fr).to(E.freqs.dtype))
        if bias is not None:
            E.bias.copy_(torch.from_numpy(bias).to(E.bias.dtype).reshape(E.bias.shape))


def graph_arrays(d_edge):
    X, rows, cols, vals, ef = graph(d_edge)
    f32 = lambda a: a.astype(np.float32)
    assert all(np.array_equal(f32(a).astype(np.float64), a) for a in (X, vals, ef))
    return {"X": f32(X), "rows": rows, "cols": cols, "vals": f32(vals), "ef": f32(ef), "num_rows": np.array(len(DEGREES))}


def base_case(kw, d_edge, squeeze, V, fr, bias):
    c = {"graph": np.array("graph%d" % d_edge), "V": V, "freqs": fr, "d_edge": np.array(d_edge),
         "squeeze": np.array(squeeze), "collapse": np.array(kw.get("collapse", False)), "mass": np.array(kw.get("mass", False)),
         "method": np.array(kw.get("method", "plain")), "fn": np.array(kw.get("fn", "identity")), "scale": np.array(kw.get("scale", 1.0))}
    if bias is not None:
        c["bias"] = bias
    return c


def forward_cases(emb):
    specs = [
        ("collapsed_bias", dict(collapse=True), D_EDGE, False, (S * F,)),
        ("matrix_bias", dict(collapse=False), D_EDGE, False, (S, F)),
        ("mass_plain", dict(collapse=True, mass=True, method="plain", bias=False, scale=0.7), D_EDGE, False, None),
        ("mass_homog_sqrt", dict(collapse=True, mass=True, method="homog", fn="sqrt", bias=False), D_EDGE, False, None),
        ("d_edge1_squeezed", dict(collapse=True), 1, True, (S * F,)),
    ]
    cases = {}
    for i, (name, kw, d_edge, squeeze, bshape) in enumerate(specs):
        X, rows, cols, vals, ef = graph(d_edge)
        V, fr, bias = params(510 + 7 * i, d_edge, bshape, FREQS)
        c = base_case(kw, d_edge, squeeze, V, fr, bias)
        for dt, tag in ((torch.float64, "out"), (torch.float32, "out_f32")):
            E = make_module(emb, dt, d_edge, **kw)
            set_params(E, V, fr, bias)
            W, Xe = dense(rows, cols, vals, ef, dt, squeeze)
            with torch.no_grad():
                c[tag] = E(torch.from_numpy(X).to(dt), W, X_edge=Xe, graph_mode=True).numpy().astype(np.float64)
        print(name, c["out"].shape, flush=True)
        cases[name] = c
    return cases


def grad_case(emb):
    kw = dict(collapse=True)
    X, rows, cols, vals, ef = graph(D_EDGE)
    V, fr, bias = params(610, D_EDGE, (S * F,), FREQS_GRAD)
    E = make_module(emb, torch.float64, D_EDGE, learn=True, **kw)
    set_params(E, V, fr, bias)
    W, Xe = dense(rows, cols, vals, ef, torch.float64, False)
    Xt, Xe = torch.from_numpy(X).requires_grad_(True), Xe.requires_grad_(True)
    out = E(Xt, W, X_edge=Xe, graph_mode=True)
    G = synth.normal(620, 1, tuple(out.shape), dtype=np.float64)
    (out * torch.from_numpy(G)).sum().backward()
    c = base_case(kw, D_EDGE, False, V, fr, bias)
    c.update({"G": G, "out": out.detach().numpy(), "gX": Xt.grad.numpy(), "gV": E.projVecs.grad.numpy(), "gfreqs": E.freqs.grad.numpy(),
              "gbias": E.bias.grad.numpy().reshape(-1),
              "gX_edge": Xe.grad[torch.from_numpy(rows).long(), torch.from_numpy(cols).long()].numpy()})
    print("grad", {k: v.shape for k, v in c.items() if k.startswith("g")}, flush=True)
    return {"grad_collapsed_bias": c}


def main():
    if not ref_harness.available():
        raise SystemExit("the reference implementation is not present: nothing to generate")
    emb, _ = ref_harness.load()
    cases = forward_cases(emb)
    cases.update(grad_case(emb))
    cases.update({"graph%d" % d: graph_arrays(d) for d in (D_EDGE, 1)})
    flat = {"%s/%s" % (cn, k): v for cn, c in cases.items() for k, v in c.items()}
    path = os.path.join(GOLD, "cartesian_edge.npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", flush=True)


if __name__ == "__main__":
    main()
