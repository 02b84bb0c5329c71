"""Generates tests/golden/cartesian.npz and tests/golden/grads_cartesian.npz: Cartesian mode (nSlices x nFreqs) of the UNMODIFIED
reference run on CPU through oracle/ref_harness.py (only where the reference exists).

    python tools/make_cartesian_goldens.py

Inputs come from fsw_gnn_amd/synth.py; parameters are written into the reference modules explicitly.  Every case is stored as
flat arrays '<case>/<name>' in float64 (inputs, parameters, outputs) plus the float32 module's output '<case>/out_f32'.
The dense-W graph is stored as its nonzero entries (rows, cols, vals) and rebuilt densely by the tests.
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
S, F, D_IN = 6, 4, 5
# in-degrees of the dense-W graph's 12 recipients: every degree class of the Cartesian kernels and their edges
GRAPH_DEGREES = (0, 1, 32, 33, 256, 257, 2047, 2048, 2049, 4500, 10, 3)
GRAPH_SENDERS = 5000
warnings.filterwarnings("ignore")


def params(seed, bias_shape=None):
    V = synth.unit_slices(S, D_IN, seed=seed).astype(np.float64)
    fr = np.sort(synth.uniform01(seed + 1, 0, 0, F) * 3.0).astype(np.float32).astype(np.float64)
    fr[0] = 0.0 if seed % 2 else fr[0]           # xi = 0 in some cases (the readout's limit)
    bias = None if bias_shape is None else (0.1 * synth.normal(seed + 2, 1, bias_shape, dtype=np.float64)).astype(np.float32).astype(np.float64)
    return V, fr, bias


def make_module(emb, dt, collapse, mass=False, method="plain", fn="identity", bias=True, scale=1.0, learn=False):
    return emb.FSW_embedding(d_in=D_IN, nSlices=S, nFreqs=F, collapse_freqs=collapse, encode_total_mass=mass,
                             total_mass_encoding_method=method, total_mass_encoding_function=fn, total_mass_encoding_scale=scale,
                             enable_bias=bias, learnable_slices=learn, learnable_freqs=learn,
                             learnable_total_mass_encoding_scale=learn and mass, device="cpu", dtype=dt,
                             load_custom_cuda_lib=False)


def set_params(E, V, fr, bias):
    with torch.no_grad():
        E.projVecs.copy_(torch.from_numpy(V).to(E.projVecs.dtype))
        E.freqs.copy_(torch.from_numpy(fr).to(E.freqs.dtype))
        if bias is not None:
            E.bias.copy_(torch.from_numpy(bias).to(E.bias.dtype).reshape(E.bias.shape))


def pointclouds():
    X1 = synth.features(40, D_IN, seed=301).astype(np.float64)
    Xb = synth.features(3 * 40, D_IN, seed=302).astype(np.float64).reshape(3, 40, D_IN)
    Wb = synth.edge_weights(120, seed=303).astype(np.float64).reshape(3, 40)
    Wb[1] *= 0.4 / Wb[1].sum()                    # total mass below tau: the pad element carries weight
    Wb[2, 7] = 0.0
    Wb = Wb.astype(np.float32).astype(np.float64)
    return X1, Xb, Wb


def graph():
    rng = np.random.default_rng(304)
    rows, cols = [], []
    for r, deg in enumerate(GRAPH_DEGREES):
        c = np.sort(rng.choice(GRAPH_SENDERS, size=deg, replace=False))
        rows.append(np.full(deg, r))
        cols.append(c)
    rows = np.concatenate(rows).astype(np.int32)
    cols = np.concatenate(cols).astype(np.int32)
    vals = rng.uniform(0.05, 1.0, size=rows.shape[0]).astype(np.float32).astype(np.float64)
    X = synth.features(GRAPH_SENDERS, D_IN, seed=305).astype(np.float64)
    return X, rows, cols, vals


def dense_w(rows, cols, vals, dt):
    W = torch.zeros((len(GRAPH_DEGREES), GRAPH_SENDERS), dtype=dt)
    W[torch.from_numpy(rows).long(), torch.from_numpy(cols).long()] = torch.from_numpy(vals).to(dt)
    return W


def forward_cases(emb):
    X1, Xb, Wb = pointclouds()
    Xg, gr, gc, gv = graph()
    cases = {}
    # name: (module kwargs, X, W spec, graph_mode, bias shape)
    specs = [
        ("pc_unit", dict(collapse=False), X1, "unit", False, (S, F)),
        ("pc_unit_collapsed", dict(collapse=True), X1, "unit", False, (S * F,)),
        ("pc_batch_unit", dict(collapse=False), Xb, "unit", False, (S, F)),
        ("pc_batch_weighted", dict(collapse=False), Xb, Wb, False, (S, F)),
        ("pc_batch_weighted_collapsed", dict(collapse=True), Xb, Wb, False, (S * F,)),
        ("pc_batch_uniform", dict(collapse=True), Xb, "uniform", False, (S * F,)),
        ("mass_plain", dict(collapse=True, mass=True, method="plain", bias=False, scale=0.7), Xb, Wb, False, None),
        ("mass_homog", dict(collapse=True, mass=True, method="homog", fn="sqrt", bias=False), Xb, Wb, False, None),
        ("mass_homog_alt", dict(collapse=True, mass=True, method="homog_alt", fn="log", bias=False), Xb, Wb, False, None),
        ("graph_weighted", dict(collapse=False), Xg, "graph_w", True, (S, F)),
        ("graph_unit_collapsed", dict(collapse=True), Xg, "graph_unit", True, (S * F,)),
    ]
    for i, (name, kw, X, Wspec, gm, bshape) in enumerate(specs):
        V, fr, bias = params(310 + 7 * i, bshape)
        c = {"X": X, "V": V, "freqs": fr, "collapse": np.array(kw.get("collapse", False)), "graph_mode": np.array(gm),
             "mass": np.array(kw.get("mass", False)), "method": np.array(kw.get("method", "plain")),
             "fn": np.array(kw.get("fn", "identity")), "scale": np.array(kw.get("scale", 1.0))}
        if bias is not None:
            c["bias"] = bias
        if isinstance(Wspec, np.ndarray):
            c["W"] = Wspec
        elif Wspec in ("graph_w", "graph_unit"):
            c["rows"], c["cols"] = gr, gc
            c["vals"] = gv if Wspec == "graph_w" else np.ones_like(gv)
        else:
            c["Wmode"] = np.array(Wspec)
        for dt, tag in ((torch.float64, "out"), (torch.float32, "out_f32")):
            E = make_module(emb, dt, **kw)
            set_params(E, V, fr, bias)
            if "W" in c:
                W = torch.from_numpy(c["W"]).to(dt)
            elif "rows" in c:
                W = dense_w(c["rows"], c["cols"], c["vals"], dt)
            else:
                W = Wspec
            with torch.no_grad():
                c[tag] = E(torch.from_numpy(X).to(dt), W, graph_mode=gm).numpy().astype(np.float64)
        print(name, c["out"].shape, flush=True)
        cases[name] = c
    return cases


def grad_cases(emb):
    X1, Xb, Wb = pointclouds()
    cases = {}
    specs = [
        ("unit_bias", dict(collapse=False), X1, None, (S, F)),
        ("weighted_collapsed_bias", dict(collapse=True), Xb, Wb, (S * F,)),
        ("weighted_mass", dict(collapse=True, mass=True, fn="sqrt", bias=False, scale=0.8), Xb, Wb, None),
        ("weighted_mass_w", dict(collapse=True, mass=True, bias=False, scale=1.3), Xb, Wb, None),
    ]
    for i, (name, kw, X, W, bshape) in enumerate(specs):
        V, fr, bias = params(410 + 7 * i, bshape)
        fr = fr + 0.25                               # gradients away from xi = 0
        E = make_module(emb, torch.float64, learn=True, **kw)
        set_params(E, V, fr, bias)
        Xt = torch.from_numpy(X).requires_grad_(True)
        Wt = torch.from_numpy(W).clone().requires_grad_(name.endswith("_w")) if W is not None else "unit"
        out = E(Xt, Wt)
        G = synth.normal(420 + i, 1, tuple(out.shape), dtype=np.float64)
        (out * torch.from_numpy(G)).sum().backward()
        c = {"X": X, "V": V, "freqs": fr, "G": G, "out": out.detach().numpy(), "gX": Xt.grad.numpy(),
             "gV": E.projVecs.grad.numpy(), "gfreqs": E.freqs.grad.numpy(), "collapse": np.array(kw.get("collapse", False)),
             "mass": np.array(kw.get("mass", False)), "fn": np.array(kw.get("fn", "identity")), "scale": np.array(kw.get("scale", 1.0))}
        if W is not None:
            c["W"] = W
        if bias is not None:
            c["bias"], c["gbias"] = bias, E.bias.grad.numpy()
        if kw.get("mass"):
            c["gscale"] = np.array(E.total_mass_encoding_scale.grad.item())
        if name.endswith("_w"):
            c["gW"] = Wt.grad.numpy()
        print(name, {k: v.shape for k, v in c.items() if k.startswith("g")}, flush=True)
        cases[name] = c
    return cases


def save(name, cases):
    flat = {"%s/%s" % (cn, k): v for cn, c in cases.items() for k, v in c.items()}
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", flush=True)


def main():
    if not ref_harness.available():
        raise SystemExit("the reference implementation is not present: nothing to generate")
    emb, _ = ref_harness.load()
    save("cartesian", forward_cases(emb))
    save("grads_cartesian", grad_cases(emb))


if __name__ == "__main__":
    main()
