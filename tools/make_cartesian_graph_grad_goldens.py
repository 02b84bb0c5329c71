"""Generates tests/golden/grads_cartesian_graph.npz: gradients of Cartesian mode in GRAPH mode on the dense-W graph of
tools/make_cartesian_goldens.py (12 recipients of in-degree 0, 1, 32, 33, 256, 257, 2047, 2048, 2049, 4500, 10, 3 over 5000
senders: every degree class of the Cartesian kernels and their edges), from the float64 autograd of the UNMODIFIED reference run
on CPU through oracle/ref_harness.py (only where the reference exists).

    python tools/make_cartesian_graph_grad_goldens.py

Two cases, S = 6 slices x F = 4 frequencies (shifted by +0.25, away from xi = 0), collapsed output:
  unit_bias       unit values, with bias
  weighted_mass   the stored weights, total mass 'sqrt' with scale 0.8, no bias
Stored as flat float64 arrays '<case>/<name>' like grads_cartesian.npz.  What the two cases share is stored once under
'graph/': the points X and the graph as its nonzero entries (rows, cols, vals; the unit case takes ones for vals), rebuilt densely
by the tests.  The two gX arrays (5000 x 5 float64 each, incompressible) are 370 of the file's 550 KiB.  cartesian.npz and
grads_cartesian.npz are not touched.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fsw_gnn_amd import synth  # noqa: E402
from oracle import ref_harness  # noqa: E402
import make_cartesian_goldens as mcg  # noqa: E402

NAME = "grads_cartesian_graph"


def grad_cases(emb):
    X, rows, cols, vals = mcg.graph()
    cases = {"graph": {"X": X, "rows": rows, "cols": cols, "vals": vals}}
    specs = [
        ("unit_bias", dict(collapse=True), np.ones_like(vals), (mcg.S * mcg.F,)),
        ("weighted_mass", dict(collapse=True, mass=True, fn="sqrt", bias=False, scale=0.8), vals, None),
    ]
    for i, (name, kw, v, bshape) in enumerate(specs):
        V, fr, bias = mcg.params(510 + 7 * i, bshape)
        fr = fr + 0.25                               # gradients away from xi = 0
        E = mcg.make_module(emb, torch.float64, learn=True, **kw)
        mcg.set_params(E, V, fr, bias)
        Xt = torch.from_numpy(X).requires_grad_(True)
        out = E(Xt, mcg.dense_w(rows, cols, v, torch.float64), graph_mode=True)
        G = synth.normal(520 + i, 1, tuple(out.shape), dtype=np.float64)
        (out * torch.from_numpy(G)).sum().backward()
        c = {"V": V, "freqs": fr, "unit": np.array(name.startswith("unit")), "G": G, "out": out.detach().numpy(),
             "gX": Xt.grad.numpy(), "gV": E.projVecs.grad.numpy(), "gfreqs": E.freqs.grad.numpy(),
             "collapse": np.array(True), "mass": np.array(kw.get("mass", False)), "fn": np.array(kw.get("fn", "identity")),
             "scale": np.array(kw.get("scale", 1.0))}
        if bias is not None:
            c["bias"], c["gbias"] = bias, E.bias.grad.numpy()
        if kw.get("mass"):
            c["gscale"] = np.array(E.total_mass_encoding_scale.grad.item())
        print(name, {k: a.shape for k, a in c.items() if k.startswith("g")}, flush=True)
        cases[name] = c
    return cases


def main():
    if not ref_harness.available():
        raise SystemExit("the reference implementation is not present: nothing to generate")
    emb, _ = ref_harness.load()
    mcg.save(NAME, grad_cases(emb))


if __name__ == "__main__":
    main()
