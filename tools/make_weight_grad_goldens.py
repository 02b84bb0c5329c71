"""Generates tests/golden/grads_w_long.npz: d loss / d W on long rows, from the float64 autograd of the UNMODIFIED reference run on
CPU through oracle/ref_harness.py (only where the reference exists).

    python tools/make_weight_grad_goldens.py

Graph: one recipient per in-degree of tests/weight_grad_ref.py::FIXTURE_DEGREES (0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4500: both
sides of the generic kernel's 256-element scan chunk and of its LDS line) over 4600 senders with 3 features; float32-representable
weights from {0.25, 0.5, 1} with exact zeros, the rows of 1 / 2 / 257 / 2049 scaled to total mass 0.3 / 0.4 / 2.0 / 0.9 and the row of
256 at 1/256 each (m == 1 exactly).  The 'nopad' weights are the same rows without the empty recipient and with no mass below 1 (the rows
of 1 and of 256 sit on it): the reference pads nothing there.  The 'cart' weights are the first ones with the masses of the rows of
255, 2047, 2048 and 4500 lowered to a power of two (weight_grad_ref.long_row_weights, dyadic_mass): the reference's dense-W path,
the only one it has in Cartesian mode, divides by the mass and then runs one sequential torch.cumsum over all 4600 senders of a row,
which costs it 1e-12 on those rows unless both steps are exact.

Cases (W requires grad in each; the frequencies hold 0, -0.75 and 4.5):
  diag_tau1_sqrt_homog       diagonal S = 8, sparse COO W, tau 1, mass column sqrt / homog, scale 0.7
  diag_tau3_log_homog_alt    the same at tau 3 with log / homog_alt
  nopad_tau1                 the 'nopad' weights, tau 1, no mass column
  cart_tau1, cart_tau3       the 'cart' weights, Cartesian 4 x 3 collapsed, dense W (sparse W asserts inside the reference in
                             Cartesian mode)
Stored per case: G, out, gW at the stored entries (float64) and the parameters; once: X, the columns and the three weight vectors.
The five gW arrays (11415 float64 each, incompressible) are most of the file, which is why the diagonal cases without a mass
column at tau 1 and tau 3 are not stored: the two mass cases run the same kernel launches, and tests/test_weight_grad_ref_cpu.py
pins the restatement to the reference for them directly where the reference is present.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fsw_gnn_amd import synth  # noqa: E402
from oracle import ref_harness  # noqa: E402
from tests import weight_grad_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAME = "grads_w_long"
S_DIAG, S_CART = 8, 4
warnings.filterwarnings("ignore")

# name: (graph, tau, cartesian, mass fn or None, method)
CASES = (
    ("diag_tau1_sqrt_homog", "pad", 1.0, False, "sqrt", "homog"),
    ("diag_tau3_log_homog_alt", "pad", 3.0, False, "log", "homog_alt"),
    ("nopad_tau1", "nopad", 1.0, False, None, "plain"),
    ("cart_tau1", "cart", 1.0, True, None, "plain"),
    ("cart_tau3", "cart", 3.0, True, None, "plain"),
)
MASS_SCALE = 0.7


def graphs():
    n, d = R.FIXTURE_SENDERS, R.FIXTURE_D
    cols = R.long_row_cols(R.FIXTURE_DEGREES, n, seed=601)
    return {"X": synth.features(n, d, seed=602), "cols": cols.astype(np.uint16), "degrees": np.array(R.FIXTURE_DEGREES, dtype=np.int32),
            "w_pad": R.long_row_weights(R.FIXTURE_DEGREES, R.PAD_MASSES, seed=603),
            "w_cart": R.long_row_weights(R.FIXTURE_DEGREES, R.PAD_MASSES, seed=603, dyadic_mass=True),
            "w_nopad": R.long_row_weights(R.FIXTURE_DEGREES[1:], R.NOPAD_MASSES, seed=605)}


def main():
    if not ref_harness.available():
        raise SystemExit("the reference implementation is not present: nothing to generate")
    emb, _ = ref_harness.load()
    g = graphs()
    flat = {"graph/" + k: v for k, v in g.items()}
    for i, (name, which, tau, cartesian, fn, method) in enumerate(CASES):
        S = S_CART if cartesian else S_DIAG
        V = synth.unit_slices(S, R.FIXTURE_D, seed=610 + i).astype(np.float64)
        fr = np.array(R.CART_FREQS if cartesian else R.DIAG_FREQS, dtype=np.float32).astype(np.float64)
        degrees = g["degrees"][1:] if which == "nopad" else g["degrees"]
        out, gW, G = R.reference_run(emb, g["X"], degrees, g["cols"], g["w_" + which], V, fr, tau, cartesian, fn, method, MASS_SCALE,
                                     seed=620 + i)
        c = {"V": V, "freqs": fr, "tau": np.array(tau), "cartesian": np.array(cartesian), "graph": np.array(which),
             "fn": np.array(fn or ""), "method": np.array(method), "scale": np.array(MASS_SCALE), "G": G, "out": out, "gW": gW}
        print(name, out.shape, gW.shape, float(np.abs(gW).max()), flush=True)
        flat.update({"%s/%s" % (name, k): v for k, v in c.items()})
    path = os.path.join(GOLD, NAME + ".npz")
    np.savez_compressed(path, **flat)
    print("wrote", path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
