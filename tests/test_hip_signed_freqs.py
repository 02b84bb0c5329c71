"""Frequencies of either sign: every kernel class against the oracle, checked per row, per frequency column and per entry.

The reference accepts any finite frequency (freqs_init = -2.0, (a, b) with a < 0, spread_freqs_at_interval(c, r) with c - r < 0), and
the readout F(xi; c) = (1 + xi) sin(2 pi xi c) / (pi xi) is defined for xi < 0.  The contract (DESIGN.md "frequencies"): any finite
xi; xi = 0 and -0.0 take the linear branch; xi = -1 gives the bias only, because every coefficient carries the factor (1 + xi).  The
yardstick is the float64 oracle, pinned to the reference at signed frequencies by tests/test_oracle_vs_golden.py::
test_signed_frequencies; tests/golden/signed_freqs.npz is also the one comparison with the reference itself made here (module level).

Inputs: the harness of tests/test_hip_ties.py (one recipient at both ends of every degree class, three weight modes) with distinct
keys in every column (ties are not the subject) and the frequencies SIGNED.  The +0.37 / +2.5 columns are the controls: the same
kernels at frequencies the rest of the suite bounds.  Bounds: TOL, F32_BOUND, PER_ENTRY and G64_ROW of tests/test_hip_ties.py,
unchanged.  A mirrored frequency runs the arithmetic of its positive twin with every coefficient scaled by (1 - |xi|) / (1 + |xi|), so
its relative error is expected to be the twin's.  On top of the per-row checks of the ties tests, every frequency column is compared
on its own over all rows (one wrong column cannot hide in a row norm), and the columns at xi = -1 are asserted to be exactly
out_scale * bias (output) and exactly zero (key gradients); they are left out of the relative checks (their line maximum is 0).
In Cartesian mode a key gradient is a sum over the frequencies and has no column of its own at xi = -1.

Measured on an MI355X, largest figure over the three weight modes, columns at xi <= 0 | columns at +0.37 and +2.5:
    fsw_embed_f32                        per row 2.1e-6; per column 2.9e-6 (xi = -13, general weights) | 1.5e-7; -0.37: 1.1e-7 next to +0.37: 8.2e-8,
                                         -2.5: 1.1e-7 next to +2.5: 1.4e-7 (general weights); unit weights 7.0e-7 | 1.5e-7
    fsw_embed_backward_f32 / _keys_f32   gkey per column 6.5e-7 (xi = -13) | 5.1e-8; per entry / line maximum, unit weights 1.5e-7 | 1.3e-7, general
                                         weights 2.6e-6 | 4.7e-7; per row 2.0e-6; gfreq 1.7e-7; stored == atomics in every entry
    fsw_embed_cart_f32                   per row 1.8e-6; per (slice, frequency) column 2.8e-6 | 1.6e-7
    fsw_embed_cart_backward_keys_f32     gkey per slice column 5.7e-7; per entry unit weights 8.5e-7, general weights 2.3e-6; gfreq 3.9e-7
    fsw_embed_generic, float64 storage   forward per row 5.9e-15, per column 1.5e-11 (xi = -13) | 7.5e-13; gkey per column 2.4e-13 | 3.6e-14, per row
                                         5.9e-12, per entry 2.9e-11 | 3.1e-12;  float32 storage: forward per column 4.3e-8 | 3.7e-8, per entry 1.0e-7 | 1.2e-7
    Cartesian hub classes, S 3 x F 5     unit rows: forward per row 2.0e-7, gkey per entry 1.3e-7, gfreq 1.3e-7; weighted lines: forward per row 2.7e-7
                                         (mass > 1), 1.7e-6 (mass 0.4), 1.5e-7 (tau 3), gkey per entry 1.2e-7 / 1.9e-6 / 1.5e-7, gfreq <= 4.7e-7
                                         forward per column (printed only), largest at |xi| = 13, -13 | the same run at +13: unit rows 2.9e-6 | 4.2e-6,
                                         weighted mass > 1: 9.9e-6 | 1.2e-5, mass 0.4: 3.1e-5 | 2.7e-5, tau 3: 5.2e-6 | 6.1e-6
    modules                              FSW_embedding (-3 .. 3 and -3 .. 1): out per row 3.6e-7, per column 2.2e-6, gX 1.4e-7, gV 5.9e-7 (per slice 1.6e-6),
                                         gfreqs 1.1e-7; Cartesian: out per column 1.6e-6, gV per slice 2.6e-6; FSW_conv: out 1.2e-7 (fused, rows of 40 /
                                         300 / 2500 <= 1.2e-7), gfreqs 3.0e-7, gV 6.5e-7; fixture: float32 out <= 4.5e-7, gradients <= 4.0e-7
                                         (gW 2.2e-7), float64 out <= 5.3e-15, gradients <= 1.6e-14
The negative columns sit where their twins sit; the largest figures belong to xi = -13, which has no positive twin here (13.0 in
tests/test_hip_ties.py: 2.1e-6 per entry with general weights), and to the rows of total mass 0.4 (the float32 rounding of the pad
element's weight, see there).  With the kernels of the commit before the fix every diagonal, Cartesian and module test here fails, e.g.
fsw_embed_f32 with general weights per column -0.37: 0.95, -1e-3: 1.0e-3, -13: 3.1, -2.5: 1.6 while +0.37: 8.2e-8, -0.0: 1.5e-7,
+2.5: 1.4e-7, and the generic-kernel tests pass.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests.conftest import golden, relerr
from tests import test_hip_cart_hub as hub
from tests import test_hip_cart_hub_w as hub_w
from tests.test_hip_ties import (CONTROL, DEGREES, F32_BOUND, G64_ROW, HAS_MASS, MODES, MODULE_DEGREES, OUT_SCALE, PER_ENTRY, TOL,
                                 cartesian_reference, check_forward, check_key_gradients, dev, diagonal_reference, hip_projection, per_row,
                                 run_cartesian_kernels, run_generic_kernel, run_tuned_kernels, t, tied_case)

pytestmark = pytest.mark.gpu

SIGNED = (-0.37, 0.37, -1.0, -1e-3, -13.0, -0.0, 2.5, -2.5)
KINDS = (CONTROL,) * 8                  # every key column distinct inside every row
NAMES = tuple(CONTROL if (xi > 0) else "neg" for xi in SIGNED)      # the report of check_key_gradients: "tied" = xi <= 0, "control" = xi > 0


def columns_report(got, ref, cols, what):
    """relerr of every column `cols` over all rows; -> the largest over the negative-or-zero and over the positive frequencies."""
    errs = {c: relerr(got[:, c], ref[:, c]) for c in cols}
    neg = max([e for c, e in errs.items() if not SIGNED[c % len(SIGNED)] > 0] or [0.0])
    pos = max([e for c, e in errs.items() if SIGNED[c % len(SIGNED)] > 0] or [0.0])
    print("%s: per column max, xi <= 0: %.2e | xi > 0: %.2e   " % (what, neg, pos) + "  ".join("%d: %.1e" % ce for ce in errs.items()))
    return errs


def check_diagonal(out, gkeys, gfreqs, ref, rowptr, S, what, fwd_bound=TOL, row_bound=F32_BOUND, entry_bound=PER_ENTRY, floor=1e-6,
                   fwd_rows=True):
    """The assertions of the ties tests on the columns with xi != -1, the per-column comparison, and the exact zeros at xi = -1.
    gkeys: {name: gkey [nnz, S]}; gfreqs: {name: gfreq [S]}."""
    keep = [c for c in range(S) if SIGNED[c] != -1.0]
    dead = [c for c in range(S) if SIGNED[c] == -1.0]
    names = [NAMES[c] for c in keep]
    col_errs = columns_report(out[:, HAS_MASS:], ref["out"][:, HAS_MASS:], keep, what + " forward")     # printed before anything is asserted
    if fwd_rows:
        check_forward(out, ref["out"], what)
    else:                                                           # float64 storage: per row at fwd_bound
        errs = np.array([relerr(out[r], ref["out"][r]) for r in range(len(DEGREES))])
        print("%s: forward per row max %.2e" % (what, errs.max()))
        assert np.isfinite(out).all() and errs.max() <= fwd_bound, (what, errs)
    assert np.abs(out[:, [HAS_MASS + c for c in dead]]).max() == 0.0, what           # out_scale * bias, no bias here
    assert relerr(out[:, 0], ref["out"][:, 0]) <= fwd_bound
    assert max(col_errs.values()) <= fwd_bound, (what, col_errs)
    for name, gk in gkeys.items():
        errs = columns_report(gk, ref["gkey"], keep, "%s %s gkey" % (what, name))
        assert np.isfinite(gk).all() and np.abs(gk[:, dead]).max() == 0.0, (what, name)
        check_key_gradients(gk[:, keep], ref["gkey"][:, keep], rowptr, names, "%s %s" % (what, name), ref["scale"][:, keep],
                            row_bound=row_bound, entry_bound=entry_bound, floor=floor)
        assert max(errs.values()) <= row_bound, (what, name, errs)
    for name, gf in gfreqs.items():
        e = relerr(gf, ref["gfreq"])
        print("%s %s: gfreq %.2e; per frequency |got - ref| / |ref|: %s" % (
            what, name, e, "  ".join("%g: %.1e" % (xi, abs(a - b) / abs(b)) for xi, a, b in zip(SIGNED, gf, ref["gfreq"]))))
        assert np.isfinite(gf).all() and e <= row_bound, (what, name, e)
        assert ref["gfreq"][dead].all() and gf[dead].all()          # d/dxi at xi = -1 is not zero


# ---- 2. kernel level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 6])
@pytest.mark.parametrize("weights,tau", MODES)
def test_tuned_kernels_at_signed_frequencies(dev, weights, tau, S):
    """fsw_embed_f32, fsw_embed_backward_f32 (atomics) and fsw_embed_backward_keys_f32 (stored) on the graph of DEGREES at SIGNED[:S]:
    S = 8 the quad / 16-byte forms, S = 6 the 4-byte forms.  The assertions of test_tuned_kernels_on_tied_keys, every column over all
    rows (forward <= TOL, gkey <= F32_BOUND), exact zeros at xi = -1."""
    ref = diagonal_reference(weights, tau, S, SIGNED, KINDS)
    rowptr = tied_case(weights, KINDS)["rowptr"]
    what = "signed %s tau %g S %d" % (weights, tau, S)
    out, atomic, keys, gfreq = run_tuned_kernels(dev, weights, tau, S, SIGNED, KINDS)
    check_diagonal(out, {"atomics": atomic, "stored": keys}, gfreq, ref, rowptr, S, what)
    keep = [c for c in range(S) if SIGNED[c] != -1.0]
    check_key_gradients(keys[:, keep], atomic[:, keep], rowptr, [NAMES[c] for c in keep], what + " stored vs atomics", ref["scale"][:, keep])


@pytest.mark.parametrize("storage", ["float64", "float32"])
@pytest.mark.parametrize("weights,tau", MODES)
def test_generic_kernel_at_signed_frequencies(dev, weights, tau, storage):
    """fsw_embed_generic, forward and backward, at SIGNED: float64 storage per row, per column and per entry <= G64_ROW (the yardstick
    of the Cartesian and weight-gradient tests, pinned here at negative frequencies; the per-entry floor of
    test_generic_kernel_on_tied_keys), float32 storage at the bounds of the tuned kernels.  The generic kernel never branched on the
    sign of a frequency."""
    S = 8
    ref = diagonal_reference(weights, tau, S, SIGNED, KINDS)
    rowptr = tied_case(weights, KINDS)["rowptr"]
    out, gkey, gf = run_generic_kernel(dev, weights, tau, storage, SIGNED, KINDS)
    what = "signed generic %s %s tau %g" % (storage, weights, tau)
    if storage == "float64":
        check_diagonal(out, {"": gkey}, {"": gf}, ref, rowptr, S, what, fwd_bound=G64_ROW, row_bound=G64_ROW, entry_bound=G64_ROW, floor=2e-4,
                       fwd_rows=False)
    else:
        check_diagonal(out, {"": gkey}, {"": gf}, ref, rowptr, S, what)


@pytest.mark.parametrize("F", [5, 8])
@pytest.mark.parametrize("weights,tau", MODES)
def test_cartesian_kernels_at_signed_frequencies(dev, weights, tau, F):
    """fsw_embed_cart_f32 and fsw_embed_cart_backward_keys_f32, S = 4 slices x F frequencies SIGNED[:F] (F = 8: the F % 4 == 0 vector
    forms), distinct keys; the rows above 2048 neighbours run the generic kernel (unit weights: the hub kernels) inside these entries.
    The assertions of test_cartesian_kernels_on_tied_keys, every (slice, frequency) column over all rows <= TOL and every gkey
    column <= F32_BOUND, the columns at xi = -1 exactly zero."""
    S, cols = 4, (0, 1, 2, 3)
    ref = cartesian_reference(weights, tau, cols, F, SIGNED, KINDS)
    rowptr = tied_case(weights, KINDS)["rowptr"]
    what = "signed cartesian %s tau %g F %d" % (weights, tau, F)
    out, gkey, gf = run_cartesian_kernels(dev, weights, tau, cols, F, SIGNED, KINDS)
    live = [s * F + f for s in range(S) for f in range(F) if SIGNED[f] != -1.0]
    dead = [s * F + f for s in range(S) for f in range(F) if SIGNED[f] == -1.0]
    errs = {c: relerr(out[:, HAS_MASS + c], ref["out"][:, HAS_MASS + c]) for c in live}
    neg = max(e for c, e in errs.items() if not SIGNED[c % F] > 0)
    pos = max(e for c, e in errs.items() if SIGNED[c % F] > 0)
    print("%s forward: per (slice, frequency) column max, xi <= 0: %.2e | xi > 0: %.2e" % (what, neg, pos))     # before anything is asserted
    check_forward(out, ref["out"], what)
    assert np.abs(out[:, [HAS_MASS + c for c in dead]]).max() == 0.0, what
    assert max(errs.values()) <= TOL, (what, errs)
    check_key_gradients(gkey, ref["gkey"], rowptr, ["mixed"] * S, what, ref["scale"])
    errs = [relerr(gkey[:, s], ref["gkey"][:, s]) for s in range(S)]
    print("%s gkey per slice column: %s" % (what, "  ".join("%.1e" % e for e in errs)))
    assert max(errs) <= F32_BOUND, (what, errs)
    e = relerr(gf, ref["gfreq"])
    print("%s: gfreq %.2e; per frequency |got - ref| / |ref|: %s" % (
        what, e, "  ".join("%g: %.1e" % (xi, abs(a - b) / abs(b)) for xi, a, b in zip(SIGNED, gf, ref["gfreq"]))))
    assert np.isfinite(gf).all() and e <= F32_BOUND, (what, e)


def check_hub_forward(out, ref, bias, F, degrees, what):
    """check_rows of tests/test_hip_cart_hub.py (the drivers' own assertion); the columns at xi = -1 equal out_scale * bias exactly.
    Every other column over all rows is printed, not asserted: on these rows a column at |xi| = 13 is a sum that cancels to a small
    fraction of its terms, and the rows of total mass 0.4 carry the float32 rounding of the pad element's weight (see
    tests/test_hip_ties.py) -- the figures of -13 and of +13 are next to each other in this file's docstring."""
    hub.check_rows(out, ref, degrees, what)
    dead = [HAS_MASS + s * F + f for s in range((out.shape[1] - HAS_MASS) // F) for f in range(F) if SIGNED[f] == -1.0]
    want = (np.float32(OUT_SCALE) * bias[dead]).astype(np.float64)
    assert np.array_equal(out[:, dead], np.broadcast_to(want, (out.shape[0], len(dead)))), what       # out_scale * bias, exactly
    errs = {c: relerr(out[:, c], ref[:, c]) for c in range(HAS_MASS, out.shape[1]) if c not in dead}
    print("%s: per (slice, frequency) column max %.2e (column %d)" % (what, max(errs.values()), max(errs, key=errs.get)))


def test_cartesian_unit_hub_kernels_at_signed_frequencies():
    """k_cart_hub / k_cart_bwd_long (unit rows of 2049 .. 32768 neighbours, all four workgroup sizes): the drivers of
    tests/test_hip_cart_hub.py at their smallest shape with the frequencies SIGNED[:F], under their own assertions; the columns at
    xi = -1 equal out_scale * bias exactly."""
    S, F = hub.SHAPES[0]
    from fsw_gnn_amd import _lib
    c = hub.graph_case(False)
    rc, out = hub.run_forward(c, S, F, None, SIGNED)
    assert rc == 0, _lib.lib().fsw_last_error().decode()
    ref = hub.forward_reference(S, F, SIGNED)[:len(hub.DEGREES)]
    check_hub_forward(out, ref, hub.inputs(S, F, SIGNED)["bias"], F, hub.DEGREES, "signed hub forward S %d F %d" % (S, F))
    hub.check_backward(S, F, SIGNED)


@pytest.mark.parametrize("mode", list(hub_w.MODES))
def test_cartesian_weighted_hub_kernels_at_signed_frequencies(mode):
    """k_cart_hub_w / k_cart_bwd_long_w (weighted lines of 2049 .. 16384 elements, all three workgroup sizes): the drivers of
    tests/test_hip_cart_hub_w.py at their smallest shape with the frequencies SIGNED[:F], under their own assertions."""
    S, F = hub.SHAPES[0]
    from fsw_gnn_amd import _lib
    c = hub_w.graph_case(mode, False)
    rc, out = hub_w.run_forward(c, S, F, None, SIGNED)
    assert rc == 0, _lib.lib().fsw_last_error().decode()
    ref = hub_w.forward_reference(mode, S, F, SIGNED)[:len(hub_w.DEGREES)]
    check_hub_forward(out, ref, hub_w.inputs(S, F, SIGNED)["bias"], F, hub_w.DEGREES, "signed weighted hub forward %s S %d F %d" % (mode, S, F))
    hub_w.check_backward(mode, S, F, SIGNED)


# ---- 3. module level ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def module_graph(weighted):
    """Readout-shaped graph of MODULE_DEGREES, one sender per entry, distinct random features; weighted: weights from {0.25, 0.5, 1}
    and the row of 20 scaled to total mass 0.4."""
    rng = np.random.default_rng(61)
    n, d = sum(MODULE_DEGREES), 5
    X = rng.standard_normal((n, d)).astype(np.float32)
    rec = np.repeat(np.arange(len(MODULE_DEGREES)), MODULE_DEGREES).astype(np.int64)
    w = None
    if weighted:
        w = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), size=n)
        w[rec == 0] *= np.float32(0.4) / w[rec == 0].sum(dtype=np.float32)
    return X, rec, w, np.concatenate([[0], np.cumsum(MODULE_DEGREES)])


def check_module(got, ref, rowptr, what, out_dead=()):
    """got / ref: out [rows, q], gX [n, d], gV [S, d], gfreqs.  out per row and per column <= TOL (the columns out_dead are exactly
    zero), gX per recipient row and as a whole, gV as a whole and per slice, gfreqs <= F32_BOUND."""
    for k in got:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (what, k)
    q = ref["out"].shape[1]
    live = [c for c in range(q) if c not in out_dead]
    rows = np.array([relerr(got["out"][r], ref["out"][r]) for r in range(ref["out"].shape[0])])
    colerr = np.array([relerr(got["out"][:, c], ref["out"][:, c]) for c in live])
    gx_rows = per_row(lambda a, b: relerr(got["gX"][a:b], ref["gX"][a:b]), rowptr)
    gv_rows = np.array([relerr(got["gV"][k], ref["gV"][k]) for k in range(ref["gV"].shape[0]) if np.abs(ref["gV"][k]).max() > 0])
    errs = {k: relerr(got[k], ref[k]) for k in ("gX", "gV", "gfreqs")}
    print("%s: out per row %.2e, per column %.2e; gX per row %.2e; gV per slice %.2e; %s" % (
        what, rows.max(), colerr.max(), gx_rows.max(), gv_rows.max(), "  ".join("%s %.2e" % ke for ke in errs.items())))
    if len(out_dead):
        assert np.abs(got["out"][:, list(out_dead)]).max() == 0.0, what
    assert rows.max() <= TOL and colerr.max() <= TOL, (what, rows, colerr)
    assert gx_rows.max() <= F32_BOUND and gv_rows.max() <= F32_BOUND and max(errs.values()) <= F32_BOUND, (what, gx_rows, gv_rows, errs)


def sparse_weights(rec, w, shape, dev, dtype=torch.float32, requires_grad=False):
    idx = torch.from_numpy(np.stack([rec, np.arange(rec.size)])).to(dev)
    vals = t(np.ones(rec.size) if w is None else w, dev, dtype).requires_grad_(requires_grad)
    return torch.sparse_coo_tensor(idx, vals, shape, is_coalesced=True), vals


@pytest.mark.parametrize("weighted", [False, True])
def test_embedding_module_with_negative_frequencies(dev, weighted):
    """FSW_embedding(d_in=5, d_out=12, freqs_init=(-3, 3)) through forward(X, W, graph_mode=True) on rows of 20 / 130 / 700 / 3000
    neighbours with general weights (a row of total mass 0.4), and through embed_autograd on the same graph without a weight array (the
    unit-weight kernels; forward() in graph mode always carries a weight array); then again after spread_freqs_at_interval(-1, 2)
    (frequencies in [-3, 1]).  out, gX, gV and gfreqs against the oracle at the module's own float32 frequencies, ranked by the HIP
    projection."""
    from fsw_gnn_amd import FSW_embedding, build_csr
    X, rec, w, rowptr = module_graph(weighted)
    n, nrows = X.shape[0], len(MODULE_DEGREES)
    torch.manual_seed(62)
    E = FSW_embedding(d_in=5, d_out=12, freqs_init=(-3.0, 3.0), learnable_slices=True, learnable_freqs=True, device=dev)
    assert int((E.freqs < 0).sum()) == 6 and float(E.freqs.min()) == -3.0 and float(E.freqs.max()) == 3.0
    R = np.random.default_rng(63).standard_normal((nrows, 12))
    wv = np.ones(n) if w is None else w.astype(np.float64)
    for step in ("freqs_init=(-3, 3)", "spread_freqs_at_interval(-1, 2)"):
        if step.startswith("spread"):
            E.spread_freqs_at_interval(-1.0, 2.0)
            assert abs(float(E.freqs.min()) + 3.0) < 1e-6 and abs(float(E.freqs.max()) - 1.0) < 1e-6 and int((E.freqs < 0).sum()) == 9
        E.zero_grad(set_to_none=True)
        Xd = t(X, dev).requires_grad_(True)
        if weighted:
            W, _ = sparse_weights(rec, w, (nrows, n), dev)
            out = E(Xd, W, graph_mode=True)
        else:                                                       # no weight array at all: the unit-weight kernels
            graph = build_csr(t(rec, dev, torch.int64), torch.arange(n, device=dev), None, nrows, n)
            out = E.embed_autograd(Xd, graph)
        (out * t(R, dev)).sum().backward()
        V, fr = E.projVecs.detach().cpu().numpy().astype(np.float64), E.freqs.detach().cpu().numpy().astype(np.float64)
        xp = hip_projection(E, Xd, X.shape[1])
        ref_out = O.fsw_embed_csr(X, rowptr, np.arange(n), wv, V, fr)
        gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, np.arange(n), wv, V, fr, R, Xp_override=xp)
        got = {"out": out.detach().cpu().numpy().astype(np.float64), "gX": Xd.grad.cpu().numpy().astype(np.float64),
               "gV": E.projVecs.grad.cpu().numpy().astype(np.float64), "gfreqs": E.freqs.grad.cpu().numpy().astype(np.float64)}
        check_module(got, {"out": ref_out, "gX": gX, "gV": gV, "gfreqs": gxi}, rowptr,
                     "module %s, %s" % ("weighted" if weighted else "unit", step))


@pytest.mark.parametrize("weighted", [False, True])
def test_cartesian_module_with_negative_frequencies(dev, weighted):
    """FSW_embedding(d_in=5, nSlices=4, nFreqs=6, freqs_init=(-3, 3)) on the same graph through embed_cartesian_autograd (the tuned
    float32 kernels), against the oracle through the diagonal identity of tests/test_cartesian_cpu.py: slice s repeated F times, the
    frequencies tiled; gV[s] and gfreqs[f] are the sums over the other index."""
    from fsw_gnn_amd import FSW_embedding, build_csr
    X, rec, w, rowptr = module_graph(weighted)
    n, nrows, S, F = X.shape[0], len(MODULE_DEGREES), 4, 6
    torch.manual_seed(64)
    E = FSW_embedding(d_in=5, nSlices=S, nFreqs=F, freqs_init=(-3.0, 3.0), learnable_slices=True, learnable_freqs=True, device=dev)
    assert int((E.freqs < 0).sum()) == 3 and float(E.freqs.min()) == -3.0
    R = np.random.default_rng(65).standard_normal((nrows, S * F))
    wv = np.ones(n) if w is None else w.astype(np.float64)
    Xd = t(X, dev).requires_grad_(True)
    graph = build_csr(t(rec, dev, torch.int64), torch.arange(n, device=dev), None if w is None else t(w, dev), nrows, n)
    out = E.embed_cartesian_autograd(Xd, graph)
    (out * t(R, dev)).sum().backward()
    V, fr = E.projVecs.detach().cpu().numpy().astype(np.float64), E.freqs.detach().cpu().numpy().astype(np.float64)
    xp = np.repeat(hip_projection(E, Xd, X.shape[1]), F, axis=1)
    Vd, frd = np.repeat(V, F, axis=0), np.tile(fr, S)
    ref_out = O.fsw_embed_csr(X, rowptr, np.arange(n), wv, Vd, frd)
    gX, gV, gxi = O.fsw_embed_csr_backward(X, rowptr, np.arange(n), wv, Vd, frd, R, Xp_override=xp)
    got = {"out": out.detach().cpu().numpy().astype(np.float64).reshape(nrows, S * F), "gX": Xd.grad.cpu().numpy().astype(np.float64),
           "gV": E.projVecs.grad.cpu().numpy().astype(np.float64), "gfreqs": E.freqs.grad.cpu().numpy().astype(np.float64)}
    ref = {"out": ref_out, "gX": gX, "gV": gV.reshape(S, F, -1).sum(axis=1), "gfreqs": gxi.reshape(S, F).sum(axis=0)}
    check_module(got, ref, rowptr, "cartesian module %s" % ("weighted" if weighted else "unit"))


@functools.lru_cache(maxsize=None)
def conv_graph():
    """3000 nodes, in-degrees 0 .. 32 (mostly), three rows of 40, 300 and 2500 neighbours; no parallel edges, no self loops."""
    rng = np.random.default_rng(66)
    n = 3000
    deg = rng.integers(0, 33, size=n)
    deg[[7, 1500, 2999]] = (40, 300, 2500)
    src = np.concatenate([rng.choice(n - 1, size=k, replace=False) for k in deg])
    dst = np.repeat(np.arange(n), deg)
    src += src >= dst                                               # no self loops of its own
    order = rng.permutation(src.size)
    return n, np.stack([src[order], dst[order]]).astype(np.int64)


@pytest.mark.parametrize("kw", [{}, {"edge_weighting": "gcn", "self_loop_weight": 1.0}], ids=["unit", "gcn_selfloops"])
def test_conv_layer_with_alternating_frequency_signs(dev, kw):
    """FSW_conv (default fused first layer, learnable_embedding=True) with frequencies +-13 (k + 1) / 16 of alternating sign, on a graph
    whose rows are mostly <= 32 neighbours plus rows of 40, 300 and 2500: under no_grad the fused kernel and fsw_embed_f32 on the long
    rows, under autograd the unfused forward and the backward kernels.  unit weights, and 'gcn' + self loops (general weights: the
    unfused general-weight kernels in both passes).
    Output <= TOL against O.fsw_embedding_forward + O.conv_tail; gradients of X, projVecs, freqs and the Linear layer <= 2e-5 against
    O.fsw_embed_csr_backward on the HIP projection, as in test_backward_conv10k_training_step."""
    from fsw_gnn_amd import FSW_conv
    from tests.test_hip_parity import _hip_projection
    n, ei = conv_graph()
    d, out_ch, E_ = 6, 8, 17
    torch.manual_seed(67)
    conv = FSW_conv(d, out_ch, embed_dim=E_, device=dev, **kw)
    S = E_ - 1
    fr = (13.0 * (np.arange(S) + 1) / S * np.where(np.arange(S) % 2 == 1, -1.0, 1.0)).astype(np.float32)
    with torch.no_grad():
        conv.fsw_embed.freqs.copy_(t(fr, dev))
    assert conv._fusable() == (not kw) and conv.fsw_embed.freqs.requires_grad and (fr < 0).sum() == S // 2
    rng = np.random.default_rng(68)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Rc = rng.standard_normal((n, out_ch))
    Xd, eid = t(X, dev).requires_grad_(True), t(ei, dev, torch.int64)
    with torch.no_grad():
        y_fused = conv(Xd.detach(), eid)
    y = conv(Xd, eid)
    (y * t(Rc, dev)).sum().backward()
    V = conv.fsw_embed.projVecs.detach().cpu().numpy().astype(np.float64)
    Wl, bl = conv.mlp[0].weight.detach().cpu().numpy().astype(np.float64), conv.mlp[0].bias.detach().cpu().numpy().astype(np.float64)
    rowptr, col, w, _ = O.coalesce_edge_index(ei, n, **kw)
    assert w.shape[0] == ei.shape[1] + (n if kw else 0) and np.diff(rowptr).max() >= 2500
    X64 = X.astype(np.float64)
    emb = O.fsw_embedding_forward(X64, rowptr, col, w, V, fr.astype(np.float64), encode_total_mass=True)
    ref = O.conv_tail(emb, X64, linear_weight=Wl, linear_bias=bl)
    e_fused, e_train = relerr(y_fused.cpu().numpy(), ref), relerr(y.detach().cpu().numpy(), ref)
    rows = np.array([relerr(y_fused.cpu().numpy()[r], ref[r]) for r in (7, 1500, 2999)])
    h = np.concatenate([emb, X64], axis=1)
    pre = h @ Wl.T + bl
    gpre = Rc * np.where(pre >= 0, 1.0, 0.2)
    gh = gpre @ Wl
    gX_o, gV_o, gxi_o = O.fsw_embed_csr_backward(X64, rowptr, col, w, V, fr.astype(np.float64), gh[:, 1:E_], Xp_override=_hip_projection(conv.fsw_embed, Xd))
    errs = {"gX": relerr(Xd.grad.cpu().numpy(), gX_o + gh[:, E_:]), "gV": relerr(conv.fsw_embed.projVecs.grad.cpu().numpy(), gV_o),
            "gfreqs": relerr(conv.fsw_embed.freqs.grad.cpu().numpy(), gxi_o),
            "gW": relerr(conv.mlp[0].weight.grad.cpu().numpy(), gpre.T @ h), "gb": relerr(conv.mlp[0].bias.grad.cpu().numpy(), gpre.sum(axis=0))}
    gf = conv.fsw_embed.freqs.grad.cpu().numpy()
    print("conv %s: out fused %.2e (rows of 40 / 300 / 2500: %s), training forward %.2e; %s; gfreqs per frequency: %s" % (
        kw or "unit", e_fused, "  ".join("%.1e" % e for e in rows), e_train, "  ".join("%s %.2e" % ke for ke in errs.items()),
        "  ".join("%.1e" % (abs(a - b) / abs(b)) for a, b in zip(gf, gxi_o))))
    assert e_fused <= TOL and e_train <= TOL and rows.max() <= TOL
    assert max(errs.values()) <= 2e-5, errs


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_modules_on_the_signed_frequency_fixture(dev, dtype):
    """tests/golden/signed_freqs.npz (the reference's float64 autograd at frequencies -13 .. 13 with -1, -0.0 and +-1e-3 among them,
    rows of 1 .. 50 neighbours, unit / general weights with a row of total mass 0.4 / the same at tau = 3): the float32 and float64
    modules with the weights requiring grad (the generic kernel: out, gX, gV, gfreqs, gW) and the float32 module without (the tuned
    kernels: out, gX, gV, gfreqs), at the bounds of test_weight_gradients_vs_reference_autograd: forward 1e-5 / 1e-12, gradients
    2e-5 / 1e-10.  The column at xi = -1 is exactly zero.  The unit-weight case holds a row of one neighbour, whose mass equals the
    pad threshold: no row is deficient, the reference pads nothing, and that entry's gW is 0 (_GenericEmbedFn.key_grads).  A
    unit-weight row of one neighbour under weights that require grad occurs in no other test."""
    from fsw_gnn_amd import FSW_embedding
    from tests.test_hip_float64 import F64, G64
    g = golden("signed_freqs")
    degs, snd, fr = g["degrees"], g["senders"], g["freqs"]
    rec = np.repeat(np.arange(degs.size), degs)
    idx = torch.from_numpy(np.stack([rec, snd])).to(dev)
    fwd, tol = (F64, G64) if dtype == torch.float64 else (1e-5, 2e-5)
    dead = int(np.nonzero(fr == -1.0)[0][0])
    for tag, wv, tau in (("unit", np.ones(rec.size), 1.0), ("general", g["w_general"], 1.0), ("general_tau3", g["w_general"], 3.0)):
        for w_grad in ((True, False) if dtype == torch.float32 else (True,)):
            E = FSW_embedding(d_in=g["X"].shape[1], d_out=fr.size, total_mass_pad_thresh=tau, learnable_slices=True, learnable_freqs=True,
                              enable_bias=False, device=dev, dtype=dtype)
            with torch.no_grad():
                E.projVecs.copy_(t(g["V"], dev, dtype))
                E.freqs.copy_(t(fr, dev, dtype))
            assert np.array_equal(E.freqs.detach().cpu().numpy().astype(np.float64), fr)      # the fixture's frequencies are float32 values
            vals = t(wv, dev, dtype).requires_grad_(w_grad)
            A = torch.sparse_coo_tensor(idx, vals, (degs.size, g["X"].shape[0]), is_coalesced=True)
            X = t(g["X"], dev, dtype).requires_grad_(True)
            out = E(X, A, graph_mode=True)
            (out * t(g["R"], dev, dtype)).sum().backward()
            got_out = out.detach().cpu().numpy().astype(np.float64)
            live = [c for c in range(fr.size) if c != dead]
            errs = {"out": relerr(got_out, g["out_" + tag]), "out per column": max(relerr(got_out[:, c], g["out_" + tag][:, c]) for c in live),
                    "gX": relerr(X.grad.cpu().numpy(), g["gX_" + tag]), "gV": relerr(E.projVecs.grad.cpu().numpy(), g["gV_" + tag]),
                    "gfreqs": relerr(E.freqs.grad.cpu().numpy(), g["gfreqs_" + tag])}
            if w_grad:
                errs["gW"] = relerr(vals.grad.cpu().numpy(), g["gW_" + tag])
            print("fixture %s %s, weights %s grad: %s" % (dtype, tag, "with" if w_grad else "without", "  ".join("%s %.2e" % ke for ke in errs.items())))
            assert np.abs(got_out[:, dead]).max() == 0.0 and np.abs(E.projVecs.grad[dead].cpu().numpy()).max() == 0.0, tag
            assert errs.pop("out") <= fwd and errs.pop("out per column") <= fwd, tag
            assert max(errs.values()) <= tol, (tag, errs)
