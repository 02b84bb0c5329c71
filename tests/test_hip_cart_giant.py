"""Cartesian mode on the longest rows: k_cart_giant (unit weights, rows above 32768 neighbours) and k_cart_mergepath_w (general weights,
lines of 16385 elements and more) through fsw_embed_cart_f32 and through the modules.

Graphs with one recipient per degree, senders drawn without replacement, at both sides of every block-count change up to five blocks
(levels with an absent partner block occur): a block is 32768 keys for unit weights and 8192 (key, weight) elements for general
weights, whose lines hold D + 1 elements.  Keys, weight modes and helpers are those of tests/test_hip_cart_hub.py and
tests/test_hip_cart_hub_w.py: 200 sender pairs with bit-identical keys, one constant column, one control column without ties and,
for weights, one column of zeros, which ties with the pad element; random weights with row mass > 1, the same scaled to row mass 0.4,
and w = NULL with tau = 3.  The yardstick is the float64 oracle through the diagonal identity; bounds: the project's TOL per row and
for the mass column (tests/test_hip_ties.py), 1e-5 / 3e-5 at module level.  The backward of these rows is the generic kernel, as before.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests.conftest import relerr
from tests.test_hip_cart_hub import COLUMN_KINDS as UNIT_KINDS
from tests.test_hip_cart_hub import DEV, HAS_MASS, OUT_SCALE, SHAPES, cart_args, check_rows, t, unit_tables
from tests.test_hip_cart_hub_w import COLUMN_KINDS as W_KINDS
from tests.test_hip_cart_hub_w import LOW_MASS, MODES, MODULE_FWD, MODULE_GRAD, weighted_args
from tests.test_hip_signed_freqs import SIGNED
from tests.test_hip_ties import FREQS

pytestmark = pytest.mark.gpu

TIED_PAIRS = 200
# unit weights, blocks of 32768 keys: 1 | 2, 2 | 3 blocks, then 4 and 5; general weights, blocks of 8192 elements of lines of D + 1:
# 2 | 3, 3 | 4 blocks, 5 (32769 elements), 5 and 9
UNIT = {"degrees": (0, 7, 32768, 32769, 65536, 65537, 100000, 140000), "senders": 150000, "kinds": UNIT_KINDS, "seed": 171}
WEIGHTED = {"degrees": (0, 7, 16383, 16384, 24575, 24576, 32768, 40000, 70000), "senders": 75000, "kinds": W_KINDS, "seed": 181}
KINDS = ("unit",) + tuple(MODES)                      # "unit" | "random" | "low_mass" | "tau3"
SUB = {"unit": (7, 32769, 65537), "weighted": (7, 16384, 24576)}     # a short row, the first giant row, a row of three / four blocks
# test_more_frequencies_than_a_batch_and_a_wavefront: 0.0, -0.0, -1.0 and every other value next to its negative twin
TWINS = (0.37, 1.5, 2.5, 4.0, 7.25, 13.0, 0.05, 0.11, 0.2, 0.29, 0.43, 0.5, 0.61, 0.74, 0.88, 1.13, 1.27, 1.9, 2.2, 2.75, 3.1, 3.6, 4.4, 5.0,
         5.5, 6.3, 8.0, 9.1, 10.4, 11.0, 12.2, 1e-3, 0.9)
MANY = (0.0, -0.0, -1.0, 1.0) + tuple(v for x in TWINS for v in (x, -x))
assert len(MANY) == 70 and SHAPES == [(3, 5), (4, 8)]


def family(kind):
    return UNIT if kind == "unit" else WEIGHTED


@functools.lru_cache(maxsize=None)
def graph_case(kind, degrees=None):
    """The graph of `degrees` (default: all of the family's) in weight mode `kind`; a row's senders and weights depend on its degree
    only, so a sub-graph holds the same rows as the full graph."""
    from fsw_gnn_amd import _lib, build_csr
    fam = family(kind)
    degrees = fam["degrees"] if degrees is None else degrees
    rec, snd, w = [], [], []
    for r, deg in enumerate(degrees):
        rng = np.random.default_rng(fam["seed"] + deg)
        rec.append(np.full(deg, r, dtype=np.int64))
        snd.append(rng.choice(fam["senders"], size=deg, replace=False).astype(np.int64))
        w.append(rng.uniform(0.05, 1.0, size=deg).astype(np.float32))
    rec, snd, w = np.concatenate(rec), np.concatenate(snd), np.concatenate(w)
    nnz = rec.size
    if kind == "low_mass":
        mass = np.bincount(rec, weights=w.astype(np.float64), minlength=len(degrees))
        w = (w * (LOW_MASS / mass[rec])).astype(np.float32)
    graph = build_csr(t(rec, torch.int64), t(snd, torch.int64), t(w) if kind in ("random", "low_mass") else None, len(degrees), fam["senders"])
    st = graph.read_stats()
    rowptr = graph.rowptr.cpu().numpy().astype(np.int64)
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_NNZ] == nnz and tuple(np.diff(rowptr)) == tuple(degrees)
    assert st[_lib.STAT_MAX_DEGREE] == max(degrees)
    col = graph.col[:nnz].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(col), np.sort(snd))
    w64 = np.ones(nnz) if graph.w is None else graph.w[:nnz].cpu().numpy().astype(np.float64)
    assert (graph.w is None) == (kind in ("unit", "tau3"))
    return {"graph": graph, "st": st, "rowptr": rowptr, "col": col, "nnz": nnz, "degrees": tuple(degrees), "w64": w64,
            "tau": 1.0 if kind == "unit" else MODES[kind], "kind": kind}


@functools.lru_cache(maxsize=None)
def inputs(weighted, S, F, freqs=FREQS):
    """Xp [senders, round_up(S, 32)] float32 with the column kinds of the hub tests, frequencies freqs[:F], bias."""
    fam = WEIGHTED if weighted else UNIT
    n = fam["senders"]
    rng = np.random.default_rng(fam["seed"] + 1000 + S)
    ldp = (S + 31) // 32 * 32
    Xp = rng.standard_normal((n, ldp)).astype(np.float32)
    pairs = rng.permutation(n)[:2 * TIED_PAIRS].reshape(2, TIED_PAIRS)
    Xp[pairs[1]] = Xp[pairs[0]]                                    # exactly tied keys in every column ...
    kinds = fam["kinds"][:S]
    for c, kind in enumerate(kinds):
        if kind == "a":
            Xp[:, c] = 0.75
        elif kind == "z":                                           # ties with the pad element (key 0)
            Xp[:, c] = 0.0
        elif kind == "e":                                           # ... but the control column: distinct, exact in float32
            Xp[:, c] = (rng.permutation(n).astype(np.float32) - n // 2) / 32768.0
            assert np.unique(Xp[:, c]).size == n
    assert np.array_equal(Xp[pairs[0], 0], Xp[pairs[1], 0])
    fr = np.array(freqs[:F], dtype=np.float32)
    bias = (0.1 * rng.standard_normal(HAS_MASS + S * F)).astype(np.float32)
    for a in (Xp, fr, bias):
        a.setflags(write=False)
    return {"Xp": Xp, "fr": fr, "bias": bias, "kinds": kinds, "ldp": ldp}


@functools.lru_cache(maxsize=None)
def forward_reference(kind, degrees, S, F, freqs=FREQS):
    """The float64 oracle with the graph's weights and tau through the diagonal identity: [rows, HAS_MASS + S F] with bias and out_scale."""
    c, x = graph_case(kind, degrees), inputs(kind != "unit", S, F, freqs)
    X = x["Xp"][:, :S].astype(np.float64)
    V = np.repeat(np.eye(S), F, axis=0)
    emb, mass = O.fsw_embed_csr(X, c["rowptr"], c["col"], c["w64"], V, np.tile(x["fr"].astype(np.float64), S),
                                total_mass_pad_thresh=c["tau"], return_mass=True)
    ref = OUT_SCALE * (np.concatenate([mass[:, None], emb], axis=1) + x["bias"].astype(np.float64)[None, :])
    ref.setflags(write=False)
    return ref


class Call:
    """The arguments of one fsw_embed_cart_f32 call on a graph case (the device tensors stay alive with the object)."""

    def __init__(self, c, S, F, freqs=FREQS):
        self.c, self.S, self.F = c, S, F
        self.x = inputs(c["kind"] != "unit", S, F, freqs)
        self.stream = torch.cuda.current_stream(DEV).cuda_stream
        self.Xp, self.fr, self.bias = t(self.x["Xp"]), t(self.x["fr"]), t(self.x["bias"])
        self.table = unit_tables(self.fr, F, self.stream)[0] if c["kind"] == "unit" else None

    def args(self, scratch=None):
        if self.c["kind"] == "unit":
            a, keep = cart_args(self.c, self.x, self.S, self.F, self.Xp, self.fr, self.table, scratch), None
        else:
            a, keep = weighted_args(self.c, self.x, self.S, self.F, self.Xp, self.fr, scratch)
        return a, keep

    def query(self):
        """fsw_embed_cart_forward_scratch_bytes for this call."""
        from fsw_gnn_amd import _lib
        a, _keep = self.args()
        return int(_lib.lib().fsw_embed_cart_forward_scratch_bytes(ctypes.byref(a)))

    def one_line(self):
        """The new query on a one-row, S = 1 copy of the arguments: the bytes of one scratch line."""
        from fsw_gnn_amd import _lib
        a, _keep = self.args()
        bs = np.zeros(_lib.NUM_BINS + 1, dtype=np.int32)
        bs[_lib.NUM_BINS] = 1                                        # one row, in the last bin
        a.bin_start_host, a.S = bs.ctypes.data, 1
        return int(_lib.lib().fsw_embed_cart_forward_scratch_bytes(ctypes.byref(a)))

    def run(self, nbytes):
        """(status, out) with a scratch buffer of nbytes; out pre-filled with NaN."""
        from fsw_gnn_amd import _lib
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
        out = torch.full((len(self.c["degrees"]), HAS_MASS + self.S * self.F), float("nan"), device=DEV)
        a, _keep = self.args(scratch)
        a.out, a.ldo, a.bias = out.data_ptr(), out.stride(0), self.bias.data_ptr()
        rc = _lib.lib().fsw_embed_cart_f32(ctypes.byref(a), self.stream)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy().astype(np.float64)


def last_error():
    from fsw_gnn_amd import _lib
    return _lib.lib().fsw_last_error().decode()


@pytest.mark.parametrize("S,F", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_forward(kind, S, F):
    """fsw_embed_cart_f32 with the scratch of fsw_embed_cart_forward_scratch_bytes: status 0, every row (mass column included) within
    TOL of the float64 oracle, the NaN-prefilled output finite everywhere."""
    c = graph_case(kind)
    call = Call(c, S, F)
    nbytes = call.query()
    assert nbytes > 0 and nbytes % call.one_line() == 0
    rc, out = call.run(nbytes)
    assert rc == 0, last_error()
    assert np.isfinite(out).all()
    check_rows(out, forward_reference(kind, None, S, F), c["degrees"], "giant forward %s S %d F %d" % (kind, S, F))


@pytest.mark.parametrize("F", (19, 70))
@pytest.mark.parametrize("kind", ("unit", "random"))
def test_more_frequencies_than_a_batch_and_a_wavefront(kind, F):
    """S = 2 and F = 19 / 70 frequencies of MANY (more than one readout batch of 16, more than the 64 lanes of a wavefront) on the
    sub-graph of a short row, the first giant row and a longer one: rows within TOL, the columns at xi = -1 exactly out_scale * bias."""
    S = 2
    degrees = SUB["unit" if kind == "unit" else "weighted"]
    c = graph_case(kind, degrees)
    call = Call(c, S, F, MANY)
    rc, out = call.run(call.query())
    assert rc == 0, last_error()
    what = "giant forward %s S %d F %d" % (kind, S, F)
    check_rows(out, forward_reference(kind, degrees, S, F, MANY), degrees, what)
    dead = [HAS_MASS + s * F + f for s in range(S) for f in range(F) if MANY[f] == -1.0]
    want = (np.float32(OUT_SCALE) * call.x["bias"][dead]).astype(np.float64)
    assert len(dead) == S and np.array_equal(out[:, dead], np.broadcast_to(want, (out.shape[0], len(dead)))), what


@pytest.mark.parametrize("kind", ("unit", "random"))
def test_signed_frequencies(kind):
    """The frequencies SIGNED[:5] of tests/test_hip_signed_freqs.py at (S, F) = (3, 5): per row within TOL."""
    S, F = SHAPES[0]
    c = graph_case(kind)
    call = Call(c, S, F, SIGNED)
    rc, out = call.run(call.query())
    assert rc == 0, last_error()
    check_rows(out, forward_reference(kind, None, S, F, SIGNED), c["degrees"], "giant forward %s at signed frequencies" % kind)


@pytest.mark.parametrize("kind", ("unit", "random"))
def test_one_scratch_line_suffices(kind):
    """fsw_embed_cart_f32 on the full graph with S = 3 and a scratch of exactly ONE line -- smaller than the smallest buffer the generic
    kernel accepted for these rows, so a library without the kernels of the longest rows refuses the call: status 0, rows within TOL."""
    from fsw_gnn_amd import _lib
    S, F = SHAPES[0]
    c = graph_case(kind)
    call = Call(c, S, F)
    line = call.one_line()
    assert 0 < line < int(_lib.lib().fsw_embed_cart_generic_scratch_bytes(max(c["degrees"]), 1)) and line < call.query()
    rc, out = call.run(line)
    assert rc == 0, last_error()
    check_rows(out, forward_reference(kind, None, S, F), c["degrees"], "giant forward %s, one scratch line" % kind)


@pytest.mark.parametrize("kind", ("unit", "random"))
def test_output_does_not_depend_on_the_workgroup_count(kind):
    """Two rows of the longest class and S = 4: with one line of scratch one workgroup takes the eight lines one after the other through
    the same scratch line; the output is bit-identical to the run with the buffer of the query (eight workgroups)."""
    S, F = SHAPES[1]
    degrees = SUB["unit" if kind == "unit" else "weighted"]
    c = graph_case(kind, degrees)
    call = Call(c, S, F)
    line, full = call.one_line(), call.query()
    assert full == 8 * line
    rc1, one = call.run(line)
    assert rc1 == 0, last_error()
    rc8, eight = call.run(full)
    assert rc8 == 0, last_error()
    assert np.isfinite(one).all() and np.array_equal(one, eight)


# ---- module level -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cloud", [(40000, "unit_line"), (40000, "unit_gauss"), (20000, "weighted")])
def test_embedding_module_on_one_long_cloud(n, cloud):
    """FSW_embedding(d_in=3, nSlices=4, nFreqs=8) on one cloud of 40 000 points with W = 'unit' / of 20 000 points with random positive
    weights: the float32 module (forward on the kernels of the longest rows, backward on the generic kernel out of a buffer of its own
    size) against the float64 module with the same state: output <= 1e-5, gradients of X, projVecs and freqs <= 3e-5.

    The unit cloud lies on a line through the origin, 40 000 distinct positions 2e-4 apart in shuffled order, along the candidate
    direction that no slice is orthogonal to: its keys in every slice are separated by 5e-5 of the largest key, a few hundred times the
    float32 rounding of projVecs and of the projection, so both modules sort the same order and the key gradient -- piecewise
    constant in the order -- is compared where it exists.  On 40 000 Gaussian points that is not so: about a hundred pairs of keys
    per cloud lie within float32 rounding of each other, the two modules rank them differently, and gX differs by 1.43e-4 (gV
    1.41e-5, gfreqs 1.40e-6, output 1.6e-6) -- measured with these kernels and, to every digit, with the generic forward they
    replace: the backward is the same generic kernel on the same float32 keys.  The Gaussian unit cloud ("unit_gauss") runs too, so
    that 40 000 keys in general position pass through k_cart_giant and the scratch hand-over at module level: its output and the
    gradients of projVecs and freqs, which average over the points, are asserted at the same bounds; its gX is printed.  The weighted
    cloud is Gaussian (gX 9.1e-6)."""
    weighted = cloud == "weighted"
    from fsw_gnn_amd import FSW_embedding
    from tests.test_hip_cartesian_train import autograd_functions
    d, S, F = 3, 4, 8
    torch.manual_seed(191)
    ref = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV, dtype=torch.float64)
    low = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV, dtype=torch.float32)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    rng = np.random.default_rng(192 + n)
    if cloud != "unit_line":
        X = t(rng.standard_normal((1, n, d)), torch.float64)
        W = t(rng.uniform(0.05, 1.0, size=(1, n)), torch.float64) if weighted else "unit"
    else:
        V = ref.projVecs.detach().cpu().numpy()
        cands = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [-1.0, 1.0, 1.0], [1.0, 2.0, 3.0], [3.0, -1.0, 2.0]])
        cands /= np.linalg.norm(cands, axis=1, keepdims=True)
        along = np.abs(cands @ V.T).min(axis=1) / np.linalg.norm(V, axis=1).max()
        e = cands[along.argmax()]
        assert along.max() >= 0.02                                  # no slice (nearly) orthogonal to the line
        a = (rng.permutation(n).astype(np.float64) - n // 2) * (8.0 / n)
        X = t((a[:, None] * e[None, :])[None], torch.float64)
        W = "unit"
    G = t(rng.standard_normal((1, S, F)), torch.float64)

    def grads(E, dt):
        E.zero_grad(set_to_none=True)
        Xl = X.to(dt).clone().requires_grad_(True)
        out = E(Xl, W if isinstance(W, str) else W.to(dt))
        names = autograd_functions(out)
        (out * G.to(dt).reshape(out.shape)).sum().backward()
        return {"out": out.detach(), "gX": Xl.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad}, names

    want, _ = grads(ref, torch.float64)
    got, names = grads(low, torch.float32)
    assert "_CartEmbedFnBackward" in names
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("one cloud of %d points (%s), float32 vs float64 module:" % (n, cloud), {k: "%.2e" % e for k, e in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    if cloud == "unit_gauss":
        errs.pop("gX")                                              # near-tied keys ranked differently by the two modules: see above
    assert max(errs.values()) <= MODULE_GRAD, errs


def test_readout_on_a_graph_above_the_hub_classes():
    """FSW_readout(5, 8, embed_slices=4, embed_freqs=8) on a batch of two graphs of 33 000 and 500 vertices against the float64 layer
    with the same state: forward <= 1e-5."""
    from fsw_gnn_amd import FSW_readout
    from tests.test_hip_cartesian_conv import features, make_pair
    from tests.test_hip_cartesian_conv import relerr as rel
    S, F, in_ch, out_ch = 4, 8, 5, 8
    sizes = {0: 33000, 1: 500}
    gi = torch.cat([torch.full((m,), g, dtype=torch.int64) for g, m in sizes.items()])
    gi = gi[torch.randperm(gi.numel(), generator=torch.Generator().manual_seed(7))].to(DEV)
    ref, low = make_pair(FSW_readout, in_ch, out_ch, S, F, concat_self=False, mlp_layers=2)
    x64 = features(gi.numel(), in_ch)
    with torch.no_grad():
        want = ref(x64, gi, 2)
        got = low(x64.float(), gi, 2)
    err = rel(got, want)
    print("readout on graphs of 33000 and 500 vertices, float32 vs float64: %.2e" % err)
    assert err <= MODULE_FWD
