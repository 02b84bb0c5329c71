"""Cartesian mode, the split form of the longest general-weight rows (csrc/embed_split_cart_w.hip): fsw_embed_cart_f32 with
FSW_CART_SPLIT_W_LINES runs every phase of k_cart_mergepath_w as a launch of its own over (line, piece), and the host layer asks for it
when a forward has few such lines.

One sender set of 50 000 points in R^8 and a graph with one recipient per in-degree, blocks of 8192 (key, weight) elements of lines of
D + 1 elements:
  16383   the class below: it shares the degree bin, the split form skips it and it runs as without the flag
  16384   the smallest line: 16385 elements, 3 blocks, one run without a partner
  24575   exactly 3 blocks, the pad element is the line's last element
  24576   the pad element alone in a 4th block
  40000   5 blocks, 3 levels
  0, 7, 300, 3000   other classes
S = 3 (no multiple of 4), F = 5 and F = 17 (more than one readout batch of 16); the frequencies hold 0 and negative values.  Rows from 300
neighbours on name 50 of their senders twice, 300 pairs of points coincide (tied keys).  Weight modes: "random" -- float32 weights with 2 %
exact zeros, tau = 1, the row of 24575 scaled to mass 0.4 < tau so that the pad element carries weight --, and "tau" -- w = NULL with
tau = 50000.5: every weight is 1 and every row is deficient.  Mass column, bias and out_scale are on.

The yardstick is the float64 module (FSW_embedding in float64: the generic kernel, pinned to the reference goldens) on the same inputs:
points and slices are dyadic (points k / 4096 with |k| <= 2^15, slice entries k / 8 with |k| <= 8), so the projection of 8 terms of 20
bits is exact in float32 and both sides sort bit-identical keys; weights, frequencies and bias are float32 values.  The bound is the
project's: norm-wise relative error <= 1e-5 per row (TOL) and for the mass column, 1e-5 / 3e-5 at module level.  The rows' norms are far
from zero for these seeds (float64 NumPy oracle: 9.5 .. 29 for the rows of 16383 neighbours and more in every mode and F, at least 0.27 --
the bias -- for every row), so the norm-wise scale is each row's own.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.conftest import relerr
from tests.test_hip_cart_hub import DEV, t
from tests.test_hip_cart_hub_w import MODULE_FWD, MODULE_GRAD
from tests.test_hip_ties import TOL

pytestmark = pytest.mark.gpu

N, D_IN, S = 50000, 8, 3
DEGREES = (0, 7, 300, 3000, 16383, 16384, 24575, 24576, 40000)
SPLIT_ROWS = tuple(r for r, d in enumerate(DEGREES) if d >= 16384)
LOW_ROW, LOW_MASS = DEGREES.index(24575), 0.4
FREQS17 = (0.0, -0.37, 1.0, 2.5, 7.25, -1.5, 0.37, 4.0, 13.0, -2.5, 0.05, 0.5, -0.11, 1.13, 3.1, -5.0, 0.9)
TAUS = {"random": 1.0, "tau": 50000.5}
OUT_SCALE, HAS_MASS = 0.7, 1
SEED = 401


@functools.lru_cache(maxsize=None)
def points():
    """X [N, 8] float64 (dyadic), V [S, 8] float64 (dyadic), Xp [N, 32] float32 = X V^T exactly, with 300 coinciding pairs of points."""
    rng = np.random.default_rng(SEED)
    X = rng.integers(-(1 << 15), (1 << 15) + 1, size=(N, D_IN)).astype(np.float64) / 4096.0
    pairs = rng.permutation(N)[:600].reshape(2, 300)
    X[pairs[1]] = X[pairs[0]]
    V = rng.integers(-8, 9, size=(S, D_IN)).astype(np.float64) / 8.0
    assert (np.abs(V).sum(axis=1) > 0).all()
    P = X @ V.T
    Xp = np.zeros((N, 32), dtype=np.float32)
    Xp[:, :S] = P.astype(np.float32)
    assert np.array_equal(Xp[:, :S].astype(np.float64), P)          # the projection is exact in float32
    for a in (X, V, Xp):
        a.setflags(write=False)
    return X, V, Xp


def edge_lists(degrees=DEGREES):
    """(recipients, senders, float32 weights) sorted by recipient; a row's senders and weights depend on its degree only."""
    rec, snd, w = [], [], []
    for r, deg in enumerate(degrees):
        rng = np.random.default_rng(SEED + 1 + deg)
        s = rng.choice(N, size=deg, replace=False).astype(np.int64)
        if deg >= 300:
            s[:50] = s[50:100]                                       # duplicate senders
        ww = rng.uniform(0.05, 1.0, size=deg).astype(np.float32)
        ww[rng.random(deg) < 0.02] = 0.0                             # exact zeros
        if deg == DEGREES[LOW_ROW]:
            ww = (ww * np.float32(LOW_MASS / ww.astype(np.float64).sum())).astype(np.float32)
        rec.append(np.full(deg, r, dtype=np.int64))
        snd.append(s)
        w.append(ww)
    return np.concatenate(rec), np.concatenate(snd), np.concatenate(w)


def params(F):
    rng = np.random.default_rng(SEED + 100 + F)
    fr = np.array(FREQS17[:F], dtype=np.float32)
    bias = (0.1 * rng.standard_normal(HAS_MASS + S * F)).astype(np.float32)
    return fr, bias


@functools.lru_cache(maxsize=None)
def graph_case(kind, degrees=DEGREES):
    from fsw_gnn_amd import _lib, build_csr
    rec, snd, w = edge_lists(degrees)
    graph = build_csr(t(rec, torch.int64), t(snd, torch.int64), t(w) if kind == "random" else None, len(degrees), N)
    st = graph.read_stats()
    assert st[_lib.STAT_FLAGS] == 0 and st[_lib.STAT_MAX_DEGREE] == max(degrees)
    assert tuple(np.diff(graph.rowptr.cpu().numpy().astype(np.int64))) == tuple(degrees)
    return {"graph": graph, "st": st, "degrees": tuple(degrees), "tau": TAUS.get(kind, 1.0), "kind": kind}


@functools.lru_cache(maxsize=None)
def reference(kind, F):
    """out_scale * the float64 module's output [rows, 1 + S F] on the same points, slices, weights, frequencies and bias."""
    from fsw_gnn_amd import FSW_embedding
    X, V, _ = points()
    fr, bias = params(F)
    rec, snd, w = edge_lists()
    E = FSW_embedding(d_in=D_IN, nSlices=S, nFreqs=F, collapse_freqs=True, encode_total_mass=True, total_mass_pad_thresh=TAUS[kind],
                      device=DEV, dtype=torch.float64)
    with torch.no_grad():
        E.projVecs.copy_(t(V, torch.float64))
        E.freqs.copy_(t(fr, torch.float64))
        E.bias.copy_(t(bias, torch.float64).reshape(E.bias.shape))
        E.total_mass_encoding_scale.fill_(1.0)
        wv = t(w, torch.float64) if kind == "random" else None
        out = E._forward_cartesian(t(X, torch.float64), t(rec, torch.int64), t(snd, torch.int64), wv, len(DEGREES), True, False, None)
    ref = OUT_SCALE * out.cpu().numpy()
    norms = np.linalg.norm(ref[:, HAS_MASS:], axis=1)
    print("float64 module, %s F %d: row norms " % (kind, F) + "  ".join("%d: %.3g" % kv for kv in zip(DEGREES, norms)))
    assert norms[1:].min() > 0.1                                     # the norm-wise scale of every row is its own
    ref.setflags(write=False)
    return ref


def last_error():
    from fsw_gnn_amd import _lib
    return _lib.lib().fsw_last_error().decode()


class Call:
    """One fsw_embed_cart_f32 call on a graph case; slices: the columns of Xp the call reads (S of them from column slices[0] on)."""

    def __init__(self, c, F, first_slice=0, slices=S):
        self.c, self.F, self.S, self.s0 = c, F, slices, first_slice
        fr, bias = params(F)
        self.Xp, self.fr = t(points()[2]), t(fr)
        # the bias of the mass column and of the call's slices
        cols = [0] + [HAS_MASS + s * F + f for s in range(first_slice, first_slice + slices) for f in range(F)]
        self.bias = t(bias[cols])
        self.stream = torch.cuda.current_stream(DEV).cuda_stream

    def args(self, scratch=None, offset=0):
        from fsw_gnn_amd import _lib
        graph = self.c["graph"]
        a = _lib.CartArgs()
        a.value_dtype, a.S, a.F, a.has_mass = 0, self.S, self.F, HAS_MASS
        a.rowptr, a.col = graph.rowptr.data_ptr(), graph.col.data_ptr()
        a.w = graph.w.data_ptr() if graph.w is not None else None
        a.perm, a.bin_start, a.bin_start_host = graph.perm.data_ptr(), graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data
        a.num_rows, a.max_degree = len(self.c["degrees"]), self.c["st"][_lib.STAT_MAX_DEGREE]
        a.Xp, a.ldp, a.freqs = self.Xp.data_ptr() + 4 * self.s0, self.Xp.stride(0), self.fr.data_ptr()
        a.tau, a.out_scale, a.mass_fn, a.mass_scale = self.c["tau"], OUT_SCALE, 0, 1.0
        if self.c["kind"] == "unit":
            self.table = torch.empty((int(_lib.lib().fsw_unit_table_rows(_lib.REG_MAX_DEG)), self.F), device=DEV)
            _lib.check(_lib.lib().fsw_unit_coeff_table(_lib.ptr(self.fr), self.F, _lib.REG_MAX_DEG, _lib.ptr(self.table), self.F, self.stream),
                       "fsw_unit_coeff_table")
            a.unit_table, a.ldt = self.table.data_ptr(), self.F
        if scratch is not None:
            a.scratch, a.scratch_bytes = scratch.data_ptr() + offset, scratch.numel() - offset
        return a

    def queries(self):
        """(forward query, split query, split lines)"""
        from fsw_gnn_amd import _lib
        L, a = _lib.lib(), self.args()
        return (int(L.fsw_embed_cart_forward_scratch_bytes(ctypes.byref(a))), int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(a))),
                int(L.fsw_embed_cart_split_w_lines(ctypes.byref(a))))

    def run(self, nbytes, flags, fill=None, offset=0):
        """(status, out) with a scratch of nbytes from `offset` bytes into a buffer (filled with the byte `fill` when given); out is
        pre-filled with NaN."""
        from fsw_gnn_amd import _lib
        scratch = None
        if nbytes:
            scratch = torch.empty(nbytes + offset, dtype=torch.uint8, device=DEV)
            if fill is not None:
                scratch.fill_(fill)
        out = torch.full((len(self.c["degrees"]), HAS_MASS + self.S * self.F), float("nan"), device=DEV)
        a = self.args(scratch, offset)
        a.out, a.ldo, a.bias, a.flags = out.data_ptr(), out.stride(0), self.bias.data_ptr(), flags
        rc = _lib.lib().fsw_embed_cart_f32(ctypes.byref(a), self.stream)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy().astype(np.float64)

    def run_split(self, fill=None):
        from fsw_gnn_amd import _lib
        forward, nbytes, lines = self.queries()
        assert nbytes > 0 and lines == sum(d > 8192 for d in self.c["degrees"]) * self.S     # every row from the class's first bin on
        rc, out = self.run(max(forward, nbytes), _lib.CART_SPLIT_W_LINES, fill)
        assert rc == 0, last_error()
        return out

    def run_plain(self):
        rc, out = self.run(self.queries()[0], 0)
        assert rc == 0, last_error()
        return out


def row_errors(got, ref):
    return np.array([relerr(got[r, HAS_MASS:], ref[r, HAS_MASS:]) for r in range(got.shape[0])])


@pytest.mark.parametrize("F", (5, 17))
@pytest.mark.parametrize("kind", sorted(TAUS))
def test_forward(kind, F):
    """Flag set: status 0, the NaN-prefilled output finite, every row and the mass column within TOL of the float64 module and every row
    within TOL of the call with flags == 0; the rows of every other class (16383 neighbours included) bit-identical to flags == 0."""
    call = Call(graph_case(kind), F)
    out = call.run_split()
    plain = call.run_plain()
    ref = reference(kind, F)
    assert out.shape == ref.shape and np.isfinite(out).all() and np.isfinite(plain).all()
    errs, against = row_errors(out, ref), row_errors(out, plain)
    mass = np.abs(out[:, 0] - ref[:, 0]) / np.maximum(np.abs(ref[:, 0]), 1e-300)
    print("split form %s F %d against the float64 module: " % (kind, F) + "  ".join("%d: %.1e" % kv for kv in zip(DEGREES, errs)))
    print("   against flags == 0: " + "  ".join("%d: %.1e" % kv for kv in zip(DEGREES, against)) + "   mass column max %.1e" % mass.max())
    print("   flags == 0 against the float64 module: " + "  ".join("%d: %.1e" % kv for kv in zip(DEGREES, row_errors(plain, ref))))
    assert errs.max() <= TOL, dict(zip(DEGREES, errs.tolist()))
    assert against.max() <= TOL, dict(zip(DEGREES, against.tolist()))
    assert mass.max() <= TOL
    others = [r for r in range(len(DEGREES)) if r not in SPLIT_ROWS]
    assert DEGREES.index(16383) in others and np.array_equal(out[others], plain[others])
    assert np.array_equal(out[:, 0], plain[:, 0])


def test_a_line_depends_on_the_line_only():
    """The lines of the row of 40000 neighbours come out bit-identical from the full graph with the scratch full of 0x00, full of 0xFF
    (NaN keys, sums and masses) and in a second run, from the row embedded alone, and from S = 1 calls on each slice's column."""
    F = 5
    r = DEGREES.index(40000)
    call = Call(graph_case("random"), F)
    zero = call.run_split(fill=0)
    ones = call.run_split(fill=0xFF)
    again = call.run_split(fill=0)
    assert np.isfinite(zero).all() and np.array_equal(zero, ones) and np.array_equal(zero, again)
    alone = Call(graph_case("random", (40000,)), F).run_split(fill=0xFF)
    assert np.array_equal(alone[0], zero[r])
    for s in range(S):
        one = Call(graph_case("random", (40000,)), F, first_slice=s, slices=1).run_split()
        assert np.array_equal(one[0, HAS_MASS:], zero[r, HAS_MASS + s * F:HAS_MASS + (s + 1) * F]), s
        assert one[0, 0] == zero[r, 0]


def test_short_or_misaligned_scratch_is_refused():
    """Flag set with a scratch 16 bytes short of the query, or 4 bytes off a 16-byte boundary: non-zero status, fsw_last_error() names the
    query, nothing is written."""
    from fsw_gnn_amd import _lib
    call = Call(graph_case("random"), 5)
    _forward, nbytes, _lines = call.queries()
    for short, offset in ((16, 0), (0, 4)):
        rc, out = call.run(nbytes - short, _lib.CART_SPLIT_W_LINES, offset=offset)
        assert rc != 0 and "fsw_embed_cart_split_w_scratch_bytes" in last_error(), (short, offset)
        assert np.isnan(out).all()               # refused before any launch


@pytest.mark.parametrize("kind,degrees", [("unit", (7, 3000, 40000)), ("random", (7, 3000, 16383))])
def test_flag_is_ignored_without_a_split_form(kind, degrees):
    """A unit-weight graph with a row of 40000 neighbours, and a weighted graph whose longest row has 16383: the query is 0 and the call
    with the bit is bit-identical to the call without it (next to the other bits too)."""
    from fsw_gnn_amd import _lib
    call = Call(graph_case(kind, degrees), 5)
    forward, nbytes, lines = call.queries()
    assert (nbytes, lines) == (0, 0)
    for other in (0, _lib.CART_SPLIT_LINES | _lib.CART_SPLIT_BWD_LINES):
        a = call.args()
        need = max(forward, int(_lib.lib().fsw_embed_cart_split_scratch_bytes(ctypes.byref(a)))) if other else forward
        rc0, off = call.run(need, other)
        assert rc0 == 0, last_error()
        rc1, on = call.run(need, other | _lib.CART_SPLIT_W_LINES)
        assert rc1 == 0, last_error()
        assert np.isfinite(off).all() and np.array_equal(off, on)


# ---- module level -------------------------------------------------------------------------------------------------------------------
def module_pair(nS, F, **kw):
    from fsw_gnn_amd import FSW_embedding
    torch.manual_seed(411)
    ref = FSW_embedding(d_in=D_IN, nSlices=nS, nFreqs=F, device=DEV, dtype=torch.float64, **kw)
    low = FSW_embedding(d_in=D_IN, nSlices=nS, nFreqs=F, device=DEV, dtype=torch.float32, **kw)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return ref, low


def cloud(n=20000):
    rng = np.random.default_rng(SEED + 7)
    return t(rng.standard_normal((1, n, D_IN)), torch.float64), t(rng.uniform(0.05, 1.0, size=(1, n)), torch.float64)


def prepared_for(low, X, W):
    """prepare_cartesian on the graph forward() builds for one cloud."""
    from fsw_gnn_amd import build_csr
    n = X.shape[1]
    wv = torch.full((n,), 1.0 / n, device=DEV) if isinstance(W, str) else W.reshape(-1).float().contiguous()
    graph = build_csr(torch.zeros(n, dtype=torch.int64, device=DEV), torch.arange(n, device=DEV), wv, 1, n)
    return low.prepare_cartesian(X[0].float().contiguous(), graph)


@pytest.mark.parametrize("weights", ("random", "uniform"))
def test_embedding_module_on_one_weighted_cloud(weights):
    """FSW_embedding(d_in=8, nSlices=4, nFreqs=5) on one cloud of 20 000 points (three blocks, four lines) with random weights and with
    W = 'uniform': prepare_cartesian chooses the split form of general weights, not the unit one; the output is within 1e-5 of the float64
    module; serialize_num_slices = 3 gives the same values within 1e-6 of the largest entry."""
    ref, low = module_pair(4, 5)
    X, Wr = cloud()
    W = "uniform" if weights == "uniform" else Wr
    prepared = prepared_for(low, X, W)
    assert prepared["split_w"] is True and prepared["split"] is False and prepared["scratch"] is not None
    with torch.no_grad():
        want = ref(X, W)
        got = low(X.float(), W if isinstance(W, str) else W.float())
        chunked = low(X.float(), W if isinstance(W, str) else W.float(), serialize_num_slices=3)
    err = relerr(got.double().cpu().numpy(), want.cpu().numpy())
    print("one cloud of 20000 points, %s weights, split form, float32 vs float64 module: %.2e" % (weights, err))
    assert err <= MODULE_FWD
    assert torch.allclose(got, chunked, rtol=0, atol=1e-6 * float(got.abs().max()))


def line_cloud(ref, n=20000):
    """One cloud of n distinct positions 4e-4 apart in shuffled order on a line through the origin, along the candidate direction that no
    slice of `ref` is orthogonal to (as tests/test_hip_cart_giant.py::test_embedding_module_on_one_long_cloud does in R^3), with random
    weights."""
    rng = np.random.default_rng(SEED + 9)
    V = ref.projVecs.detach().cpu().numpy()
    cands = rng.standard_normal((16, D_IN))
    cands /= np.linalg.norm(cands, axis=1, keepdims=True)
    along = np.abs(cands @ V.T).min(axis=1) / np.linalg.norm(V, axis=1).max()
    e = cands[along.argmax()]
    assert along.max() >= 0.02                                      # no slice (nearly) orthogonal to the line
    a = (rng.permutation(n).astype(np.float64) - n // 2) * (8.0 / n)
    return t((a[:, None] * e[None, :])[None], torch.float64), t(rng.uniform(0.05, 1.0, size=(1, n)), torch.float64)


def test_training_step_on_one_weighted_cloud():
    """learnable_slices and learnable_freqs: output <= 1e-5, gradients of X, projVecs and freqs <= 3e-5 against the float64 module (the
    backward is the unchanged kernel on the same projection; it does not read the forward's output).

    The cloud lies on a line, so that its keys in every slice are separated by 1e-4 of the largest key, far above the float32 rounding of
    projVecs and of the projection: both modules sort the same order and the key gradient -- piecewise constant in the order -- is
    compared where it exists.  On the Gaussian cloud of the forward tests that is not so: near-tied keys are ranked differently by the
    two modules and gX differs by 6.4e-5 (gV 1.6e-5, gfreqs 8.2e-8, output 2.6e-7), the effect
    tests/test_hip_cart_giant.py::test_embedding_module_on_one_long_cloud describes for its Gaussian unit cloud."""
    from tests.test_hip_cartesian_train import autograd_functions
    nS, F = 4, 5
    ref, low = module_pair(nS, F, learnable_slices=True, learnable_freqs=True)
    X, W = line_cloud(ref)
    G = t(np.random.default_rng(SEED + 8).standard_normal((1, nS, F)), torch.float64)
    assert prepared_for(low, X, W)["split_w"] is True

    def grads(E, dt):
        E.zero_grad(set_to_none=True)
        Xl = X.to(dt).clone().requires_grad_(True)
        out = E(Xl, W.to(dt))
        names = autograd_functions(out)
        (out * G.to(dt).reshape(out.shape)).sum().backward()
        return {"out": out.detach(), "gX": Xl.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad}, names

    want, _ = grads(ref, torch.float64)
    got, names = grads(low, torch.float32)
    assert "_CartEmbedFnBackward" in names
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("training step on one weighted cloud, split form, float32 vs float64 module:", {k: "%.2e" % v for k, v in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs


def test_policy_keeps_the_one_workgroup_kernel_above_the_threshold():
    """nSlices = fsw_embed_cart_split_w_max_lines() + 1 on the same cloud: prepare_cartesian()["split_w"] is false and the output is still
    within 1e-5 of the float64 module."""
    from fsw_gnn_amd import _lib
    nS = int(_lib.lib().fsw_embed_cart_split_w_max_lines()) + 1
    ref, low = module_pair(nS, 1)
    X, W = cloud()
    prepared = prepared_for(low, X, W)
    assert prepared["split_w"] is False and prepared["split"] is False and prepared["scratch"] is not None
    with torch.no_grad():
        want = ref(X, W)
        got = low(X.float(), W.float())
    err = relerr(got.double().cpu().numpy(), want.cpu().numpy())
    print("one cloud of 20000 points, S = %d: float32 vs float64 module %.2e" % (nS, err))
    assert err <= MODULE_FWD
