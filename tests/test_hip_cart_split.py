"""Cartesian mode, the split form of the longest unit-weight rows (csrc/embed_split_cart.hip): fsw_embed_cart_f32 with
FSW_CART_SPLIT_LINES runs every phase of k_cart_giant as a launch of its own over (line, block), and the host layer asks for it when a
forward has few such lines.

Graphs, keys and helpers are those of tests/test_hip_cart_giant.py (a row's senders depend on its degree only), the yardstick is the
float64 oracle through the diagonal identity, the bounds are the project's: TOL per row and for the mass column, 1e-5 / 3e-5 at module
level.  The smallest shapes at which the form can go wrong, blocks of 32768 keys:
  A = (7, 32769, 65537)           two blocks with a nearly empty second one; three blocks: a level with an absent partner block
  B = (0, 65536, 100000, 140000)  two full blocks; four blocks; five blocks: three levels, three absent blocks
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import relerr
from tests.test_hip_cart_giant import MANY, Call, forward_reference, graph_case, last_error
from tests.test_hip_cart_hub import DEV, HAS_MASS, OUT_SCALE, SHAPES, check_rows, t
from tests.test_hip_cart_hub_w import MODULE_FWD, MODULE_GRAD
from tests.test_hip_signed_freqs import SIGNED
from tests.test_hip_ties import TOL

pytestmark = pytest.mark.gpu

A = (7, 32769, 65537)
B = (0, 65536, 100000, 140000)
UNION = A + B[1:]
GRAPHS = {"A": A, "B": B}


class SplitCall(Call):
    """Call of tests/test_hip_cart_giant.py with the flags field and a choice of what the scratch holds before the call."""

    def split_query(self):
        from fsw_gnn_amd import _lib
        a, _keep = self.args()
        lines = int(_lib.lib().fsw_embed_cart_split_lines(ctypes.byref(a)))
        return int(_lib.lib().fsw_embed_cart_split_scratch_bytes(ctypes.byref(a))), lines

    def run_flags(self, nbytes, flags, fill=None):
        """(status, out) with a scratch buffer of nbytes (filled with the byte `fill` when given); out pre-filled with NaN."""
        from fsw_gnn_amd import _lib
        scratch = None
        if nbytes:
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            if fill is not None:
                scratch.fill_(fill)
        out = torch.full((len(self.c["degrees"]), HAS_MASS + self.S * self.F), float("nan"), device=DEV)
        a, _keep = self.args(scratch)
        a.out, a.ldo, a.bias, a.flags = out.data_ptr(), out.stride(0), self.bias.data_ptr(), flags
        rc = _lib.lib().fsw_embed_cart_f32(ctypes.byref(a), self.stream)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy().astype(np.float64)

    def run_split(self, fill=None):
        from fsw_gnn_amd import _lib
        nbytes, lines = self.split_query()
        split_rows = sum(d > 32768 for d in self.c["degrees"])
        assert nbytes > 0 and lines == split_rows * self.S
        rc, out = self.run_flags(nbytes, _lib.CART_SPLIT_LINES, fill)
        assert rc == 0, last_error()
        return out


@pytest.mark.parametrize("S,F", SHAPES)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_forward(name, S, F):
    """Flag set, scratch of the split query: status 0, the NaN-prefilled output finite everywhere, every row (mass column included) within
    TOL of the float64 oracle; the rows of 0 and 7 neighbours bit-identical to the call with flags == 0."""
    degrees = GRAPHS[name]
    call = SplitCall(graph_case("unit", degrees), S, F)
    out = call.run_split()
    assert np.isfinite(out).all()
    check_rows(out, forward_reference("unit", degrees, S, F), degrees, "split forward %s S %d F %d" % (name, S, F))
    rc, plain = call.run_flags(call.query(), 0)
    assert rc == 0, last_error()
    short = [r for r, d in enumerate(degrees) if d <= 32768]
    assert short and np.array_equal(out[short], plain[short])


@pytest.mark.parametrize("F", (19, 70))
def test_more_frequencies_than_a_batch_and_a_wavefront(F):
    """S = 2 and F = 19 / 70 frequencies of MANY on A: rows within TOL, the columns at xi = -1 exactly out_scale * bias."""
    S = 2
    call = SplitCall(graph_case("unit", A), S, F, MANY)
    out = call.run_split()
    what = "split forward S %d F %d" % (S, F)
    check_rows(out, forward_reference("unit", A, S, F, MANY), A, what)
    dead = [HAS_MASS + s * F + f for s in range(S) for f in range(F) if MANY[f] == -1.0]
    want = (np.float32(OUT_SCALE) * call.x["bias"][dead]).astype(np.float64)
    assert len(dead) == S and np.array_equal(out[:, dead], np.broadcast_to(want, (out.shape[0], len(dead)))), what


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_signed_frequencies(name):
    """The frequencies SIGNED[:5] of tests/test_hip_signed_freqs.py at (S, F) = (3, 5): per row within TOL."""
    S, F = SHAPES[0]
    degrees = GRAPHS[name]
    call = SplitCall(graph_case("unit", degrees), S, F, SIGNED)
    out = call.run_split()
    check_rows(out, forward_reference("unit", degrees, S, F, SIGNED), degrees, "split forward %s at signed frequencies" % name)


def test_a_line_depends_on_the_line_only():
    """The rows of 32769 and 65537 neighbours come out bit-identical from A with zero-filled scratch, from A with scratch full of 0xFF
    bytes (NaN keys, NaN partial sums) and from the union graph of A and B (other grids, other levels, twice the lines)."""
    S, F = SHAPES[1]
    call = SplitCall(graph_case("unit", A), S, F)
    zero = call.run_split(fill=0)
    ones = call.run_split(fill=0xFF)
    union = SplitCall(graph_case("unit", UNION), S, F).run_split(fill=0)
    assert np.isfinite(zero).all() and np.isfinite(union).all()
    assert np.array_equal(zero, ones)
    assert UNION[:3] == A and np.array_equal(zero[1:3], union[1:3])


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_split_against_the_one_workgroup_kernel(name):
    """The same call with the flag off (k_cart_giant): per row relerr <= 2 TOL -- both are within TOL of the oracle, the order of
    summation differs (blocks last there, blocks after the workgroup here)."""
    S, F = SHAPES[1]
    degrees = GRAPHS[name]
    call = SplitCall(graph_case("unit", degrees), S, F)
    out = call.run_split()
    rc, giant = call.run_flags(call.query(), 0)
    assert rc == 0, last_error()
    errs = {d: relerr(out[r, HAS_MASS:], giant[r, HAS_MASS:]) for r, d in enumerate(degrees) if d > 0}
    print("split against k_cart_giant, %s: " % name + "  ".join("%d: %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 2 * TOL, errs
    assert np.array_equal(out[:, 0], giant[:, 0])


def test_short_scratch_is_refused():
    """Flag set with a scratch 16 bytes short of the query: non-zero status, fsw_last_error() names the query, nothing is written."""
    from fsw_gnn_amd import _lib
    S, F = SHAPES[0]
    call = SplitCall(graph_case("unit", A), S, F)
    nbytes, _lines = call.split_query()
    rc, out = call.run_flags(nbytes - 16, _lib.CART_SPLIT_LINES)
    assert rc != 0 and "fsw_embed_cart_split_scratch_bytes" in last_error()
    assert np.isnan(out).all()               # refused before any launch


@pytest.mark.parametrize("kind", ("random", "tau3"))
def test_flag_is_ignored_without_a_split_form(kind):
    """General weights and tau = 3 on the weighted graph of tests/test_hip_cart_giant.py: the query is 0 and the call with the flag is
    bit-identical to the call without it."""
    from fsw_gnn_amd import _lib
    S, F = SHAPES[0]
    call = SplitCall(graph_case(kind), S, F)
    assert call.split_query() == (0, 0)
    nbytes = call.query()
    rc0, off = call.run_flags(nbytes, 0)
    assert rc0 == 0, last_error()
    rc1, on = call.run_flags(nbytes, _lib.CART_SPLIT_LINES)
    assert rc1 == 0, last_error()
    assert np.isfinite(off).all() and np.array_equal(off, on)


# ---- module level -------------------------------------------------------------------------------------------------------------------
def cloud_graph(sizes):
    """The CSR graph the module builds for clouds of these sizes with W = 'unit': row g holds the points of cloud g."""
    from fsw_gnn_amd import build_csr
    gi = torch.cat([torch.full((m,), g, dtype=torch.int64) for g, m in enumerate(sizes)]).to(DEV)
    return build_csr(gi.contiguous(), torch.arange(gi.numel(), device=DEV), None, len(sizes), gi.numel())


def test_embedding_module_on_one_cloud_of_three_blocks():
    """FSW_embedding(d_in=3, nSlices=4, nFreqs=8) on one unit cloud of 70 000 points (three blocks, four lines: the split form) against
    the float64 module with the same state: output <= 1e-5, gradients of X, projVecs and freqs <= 3e-5 -- the backward is the one of
    tests/test_hip_cart_giant_bwd.py out of the forward's (larger) buffer.  The cloud is the line cloud of
    tests/test_hip_cart_giant.py::test_embedding_module_on_one_long_cloud: distinct positions along a direction that no slice is
    orthogonal to, so that both modules sort the same order and the key gradient is compared where it exists."""
    from fsw_gnn_amd import FSW_embedding
    from tests.test_hip_cartesian_train import autograd_functions
    n, d, S, F = 70000, 3, 4, 8
    torch.manual_seed(191)
    ref = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV, dtype=torch.float64)
    low = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV, dtype=torch.float32)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    rng = np.random.default_rng(192 + n)
    V = ref.projVecs.detach().cpu().numpy()
    cands = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [-1.0, 1.0, 1.0], [1.0, 2.0, 3.0], [3.0, -1.0, 2.0]])
    cands /= np.linalg.norm(cands, axis=1, keepdims=True)
    along = np.abs(cands @ V.T).min(axis=1) / np.linalg.norm(V, axis=1).max()
    e = cands[along.argmax()]
    assert along.max() >= 0.02                                      # no slice (nearly) orthogonal to the line
    a = (rng.permutation(n).astype(np.float64) - n // 2) * (8.0 / n)
    X = t((a[:, None] * e[None, :])[None], torch.float64)
    G = t(rng.standard_normal((1, S, F)), torch.float64)

    prepared = low.prepare_cartesian(X[0].float().contiguous(), cloud_graph([n]))
    assert prepared["split"] is True and prepared["scratch"] is not None

    def grads(E, dt):
        E.zero_grad(set_to_none=True)
        Xl = X.to(dt).clone().requires_grad_(True)
        out = E(Xl, "unit")
        names = autograd_functions(out)
        (out * G.to(dt).reshape(out.shape)).sum().backward()
        return {"out": out.detach(), "gX": Xl.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad}, names

    want, _ = grads(ref, torch.float64)
    got, names = grads(low, torch.float32)
    assert "_CartEmbedFnBackward" in names
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("one cloud of %d points, split form, float32 vs float64 module:" % n, {k: "%.2e" % v for k, v in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs


def test_readout_on_one_graph_of_two_blocks():
    """FSW_readout(5, 8, embed_slices=4, embed_freqs=8) on one graph of 40 000 vertices (two blocks, four lines: the split form
    through prepare_cartesian) against the float64 layer with the same state: forward <= 1e-5."""
    from fsw_gnn_amd import FSW_readout
    from tests.test_hip_cartesian_conv import features, make_pair
    S, F, in_ch, out_ch, n = 4, 8, 5, 8, 40000
    gi = torch.zeros(n, dtype=torch.int64, device=DEV)
    ref, low = make_pair(FSW_readout, in_ch, out_ch, S, F, concat_self=False, mlp_layers=2)
    x64 = features(n, in_ch)
    emb = low.fsw_embed
    assert emb.prepare_cartesian(x64.float().contiguous(), cloud_graph([n]))["split"] is True
    with torch.no_grad():
        want = ref(x64, gi, 1)
        got = low(x64.float(), gi, 1)
    err = relerr(got.double().cpu().numpy(), want.cpu().numpy())
    print("readout on one graph of %d vertices, split form, float32 vs float64: %.2e" % (n, err))
    assert err <= MODULE_FWD


def test_policy_keeps_the_one_workgroup_kernel_above_the_threshold():
    """Two clouds of 32769 points with nSlices = max_lines // 2 + 1 and nFreqs = 1: two lines more than
    fsw_embed_cart_split_max_lines(), so prepare_cartesian()["split"] is false; the output is within 1e-5 of the float64 module."""
    from fsw_gnn_amd import FSW_embedding, _lib
    n, d, F = 32769, 3, 1
    S = int(_lib.lib().fsw_embed_cart_split_max_lines()) // 2 + 1
    torch.manual_seed(193)
    ref = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, device=DEV, dtype=torch.float64)
    low = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, device=DEV, dtype=torch.float32)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    X = t(np.random.default_rng(194).standard_normal((2, n, d)), torch.float64)
    prepared = low.prepare_cartesian(X.reshape(-1, d).float().contiguous(), cloud_graph([n, n]))
    assert prepared["split"] is False and prepared["scratch"] is not None
    with torch.no_grad():
        want = ref(X, "unit")
        got = low(X.float(), "unit")
    err = relerr(got.double().cpu().numpy(), want.cpu().numpy())
    print("two clouds of %d points, S = %d: float32 vs float64 module %.2e" % (n, S, err))
    assert err <= MODULE_FWD
