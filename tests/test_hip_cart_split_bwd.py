"""Cartesian mode, the split form of the longest unit-weight rows' backward (csrc/embed_split_cart_bwd.hip):
fsw_embed_cart_backward_keys_f32 with FSW_CART_SPLIT_BWD_LINES runs every phase of k_cart_giant_bwd<false> as a launch of its own over
(line, piece), and the host layer asks for it when a backward has few such lines.

Graphs, keys, the upstream gradient, the yardstick (the generic kernel in backward mode with float64 storage, never the kernel under
test) and the bounds are those of tests/test_hip_cart_giant_bwd.py: F32_BOUND per row and for gfreq, PER_ENTRY of the line maximum per
entry; MODULE_FWD / MODULE_GRAD at module level.  The smallest shapes at which the form can go wrong (runs of 2048 words, walk tiles of
4096 ranks):
  A = (7, 32769, 65537)           17 and 33 runs, the last nearly empty; a run without a partner at the first and the last level; a last
                                  walk tile of one rank
  B = (0, 65536, 100000, 140000)  32 runs exactly, 49 runs, 69 runs; runs without a partner at several levels; lines with different
                                  level counts in one launch
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import relerr
from tests.test_hip_cart_giant import MANY, SHAPES, graph_case
from tests.test_hip_cart_giant_bwd import Call, last_error, reference
from tests.test_hip_cart_hub import DEV, t
from tests.test_hip_cart_hub_w import MODULE_FWD, MODULE_GRAD
from tests.test_hip_cart_split import cloud_graph
from tests.test_hip_ties import F32_BOUND

pytestmark = pytest.mark.gpu

A = (7, 32769, 65537)
B = (0, 65536, 100000, 140000)
UNION = A + B[1:]
GRAPHS = {"A": A, "B": B}


class SplitCall(Call):
    """Call of tests/test_hip_cart_giant_bwd.py with the flags field and a choice of what the scratch holds before the call."""

    def split_query(self):
        from fsw_gnn_amd import _lib
        a, _keep = self.args()
        lines = int(_lib.lib().fsw_embed_cart_split_backward_lines(ctypes.byref(a)))
        return int(_lib.lib().fsw_embed_cart_split_backward_scratch_bytes(ctypes.byref(a))), lines

    def run_flags(self, nbytes, flags, fill=None, with_gfreq=True):
        """(status, gkey, gfreq) with a scratch buffer of nbytes (filled with the byte `fill` when given); gkey pre-filled with NaN."""
        from fsw_gnn_amd import _lib
        scratch = None
        if nbytes:
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            if fill is not None:
                scratch.fill_(fill)
        gkey = torch.full((self.c["nnz"], self.S), float("nan"), device=DEV)
        gf = torch.zeros(self.F, device=DEV) if with_gfreq else None
        a, _keep = self.args(scratch)
        a.g, a.ldg, a.gkey, a.ldk, a.flags = self.g.data_ptr(), self.g.stride(0), gkey.data_ptr(), self.S, flags
        a.gfreq = gf.data_ptr() if with_gfreq else None
        rc = _lib.lib().fsw_embed_cart_backward_keys_f32(ctypes.byref(a), _lib.ptr(self.dtable), self.F if self.dtable is not None else 0,
                                                         self.stream)
        torch.cuda.synchronize()
        return rc, gkey.cpu().numpy(), (gf.cpu().numpy() if with_gfreq else None)

    def run_split(self, fill=None, with_gfreq=True):
        from fsw_gnn_amd import _lib
        nbytes, lines = self.split_query()
        split_rows = sum(d > 32768 for d in self.c["degrees"])
        assert nbytes > 0 and nbytes % 16 == 0 and lines == split_rows * self.S
        rc, gkey, gf = self.run_flags(nbytes, _lib.CART_SPLIT_BWD_LINES, fill, with_gfreq)
        assert rc == 0, last_error()
        return gkey, gf

    def run_plain(self):
        """Flags 0 with the buffer of the older query: k_cart_giant_bwd<false> on the same rows."""
        rc, gkey, gf = self.run_flags(self.query(), 0)
        assert rc == 0, last_error()
        return gkey, gf


def entries(call, degrees):
    """The rows of gkey that belong to the recipients of these degrees."""
    rp = call.c["rowptr"]
    return np.concatenate([np.arange(rp[r], rp[r + 1]) for r, d in enumerate(call.c["degrees"]) if d in degrees])


@pytest.mark.parametrize("S,F", SHAPES)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_backward(name, S, F):
    """Flag set, scratch of the split query: status 0, the NaN-prefilled gkey finite everywhere, per row <= F32_BOUND, per entry <=
    PER_ENTRY of the line maximum, gfreq <= F32_BOUND."""
    call = SplitCall("unit", GRAPHS[name], S, F)
    gkey, gf = call.run_split()
    call.check(gkey, gf, "split backward %s S %d F %d" % (name, S, F))


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_gkey_is_bit_identical_to_the_one_workgroup_kernel(name):
    """The same call with flags 0 and the older query's buffer: gkey is equal bit for bit (the sorted line is unique, the walk's
    arithmetic and order of accumulation are the same); both gfreq are within F32_BOUND of the reference."""
    S, F = SHAPES[1]
    call = SplitCall("unit", GRAPHS[name], S, F)
    split, gf_split = call.run_split()
    plain, gf_plain = call.run_plain()
    assert np.isfinite(split).all() and np.array_equal(split, plain)
    _ref, gf_ref = reference("unit", GRAPHS[name], S, F)
    errs = relerr(gf_split, gf_ref), relerr(gf_plain, gf_ref)
    print("gfreq against the reference, %s: split %.2e, one workgroup per line %.2e" % ((name,) + errs))
    assert max(errs) <= F32_BOUND, errs


def test_a_line_depends_on_the_line_only():
    """gkey of the rows of 32769 and 65537 neighbours comes out bit-identical from A with zero-filled scratch, from A with scratch full
    of 0xFF bytes and from the union graph of A and B (other grids, other level counts, other spans).  The upstream gradient is drawn
    per graph, so the union's first three rows take A's."""
    S, F = SHAPES[1]
    call = SplitCall("unit", A, S, F)
    zero, _ = call.run_split(fill=0)
    ones, _ = call.run_split(fill=0xFF)
    big = SplitCall("unit", UNION, S, F)
    big.g = torch.cat([call.g, big.g[len(A):]])
    union, _ = big.run_split(fill=0)
    assert np.isfinite(zero).all() and np.isfinite(union).all()
    assert np.array_equal(zero, ones)
    assert UNION[:3] == A
    assert np.array_equal(zero[entries(call, A[1:])], union[entries(big, A[1:])])


def test_more_frequencies_than_a_wavefront():
    """S = 2 and the 70 frequencies of MANY on A (a second block of frequencies past 64): the bounds of test_backward, and gkey
    bit-identical to the flag-off call.  xi = -1 alone (F = 1): gkey and the gfreq entry are exactly 0 wherever the reference's are."""
    S, F = 2, 70
    call = SplitCall("unit", A, S, F, MANY)
    gkey, gf = call.run_split()
    call.check(gkey, gf, "split backward S %d F %d" % (S, F))
    assert np.array_equal(gkey, call.run_plain()[0])
    dead = SplitCall("unit", A, S, 1, (-1.0,))
    gkey, gf = dead.run_split()
    ref, gf_ref = reference("unit", A, S, 1, (-1.0,))
    print("xi = -1 alone: the reference's gkey is exactly 0 in %d of %d entries, its gfreq in %d of 1" % ((ref == 0).sum(), ref.size, (gf_ref == 0).sum()))
    assert np.isfinite(gkey).all() and np.isfinite(gf).all()
    assert not gkey[ref == 0].any() and not gf[gf_ref == 0].any()


def test_gfreq_null():
    """gfreq = NULL on A: status 0 and gkey bit-identical to the run with gfreq."""
    S, F = SHAPES[0]
    call = SplitCall("unit", A, S, F)
    without, none = call.run_split(with_gfreq=False)
    with_gf, _gf = call.run_split()
    assert none is None and np.isfinite(without).all() and np.array_equal(without, with_gf)


def test_short_scratch_is_refused():
    """Flag set with a scratch 16 bytes short of the query: non-zero status, fsw_last_error() names the query, nothing is written."""
    from fsw_gnn_amd import _lib
    S, F = SHAPES[0]
    call = SplitCall("unit", A, S, F)
    nbytes, _lines = call.split_query()
    rc, gkey, _gf = call.run_flags(nbytes - 16, _lib.CART_SPLIT_BWD_LINES)
    assert rc != 0 and "fsw_embed_cart_split_backward_scratch_bytes" in last_error()
    assert np.isnan(gkey).all()              # refused before any launch


@pytest.mark.parametrize("kind", ("random", "tau3"))
def test_flag_is_ignored_without_a_split_form(kind):
    """General weights and tau = 3 on the weighted graph of tests/test_hip_cart_giant.py: query and lines are (0, 0) and gkey with the
    flag is bit-identical to gkey without it."""
    from fsw_gnn_amd import _lib
    S, F = SHAPES[0]
    call = SplitCall(kind, None, S, F)
    assert call.split_query() == (0, 0)
    nbytes = call.query()
    rc0, off, _ = call.run_flags(nbytes, 0)
    assert rc0 == 0, last_error()
    rc1, on, _ = call.run_flags(nbytes, _lib.CART_SPLIT_BWD_LINES)
    assert rc1 == 0, last_error()
    assert np.isfinite(off).all() and np.array_equal(off, on)


def test_forward_ignores_the_backward_flag():
    """fsw_embed_cart_f32 on A with flags 2 is bit-identical to flags 0."""
    from fsw_gnn_amd import _lib
    from tests.test_hip_cart_split import SplitCall as ForwardCall
    S, F = SHAPES[1]
    call = ForwardCall(graph_case("unit", A), S, F)
    nbytes = call.query()
    rc0, off = call.run_flags(nbytes, 0)
    assert rc0 == 0, last_error()
    rc1, on = call.run_flags(nbytes, _lib.CART_SPLIT_BWD_LINES)
    assert rc1 == 0, last_error()
    assert np.isfinite(off).all() and np.array_equal(off, on)


# ---- module level -------------------------------------------------------------------------------------------------------------------
def line_cloud(ref, sizes, seed):
    """The line cloud of tests/test_hip_cart_split.py::test_embedding_module_on_one_cloud_of_three_blocks, one per size: distinct
    positions along a direction that no slice is orthogonal to, so that the float32 and the float64 module sort the same order and the
    key gradient is compared where it exists.  [len(sizes), n, 3] float64 (all sizes equal)."""
    rng = np.random.default_rng(seed)
    V = ref.projVecs.detach().cpu().numpy()
    cands = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [-1.0, 1.0, 1.0], [1.0, 2.0, 3.0], [3.0, -1.0, 2.0]])
    cands = np.concatenate([cands, rng.standard_normal((58, 3))])   # many slices: more directions to choose from
    cands /= np.linalg.norm(cands, axis=1, keepdims=True)
    along = np.abs(cands @ V.T).min(axis=1) / np.linalg.norm(V, axis=1).max()
    e = cands[along.argmax()]
    assert along.max() >= 0.02                                      # no slice (nearly) orthogonal to the line
    clouds = [(rng.permutation(n).astype(np.float64) - n // 2) * (8.0 / n) for n in sizes]
    return t(np.stack([a[:, None] * e[None, :] for a in clouds]), torch.float64), rng


def module_grads(E, X, G, dt):
    from tests.test_hip_cartesian_train import autograd_functions
    E.zero_grad(set_to_none=True)
    Xl = X.to(dt).clone().requires_grad_(True)
    out = E(Xl, "unit")
    names = autograd_functions(out)
    (out * G.to(dt).reshape(out.shape)).sum().backward()
    return {"out": out.detach(), "gX": Xl.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad}, names


def test_embedding_module_trains_on_one_cloud():
    """FSW_embedding(d_in=3, nSlices=4, nFreqs=8) on one unit cloud of 70 000 points: four lines, so the policy asks for the split form
    in both directions.  Against the float64 module with the same state: output <= MODULE_FWD; gX, gV and gfreqs <= MODULE_GRAD."""
    from fsw_gnn_amd import FSW_embedding
    n, d, S, F = 70000, 3, 4, 8
    torch.manual_seed(191)
    kw = dict(d_in=d, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV)
    ref = FSW_embedding(dtype=torch.float64, **kw)
    low = FSW_embedding(dtype=torch.float32, **kw)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    X, rng = line_cloud(ref, [n], 192 + n)
    G = t(rng.standard_normal((1, S, F)), torch.float64)
    graph = cloud_graph([n])
    assert low._cart_split_backward(graph, graph.read_stats()) > 0
    want, _ = module_grads(ref, X, G, torch.float64)
    got, names = module_grads(low, X, G, torch.float32)
    assert "_CartEmbedFnBackward" in names
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("one cloud of %d points, split backward, float32 vs float64 module:" % n, {k: "%.2e" % v for k, v in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs


def test_readout_trains_on_one_graph():
    """FSW_readout(5, 8, embed_slices=4, embed_freqs=8) on one graph of 40 000 vertices (four lines: the split form in both directions):
    the gradients of the input and of fsw_embed.projVecs are within MODULE_GRAD of the float64 layer with the same state.  The vertex
    features lie on the line cloud's line, so that both precisions sort the same order."""
    from fsw_gnn_amd import FSW_readout
    from tests.test_hip_cartesian_conv import make_pair
    S, F, in_ch, out_ch, n = 4, 8, 5, 8, 40000
    gi = torch.zeros(n, dtype=torch.int64, device=DEV)
    ref, low = make_pair(FSW_readout, in_ch, out_ch, S, F, concat_self=False, mlp_layers=2, learnable_embedding=True)
    emb = low.fsw_embed
    rng = np.random.default_rng(195 + n)
    V = ref.fsw_embed.projVecs.detach().cpu().numpy()
    cands = rng.standard_normal((16, in_ch))
    cands /= np.linalg.norm(cands, axis=1, keepdims=True)
    along = np.abs(cands @ V.T).min(axis=1) / np.linalg.norm(V, axis=1).max()
    assert along.max() >= 0.02                                      # no slice (nearly) orthogonal to the line
    pos = (rng.permutation(n).astype(np.float64) - n // 2) * (8.0 / n)
    x64 = t(pos[:, None] * cands[along.argmax()][None, :], torch.float64)
    graph = cloud_graph([n])
    assert emb._cart_split_backward(graph, graph.read_stats()) > 0
    G = t(rng.standard_normal((1, out_ch)), torch.float64)

    def grads(layer, dt):
        layer.zero_grad(set_to_none=True)
        xl = x64.to(dt).clone().requires_grad_(True)
        (layer(xl, gi, 1) * G.to(dt)).sum().backward()
        return {"gx": xl.grad, "gV": layer.fsw_embed.projVecs.grad}

    want, got = grads(ref, torch.float64), grads(low, torch.float32)
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("readout on one graph of %d vertices, split backward, float32 vs float64:" % n, {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) <= MODULE_GRAD, errs


def test_policy_keeps_the_one_workgroup_kernel_above_the_threshold():
    """Two clouds of 32769 points with nSlices = max_lines // 2 + 1 and nFreqs = 1: two lines more than
    fsw_embed_cart_split_backward_max_lines(), so _cart_split_backward returns 0 and the backward runs k_cart_giant_bwd; the gradients
    stay within MODULE_GRAD of the float64 module."""
    from fsw_gnn_amd import FSW_embedding, _lib
    n, d, F = 32769, 3, 1
    S = int(_lib.lib().fsw_embed_cart_split_backward_max_lines()) // 2 + 1
    torch.manual_seed(193)
    kw = dict(d_in=d, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV)
    ref = FSW_embedding(dtype=torch.float64, **kw)
    low = FSW_embedding(dtype=torch.float32, **kw)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    X, rng = line_cloud(ref, [n, n], 194)
    G = t(rng.standard_normal((2, S, F)), torch.float64)
    graph = cloud_graph([n, n])
    assert low._cart_split_backward(graph, graph.read_stats()) == 0
    want, _ = module_grads(ref, X, G, torch.float64)
    got, names = module_grads(low, X, G, torch.float32)
    assert "_CartEmbedFnBackward" in names
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("two clouds of %d points, S = %d, float32 vs float64 module:" % (n, S), {k: "%.2e" % v for k, v in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs
