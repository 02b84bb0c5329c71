"""Cartesian mode, the split form of the longest general-weight rows' backward (csrc/embed_split_cart_w_bwd.hip):
fsw_embed_cart_backward_keys_f32 with FSW_CART_SPLIT_W_BWD_LINES runs every phase of k_cart_giant_bwd<true> as a launch of its own over
(line, piece), and the host layer asks for it when a backward has few such lines.

Graphs, keys, weight modes, the upstream gradient, the yardstick (the generic kernel in backward mode with float64 storage, never the
kernel under test) and the bounds are those of tests/test_hip_cart_giant_bwd.py on the weighted family of tests/test_hip_cart_giant.py
(75 000 senders, tied keys, a zero column that ties with the pad element; kinds random, low_mass, tau3): F32_BOUND per row and for gfreq,
PER_ENTRY of the line maximum per entry; MODULE_FWD / MODULE_GRAD at module level.  The smallest shapes at which the form can go wrong
(runs and walk tiles of 2048 elements, lines of D + 1 elements):
  A = (7, 16383, 16384, 24575)           16383: a row of the class below in the shared degree bin -- the split form skips it, and it runs
                                         out of the same scratch; 16384: 16385 elements = 9 runs, the pad element alone in its run, a run
                                         without a partner at the first and the last level; 24575: exactly 12 runs, the pad element is the
                                         line's last word
  B = (0, 24576, 32768, 40000, 70000)    13, 17, 20 and 35 runs; runs without a partner at several levels; lines with different level
                                         counts in one launch
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import relerr
from tests.test_hip_cart_giant import MANY, SHAPES, SUB, graph_case
from tests.test_hip_cart_giant_bwd import Call, last_error, reference
from tests.test_hip_cart_hub import DEV, t
from tests.test_hip_cart_hub_w import MODULE_FWD, MODULE_GRAD
from tests.test_hip_cart_split import cloud_graph
from tests.test_hip_cart_split_bwd import line_cloud, module_grads
from tests.test_hip_ties import F32_BOUND

pytestmark = pytest.mark.gpu

A = (7, 16383, 16384, 24575)
B = (0, 24576, 32768, 40000, 70000)
UNION = A + B[1:]
GRAPHS = {"A": A, "B": B}
KINDS = ("random", "low_mass", "tau3")
FIRST = 16384                               # the shortest row of the class
SHARED_BIN = 8192                           # rows above this many neighbours lie in the class's degree bins and count as lines


class SplitCall(Call):
    """Call of tests/test_hip_cart_giant_bwd.py with the flags field and a choice of what the scratch holds before the call."""

    def split_query(self):
        from fsw_gnn_amd import _lib
        a, _keep = self.args()
        lines = int(_lib.lib().fsw_embed_cart_split_w_backward_lines(ctypes.byref(a)))
        return int(_lib.lib().fsw_embed_cart_split_w_backward_scratch_bytes(ctypes.byref(a))), lines

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
        counted = sum(d > SHARED_BIN for d in self.c["degrees"])       # the row of 16383 neighbours shares the bin: counted, then skipped
        assert nbytes > 0 and nbytes % 16 == 0 and lines == counted * self.S
        rc, gkey, gf = self.run_flags(nbytes, _lib.CART_SPLIT_W_BWD_LINES, fill, with_gfreq)
        assert rc == 0, last_error()
        return gkey, gf

    def run_plain(self):
        """Flags 0 with the buffer of the older query: k_cart_giant_bwd<true> on the same rows."""
        rc, gkey, gf = self.run_flags(self.query(), 0)
        assert rc == 0, last_error()
        return gkey, gf


def entries(call, degrees):
    """The rows of gkey that belong to the recipients of these degrees."""
    rp = call.c["rowptr"]
    return np.concatenate([np.arange(rp[r], rp[r + 1]) for r, d in enumerate(call.c["degrees"]) if d in degrees])


@pytest.mark.parametrize("S,F", SHAPES)
@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("kind", KINDS)
def test_backward(kind, name, S, F):
    """Flag set, scratch of the new query: status 0, the NaN-prefilled gkey finite everywhere, per row <= F32_BOUND, per entry <=
    PER_ENTRY of the line maximum, gfreq <= F32_BOUND."""
    call = SplitCall(kind, GRAPHS[name], S, F)
    gkey, gf = call.run_split()
    call.check(gkey, gf, "split backward %s %s S %d F %d" % (kind, name, S, F))


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_against_the_one_workgroup_kernel(name):
    """The same call with flags 0 and the older query's buffer.  No bit-identity is claimed (csrc/embed_split_cart_w_bwd.hip: the row
    mass and the carries are added in another float64 order); both runs are within the bounds of the reference, and the largest
    per-entry difference relative to the line maximum is printed."""
    S, F = SHAPES[1]
    call = SplitCall("random", GRAPHS[name], S, F)
    split, gf_split = call.run_split()
    plain, gf_plain = call.run_plain()
    call.check(split, gf_split, "split backward %s" % name)
    call.check(plain, gf_plain, "one workgroup per line %s" % name)
    rp, worst = call.c["rowptr"], 0.0
    for r, d in enumerate(call.c["degrees"]):
        if d >= FIRST:
            a, b = split[rp[r]:rp[r + 1]].astype(np.float64), plain[rp[r]:rp[r + 1]].astype(np.float64)
            worst = max(worst, float((np.abs(a - b).max(axis=0) / np.maximum(np.abs(b).max(axis=0), np.finfo(np.float64).tiny)).max()))
    below = entries(call, [d for d in call.c["degrees"] if d < FIRST])
    print("split against one workgroup per line, %s: largest per-entry difference / line maximum %.2e (%d of %d entries differ)"
          % (name, worst, int((split != plain).sum()), split.size))
    assert np.array_equal(split[below], plain[below])          # the rows of the other classes run the same kernels


def test_a_line_depends_on_the_line_only():
    """gkey of the rows of 16384 and 24575 neighbours comes out bit-identical from A with zero-filled scratch, from A with scratch full
    of 0xFF bytes and from the union graph of A and B (other grids, other level counts, other spans).  The upstream gradient is drawn
    per graph, so the union's first four rows take A's."""
    S, F = SHAPES[1]
    call = SplitCall("random", A, S, F)
    zero, _ = call.run_split(fill=0)
    ones, _ = call.run_split(fill=0xFF)
    big = SplitCall("random", UNION, S, F)
    big.g = torch.cat([call.g, big.g[len(A):]])
    union, _ = big.run_split(fill=0)
    assert np.isfinite(zero).all() and np.isfinite(union).all()
    assert np.array_equal(zero, ones)
    assert UNION[:len(A)] == A
    assert np.array_equal(zero[entries(call, A[2:])], union[entries(big, A[2:])])


def test_run_to_run():
    """Two runs of the same call give bit-identical gkey."""
    S, F = SHAPES[1]
    call = SplitCall("low_mass", B, S, F)
    first, _ = call.run_split()
    second, _ = call.run_split()
    assert np.isfinite(first).all() and np.array_equal(first, second)


def test_more_frequencies_than_a_wavefront():
    """S = 2 and the 70 frequencies of MANY on A (a second block of frequencies past 64): the bounds of test_backward.  xi = -1 alone
    (F = 1): gkey and the gfreq entry are exactly 0 wherever the reference's are."""
    S, F = 2, 70
    call = SplitCall("random", A, S, F, MANY)
    gkey, gf = call.run_split()
    call.check(gkey, gf, "split backward S %d F %d" % (S, F))
    dead = SplitCall("random", A, S, 1, (-1.0,))
    gkey, gf = dead.run_split()
    ref, gf_ref = reference("random", A, S, 1, (-1.0,))
    print("xi = -1 alone: the reference's gkey is exactly 0 in %d of %d entries, its gfreq in %d of 1" % ((ref == 0).sum(), ref.size, (gf_ref == 0).sum()))
    assert np.isfinite(gkey).all() and np.isfinite(gf).all()
    assert not gkey[ref == 0].any() and not gf[gf_ref == 0].any()


def test_gfreq_null():
    """gfreq = NULL on A: status 0 and gkey bit-identical to the run with gfreq."""
    S, F = SHAPES[0]
    call = SplitCall("random", A, S, F)
    without, none = call.run_split(with_gfreq=False)
    with_gf, _gf = call.run_split()
    assert none is None and np.isfinite(without).all() and np.array_equal(without, with_gf)


def test_short_scratch_is_refused():
    """Flag set with a scratch 16 bytes short of the query: non-zero status, fsw_last_error() names the query, nothing is written."""
    from fsw_gnn_amd import _lib
    S, F = SHAPES[0]
    call = SplitCall("random", A, S, F)
    nbytes, _lines = call.split_query()
    rc, gkey, _gf = call.run_flags(nbytes - 16, _lib.CART_SPLIT_W_BWD_LINES)
    assert rc != 0 and "fsw_embed_cart_split_w_backward_scratch_bytes" in last_error()
    assert np.isnan(gkey).all()              # refused before any launch


def test_flag_is_ignored_on_a_unit_weight_graph():
    """The unit family with tau = 1: the new query is (0, 0) and gkey with bit 8 is bit-identical to gkey without it."""
    from fsw_gnn_amd import _lib
    S, F = SHAPES[0]
    call = SplitCall("unit", SUB["unit"], S, F)
    assert call.split_query() == (0, 0)
    nbytes = call.query()
    rc0, off, _ = call.run_flags(nbytes, 0)
    assert rc0 == 0, last_error()
    rc1, on, _ = call.run_flags(nbytes, _lib.CART_SPLIT_W_BWD_LINES)
    assert rc1 == 0, last_error()
    assert np.isfinite(off).all() and np.array_equal(off, on)


def test_forward_ignores_the_backward_flag():
    """fsw_embed_cart_f32 on A (random weights) with flags 8 is bit-identical to flags 0."""
    from fsw_gnn_amd import _lib
    from tests.test_hip_cart_split import SplitCall as ForwardCall
    S, F = SHAPES[1]
    call = ForwardCall(graph_case("random", A), S, F)
    nbytes = call.query()
    rc0, off = call.run_flags(nbytes, 0)
    assert rc0 == 0, last_error()
    rc1, on = call.run_flags(nbytes, _lib.CART_SPLIT_W_BWD_LINES)
    assert rc1 == 0, last_error()
    assert np.isfinite(off).all() and np.array_equal(off, on)


# ---- module level -------------------------------------------------------------------------------------------------------------------
def weighted_graph(W):
    """The CSR graph the module builds for clouds with the weights W [clouds, n]: row g holds the points of cloud g."""
    from fsw_gnn_amd import build_csr
    clouds, n = W.shape
    gi = torch.arange(clouds, device=DEV).repeat_interleave(n)
    return build_csr(gi.contiguous(), torch.arange(clouds * n, device=DEV), W.reshape(-1).float().contiguous(), clouds, clouds * n)


def weighted_grads(E, X, W, G, dt):
    """module_grads of tests/test_hip_cart_split_bwd.py with a weight argument: a tensor [clouds, n] or a string."""
    from tests.test_hip_cartesian_train import autograd_functions
    E.zero_grad(set_to_none=True)
    Xl = X.to(dt).clone().requires_grad_(True)
    out = E(Xl, W if isinstance(W, str) else W.to(dt))
    names = autograd_functions(out)
    (out * G.to(dt).reshape(out.shape)).sum().backward()
    return {"out": out.detach(), "gX": Xl.grad, "gV": E.projVecs.grad, "gfreqs": E.freqs.grad}, names


def module_pair(S, F, seed, **kw):
    from fsw_gnn_amd import FSW_embedding
    torch.manual_seed(seed)
    kw = dict(d_in=3, nSlices=S, nFreqs=F, learnable_slices=True, learnable_freqs=True, device=DEV, **kw)
    ref = FSW_embedding(dtype=torch.float64, **kw)
    low = FSW_embedding(dtype=torch.float32, **kw)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return ref, low


@pytest.mark.parametrize("weights", ("random", "uniform", "tau3"))
def test_embedding_module_trains_on_one_weighted_cloud(weights):
    """FSW_embedding(d_in=3, nSlices=4, nFreqs=8) on one cloud of 20 000 points on the line of line_cloud with a float32 tensor of random
    positive weights, with W = 'uniform' and with unit weights and total_mass_pad_thresh = 3: four lines of 20 001 elements, so the
    policy asks for the split form of general weights in the backward.  Against the float64 module with the same state: output <=
    MODULE_FWD; gX, gV and gfreqs <= MODULE_GRAD."""
    n, S, F = 20000, 4, 8
    ref, low = module_pair(S, F, 431, **({"total_mass_pad_thresh": 3.0} if weights == "tau3" else {}))
    X, rng = line_cloud(ref, [n], 432 + n)
    G = t(rng.standard_normal((1, S, F)), torch.float64)
    Wr = t(rng.uniform(0.05, 1.0, size=(1, n)).astype(np.float32).astype(np.float64), torch.float64)
    if weights == "tau3":
        graph = cloud_graph([n])
        want, _ = module_grads(ref, X, G, torch.float64)
        got, names = module_grads(low, X, G, torch.float32)
    else:
        W = "uniform" if weights == "uniform" else Wr
        graph = weighted_graph(torch.full((1, n), 1.0 / n, device=DEV) if weights == "uniform" else Wr)
        want, _ = weighted_grads(ref, X, W, G, torch.float64)
        got, names = weighted_grads(low, X, W, G, torch.float32)
    assert low._cart_split_w_backward(graph, graph.read_stats()) > 0 and low._cart_split_backward(graph, graph.read_stats()) == 0
    assert "_CartEmbedFnBackward" in names
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("one cloud of %d points, %s, split backward of general weights, float32 vs float64 module:" % (n, weights),
          {k: "%.2e" % v for k, v in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs


def test_readout_trains_on_one_graph():
    """FSW_readout(5, 8, embed_slices=4, embed_freqs=8, vertex_degree_pad_thresh=3) on one graph of 20 000 vertices: unit weights with
    tau > 1 take the general-weight kernels, four lines of 20 001 elements the split form in both directions.  The gradients of the
    input and of fsw_embed.projVecs are within MODULE_GRAD of the float64 layer with the same state.  The vertex features lie on a
    line, so that both precisions sort the same order."""
    from fsw_gnn_amd import FSW_readout
    from tests.test_hip_cartesian_conv import make_pair
    S, F, in_ch, out_ch, n = 4, 8, 5, 8, 20000
    gi = torch.zeros(n, dtype=torch.int64, device=DEV)
    ref, low = make_pair(FSW_readout, in_ch, out_ch, S, F, concat_self=False, mlp_layers=2, learnable_embedding=True,
                         vertex_degree_pad_thresh=3.0)
    emb = low.fsw_embed
    rng = np.random.default_rng(435 + n)
    V = ref.fsw_embed.projVecs.detach().cpu().numpy()
    cands = rng.standard_normal((16, in_ch))
    cands /= np.linalg.norm(cands, axis=1, keepdims=True)
    along = np.abs(cands @ V.T).min(axis=1) / np.linalg.norm(V, axis=1).max()
    assert along.max() >= 0.02                                      # no slice (nearly) orthogonal to the line
    pos = (rng.permutation(n).astype(np.float64) - n // 2) * (8.0 / n)
    x64 = t(pos[:, None] * cands[along.argmax()][None, :], torch.float64)
    graph = cloud_graph([n])
    assert emb.total_mass_pad_thresh == 3.0 and emb._cart_split_w_backward(graph, graph.read_stats()) > 0
    G = t(rng.standard_normal((1, out_ch)), torch.float64)

    def grads(layer, dt):
        layer.zero_grad(set_to_none=True)
        xl = x64.to(dt).clone().requires_grad_(True)
        (layer(xl, gi, 1) * G.to(dt)).sum().backward()
        return {"gx": xl.grad, "gV": layer.fsw_embed.projVecs.grad}

    want, got = grads(ref, torch.float64), grads(low, torch.float32)
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("readout on one graph of %d vertices, tau = 3, split backward, float32 vs float64:" % n, {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) <= MODULE_GRAD, errs


def test_policy_keeps_the_one_workgroup_kernel_above_the_threshold():
    """Two weighted clouds of 16384 points with nSlices = max_lines // 2 + 1 and nFreqs = 1: two lines more than
    fsw_embed_cart_split_w_backward_max_lines(), so _cart_split_w_backward returns 0 and the backward runs k_cart_giant_bwd<true>; the
    gradients stay within MODULE_GRAD of the float64 module."""
    from fsw_gnn_amd import _lib
    n, F = 16384, 1
    S = int(_lib.lib().fsw_embed_cart_split_w_backward_max_lines()) // 2 + 1
    ref, low = module_pair(S, F, 433)
    for seed in range(434, 450):            # many slices leave few directions that none of them is nearly orthogonal to: the first
        try:                                # seed whose candidates hold one (line_cloud asserts it)
            X, rng = line_cloud(ref, [n, n], seed)
            break
        except AssertionError:
            continue
    else:
        pytest.fail("no candidate direction of sixteen seeds is away from all %d slices" % S)
    G = t(rng.standard_normal((2, S, F)), torch.float64)
    W = t(rng.uniform(0.05, 1.0, size=(2, n)).astype(np.float32).astype(np.float64), torch.float64)
    graph = weighted_graph(W)
    assert low._cart_split_w_backward(graph, graph.read_stats()) == 0
    want, _ = weighted_grads(ref, X, W, G, torch.float64)
    got, names = weighted_grads(low, X, W, G, torch.float32)
    assert "_CartEmbedFnBackward" in names
    errs = {k: relerr(got[k].double().cpu().numpy(), want[k].cpu().numpy()) for k in want}
    print("two weighted clouds of %d points, S = %d, float32 vs float64 module:" % (n, S), {k: "%.2e" % v for k, v in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs
