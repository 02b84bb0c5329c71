"""Cartesian mode, backward of the longest rows: k_cart_giant_bwd (csrc/embed_giant_cart_bwd.hip; unit weights: rows above 32768
neighbours, general weights: lines of 16385 elements and more) through fsw_embed_cart_backward_keys_f32 and through the module.

Graphs, keys, weight modes and frequencies are those of tests/test_hip_cart_giant.py: one recipient per degree -- the last row of the
class below, the first row of this class, run counts (runs of 2048 packed words) that are a power of two and one more, runs without a
partner at several merge levels, a pad element that opens a run of its own (16384, 24576, 32768 neighbours with general weights) --,
200 sender pairs with bit-identical keys, one constant column, one control column without ties and, for weights, one column of zeros,
which ties with the pad element.  The upstream gradient is drawn with a seeded generator.  The yardstick is the generic kernel in
backward mode with float64 storage on the same Xp, g and frequencies (as tests/test_hip_cart_hub.py::check_backward), never the
kernel under test.  Bounds: F32_BOUND per row and for gfreq, PER_ENTRY of the line maximum per entry (tests/test_hip_ties.py);
MODULE_FWD / MODULE_GRAD at module level.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.conftest import relerr
from tests.test_hip_cart_giant import KINDS, MANY, SHAPES, SUB, graph_case, inputs
from tests.test_hip_cart_hub import DEV, HAS_MASS, OUT_SCALE, cart_args, t, unit_tables
from tests.test_hip_cart_hub_w import MODULE_FWD, MODULE_GRAD, weighted_args
from tests.test_hip_ties import F32_BOUND, FREQS, PER_ENTRY, check_key_gradients, coefficient_scale

pytestmark = pytest.mark.gpu

NEW = "fsw_embed_cart_backward_keys_scratch_bytes"


def sub(kind):
    return SUB["unit" if kind == "unit" else "weighted"]


@functools.lru_cache(maxsize=None)
def upstream(nrows, S, F):
    """The output gradient [nrows, HAS_MASS + S F] float32, seeded."""
    g = np.random.default_rng(211 + 1000 * nrows + 10 * S + F).standard_normal((nrows, HAS_MASS + S * F)).astype(np.float32)
    g.setflags(write=False)
    return g


def args_for(c, x, S, F, Xp, fr, table, scratch, dtype=0):
    if c["kind"] == "unit":
        return cart_args(c, x, S, F, Xp, fr, table, scratch, dtype=dtype), None
    return weighted_args(c, x, S, F, Xp, fr, scratch, dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(kind, degrees, S, F, freqs=FREQS):
    """(gkey [nnz, S], gfreq [F]) float64 of the generic kernel with float64 storage in backward mode."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    c, x = graph_case(kind, degrees), inputs(kind != "unit", S, F, freqs)
    nrows = len(c["degrees"])
    stream = torch.cuda.current_stream(DEV).cuda_stream
    Xp64, fr64, g64 = t(x["Xp"], torch.float64), t(x["fr"], torch.float64), t(upstream(nrows, S, F), torch.float64)
    gkey = torch.full((c["nnz"], S), float("nan"), dtype=torch.float64, device=DEV)
    gf = torch.zeros(F, dtype=torch.float64, device=DEV)
    scratch = torch.empty(int(L.fsw_embed_cart_generic_scratch_bytes(max(c["degrees"]), nrows)), dtype=torch.uint8, device=DEV)
    a, _keep = args_for(c, x, S, F, Xp64, fr64, None, scratch, dtype=1)
    a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g64.data_ptr(), g64.stride(0), gkey.data_ptr(), S, gf.data_ptr()
    _lib.check(L.fsw_embed_cart_generic(ctypes.byref(a), stream), "fsw_embed_cart_generic (backward, float64)")
    torch.cuda.synchronize()
    out = gkey.cpu().numpy(), gf.cpu().numpy()
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    for o in out:
        o.setflags(write=False)
    return out


class Call:
    """The arguments of one fsw_embed_cart_backward_keys_f32 call on a graph case (the device tensors stay alive with the object)."""

    def __init__(self, kind, degrees, S, F, freqs=FREQS):
        self.c, self.S, self.F, self.freqs, self.kind, self.degrees = graph_case(kind, degrees), S, F, freqs, kind, degrees
        self.x = inputs(kind != "unit", S, F, freqs)
        self.nrows = len(self.c["degrees"])
        self.stream = torch.cuda.current_stream(DEV).cuda_stream
        self.Xp, self.fr, self.g = t(self.x["Xp"]), t(self.x["fr"]), t(upstream(self.nrows, S, F))
        self.table, self.dtable = unit_tables(self.fr, F, self.stream) if kind == "unit" else (None, None)

    def args(self, scratch=None):
        return args_for(self.c, self.x, self.S, self.F, self.Xp, self.fr, self.table, scratch)

    def query(self):
        from fsw_gnn_amd import _lib
        a, _keep = self.args()
        return int(getattr(_lib.lib(), NEW)(ctypes.byref(a)))

    def one_line(self):
        """The new query on a one-row, S = 1 copy of the arguments: the bytes of one scratch line."""
        from fsw_gnn_amd import _lib
        a, _keep = self.args()
        bs = np.zeros(_lib.NUM_BINS + 1, dtype=np.int32)
        bs[_lib.NUM_BINS] = 1                                        # one row, in the last bin
        a.bin_start_host, a.S = bs.ctypes.data, 1
        return int(getattr(_lib.lib(), NEW)(ctypes.byref(a)))

    def generic_size(self):
        from fsw_gnn_amd import _lib
        return int(_lib.lib().fsw_embed_cart_generic_scratch_bytes(max(self.c["degrees"]), 1))

    def run(self, nbytes, with_gfreq=True):
        """(status, gkey, gfreq) with a scratch buffer of nbytes; gkey pre-filled with NaN, gfreq zeroed (None without)."""
        from fsw_gnn_amd import _lib
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
        gkey = torch.full((self.c["nnz"], self.S), float("nan"), device=DEV)
        gf = torch.zeros(self.F, device=DEV) if with_gfreq else None
        a, _keep = self.args(scratch)
        a.g, a.ldg, a.gkey, a.ldk = self.g.data_ptr(), self.g.stride(0), gkey.data_ptr(), self.S
        a.gfreq = gf.data_ptr() if with_gfreq else None
        rc = _lib.lib().fsw_embed_cart_backward_keys_f32(ctypes.byref(a), _lib.ptr(self.dtable), self.F if self.dtable is not None else 0,
                                                         self.stream)
        torch.cuda.synchronize()
        return rc, gkey.cpu().numpy(), (gf.cpu().numpy() if with_gfreq else None)

    def check(self, gkey, gf, what):
        """The bounds of test_backward against the generic kernel with float64 storage."""
        ref, gf_ref = reference(self.kind, self.degrees, self.S, self.F, self.freqs)
        assert np.isfinite(gkey).all(), what
        G = OUT_SCALE * upstream(self.nrows, self.S, self.F)[:, HAS_MASS:].astype(np.float64)
        scale = coefficient_scale(G, np.tile(self.x["fr"].astype(np.float64), self.S)).reshape(self.nrows, self.S, self.F).sum(axis=2)
        check_key_gradients(gkey.astype(np.float64), ref, self.c["rowptr"], list(self.x["kinds"]), what, scale,
                            row_bound=F32_BOUND, entry_bound=PER_ENTRY)
        if gf is not None:
            e = relerr(gf, gf_ref)
            print("%s: gfreq %.2e" % (what, e))
            assert np.isfinite(gf).all() and e <= F32_BOUND, (what, e)


def last_error():
    from fsw_gnn_amd import _lib
    return _lib.lib().fsw_last_error().decode()


@pytest.mark.parametrize("S,F", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_backward(kind, S, F):
    """fsw_embed_cart_backward_keys_f32 with the scratch of fsw_embed_cart_backward_keys_scratch_bytes on the full graph: status 0, the
    NaN-prefilled gkey finite everywhere, per row <= F32_BOUND, per entry <= PER_ENTRY of the line maximum, gfreq <= F32_BOUND."""
    call = Call(kind, None, S, F)
    nbytes = call.query()
    assert nbytes > 0 and nbytes % 16 == 0
    rc, gkey, gf = call.run(nbytes)
    assert rc == 0, last_error()
    call.check(gkey, gf, "giant backward %s S %d F %d" % (kind, S, F))


@pytest.mark.parametrize("kind", ("unit", "random"))
def test_one_scratch_line_suffices(kind):
    """The full graph with S = 3 and a scratch of exactly ONE line -- smaller than the smallest buffer the generic kernel accepted for
    these rows, so a library without the backward kernel of the longest rows refuses the call on the host: status 0, same bounds."""
    S, F = SHAPES[0]
    call = Call(kind, None, S, F)
    line = call.one_line()
    assert 0 < line < call.generic_size() and line <= call.query()
    rc, gkey, gf = call.run(line)
    assert rc == 0, last_error()
    call.check(gkey, gf, "giant backward %s, one scratch line" % kind)


@pytest.mark.parametrize("kind", ("unit", "random"))
def test_gkey_does_not_depend_on_the_buffer(kind):
    """The sub-graph (a short row, the first row of the class, a longer one) at S = 4 with one line of scratch (one workgroup takes the
    eight lines one after the other), the buffer of the query (eight workgroups) and the smallest buffer that worked before: gkey is
    bit-identical; gfreq, formed with atomics, is within F32_BOUND of the reference in each."""
    S, F = SHAPES[1]
    call = Call(kind, sub(kind), S, F)
    sizes = {"one line": call.one_line(), "query": call.query(), "generic": call.generic_size()}
    assert sizes["query"] == 8 * sizes["one line"] and sizes["one line"] < sizes["generic"]
    got = {}
    for name, nbytes in sizes.items():
        rc, gkey, gf = call.run(nbytes)
        assert rc == 0, (name, last_error())
        got[name] = gkey
        call.check(gkey, gf, "giant backward %s, buffer: %s" % (kind, name))
    assert np.array_equal(got["one line"], got["query"]) and np.array_equal(got["query"], got["generic"])


@pytest.mark.parametrize("kind", ("unit", "random"))
def test_more_frequencies_than_a_wavefront(kind):
    """S = 2 and the 70 frequencies of MANY (a second walk over the line past 64; xi = 0, +-0, -1 and negative twins) on the sub-graph:
    the bounds of test_backward.  xi = -1 alone (F = 1): the factor 1 + xi makes every key gradient exactly 0 -- gkey and the gfreq
    entry are exactly 0 wherever the reference's are."""
    S, F = 2, 70
    call = Call(kind, sub(kind), S, F, MANY)
    rc, gkey, gf = call.run(call.query())
    assert rc == 0, last_error()
    call.check(gkey, gf, "giant backward %s S %d F %d" % (kind, S, F))
    dead = Call(kind, sub(kind), S, 1, (-1.0,))
    rc, gkey, gf = dead.run(dead.query())
    assert rc == 0, last_error()
    ref, gf_ref = reference(kind, dead.degrees, S, 1, (-1.0,))
    print("xi = -1 alone: the reference's gkey is exactly 0 in %d of %d entries, its gfreq in %d of 1" % ((ref == 0).sum(), ref.size, (gf_ref == 0).sum()))
    assert np.isfinite(gkey).all() and np.isfinite(gf).all()
    assert not gkey[ref == 0].any() and not gf[gf_ref == 0].any()


def test_gfreq_null():
    """gfreq = NULL on the weighted sub-graph: status 0 and gkey bit-identical to the run with gfreq."""
    S, F = SHAPES[0]
    call = Call("random", sub("random"), S, F)
    nbytes = call.query()
    rc0, without, none = call.run(nbytes, with_gfreq=False)
    assert rc0 == 0 and none is None, last_error()
    rc1, with_gf, _gf = call.run(nbytes)
    assert rc1 == 0, last_error()
    assert np.isfinite(without).all() and np.array_equal(without, with_gf)


# ---- module level -------------------------------------------------------------------------------------------------------------------
def test_embedding_module_unit_cloud_with_pad_threshold():
    """FSW_embedding(d_in=3, nSlices=4, nFreqs=8, total_mass_pad_thresh=3) on one cloud of 20 000 points with W = 'unit': the w = NULL,
    tau > 1 path on a line of 20 001 elements (general-weight kernels in both directions).  The cloud is the "unit_line" construction
    of tests/test_hip_cart_giant.py::test_embedding_module_on_one_long_cloud: 20 000 distinct positions on a line through the origin
    along a direction that no slice is orthogonal to, so the keys of every slice are well separated and the float32 and the float64
    module sort the same order.  Output <= MODULE_FWD; gradients of X, projVecs and freqs <= MODULE_GRAD."""
    from fsw_gnn_amd import FSW_embedding
    from tests.test_hip_cartesian_train import autograd_functions
    d, S, F, n = 3, 4, 8, 20000
    torch.manual_seed(191)
    kw = dict(d_in=d, nSlices=S, nFreqs=F, total_mass_pad_thresh=3.0, learnable_slices=True, learnable_freqs=True, device=DEV)
    ref = FSW_embedding(dtype=torch.float64, **kw)
    low = FSW_embedding(dtype=torch.float32, **kw)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    rng = np.random.default_rng(192 + n)
    V = ref.projVecs.detach().cpu().numpy()
    cands = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [-1.0, 1.0, 1.0], [1.0, 2.0, 3.0], [3.0, -1.0, 2.0]])
    cands /= np.linalg.norm(cands, axis=1, keepdims=True)
    along = np.abs(cands @ V.T).min(axis=1) / np.linalg.norm(V, axis=1).max()
    e = cands[along.argmax()]
    assert along.max() >= 0.02                                      # no slice (nearly) orthogonal to the line
    pos = (rng.permutation(n).astype(np.float64) - n // 2) * (8.0 / n)
    X = t((pos[:, None] * e[None, :])[None], torch.float64)
    G = t(rng.standard_normal((1, S, F)), torch.float64)

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
    print("one cloud of %d points, W = 'unit', tau = 3, float32 vs float64 module:" % n, {k: "%.2e" % v for k, v in errs.items()})
    assert errs.pop("out") <= MODULE_FWD
    assert max(errs.values()) <= MODULE_GRAD, errs
