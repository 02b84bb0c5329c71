"""Every entry point on a non-blocking side stream while the default stream is blocked.

One harness (blocked_side_stream) for every case:
  1. the expected results: the ordinary call on the default stream, twice (which results are reproducible run to run), synchronised;
  2. the inputs allocated again and prefilled with harmless poison (NaN features and weights, all-zero index tensors), then a fixed
     1.5 s wait queued on the DEFAULT stream with an event recorded behind it -- its length comes from a calibration of
     torch.cuda._sleep on the idle device, never from the code under test;
  3. on side = torch.cuda.Stream(): queued matmuls, the real inputs copied into the poisoned tensors, the call (and its backward),
     the results copied to the host -- no synchronisation other than what .cpu() does on `side`;
  4. the event behind the blocker has NOT completed: the call neither waited for nor launched into the null stream and made no
     device-wide synchronisation (a blocker that ended early fails the case as inconclusive; it never passes);
  5. the results equal step 1's: bit for bit where step 1 was reproducible, within the oracle bound of tests/test_hip_layouts.py
     otherwise (a non-reproducible result without an oracle reference fails);
  6. torch.cuda.synchronize(); every tensor of the case, its autograd graph included, stays referenced until then.
A launch misplaced on the null stream sits behind the blocker, its writes are missing when `side` drains: step 5 fails.  A hidden
device-wide wait fails step 4.  test_harness_control runs a pure-torch chain through the same steps first: where that fails step 4
the harness proves nothing on this runtime and the whole file skips with that reason (DESIGN.md "Call conditions").
No graph capture, no multi-rank paths, not the legacy wrappers (their device-wide wait is their contract, tests/test_hip_parity.py)."""
import time

import numpy as np
import pytest
import torch

from tests import layout_cases as LC
from tests import test_hip_layouts as TL
from tests.conftest import relerr

pytestmark = pytest.mark.gpu
BLOCKER_SECONDS = 1.5
F32_BOUND, F64_BOUND = TL.F32_BOUND, TL.F64_BOUND
N = LC.N_VERT
_STATE = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


t = TL.t


def calibration(dev):
    """Once per session, on the idle device with events: cycles of torch.cuda._sleep per second, and the number of 2048^2 matmuls
    that take roughly 50 ms."""
    if "cal" not in _STATE:
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles, ms = 1_000_000, 0.0
        torch.cuda._sleep(cycles)                      # first launch
        for _ in range(6):
            torch.cuda.synchronize()
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 20.0:
                break
            cycles *= 8
        assert ms >= 20.0, "torch.cuda._sleep cannot be calibrated on this runtime (%d cycles took %.3f ms)" % (cycles, ms)
        big = torch.randn((2048, 2048), device=dev)
        acc = big @ big
        torch.cuda.synchronize()
        a.record()
        for _ in range(20):
            acc = acc @ big * 1e-2
        b.record()
        torch.cuda.synchronize()
        per = a.elapsed_time(b) / 20
        _STATE["cal"] = {"cycles_per_second": cycles / (ms * 1e-3), "matmuls": int(min(max(50.0 / max(per, 1e-3), 20), 400)), "big": big}
    return _STATE["cal"]


class Case:
    """inputs: {name: device tensor} of real values; run(inputs, keep) -> {name: tensor} (keep: a list the run appends what must
    outlive it to -- the output with its autograd graph); refs(expected) -> oracle references of the results that are not
    reproducible run to run; dtype decides the bound."""

    def __init__(self, name, inputs, run, refs=None, dtype=torch.float32, post=None):
        self.name, self.inputs, self.run, self.refs, self.dtype = name, inputs, run, refs, dtype
        self.post = post or (lambda host: host)          # host results -> what is compared (a canonical form)


def side_stream(dev):
    """A non-blocking stream that runs beside the default stream.  The runtime maps streams onto a few hardware queues; a stream that
    shares the default stream's queue would sit behind the blocker whatever the code under test does, so a candidate is vetted with
    a pure-torch op under a 50 ms wait of the default stream first (the same criterion as the harness control)."""
    cal = calibration(dev)
    x = torch.ones(1024, device=dev)
    for _ in range(8):
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        behind = torch.cuda.Event()
        torch.cuda._sleep(int(0.05 * cal["cycles_per_second"]))
        behind.record()
        with torch.cuda.stream(side):
            y = x.mul(2)
        side.synchronize()
        free = not behind.query()
        torch.cuda.synchronize()
        del y
        if free:
            return side
    pytest.skip("no side stream runs beside the default stream on this runtime: the side-stream tests prove nothing here")


def poison_like(x):
    return torch.full_like(x, float("nan")) if x.is_floating_point() else torch.zeros_like(x)


def blocked_side_stream(dev, cases, control=False):
    cal = calibration(dev)
    expected = []
    # 1 (its autograd graphs are dropped before step 2: a graph that lives on keeps the parameters' gradient accumulators, and torch
    #    runs an accumulator on the stream it was made on -- the default stream here, behind the blocker)
    for c in cases:
        first = []
        a, b = (c.post({k: v.detach().cpu() for k, v in c.run({k: v.clone() for k, v in c.inputs.items()}, first).items()})
                for _ in range(2))
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        c.run({k: v.clone() for k, v in c.inputs.items()}, first)
        ev1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        del first
        repro = {k: torch.equal(a[k], b[k]) and k not in TL.ATOMIC_BY_DESIGN for k in a}
        expected.append((a, repro))
        print("STREAMS %s: step 1 takes %.1f ms on the device, %.1f ms with the host; not reproducible: %s"
              % (c.name, ev0.elapsed_time(ev1), wall * 1e3, sorted(k for k, same in repro.items() if not same)))
    # 2
    poisoned = [{k: poison_like(v) for k, v in c.inputs.items()} for c in cases]
    keep = []
    side = side_stream(dev)
    torch.cuda.synchronize()
    assert torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev)
    behind = torch.cuda.Event()
    started = time.perf_counter()
    torch.cuda._sleep(int(BLOCKER_SECONDS * cal["cycles_per_second"]))
    behind.record()
    # 3
    got = []
    with torch.cuda.stream(side):
        for c, p in zip(cases, poisoned):
            acc = cal["big"]
            for _ in range(cal["matmuls"]):
                acc = acc @ cal["big"] * 1e-2                    # queued producer work
            keep.append(acc)
            for k, v in p.items():
                v.copy_(c.inputs[k])
            got.append(c.post({k: v.detach().cpu() for k, v in c.run(p, keep).items()}))
    # 4
    still_blocked = not behind.query()
    elapsed = time.perf_counter() - started
    # 6 (before any assertion: nothing stays queued behind a failure)
    torch.cuda.synchronize()
    del keep
    if control:
        return still_blocked, elapsed, got, expected
    assert still_blocked, ("the default stream's blocker had ended after %.2f s: %s" % (
        elapsed, "the calls waited for the default stream or for the whole device" if elapsed >= 0.9 * BLOCKER_SECONDS
        else "inconclusive, the blocker ended early"))
    # 5
    for c, g, (want, repro) in zip(cases, got, expected):
        same_results(c.name, g, want, repro, c.refs, c.dtype)
    return elapsed


def same_results(name, got, want, repro, refs_of, dtype=torch.float32):
    """Step 5: bit for bit where the default-stream call is reproducible run to run, the oracle bound otherwise."""
    assert set(got) == set(want), name
    refs = None
    for k in got:
        if repro[k] and k not in TL.ATOMIC_BY_DESIGN:
            assert torch.equal(got[k].cpu(), want[k].cpu()), (name, k, "differs from the default-stream call")
        else:
            if refs is None:
                assert refs_of is not None, (name, k, "not reproducible run to run and no oracle reference")
                refs = refs_of(want)
            assert k in refs, (name, k, "not reproducible run to run and no oracle reference")
            e = relerr(got[k].cpu().numpy(), refs[k])
            assert e <= (F64_BOUND if dtype == torch.float64 else F32_BOUND), (name, k, e)


def test_harness_control(dev):
    """x.mul(2).cumsum(0).cpu() through steps 2-6, and a pure-torch backward: both leave the blocker running and give the right
    values.  The outcome is kept for the other tests of the file."""
    x = torch.randint(-8, 9, (100_000,), device=dev).double()          # whole numbers: the scan is exact in any order of summation
    chain = Case("control chain", {"x": x}, lambda i, keep: {"y": i["x"].mul(2).cumsum(0)})

    def backward(i, keep):
        xl = i["x"].requires_grad_()
        y = (xl * xl).sum()
        y.backward()
        keep.append(y)
        return {"g": xl.grad}

    blocked, elapsed, got, expected = blocked_side_stream(dev, [chain, Case("control backward", {"x": x}, backward)], control=True)
    _STATE["control"] = (blocked, elapsed)
    print("STREAMS harness control: blocker still running after the side stream drained: %s (%.3f s after its launch)" % (blocked, elapsed))
    if not blocked:
        pytest.skip("harness control: a pure-torch chain on a side stream waits for the default stream on this runtime (%.2f s)" % elapsed)
    assert elapsed < 0.5 * BLOCKER_SECONDS
    for g, (want, _) in zip(got, expected):
        for k in g:
            assert torch.equal(g[k], want[k])


@pytest.fixture()
def harness(dev):
    if "control" not in _STATE:
        test_harness_control(dev)
    if not _STATE["control"][0]:
        pytest.skip("harness control failed step 4 on this runtime: the side-stream tests prove nothing here")
    return lambda cases: blocked_side_stream(dev, cases)


# ---- graph builds --------------------------------------------------------------------------------------------------------------
def graph_results(g, nnz=None, ef=False):
    res = {"rowptr": g.rowptr, "col": g.col[:nnz], "perm": g.perm, "meta": g._meta}
    if g.w is not None:
        res["w"] = g.w[:nnz]
    if g.invperm is not None:
        res["invperm"] = g.invperm
    if ef:
        res["ef"], res["slot"] = g.ef[:nnz], g.slot_of_edge
    return res


def canonical_graph(host):
    """perm lists the rows bin by bin, in any order inside a bin (the builds place them with atomics): sorted inside every bin here;
    invperm must invert perm and is dropped."""
    from fsw_gnn_amd import _lib
    host = dict(host)
    perm = host["perm"].clone()
    bins = host["meta"][_lib.NUM_STATS:_lib.NUM_STATS + _lib.NUM_BINS + 1].tolist()
    assert bins[0] == 0 and bins[-1] == perm.numel() and all(a <= b for a, b in zip(bins[:-1], bins[1:]))
    for a, b in zip(bins[:-1], bins[1:]):
        perm[a:b] = perm[a:b].sort().values
    if "invperm" in host:
        inv = host.pop("invperm").long()
        assert torch.equal(inv[host["perm"].long()], torch.arange(perm.numel())), "invperm does not invert perm"
    host["perm"] = perm
    return host


def test_csr_builds(dev, harness):
    """build_csr with algo 'lsd' and 'two_level' (weighted), the packed plan (unit weights, 32768 rows, 262144 edges), and
    build_csr_coalesced with edge features."""
    import ctypes
    from fsw_gnn_amd import _lib
    from fsw_gnn_amd.graph import build_csr, build_csr_coalesced
    ei = LC.array("edge_index")
    E = ei.shape[1]
    inp = {"rec": t(ei[1], dev), "snd": t(ei[0], dev), "w": t(LC.array("wvals")[LC.array("perm")], dev)}
    cases = [Case("build_csr " + algo, inp, lambda i, keep, algo=algo: graph_results(
        build_csr(i["rec"], i["snd"], i["w"], N, N, want_invperm=True, algo=algo)), post=canonical_graph) for algo in ("lsd", "two_level")]
    rows, edges = 32_768, 262_144
    words = (ctypes.c_int32 * 8)()
    assert _lib.lib().fsw_graph_build_plan(rows, rows, edges, 0, words) == 0 and words[0] == 1 and words[1] == 1      # two_level, packed
    rng = np.random.default_rng(91)
    big = {"rec": t(rng.integers(0, rows, edges), dev), "snd": t(rng.integers(0, rows, edges), dev)}
    cases.append(Case("build_csr packed", big, lambda i, keep: graph_results(build_csr(i["rec"], i["snd"], None, rows, rows, algo="two_level")),
                      post=canonical_graph))
    # parallel edges: every third edge twice
    rec2, snd2 = np.concatenate([ei[1], ei[1][::3]]), np.concatenate([ei[0], ei[0][::3]])
    ef = LC.array("edge_features")
    co = {"rec": t(rec2, dev), "snd": t(snd2, dev), "w": t(np.ones(rec2.size, dtype=np.float32), dev),
          "ef": t(np.concatenate([ef, ef[::3]]), dev)}
    cases.append(Case("build_csr_coalesced", co, lambda i, keep: graph_results(
        build_csr_coalesced(i["rec"], i["snd"], i["w"], i["ef"], N, N, want_slots=True), nnz=E, ef=True), post=canonical_graph))
    harness(cases)


@pytest.mark.parametrize("idx", ["i32", "i64"])
def test_import_csr_and_sender_major(dev, harness, idx):
    """import_csr with self loops and 'gcn' weights; CSRGraph.sender_major() of the imported graph (its stats read waits for the side
    stream only)."""
    from fsw_gnn_amd.graph import import_csr
    inp = {"rowptr": t(LC.array("rowptr_" + idx), dev), "col": t(LC.array("col_" + idx), dev), "w": t(LC.array("wvals"), dev)}

    def run(i, keep):
        g = import_csr(i["rowptr"], i["col"], i["w"], N, N, self_loop_weight=0.5, gcn=True, want_invperm=True)
        keep.append(g)
        res = graph_results(g)
        res["cptr"], res["order"] = g.sender_major()
        return res

    harness([Case("import_csr " + idx, inp, run, post=canonical_graph)])


# ---- layers --------------------------------------------------------------------------------------------------------------------
def train_step(call, params, inputs, grad_inputs, R, keep):
    """Forward, sum(out * R).backward(); the output, the gradients of the inputs named in grad_inputs and of the parameters."""
    for p in params.values():
        p.grad = None
    leaves = {k: inputs[k].requires_grad_() for k in grad_inputs}
    y = call(inputs)
    keep.append(y)                                          # and with it the autograd graph and what its nodes hold
    (y * R).sum().backward()
    res = {"out": y.detach()}
    res.update({"g_" + k: v.grad for k, v in leaves.items()})
    res.update({"g_" + k: p.grad for k, p in params.items() if p.requires_grad})
    return res


def embedding_case(dev, name, E, inputs, call, rowptr, col, w, train=True, ef=None, dtype=torch.float32, Xkey="X"):
    rows = rowptr.size - 1
    R = TL.weights_for((rows, E.d_out))
    Rd = t(R, dev, dtype)
    Xn = inputs[Xkey].cpu().numpy()

    def refs(expected):
        r = TL.embedding_refs(E, Xn.reshape(-1, Xn.shape[-1]), rowptr, col, w, R, ef=ef, dev=dev, gX_shape=Xn.shape)
        r.pop("g_ef", None)
        return r

    if train:
        run = lambda i, keep: train_step(lambda v: call(v).reshape(rows, E.d_out), TL.params_of(E), i, (Xkey,), Rd, keep)
    else:
        def run(i, keep):
            with torch.no_grad():
                return {"out": call(i)}
    return Case(name, inputs, run, refs, dtype)


@pytest.mark.parametrize("cart", [False, True], ids=["diagonal", "cartesian"])
def test_embedding_forward_and_backward(dev, harness, cart):
    """Unit and general weights and edge features, forward and backward; Cartesian mode includes one cloud of 40 000 points (the
    split forms of the longest lines, forward and backward) with unit and with 'uniform' weights."""
    g = LC.graph()
    idx = t(np.stack([g["rec"], g["col"]]), dev)
    wv, ef = LC.array("wvals"), LC.array("efvals")
    B, n = LC.CLOUDS, LC.CLOUD_POINTS
    Eu = TL.embedding(dev, 12, cart)
    cases = [embedding_case(dev, "unit (clouds)", Eu, {"X": t(LC.array("Xb12"), dev)}, lambda v: Eu(v["X"], "unit"),
                            np.arange(B + 1, dtype=np.int64) * n, np.arange(B * n, dtype=np.int64), None)]
    Ew = TL.embedding(dev, 12, cart)
    call = lambda v: Ew(v["X"], torch.sparse_coo_tensor(idx, v["w"], (N, N), is_coalesced=True), graph_mode=True)
    cases.append(embedding_case(dev, "weighted", Ew, {"X": t(LC.array("X12"), dev), "w": t(wv, dev)}, call, g["rowptr"], g["col"], wv))
    Ee = TL.embedding(dev, 12, cart, d_edge=LC.D_EDGE)
    inp = {"X": t(LC.array("X12"), dev), "w": t(wv, dev), "ef": t(ef, dev)}
    call = lambda v: Ee(v["X"], torch.sparse_coo_tensor(idx, v["w"], (N, N), is_coalesced=True),
                        torch.sparse_coo_tensor(idx, v["ef"], (N, N, LC.D_EDGE), is_coalesced=True), graph_mode=True)
    cases.append(embedding_case(dev, "edge features", Ee, inp, call, g["rowptr"], g["col"], wv, ef=ef))
    harness(cases)
    if cart:
        n = 40_000
        X = TL.cases.synth.features(n, 7, seed=92)
        cloud = []
        for W in ("unit", "uniform"):
            E = TL.embedding(dev, 7, True)
            w = None if W == "unit" else np.full(n, 1.0 / n)
            cloud.append(embedding_case(dev, "cloud of 40000 " + W, E, {"X": t(X, dev)}, lambda v, E=E, W=W: E(v["X"], W),
                                        np.array([0, n], dtype=np.int64), np.arange(n, dtype=np.int64), w))
        harness(cloud)
        # the shape is there for the split forms of the longest lines: the policy takes them, forward and backward, in both weight modes
        from fsw_gnn_amd.graph import build_csr
        rec, snd = torch.zeros(n, dtype=torch.int64, device=dev), torch.arange(n, device=dev)
        for w, forms in ((None, ("_cart_split", "_cart_split_backward")), (torch.full((n,), 1.0 / n, device=dev), ("_cart_split_w", "_cart_split_w_backward"))):
            graph = build_csr(rec, snd, w, 1, n)
            st = graph.read_stats()
            assert all(getattr(E, form)(graph, st) > 0 for form in forms), forms


def test_embedding_float64_generic(dev, harness):
    E = TL.embedding(dev, 12, dtype=torch.float64)
    g = LC.graph()
    idx = t(np.stack([g["rec"], g["col"]]), dev)
    inp = {"X": t(LC.array("X12_f64"), dev), "w": t(LC.array("wvals_f64"), dev)}
    call = lambda v: E(v["X"], torch.sparse_coo_tensor(idx, v["w"], (N, N), is_coalesced=True), graph_mode=True)
    harness([embedding_case(dev, "float64 generic", E, inp, call, g["rowptr"], g["col"], LC.array("wvals"), dtype=torch.float64)])


def conv_case(dev, name, C, tag="", train=False):
    ei = LC.array("edge_index" + tag)
    inp = {"X": t(LC.array("X12"), dev), "ei": t(ei, dev)}
    R = TL.weights_for((N, 16))
    Rd = t(R, dev, torch.float32)

    def refs(expected):
        return TL.conv_refs(C, LC.array("X12"), ei, R, dev=dev, control={"out": expected["out"]})

    if train:
        run = lambda i, keep: train_step(lambda v: C(v["X"], v["ei"]), TL.conv_params(C), i, ("X",), Rd, keep)
    else:
        def run(i, keep):
            with torch.no_grad():
                return {"out": C(i["X"], i["ei"])}
    return Case(name, inp, run, refs)


def test_conv_fused_inference(dev, harness):
    """The fused kernel on rows of at most 32 neighbours: projection, unit coefficient table, one kernel for the embedding and the
    first Linear layer.  Alone under its blocker.  (The test the null-stream variant of the fsw_unit_coeff_table launch fails.)"""
    C = TL.conv_layer(dev, 12)
    assert C._fusable()
    harness([conv_case(dev, "fused", C, "_short")])


def test_conv_inference(dev, harness):
    """Fused with the long rows finished, fuse_linear = False, the Cartesian fused kernel, Cartesian with long rows."""
    fused_long, unfused = TL.conv_layer(dev, 12), TL.conv_layer(dev, 12)
    unfused.fuse_linear = False
    cart, cart_long = (TL.conv_layer(dev, 12, embed_slices=TL.S_CART, embed_freqs=TL.F_CART) for _ in range(2))
    assert fused_long._fusable() and cart._fusable() and not unfused._fusable()
    harness([conv_case(dev, "fused, long rows finished", fused_long), conv_case(dev, "fuse_linear=False", unfused),
             conv_case(dev, "Cartesian fused", cart, "_short"), conv_case(dev, "Cartesian, long rows", cart_long)])


def test_conv_training_store_and_sum(dev, harness):
    """Training with store_sum_backward_max_bytes at its default: the key gradients stored, then summed sender by sender over
    sender_major() (k_segment_sum_rows).  (The test the null-stream variant of that launch fails: DESIGN.md.)"""
    C = TL.conv_layer(dev, 12)
    C.cache_graph = True           # the graph and its sender-major lists stay with the layer until the test ends
    case = conv_case(dev, "training, store and sum", C, train=True)
    harness([case])


def test_conv_training_atomic_backward(dev, harness):
    """Training with store_sum_backward_max_bytes = 0 (float atomics), and Cartesian training."""
    C = TL.conv_layer(dev, 12)
    C.fsw_embed.store_sum_backward_max_bytes = 0
    cart = TL.conv_layer(dev, 12, embed_slices=TL.S_CART, embed_freqs=TL.F_CART)
    harness([conv_case(dev, "training, store_sum_backward_max_bytes = 0", C, train=True),
             conv_case(dev, "Cartesian training", cart, train=True)])


def test_readout_gemm_tn_and_segcumsum(dev, harness):
    """FSW_readout with ptr (forward and backward), gemm_tn at K = 65 536 x 40 x 17, segcumsum forward and reverse."""
    from fsw_gnn_amd import FSW_readout, segcumsum
    from fsw_gnn_amd.fsw_embedding import gemm_tn
    ro = TL.conv_layer(dev, 12, cls=FSW_readout, concat_self=False)
    sizes = LC.READOUT_SIZES
    R = TL.weights_for((len(sizes), 16))
    Rd = t(R, dev, torch.float32)
    cases = [Case("readout ptr", {"X": t(LC.array("X12"), dev), "ptr": t(LC.array("ptr_i32"), dev)},
                  lambda i, keep: train_step(lambda v: ro(v["X"], ptr=v["ptr"]), TL.conv_params(ro), i, ("X",), Rd, keep),
                  lambda expected: TL.readout_refs(ro, R, dev, expected))]
    rng = np.random.default_rng(93)
    A, B = rng.standard_normal((65_536, 40)).astype(np.float32), rng.standard_normal((65_536, 17)).astype(np.float32)
    cases.append(Case("gemm_tn", {"A": t(A, dev), "B": t(B, dev)}, lambda i, keep: {"C": gemm_tn(i["A"], i["B"])},
                      lambda expected: {"C": A.astype(np.float64).T @ B.astype(np.float64)}))
    ids = np.cumsum(rng.random(300_000) < 0.01).astype(np.int64)
    vals = rng.standard_normal(300_000).astype(np.float32)
    for reverse in (False, True):
        cases.append(Case("segcumsum reverse=%s" % reverse, {"v": t(vals, dev), "ids": t(ids, dev)},
                          lambda i, keep, reverse=reverse: {"scan": segcumsum(i["v"], i["ids"], reverse=reverse)}))
    harness(cases)


def conv_training_expected(dev, C):
    """The default-stream training step of layer C on the test graph, twice: inputs, loss weights, results, which are reproducible,
    and the oracle of the others."""
    X, ei = t(LC.array("X12"), dev), t(LC.array("edge_index"), dev)
    R = TL.weights_for((N, 16))
    Rd = t(R, dev, torch.float32)
    keep = []
    step = lambda layer: train_step(lambda v: layer(v["X"], v["ei"]), TL.conv_params(layer), {"X": X.clone(), "ei": ei}, ("X",), Rd, keep)
    a, b = ({k: v.detach().clone() for k, v in step(C).items()} for _ in range(2))
    torch.cuda.synchronize()
    keep.clear()             # drop the graphs: the parameters' gradient accumulators go with them (blocked_side_stream, step 1)
    repro = {k: torch.equal(a[k], b[k]) for k in a}
    refs = lambda want: TL.conv_refs(C, LC.array("X12"), LC.array("edge_index"), R, dev=dev, control={"out": want["out"]})
    return X, ei, Rd, step, a, repro, refs


def test_one_graph_two_streams(dev, harness):
    """cache_graph=True: forward and backward on `side`, then other.wait_stream(side) and forward and backward again on a second
    side stream with the cached graph and its cached sender_major(); both equal the fresh-graph results of the default stream."""
    C = TL.conv_layer(dev, 12)
    X, ei, Rd, step, want, repro, refs = conv_training_expected(dev, C)              # cache_graph off: a fresh graph per call
    C.cache_graph = True
    cal = calibration(dev)
    side, other = side_stream(dev), side_stream(dev)
    assert side != other
    torch.cuda.synchronize()
    behind = torch.cuda.Event()
    torch.cuda._sleep(int(BLOCKER_SECONDS * cal["cycles_per_second"]))
    behind.record()
    got = []
    with torch.cuda.stream(side):
        got.append({k: v.detach().clone() for k, v in step(C).items()})
    graph = C._graph_cache[2]
    other.wait_stream(side)
    with torch.cuda.stream(other):
        got.append({k: v.detach().cpu() for k, v in step(C).items()})
    hit = C._graph_cache[2] is graph and graph._sender_major is not None
    side.synchronize()
    still_blocked = not behind.query()
    torch.cuda.synchronize()
    assert still_blocked, "the calls waited for the default stream or for the whole device (or the blocker ended early)"
    assert hit, "the second call did not take the cached graph and its sender-major lists"
    for i, g in enumerate(got):
        same_results("stream %d of two" % i, g, want, repro, refs)


def test_backward_from_the_default_stream_context(dev, harness):
    """loss.backward() called from the default-stream context after a forward on `side`, no blocker (torch's engine makes the
    default stream wait for the backward): the gradients equal the default-stream call's."""
    C = TL.conv_layer(dev, 12)
    X, ei, Rd, step, want, repro, refs = conv_training_expected(dev, C)
    params = TL.conv_params(C)
    for p in params.values():
        p.grad = None
    side = torch.cuda.Stream(device=dev)
    Xl = X.clone().requires_grad_()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        y = C(Xl, ei)
        loss = (y * Rd).sum()
    loss.backward()
    got = {"out": y.detach(), "g_X": Xl.grad}
    got.update({"g_" + k: p.grad for k, p in params.items()})
    side.synchronize()
    torch.cuda.current_stream(dev).synchronize()
    same_results("backward from the default-stream context", got, want, repro, refs)
    torch.cuda.synchronize()
