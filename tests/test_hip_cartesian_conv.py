"""FSW_conv / FSW_readout with a Cartesian embedding (embed_slices = S slices x embed_freqs = F frequencies) on the GPU.

The anchor needs no fixture: a Cartesian layer equals the diagonal layer with embed_dim = S F + mass, projVecs repeated F times
(repeat_interleave(F, 0)), freqs tiled S times and the same tail weights, and the diagonal layer is pinned to the reference
(testconv64.npz, conv10k.npz, grads_*.npz).  The float64 Cartesian layer is compared with that expanded diagonal layer at 1e-10;
every float32 path (fused kernel, unfused kernels, training, readout) is compared with the float64 Cartesian layer at the project's
bounds, 1e-5 norm-wise for outputs and 3e-5 for gradients (F32_BOUND of test_hip_cartesian_train.py).  Every
test prints the errors it measured before it asserts."""
import numpy as np
import pytest
import torch

from fsw_gnn_amd import FSW_conv, FSW_readout, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FWD_BOUND, F32_BOUND, F64_BOUND = 1e-5, 3e-5, 1e-10
LONG_DEGREES = (33, 64, 65, 2048, 2049)


def relerr(a, b):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _graph(long_rows):
    """Graph A (long_rows=False): 33 recipients of every in-degree 0..32 -- one full 32-row tile and one tile of a single row per
    degree -- and one more of degree 7, recipient ids scattered over the nodes, every fifth recipient with a parallel edge, 1090
    nodes (not a multiple of 32).  Graph B: five more nodes that receive 33, 64, 65, 2048 and 2049 edges.  Senders are drawn from
    the nodes that receive something, so that 'gcn' weights are finite without self loops."""
    degs = [d for d in range(33) for _ in range(33)] + [7]
    if long_rows:
        degs += list(LONG_DEGREES)
    n = len(degs)
    order = np.argsort(synth.randint(11, 1, 1 << 40, n), kind="stable")       # recipient of degs[i] is node order[i]
    pool = np.array([order[i] for i, d in enumerate(degs) if d > 0], dtype=np.int64)
    src, dst = [], []
    for i, d in enumerate(degs):
        s = pool[synth.randint(12, 2 + i, len(pool), d)]
        if d >= 2 and i % 5 == 0:
            s[1] = s[0]                                                        # a parallel edge
        src.append(s)
        dst.append(np.full(d, order[i], dtype=np.int64))
    ei = np.stack([np.concatenate(src), np.concatenate(dst)])
    return n, torch.from_numpy(ei).to(DEV)


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = _graph(name == "B")
    return _GRAPHS[name]


def test_graphs_have_the_degrees_the_tests_rely_on():
    for name, extra in (("A", ()), ("B", LONG_DEGREES)):
        n, ei = graph(name)
        deg = torch.bincount(ei[1], minlength=n).cpu().numpy()
        counts = np.bincount(deg)
        assert n % 32 != 0 and n <= 4000
        assert all(counts[d] == (34 if d == 7 else 33) for d in range(33))
        assert sorted(deg[deg > 32].tolist()) == list(extra)
        pairs = ei.t().cpu().numpy()
        assert len(np.unique(pairs, axis=0)) < len(pairs)                      # parallel edges


def features(n, d, seed=21, dtype=torch.float64):
    return torch.from_numpy(synth.features(n, d, seed=seed, dtype=np.float64)).to(DEV).to(dtype)


def make_pair(cls, in_ch, out_ch, S, F, zero_freq=True, **kw):
    """(float64 layer, float32 layer) with the same parameters; one frequency is 0 (the linear readout).

    The 'spread' frequencies k / (2 F - k) hold integers (15 at F = 8); at an integer frequency the readout of every row whose
    degree divides twice that integer is exactly 0, where the |.| of the 'homog' encodings has a kink and float32 and float64 land
    on different sides of it.  The frequencies are scaled off those points: the tests compare derivatives where they exist."""
    torch.manual_seed(1234)
    kw.setdefault("message_weight_vs_self", 0.5)
    ref = cls(in_ch, out_ch, embed_slices=S, embed_freqs=F, device=DEV, dtype=torch.float64, **kw)
    with torch.no_grad():
        ref.fsw_embed.freqs.mul_(0.937)
        if zero_freq:
            ref.fsw_embed.freqs[F // 2] = 0.0
        if ref.fsw_embed.enable_bias:
            ref.fsw_embed.bias.copy_(0.1 * torch.randn_like(ref.fsw_embed.bias))
    low = cls(in_ch, out_ch, embed_slices=S, embed_freqs=F, device=DEV, dtype=torch.float32, **kw)
    low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ref.eval(), low.eval()
    return ref, low


def expanded_diagonal(cart, cls, in_ch, out_ch, **kw):
    """The diagonal float64 layer that computes what the Cartesian layer `cart` computes."""
    S, F = cart.fsw_embed.nSlices, cart.fsw_embed.nFreqs
    diag = cls(in_ch, out_ch, embed_dim=cart.embed_dim, device=DEV, dtype=torch.float64, **kw)
    sd = dict(cart.state_dict())
    sd["fsw_embed.projVecs"] = sd["fsw_embed.projVecs"].repeat_interleave(F, 0)
    sd["fsw_embed.freqs"] = sd["fsw_embed.freqs"].repeat(S)
    diag.load_state_dict(sd)
    return diag


class FusedCalls:
    """Counts the launches of the fused Cartesian entry by wrapping the method that makes them."""

    def __init__(self, monkeypatch):
        self.count = 0
        inner = FSW_conv._fused_cart_linear

        def wrapped(layer, *args, **kwargs):
            self.count += 1
            return inner(layer, *args, **kwargs)

        monkeypatch.setattr(FSW_conv, "_fused_cart_linear", wrapped)


# ---- 1. float64: the Cartesian layer is the expanded diagonal layer ----------------------------------------------------------------
def test_float64_cartesian_layer_equals_expanded_diagonal_layer():
    S, F, in_ch, out_ch = 3, 5, 5, 7
    n, ei = graph("B")
    kw = dict(message_weight_vs_self=0.5, learnable_vertex_degree_encoding_scale=True)
    torch.manual_seed(7)
    cart = FSW_conv(in_ch, out_ch, embed_slices=S, embed_freqs=F, device=DEV, dtype=torch.float64, **kw)
    with torch.no_grad():
        cart.fsw_embed.freqs[2] = 0.0
    diag = expanded_diagonal(cart, FSW_conv, in_ch, out_ch, **kw)
    assert tuple(cart.fsw_embed.projVecs.shape) == (S, in_ch) and tuple(cart.fsw_embed.freqs.shape) == (F,)
    assert cart.embed_dim == S * F + 1 == diag.embed_dim and cart.mlp[0].in_features == S * F + 1 + in_ch
    G = features(n, out_ch, seed=31)
    outs, grads = [], []
    for layer in (cart, diag):
        x = features(n, in_ch).requires_grad_(True)
        y = layer(x, ei)
        (y * G).sum().backward()
        e = layer.fsw_embed
        gv, gf = e.projVecs.grad, e.freqs.grad
        if layer is diag:
            gv, gf = gv.reshape(S, F, in_ch).sum(1), gf.reshape(S, F).sum(0)
        outs.append(y)
        grads.append({"x": x.grad, "projVecs": gv, "freqs": gf, "mlp.0.weight": layer.mlp[0].weight.grad})
    errs = {"out": relerr(outs[0], outs[1]), **{k: relerr(grads[0][k], grads[1][k]) for k in grads[0]}}
    print("float64 Cartesian vs expanded diagonal:", errs)
    assert max(errs.values()) < F64_BOUND, errs


# ---- 2. fused forward -----------------------------------------------------------------------------------------------------------------
LEAKY, RELU = torch.nn.LeakyReLU(negative_slope=0.2), torch.nn.ReLU()
# (S, F, mass, in_channels, width of the first Linear layer, activation behind it, mlp_layers): K = 257, 15, 141, 141 -- K padding,
# F % 4 != 0, S above one wavefront; Hout 7 (partial slab), 128 (staged epilogue), 160 (wide epilogue)
FUSED_CASES = [
    (16, 16, True, 128, 128, LEAKY, 1),
    (16, 16, True, 5, 160, RELU, 2),
    (3, 5, False, 5, 7, None, 1),
    (3, 5, False, 128, 128, RELU, 2),
    (2, 70, True, 5, 160, None, 1),
    (2, 70, True, 128, 7, LEAKY, 2),
    (70, 2, True, 5, 128, RELU, 1),
    (70, 2, True, 128, 160, LEAKY, 1),
    (16, 16, True, 5, 7, None, 2),
]


@pytest.mark.parametrize("S,F,mass,in_ch,hout,act,layers", FUSED_CASES)
def test_fused_forward_float32(monkeypatch, S, F, mass, in_ch, hout, act, layers):
    n, ei = graph("A")
    kw = dict(encode_vertex_degrees=mass, mlp_layers=layers)
    if layers == 1:
        out_ch, kw["mlp_activation_final"] = hout, act
    else:
        out_ch, kw["mlp_hidden_dim"], kw["mlp_activation_hidden"] = 9, hout, act
    ref, low = make_pair(FSW_conv, in_ch, out_ch, S, F, **kw)
    assert low.mlp[0].out_features == hout and low.mlp[0].in_features == S * F + int(mass) + in_ch
    x64 = features(n, in_ch)
    x = x64.float()
    calls = FusedCalls(monkeypatch)
    with torch.no_grad():
        want = ref(x64, ei)
        assert calls.count == 0                       # the float64 layer runs the generic kernel
        fused = low(x, ei)
        assert calls.count == 1, "the fused entry did not run"
        low.fuse_linear = False
        unfused = low(x, ei)
        assert calls.count == 1, "fuse_linear=False still ran the fused entry"
    errs = (relerr(fused, want), relerr(unfused, want), relerr(fused, unfused))
    print("fused / unfused vs float64, fused vs unfused:", errs)
    assert max(errs) < FWD_BOUND, errs


# ---- 3. configurations and graphs that take the unfused kernels -----------------------------------------------------------------------
def _batchnorm_first(layer):
    bn = torch.nn.BatchNorm1d(layer.mlp[0].in_features, device=DEV, dtype=layer.mlp[0].weight.dtype)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g))
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(bn.num_features, generator=g))
    layer.mlp = torch.nn.Sequential(bn, *layer.mlp)
    layer.eval()


UNFUSED_CASES = {
    "long rows": ("B", 4, 8, 6, 8, {}),
    "tile too wide for LDS": ("A", 64, 16, 5, 7, {}),
    "mlp_layers=0, concat_self": ("A", 4, 8, 6, 8, dict(mlp_layers=0)),
    "mlp_layers=0, no concat_self": ("A", 4, 8, 6, 33, dict(mlp_layers=0, concat_self=False)),
    "gcn with self loops": ("A", 4, 8, 6, 8, dict(edge_weighting="gcn", self_loop_weight=1)),
    "pad threshold 3": ("A", 4, 8, 6, 8, dict(vertex_degree_pad_thresh=3)),
    "homog": ("A", 4, 8, 6, 8, dict(homog_degree_encoding=True)),
    "homog, mlp_layers=0": ("A", 3, 5, 6, 8, dict(homog_degree_encoding=True, mlp_layers=0)),
    "BatchNorm first": ("A", 4, 8, 6, 8, dict(_bn_first=True)),
}


@pytest.mark.parametrize("case", list(UNFUSED_CASES))
def test_unfused_routing_float32(monkeypatch, case):
    gname, S, F, in_ch, out_ch, kw = UNFUSED_CASES[case]
    kw = dict(kw)
    bn_first = kw.pop("_bn_first", False)
    n, ei = graph(gname)
    ref, low = make_pair(FSW_conv, in_ch, out_ch, S, F, **kw)
    if bn_first:
        _batchnorm_first(ref), _batchnorm_first(low)
        low.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    x64 = features(n, in_ch)
    calls = FusedCalls(monkeypatch)
    with torch.no_grad():
        want = ref(x64, ei)
        got = low(x64.float(), ei)
    assert calls.count == 0, "the fused entry ran"
    assert tuple(got.shape) == (n, out_ch)
    err = relerr(got, want)
    print("unfused (%s) vs float64: %.3g" % (case, err))
    assert err < FWD_BOUND, err


# ---- 4. training ----------------------------------------------------------------------------------------------------------------------
def _loss_grads(layer, x, G, *args):
    x = x.clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    y = layer(x, *args)
    (y * G.to(y.dtype)).sum().backward()
    grads = {"x": x.grad}
    for name, p in layer.named_parameters():
        if p.requires_grad and name != "size_coeff":          # size_coeff is never used in forward (as in the reference)
            assert p.grad is not None, name
            grads[name] = p.grad
    return y, grads


@pytest.mark.parametrize("weighting", ["unit", "gcn"])
@pytest.mark.parametrize("homog", [False, True])
def test_training_float32(weighting, homog):
    S, F, in_ch, out_ch = 4, 8, 6, 8
    n, ei = graph("B")
    ref, low = make_pair(FSW_conv, in_ch, out_ch, S, F, mlp_layers=2, edge_weighting=weighting, homog_degree_encoding=homog,
                         learnable_vertex_degree_encoding_scale=True)
    x64, G = features(n, in_ch), features(n, out_ch, seed=33)
    want_y, want = _loss_grads(ref, x64, G, ei)
    got_y, got = _loss_grads(low, x64.float(), G, ei)
    assert set(got) == set(want) and {"fsw_embed.projVecs", "fsw_embed.freqs", "fsw_embed.total_mass_encoding_scale",
                                      "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"} <= set(got)
    errs = {"out": relerr(got_y, want_y), **{k: relerr(got[k], want[k]) for k in want}}
    print("training (%s, homog=%s) vs float64:" % (weighting, homog), errs)
    assert errs.pop("out") < FWD_BOUND
    assert max(errs.values()) < F32_BOUND, errs


# ---- 5. readout -----------------------------------------------------------------------------------------------------------------------
def test_readout():
    S, F, in_ch, out_ch = 4, 8, 6, 8
    sizes = {0: 1, 1: 40, 3: 2100}                    # graph id 2 stays empty
    gi = torch.cat([torch.full((m,), g, dtype=torch.int64) for g, m in sizes.items()])
    gi = gi[torch.randperm(gi.numel(), generator=torch.Generator().manual_seed(5))].to(DEV)
    n = gi.numel()
    kw = dict(concat_self=False, mlp_layers=2, learnable_vertex_degree_encoding_scale=True)
    ref, low = make_pair(FSW_readout, in_ch, out_ch, S, F, **kw)
    diag = expanded_diagonal(ref, FSW_readout, in_ch, out_ch, message_weight_vs_self=0.5, **kw)
    x64, G = features(n, in_ch), features(4, out_ch, seed=35)
    want_y, want = _loss_grads(ref, x64, G, gi, 4)
    got_y, got = _loss_grads(low, x64.float(), G, gi, 4)
    diag_y, dg = _loss_grads(diag, x64, G, gi, 4)
    with torch.no_grad():
        inference = low(x64.float(), gi, 4)
    assert tuple(inference.shape) == (4, out_ch)
    dg["fsw_embed.projVecs"] = dg["fsw_embed.projVecs"].reshape(S, F, in_ch).sum(1)
    dg["fsw_embed.freqs"] = dg["fsw_embed.freqs"].reshape(S, F).sum(0)
    e64 = {"out": relerr(want_y, diag_y), **{k: relerr(want[k], dg[k]) for k in want}}
    e32 = {"out": relerr(got_y, want_y), "inference": relerr(inference, want_y), **{k: relerr(got[k], want[k]) for k in want}}
    print("readout float64 vs expanded diagonal:", e64)
    print("readout float32 vs float64:", e32)
    assert max(e64.values()) < F64_BOUND, e64
    assert e32.pop("out") < FWD_BOUND and e32.pop("inference") < FWD_BOUND
    assert max(e32.values()) < F32_BOUND, e32


# ---- 6. state_dict, sharding, edge features ---------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_unsupported_combinations():
    n, ei = graph("A")
    torch.manual_seed(2)
    a = FSW_conv(6, 8, embed_slices=4, embed_freqs=8, device=DEV)
    b = FSW_conv(6, 8, embed_slices=4, embed_freqs=8, device=DEV)
    sd = a.state_dict()
    assert tuple(sd["fsw_embed.projVecs"].shape) == (4, 6) and tuple(sd["fsw_embed.freqs"].shape) == (8,)
    assert "fsw_embed.bias" not in sd                 # the embedding has a bias only without an MLP, as in the diagonal layer
    c = FSW_conv(6, 8, embed_slices=4, embed_freqs=8, mlp_layers=0, device=DEV)
    assert tuple(c.state_dict()["fsw_embed.bias"].shape) == (33,)
    b.load_state_dict(sd)
    x = features(n, 6, dtype=torch.float32)
    with torch.no_grad():
        assert torch.equal(a(x, ei), b(x, ei))
    with pytest.raises(NotImplementedError, match="Cartesian layer.*enable_slice_parallel"):
        a.enable_slice_parallel()
    with pytest.raises(NotImplementedError, match="Cartesian layer.*node-parallel"):
        a.enable_node_parallel()
    a.enable_slice_parallel(enabled=False), a.enable_node_parallel(enabled=False)       # switching off is always allowed
    with pytest.raises(NotImplementedError, match="edge features"):
        FSW_conv(6, 8, edgefeat_dim=2, embed_slices=4, embed_freqs=8, device=DEV)
