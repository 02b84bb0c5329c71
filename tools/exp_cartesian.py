"""Cartesian mode against the diagonal-expansion workaround on the BASELINE config-3 graph (1M nodes, 10M edges, d_in = 128), no_grad
forward on a prebuilt graph:
  (a) Cartesian S = F = 16 (256 output columns)
  (b) the workaround: a diagonal module of 256 slices, projVecs repeated F times, freqs tiled S times (same output)
  (c) the diagonal d_out = 256 headline module (256 distinct slices)
For each: ms per forward, ms of the projection timed alone, and the rest of the forward (coefficient table, zero-degree rows, the
one stats read, the neighbourhood kernel) with the neighbourhood kernel's algorithmic bytes as a fraction of 8 TB/s -- an upper-bound
time, so a lower bound of the fraction.  Byte model of (a)'s kernel: gathers 4 E S + output 4 n S F (+ CSR indices 4 E); (b)/(c):
gathers 4 E 256 + output 4 n 256 (+ 4 E).  The per-kernel split and the name of the dominant kernel come from a kernel trace of one
configuration:
    python tools/exp_cartesian.py [--reps 20] [--only a|b|c]
    rocprofv3 --kernel-trace --stats -d DIR -o cart -- python tools/exp_cartesian.py --only a   (profiles/r04_cartesian_a_kernel_stats.csv)

--train: one float32 TRAINING step (forward + backward, learnable slices and frequencies) instead, HIP events after warm-up:
  graph  the config-3 graph with unit edges, d_in 128, S = F = 16 (graph_w, not in the default: the same graph with general weights,
         a coalesced sparse W through the public forward -- it is timed after, and together with, graph)
  pc     a point-cloud batch of 256 clouds x 1024 points, d_in 3, S = 64, F = 16, W = 'uniform'
A package with the tuned backward (fsw_embedding._CartEmbedFn) takes it; --generic, or a package without it, takes the generic
Cartesian kernel for forward and backward (what every autograd call of Cartesian mode ran on before the tuned backward):
    python tools/exp_cartesian.py --train [--workload graph,pc] [--steps 10] [--warmup 2] [--generic]

--conv: the whole FSW_conv layer on the config-3 graph, in = out = 128, one Linear layer + LeakyReLU, no_grad forward including
the CSR build (what bench.py times), one line per form and run so that runs of different forms can alternate:
  diag     the diagonal layer, embed_dim = S F + 1 (257 slices; runs on a package without the Cartesian layer too)
  unfused  FSW_conv(embed_slices=S, embed_freqs=F) with fuse_linear = False: embed_cartesian_into + two GEMMs
  fused    the same layer on k_conv_fused_cart (csrc/conv_fused.hip)
    python tools/exp_cartesian.py --conv --forms unfused,fused --runs 5 [--reps 20]
    python tools/exp_cartesian.py --conv --train --forms diag,cart [--steps 10]      one training step (forward + backward)
    rocprofv3 --kernel-trace --stats -d DIR -o conv -- python tools/exp_cartesian.py --conv --forms fused --runs 1

--hub: unit-weight rows of 2049 .. 32768 neighbours (csrc/embed_cart_hub.hip, csrc/embed_cart_hub_bwd.hip), forward (no_grad) and one
training step (forward + backward) each:
  readout  FSW_readout(embed_slices=16, embed_freqs=16), one batch of 8 graphs per degree class (2500, 6000, 12000, 24000 vertices)
           and one mixed batch of 2500 .. 30000 vertices
  rmat     FSW_embedding(nSlices=16, nFreqs=16) on the RMAT-20 graph of tools/exp_skew.py (1M nodes, 10M unit edges, prebuilt CSR)
The library is the one FSW_HIP_LIBRARY names (fsw_gnn_amd/_lib.py).  A build from before the hub kernels (no export
fsw_embed_cart_backward_scratch_bytes: a parent commit built in a copy of the tree and copied to _variants/) is driven by the same
host code with the scratch its generic kernel needs for every row above 2048 neighbours, and a build from before
fsw_embed_cart_scratch_bytes with the sizes the host layer chose then, so that builds can alternate on one box:
    python tools/exp_cartesian.py --hub [--workload readout,rmat] --steps 3 --warmup 1
    FSW_HIP_LIBRARY=_variants/libfsw_hip_parent.so python tools/exp_cartesian.py --hub --steps 3 --warmup 1
    rocprofv3 --kernel-trace --stats -d DIR -o hub -- python tools/exp_cartesian.py --hub --workload readout --steps 1
--hub --weights uniform|random [--tau T]: the same batches with general weights -- a weight per vertex, 1 / (vertices of its graph) or
random in (0.05, 1) -- through FSW_embedding(nSlices=16, nFreqs=16) on the readout-shaped CSR graph: lines of 2049 .. 16384 elements run
on csrc/embed_cart_hub_w.hip / csrc/embed_cart_hub_w_bwd.hip, the batch of 24000 vertices on the generic kernel in every build
(--weights unit --tau 3 takes the same kernels with w = NULL); and, workload pc4096, a point-cloud batch of 64 clouds x 4096 points,
d_in 3, S = 64, F = 16, W = 'uniform', through the public forward.  A build from before these classes (no export
fsw_embed_cart_weighted_backward_scratch_bytes) is driven with the generic kernel's scratch for every row of 2048 neighbours and more:
    python tools/exp_cartesian.py --hub --weights uniform [--workload readout,pc4096] --steps 3 --warmup 1
    FSW_HIP_LIBRARY=_variants/libfsw_hip_parent.so python tools/exp_cartesian.py --hub --weights uniform --steps 3 --warmup 1
--giant: the longest rows -- unit weights above 32768 neighbours, general weights from 16384 (csrc/embed_giant_cart.hip,
csrc/embed_giant_cart_w.hip) --, forward (no_grad) and one training step, S = F = --slices / --freqs: batches of 8 graphs x 24 000
weighted and 8 x 40 000 unit vertices, the mixed batch 2500 .. 30000 with weights, one cloud of 150 000 and one of 1 000 000 points,
unit and weighted, and 2 and 4 unit clouds of 150 000.  A build without fsw_embed_cart_backward_keys_scratch_bytes (the generic kernel in the backward of these rows) or
without fsw_embed_cart_forward_scratch_bytes (the generic kernel in both directions) is driven with the scratch
that kernel needs.
The forward of a unit workload with at most fsw_embed_cart_split_max_lines() lines takes the split form (csrc/embed_split_cart.hip: one line
over many workgroups); every line of the output names the form.  --form split | giant forces one form for every unit workload (the
threshold is the host layer's, the library does what the flag says); c150000x2 and c150000x4 are batches of 2 and 4 unit clouds of
150 000 points (32 and 64 lines).  A build without fsw_embed_cart_split_scratch_bytes has the one-workgroup-per-line kernel only.
The backward of such a workload takes its own split form (csrc/embed_split_cart_bwd.hip) up to fsw_embed_cart_split_backward_max_lines()
lines; every line of the output names that form too, --form-bwd split | giant forces one, and a build without
fsw_embed_cart_split_backward_scratch_bytes has the one-workgroup-per-line backward only.
--giant --weights uniform | random: 1, 2, 4, 8, 16 and 32 clouds of 150 000 points (16 .. 512 lines at S = 16) and one cloud of 1 000 000
with a weight per point -- 1 / size of the cloud, or random in (0.05, 1) --: the forward takes the split form of general weights
(csrc/embed_split_cart_w.hip), the backward its own (csrc/embed_split_cart_w_bwd.hip) up to
fsw_embed_cart_split_w_backward_max_lines() lines; --form and --form-bwd force one form here too, and a build without
fsw_embed_cart_split_w_backward_scratch_bytes has the one-workgroup-per-line backward only.
    python tools/exp_cartesian.py --giant [--workload w24000,u40000,mixed,c150000,c150000x2,c150000x4,c1000000] --steps 3 --warmup 1
    python tools/exp_cartesian.py --giant --workload u40000,c150000,c150000x2,c150000x4 --form split     (and --form giant)
    python tools/exp_cartesian.py --giant --workload u40000,c150000x2,c150000x4 --form-bwd split         (and --form-bwd giant)
    python tools/exp_cartesian.py --giant --weights uniform [--workload c150000,c150000x16,c1000000] --form-bwd split   (and giant)
    FSW_HIP_LIBRARY=_variants/libfsw_hip_parent.so python tools/exp_cartesian.py --giant --steps 3 --warmup 1
    rocprofv3 --kernel-trace --stats -d DIR -o giant -- python tools/exp_cartesian.py --giant --workload c150000 --steps 1
--giant --workload splitw: the split form of the longest general-weight rows (csrc/embed_split_cart_w.hip) against the one-workgroup-per-
line kernel of the SAME library, through the C ABI (fsw_embed_cart_f32 with and without FSW_CART_SPLIT_W_LINES on one projection): one
weighted cloud of 1 000 000 points, then 1, 2, 4, .. 32 clouds of 150 000 points (16 .. 512 lines at S = 16; the first is the one cloud of 150 000), --weights
uniform (1 / size of the cloud) | random.  Both forms alternate over --runs runs of --steps calls each, every call on the next of three
(scratch, output) buffer pairs; the medians and the error of one form against the other are printed:
    python tools/exp_cartesian.py --giant --workload splitw --weights uniform --steps 20 --warmup 3 --runs 5
    rocprofv3 --kernel-trace --stats -d DIR -o splitw -- python tools/exp_cartesian.py --giant --workload splitw,c150000 --steps 1 --runs 1
--conv --edge-features D: the Cartesian layer with D features per edge (the keys of the CSR entries from csrc/edge_keys.hip, then the
tuned Cartesian kernels) against its diagonal workaround, the same layer with every slice repeated F times, alternating over --runs runs;
--edge-keys: fsw_edge_keys_f32 alone at 10M entries against a device-to-device copy of the same byte count:
    python tools/exp_cartesian.py --conv --edge-features 4 [--train]
    python tools/exp_cartesian.py --edge-keys --edge-features 4 --slices 16"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from fsw_gnn_amd import FSW_embedding, _lib  # noqa: E402
from fsw_gnn_amd.graph import build_csr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--slices", type=int, default=16)
ap.add_argument("--freqs", type=int, default=16)
ap.add_argument("--only", default="abc", help="subset of the configurations a, b, c to time")
ap.add_argument("--train", action="store_true", help="time one training step (forward + backward) instead of the forwards")
ap.add_argument("--workload", default="graph,pc", help="--train: subset of graph, graph_w, pc; --hub: subset of readout, rmat (default both); "
                "--hub with general weights: subset of readout, pc4096 (default both)")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--generic", action="store_true", help="--train: the generic Cartesian kernel for forward and backward")
ap.add_argument("--conv", action="store_true", help="time the FSW_conv layer (diagonal / Cartesian unfused / Cartesian fused)")
ap.add_argument("--forms", default="unfused,fused", help="--conv: forms to time, alternating over the runs (--train: diag, cart)")
ap.add_argument("--runs", type=int, default=5, help="--conv: runs of every form")
ap.add_argument("--edge-features", type=int, default=0, metavar="D",
                help="--conv: D features per edge; times the Cartesian layer (form cart) against its diagonal workaround, the same layer "
                     "with every slice repeated F times (form diag), alternating over the runs")
ap.add_argument("--edge-keys", action="store_true",
                help="time fsw_edge_keys_f32 at 10M entries, --slices slices, --edge-features (default 4) features against a "
                     "device-to-device copy of the same byte count, alternating over the runs")
ap.add_argument("--hub", action="store_true", help="time the unit-weight hub rows (2049 .. 32768 neighbours), forward and training step")
ap.add_argument("--giant", action="store_true", help="time the longest rows (unit: above 32768 neighbours, weights: from 16384), forward and training step")
ap.add_argument("--weights", choices=("unit", "uniform", "random"), default="unit",
                help="--hub: unit weights (the unit hub kernels), or a weight per vertex: 1 / size of its graph, or random in (0.05, 1)")
ap.add_argument("--form", choices=("auto", "split", "giant"), default="auto",
                help="--giant: the form of the longest unit-weight rows' forward: the host layer's choice, or one form for every line count")
ap.add_argument("--form-bwd", choices=("auto", "split", "giant"), default="auto",
                help="--giant: the form of the longest rows' backward (unit and general weights): the host layer's choice, or one form for every line count")
ap.add_argument("--tau", type=float, default=1.0, help="--hub: total_mass_pad_thresh of the embedding (> 1: general-weight kernels with w = NULL)")
args = ap.parse_args()
dev = torch.device("cuda:0")


def train_leg():
    from fsw_gnn_amd import fsw_embedding as fe
    tuned = hasattr(fe, "_CartEmbedFn") and not args.generic
    path = "tuned kernels (_CartEmbedFn)" if tuned else "generic Cartesian kernel (_GenericEmbedFn)"

    def step_ms(step):
        for _ in range(args.warmup):
            step()
        return bench.timed_ms(step, args.steps, dev) if args.steps > 1 else bench.timed_ms(step, 1, dev)

    def graph_forward(mod, xg, rec, snd, rows):
        """Unit edges (no weight tensor), which the public forward cannot express in graph mode: the module's own Cartesian
        forward on the edge list.  Its signature gained the `train` flag with the tuned backward."""
        if hasattr(fe, "_CartEmbedFn"):
            return mod._forward_cartesian(xg, rec, snd, None, rows, not tuned, tuned, None)
        return mod._forward_cartesian(xg, rec, snd, None, rows, True, None)

    torch.manual_seed(7)
    if "graph" in args.workload:
        n, E, d = bench.N_NODES, bench.N_EDGES, bench.D_FEAT
        xg, ei = bench.make_inputs(n, E, dev)
        order = torch.argsort(ei[1], stable=True)            # the generic path wants the edges sorted by recipient
        rec, snd = ei[1][order].contiguous(), ei[0][order].contiguous()
        mod = FSW_embedding(d_in=d, nSlices=16, nFreqs=16, collapse_freqs=True, enable_bias=False, learnable_slices=True,
                            learnable_freqs=True, freqs_init='spread', device=dev)
        G = torch.randn((n, 256), device=dev)

        def step():
            mod.zero_grad(set_to_none=True)
            graph_forward(mod, xg, rec, snd, n).backward(G)

        print("train graph: n=%d E=%d (unit edges) d_in=%d S=16 F=16, %s: %.3f ms/step" % (n, E, d, path, step_ms(step)), flush=True)
        if "graph_w" in args.workload:      # the same graph with general weights through the public forward (coalesced sparse W)
            W = torch.sparse_coo_tensor(torch.stack([rec, snd]), torch.rand(E, device=dev) + 0.1, (n, n)).coalesce()
            W.requires_grad_(args.generic and hasattr(fe, "_CartEmbedFn"))

            def step_w():
                mod.zero_grad(set_to_none=True)
                mod(xg, W, graph_mode=True).backward(G)

            print("train graph_w: the same graph, general weights, %s: %.3f ms/step" % (path, step_ms(step_w)), flush=True)
            del W
        del xg, ei, rec, snd, G
    if "pc" in args.workload:
        B, npts = 256, 1024
        xc = torch.randn((B, npts, 3), device=dev)
        mod = FSW_embedding(d_in=3, nSlices=64, nFreqs=16, collapse_freqs=True, enable_bias=False, learnable_slices=True,
                            learnable_freqs=True, freqs_init='spread', device=dev)
        G = torch.randn((B, 64 * 16), device=dev)
        # --generic on a package with the tuned backward: only a W that requires grad selects the generic kernel (which then also
        # computes the weight gradient, a reverse cumulative sum per slice on top of what 'uniform' costs there)
        Wc = torch.full((B, npts), 1.0 / npts, device=dev).requires_grad_(True) if (args.generic and hasattr(fe, "_CartEmbedFn")) else 'uniform'

        def step():
            mod.zero_grad(set_to_none=True)
            mod(xc, Wc).backward(G)

        print("train pc: %d clouds x %d points d_in=3 S=64 F=16 W=uniform, %s: %.3f ms/step" % (B, npts, path, step_ms(step)), flush=True)


def edge_keys_leg():
    """fsw_edge_keys_f32 (csrc/edge_keys.hip) against a device-to-device copy that moves the same bytes, nnz (4 + 4 d_edge + 8 S)."""
    L = _lib.lib()
    nnz, n, S, D = 10_000_000, 1_000_000, args.slices, args.edge_features or 4
    ldp, ldk = (S + 31) // 32 * 32, (S + 3) // 4 * 4
    torch.manual_seed(7)
    col = torch.randint(0, n, (nnz,), device=dev, dtype=torch.int32)
    Xp, ef, V = torch.randn((n, ldp), device=dev), torch.randn((nnz, D), device=dev), torch.randn((S, 8 + D), device=dev)
    K = torch.empty((nnz, ldk), device=dev)
    nbytes = nnz * (4 + 4 * D + 8 * S)
    src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def keys():
        _lib.check(L.fsw_edge_keys_f32(_lib.ptr(col), nnz, _lib.ptr(Xp), ldp, _lib.ptr(ef), D, V.data_ptr() + 4 * 8, V.stride(0), S,
                                       _lib.ptr(K), ldk, stream), "fsw_edge_keys_f32")

    print("edge keys: nnz=%d senders=%d S=%d d_edge=%d ldp=%d ldk=%d, %.3f GB per call" % (nnz, n, S, D, ldp, ldk, nbytes / 1e9))
    for run in range(args.runs):
        for name, fn in (("keys", keys), ("copy", lambda: dst.copy_(src))):
            for _ in range(args.warmup if run == 0 else 1):
                fn()
            ms = bench.timed_ms(fn, args.reps, dev)
            print("run %d  %-5s %8.3f ms  %.2f TB/s" % (run, name, ms, nbytes / 1e9 / ms), flush=True)


def conv_edge_leg():
    """The Cartesian layer with edge features against its diagonal workaround (every slice repeated F times, the frequencies tiled S
    times: the same function), on the benchmark's graph."""
    from fsw_gnn_amd import FSW_conv
    n, E, d = bench.N_NODES, bench.N_EDGES, bench.D_FEAT
    S, F, D = args.slices, args.freqs, args.edge_features
    x, ei = bench.make_inputs(n, E, dev)
    torch.manual_seed(7)
    ef = torch.randn((E, D), device=dev)
    cart = FSW_conv(d, d, edgefeat_dim=D, embed_slices=S, embed_freqs=F, cartesian_edge_features=True, learnable_embedding=args.train, device=dev)
    diag = FSW_conv(d, d, edgefeat_dim=D, embed_dim=S * F + 1, learnable_embedding=args.train, device=dev)
    sd = cart.state_dict()
    sd["fsw_embed.projVecs"] = sd["fsw_embed.projVecs"].repeat_interleave(F, dim=0)
    sd["fsw_embed.freqs"] = sd["fsw_embed.freqs"].repeat(S)
    diag.load_state_dict(sd)
    layers = {"cart": cart, "diag": diag}
    print("conv with %d edge features, config 3: n=%d E=%d in=out=%d S=%d F=%d (K = %d)%s" % (
        D, n, E, d, S, F, S * F + 1, ", training step" if args.train else ""))
    with torch.no_grad():
        ya, yb = cart(x, ei, ef), diag(x, ei, ef)
        print("cart against diag: %.2e" % float((ya - yb).norm() / yb.norm()))
        del ya, yb
    if args.train:
        xg = x.clone().requires_grad_(True)
        G = torch.randn((n, d), device=dev)
    for run in range(args.runs):
        for form, layer in layers.items():
            if args.train:
                def step():
                    layer.zero_grad(set_to_none=True)
                    xg.grad = None
                    layer(xg, ei, ef).backward(G)
                for _ in range(args.warmup if run == 0 else 1):
                    step()
                ms = bench.timed_ms(step, args.steps, dev)
            else:
                with torch.no_grad():
                    for _ in range(args.warmup if run == 0 else 1):
                        layer(x, ei, ef)
                    ms = bench.timed_ms(lambda: layer(x, ei, ef), args.reps, dev)
            print("run %d  %-8s %8.3f ms" % (run, form, ms), flush=True)


def conv_leg():
    from fsw_gnn_amd import FSW_conv
    n, E, d = bench.N_NODES, bench.N_EDGES, bench.D_FEAT
    S, F = args.slices, args.freqs
    x, ei = bench.make_inputs(n, E, dev)
    forms = args.forms.split(",")
    layers = {}
    for form in forms:
        torch.manual_seed(7)
        if form == "diag":
            layers[form] = FSW_conv(d, d, embed_dim=S * F + 1, learnable_embedding=args.train, device=dev)
        else:
            layers[form] = FSW_conv(d, d, embed_slices=S, embed_freqs=F, learnable_embedding=args.train, device=dev)
            if form == "unfused":
                layers[form].fuse_linear = False
    print("conv, config 3: n=%d E=%d in=out=%d S=%d F=%d (K = %d)%s" % (n, E, d, S, F, S * F + 1, ", training step" if args.train else ""))
    if args.train:
        xg = x.clone().requires_grad_(True)
        G = torch.randn((n, d), device=dev)
    for run in range(args.runs):
        for form in forms:
            layer = layers[form]
            if args.train:
                def step():
                    layer.zero_grad(set_to_none=True)
                    xg.grad = None
                    layer(xg, ei).backward(G)
                for _ in range(args.warmup if run == 0 else 1):
                    step()
                ms = bench.timed_ms(step, args.steps, dev)
            else:
                with torch.no_grad():
                    for _ in range(args.warmup if run == 0 else 1):
                        layer(x, ei)
                    ms = bench.timed_ms(lambda: layer(x, ei), args.reps, dev)
            print("run %d  %-8s %8.3f ms" % (run, form, ms), flush=True)


def hub_leg():
    from fsw_gnn_amd import FSW_readout, synth
    handle = __import__("ctypes").CDLL(_lib.LIB_PATH)
    has_hub = hasattr(handle, "fsw_embed_cart_backward_scratch_bytes")
    has_hub_w = hasattr(handle, "fsw_embed_cart_weighted_backward_scratch_bytes")
    general = args.weights != "unit" or args.tau > 1.0

    def scratch_bytes_before(self, graph, st, backward):
        """The host layer's rules from before fsw_embed_cart_scratch_bytes, on the size functions the build has: a build without the
        classes of a weight mode runs those rows on the generic kernel, which needs its scratch in both directions."""
        L, md, bsh, S = _lib.lib(), st[_lib.STAT_MAX_DEGREE], graph.bin_start_host[0], self.nSlices
        hub0 = _lib.BIN_MID0 + len(_lib.MID_SIZES) + _lib.NUM_LDS_BINS

        def generic(first_bin):
            return int(L.fsw_embed_cart_generic_scratch_bytes(md, max(int(bsh[_lib.NUM_BINS]) - int(bsh[first_bin]), 1)))

        unit = self._unit_fast(graph)
        if not (has_hub if unit else has_hub_w):
            return 0 if md < _lib.LDS_MAX_DEG else generic(hub0 - 1)
        forward = 0 if md < (_lib.HUB_MAX_DEG + 1 if unit else _lib.CART_W_MAX_LINE) else generic(_lib.NUM_BINS - 1 if unit else hub0 + 2)
        if not backward or (int(bsh[_lib.NUM_BINS - 1]) == int(bsh[hub0]) if unit else md < _lib.LDS_MAX_DEG):
            return forward
        size, first = ((L.fsw_embed_cart_backward_scratch_bytes, hub0) if unit else
                       (L.fsw_embed_cart_weighted_backward_scratch_bytes, hub0 - 1))
        return int(size(md, int(bsh[_lib.NUM_BINS]) - int(bsh[first]), S))

    if not hasattr(handle, "fsw_embed_cart_scratch_bytes"):
        del _lib._SIGNATURES["fsw_embed_cart_scratch_bytes"]
        FSW_embedding._cart_scratch_bytes = scratch_bytes_before
    if not has_hub_w:
        del _lib._SIGNATURES["fsw_embed_cart_weighted_backward_scratch_bytes"]
    if not has_hub:
        del _lib._SIGNATURES["fsw_embed_cart_backward_scratch_bytes"]
    print("library %s: %s" % (_lib.LIB_PATH, ("general-weight hub kernels" if has_hub_w else "generic kernel on the general-weight rows of "
                                              "2048 neighbours and more") if general else
                              ("hub kernels" if has_hub else "generic kernel on the rows above 2048 neighbours")), flush=True)
    S, F = args.slices, args.freqs
    steps, warmup = args.steps, args.warmup
    workload = ("readout,pc4096" if general else "readout,rmat") if args.workload == ap.get_default("workload") else args.workload

    def time_pair(name, forward, step):
        with torch.no_grad():
            for _ in range(warmup):
                forward()
            fwd = bench.timed_ms(forward, steps, dev)
        for _ in range(warmup):
            step()
        print("%-44s forward %10.3f ms   training step %10.3f ms" % (name, fwd, bench.timed_ms(step, steps, dev)), flush=True)

    batches = [("2049..4096", [2500] * 8), ("4097..8192", [6000] * 8), ("8193..16384", [12000] * 8), ("16385..32768", [24000] * 8),
               ("mixed", [2500, 5000, 9000, 12000, 16000, 20000, 25000, 30000])]
    if general:
        weighted_workloads(workload, batches, time_pair)
        return
    if "readout" in workload:
        in_ch, out_ch = 32, 32
        torch.manual_seed(7)
        layer = FSW_readout(in_ch, out_ch, embed_slices=S, embed_freqs=F, learnable_embedding=True, device=dev)
        for name, sizes in batches:
            gi = torch.cat([torch.full((m,), g, dtype=torch.int64) for g, m in enumerate(sizes)]).to(dev)
            x = torch.randn((gi.numel(), in_ch), device=dev)
            xg = x.clone().requires_grad_(True)
            G = torch.randn((len(sizes), out_ch), device=dev)

            def step():
                layer.zero_grad(set_to_none=True)
                xg.grad = None
                layer(xg, gi, len(sizes)).backward(G)

            time_pair("readout S=%d F=%d, 8 graphs, %s" % (S, F, name), lambda: layer(x, gi, len(sizes)), step)
    if "rmat" in workload:
        scale, E, d = 20, 10_000_000, 128
        n = 1 << scale
        ei = torch.from_numpy(synth.rmat_graph(scale, E, 7)).to(dev)
        graph = build_csr(ei[1].contiguous(), ei[0].contiguous(), None, n, n)
        st = graph.read_stats()
        bins = graph.bin_start_host[0]
        hub0 = _lib.BIN_MID0 + len(_lib.MID_SIZES) + _lib.NUM_LDS_BINS
        print("RMAT-%d: n=%d E=%d max degree %d, rows per hub bin %s, above: %d" % (
            scale, n, E, st[_lib.STAT_MAX_DEGREE], [int(bins[b + 1] - bins[b]) for b in range(hub0, hub0 + _lib.NUM_HUB_BINS)],
            int(bins[_lib.NUM_BINS] - bins[_lib.NUM_BINS - 1])), flush=True)
        torch.manual_seed(7)
        mod = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, collapse_freqs=True, enable_bias=False, learnable_slices=True,
                            learnable_freqs=True, freqs_init='spread', device=dev)
        x = torch.randn((n, d), device=dev)
        xg = x.clone().requires_grad_(True)
        out = torch.empty((n, S * F), device=dev)
        G = torch.randn((n, S * F), device=dev)

        def step():
            mod.zero_grad(set_to_none=True)
            xg.grad = None
            mod.embed_cartesian_autograd(xg, graph).backward(G)

        time_pair("embedding S=%d F=%d, RMAT-%d" % (S, F, scale), lambda: mod.embed_cartesian_into(x, graph, out), step)


def weighted_workloads(workload, batches, time_pair):
    """--hub with general weights: the readout batches as CSR graphs with a weight per vertex (or w = NULL and tau > 1) through
    FSW_embedding, and the batch of 4096-point clouds through the public forward."""
    S, F = args.slices, args.freqs
    if "readout" in workload:
        d = 32
        torch.manual_seed(7)
        mod = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, collapse_freqs=True, enable_bias=False, learnable_slices=True,
                            learnable_freqs=True, freqs_init='spread', total_mass_pad_thresh=args.tau, device=dev)
        for name, sizes in batches:
            gi = torch.cat([torch.full((m,), g, dtype=torch.int64) for g, m in enumerate(sizes)]).to(dev)
            nv = gi.numel()
            if args.weights == "uniform":
                w = (1.0 / torch.tensor(sizes, dtype=torch.float32, device=dev))[gi].contiguous()
            elif args.weights == "random":
                w = (0.05 + 0.95 * torch.rand(nv, generator=torch.Generator().manual_seed(8))).to(dev)
            else:
                w = None
            graph = build_csr(gi.contiguous(), torch.arange(nv, device=dev), w, len(sizes), nv)
            graph.read_stats()
            x = torch.randn((nv, d), device=dev)
            xg = x.clone().requires_grad_(True)
            out = torch.empty((len(sizes), S * F), device=dev)
            G = torch.randn((len(sizes), S * F), device=dev)

            def step():
                mod.zero_grad(set_to_none=True)
                xg.grad = None
                mod.embed_cartesian_autograd(xg, graph).backward(G)

            time_pair("embedding S=%d F=%d, %s weights tau %g, 8 graphs, %s" % (S, F, args.weights, args.tau, name),
                      lambda: mod.embed_cartesian_into(x, graph, out), step)
    if "pc4096" in workload:
        B, npts, Spc, Fpc = 64, 4096, 64, 16
        torch.manual_seed(7)
        pc = FSW_embedding(d_in=3, nSlices=Spc, nFreqs=Fpc, collapse_freqs=True, enable_bias=False, learnable_slices=True,
                           learnable_freqs=True, freqs_init='spread', device=dev)
        X = torch.randn((B, npts, 3), device=dev)
        Xg = X.clone().requires_grad_(True)
        G = torch.randn((B, Spc * Fpc), device=dev)

        def step_pc():
            pc.zero_grad(set_to_none=True)
            Xg.grad = None
            pc(Xg, 'uniform').backward(G)

        time_pair("point clouds %d x %d, d_in 3, S=%d F=%d, W='uniform'" % (B, npts, Spc, Fpc), lambda: pc(X, 'uniform'), step_pc)


def library_exports(symbol):
    """Whether the build that FSW_HIP_LIBRARY names exports symbol."""
    return hasattr(ctypes.CDLL(_lib.LIB_PATH), symbol)


def drive_without(symbol, method, rule):
    """An older build without an export of the binding: drop its signature (lib() binds every one it lists) and let FSW_embedding.method
    follow the host rule from before the export."""
    del _lib._SIGNATURES[symbol]
    setattr(FSW_embedding, method, rule)


def giant_leg():
    has_giant = library_exports("fsw_embed_cart_forward_scratch_bytes")
    if not has_giant:      # the generic kernel runs these rows: the forward's scratch is what the older query says
        drive_without("fsw_embed_cart_forward_scratch_bytes", "_cart_forward_scratch_bytes",
                      lambda self, graph, st: self._cart_scratch_bytes(graph, st, False))
    has_giant_bwd = library_exports("fsw_embed_cart_backward_keys_scratch_bytes")
    if not has_giant_bwd:  # the backward of these rows is the generic kernel: its scratch is what the older query says
        drive_without("fsw_embed_cart_backward_keys_scratch_bytes", "_cart_backward_scratch_bytes",
                      lambda self, graph, st: self._cart_scratch_bytes(graph, st, True))
    has_split = library_exports("fsw_embed_cart_split_scratch_bytes")
    if not has_split:      # one workgroup per line only: the host layer never asks for the split form
        for symbol in ("fsw_embed_cart_split_lines", "fsw_embed_cart_split_max_lines"):
            del _lib._SIGNATURES[symbol]
        drive_without("fsw_embed_cart_split_scratch_bytes", "_cart_split", lambda self, graph, st: 0)
    elif args.form != "auto":      # the threshold is the host layer's: move it out of the way
        top = (1 << 62) if args.form == "split" else 0
        _lib.lib().fsw_embed_cart_split_max_lines = lambda: top
    if not library_exports("fsw_embed_cart_split_w_scratch_bytes"):     # general weights: one workgroup per line only
        for symbol in ("fsw_embed_cart_split_w_lines", "fsw_embed_cart_split_w_max_lines"):
            del _lib._SIGNATURES[symbol]
        drive_without("fsw_embed_cart_split_w_scratch_bytes", "_cart_split_w", lambda self, graph, st: 0)
    elif args.form != "auto":
        top_w = (1 << 62) if args.form == "split" else 0
        _lib.lib().fsw_embed_cart_split_w_max_lines = lambda: top_w
    has_split_bwd = library_exports("fsw_embed_cart_split_backward_scratch_bytes")
    if not has_split_bwd:  # one workgroup per line only: the host layer never asks for the split backward
        for symbol in ("fsw_embed_cart_split_backward_lines", "fsw_embed_cart_split_backward_max_lines"):
            del _lib._SIGNATURES[symbol]
        drive_without("fsw_embed_cart_split_backward_scratch_bytes", "_cart_split_backward", lambda self, graph, st: 0)
    elif args.form_bwd != "auto":
        top_bwd = (1 << 62) if args.form_bwd == "split" else 0
        _lib.lib().fsw_embed_cart_split_backward_max_lines = lambda: top_bwd
    has_split_w_bwd = library_exports("fsw_embed_cart_split_w_backward_scratch_bytes")
    if not has_split_w_bwd:  # general weights: one workgroup per line only in the backward
        for symbol in ("fsw_embed_cart_split_w_backward_lines", "fsw_embed_cart_split_w_backward_max_lines"):
            del _lib._SIGNATURES[symbol]
        drive_without("fsw_embed_cart_split_w_backward_scratch_bytes", "_cart_split_w_backward", lambda self, graph, st: 0)
    elif args.form_bwd != "auto":
        top_w_bwd = (1 << 62) if args.form_bwd == "split" else 0
        _lib.lib().fsw_embed_cart_split_w_backward_max_lines = lambda: top_w_bwd
    print("library %s: forward: %s; backward: %s; split form: %s; split backward: %s; split backward of general weights: %s" % (
        _lib.LIB_PATH, "kernels of the longest rows" if has_giant else "generic kernel on the longest rows",
        "kernel of the longest rows" if has_giant_bwd else "generic kernel on the longest rows",
        ("--form " + args.form if args.form != "auto" else "up to %d lines" % _lib.lib().fsw_embed_cart_split_max_lines()) if has_split else "none",
        ("--form-bwd " + args.form_bwd if args.form_bwd != "auto" else
         "up to %d lines" % _lib.lib().fsw_embed_cart_split_backward_max_lines()) if has_split_bwd else "none",
        ("--form-bwd " + args.form_bwd if args.form_bwd != "auto" else
         "up to %d lines" % _lib.lib().fsw_embed_cart_split_w_backward_max_lines()) if has_split_w_bwd else "none"), flush=True)
    S, F, d = args.slices, args.freqs, 32
    steps, warmup = args.steps, args.warmup
    workload = "w24000,u40000,mixed,c150000,c150000x2,c150000x4,c1000000" if args.workload == ap.get_default("workload") else args.workload
    cases = [("w24000", "8 graphs x 24000, weights", [24000] * 8, True), ("u40000", "8 graphs x 40000, unit", [40000] * 8, False),
             ("mixed", "mixed 2500 .. 30000, weights", [2500, 5000, 9000, 12000, 16000, 20000, 25000, 30000], True),
             ("c150000", "one cloud of 150000, unit", [150000], False), ("c150000", "one cloud of 150000, weights", [150000], True),
             ("c150000x2", "2 clouds of 150000, unit", [150000] * 2, False), ("c150000x4", "4 clouds of 150000, unit", [150000] * 4, False),
             ("c1000000", "one cloud of 1000000, unit", [1000000], False), ("c1000000", "one cloud of 1000000, weights", [1000000], True)]
    if args.weights != "unit":      # every cloud workload with a weight per point
        cases = [("c150000" if k == 1 else "c150000x%d" % k, "%d cloud(s) of 150000, %s" % (k, args.weights), [150000] * k, True)
                 for k in (1, 2, 4, 8, 16, 32)] + [("c1000000", "one cloud of 1000000, %s" % args.weights, [1000000], True)]
        if args.workload == ap.get_default("workload"):
            workload = ",".join(key for key, _name, sizes, _w in cases if len(sizes) * S <= 256)
    torch.manual_seed(7)
    mod = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, collapse_freqs=True, enable_bias=False, learnable_slices=True,
                        learnable_freqs=True, freqs_init='spread', device=dev)
    for key, name, sizes, weighted in cases:
        if key not in workload.split(","):
            continue
        gi = torch.cat([torch.full((m,), g, dtype=torch.int64) for g, m in enumerate(sizes)]).to(dev)
        nv = gi.numel()
        w = (0.05 + 0.95 * torch.rand(nv, generator=torch.Generator().manual_seed(8))).to(dev) if weighted else None
        if weighted and args.weights == "uniform":
            w = torch.cat([torch.full((m,), 1.0 / m) for m in sizes]).to(dev)
        graph = build_csr(gi.contiguous(), torch.arange(nv, device=dev), w, len(sizes), nv)
        form = "split" if max(mod._cart_split(graph, graph.read_stats()), mod._cart_split_w(graph, graph.read_stats())) > 0 else "one workgroup per line"
        form_bwd = "split" if max(mod._cart_split_backward(graph, graph.read_stats()),
                                  mod._cart_split_w_backward(graph, graph.read_stats())) > 0 else "one workgroup per line"
        x = torch.randn((nv, d), device=dev)
        xg = x.clone().requires_grad_(True)
        out = torch.empty((len(sizes), S * F), device=dev)
        G = torch.randn((len(sizes), S * F), device=dev)

        def step():
            mod.zero_grad(set_to_none=True)
            xg.grad = None
            mod.embed_cartesian_autograd(xg, graph).backward(G)

        with torch.no_grad():
            for _ in range(warmup):
                mod.embed_cartesian_into(x, graph, out)
            fwd = bench.timed_ms(lambda: mod.embed_cartesian_into(x, graph, out), steps, dev)
        for _ in range(warmup):
            step()
        print("%-36s S=%d F=%d  forward %10.3f ms   training step %10.3f ms   forward form: %s   backward form: %s" % (
            name, S, F, fwd, bench.timed_ms(step, steps, dev), form, form_bwd), flush=True)
        del graph, x, xg, out, G, gi, w


def split_w_leg():
    """One projection, then fsw_embed_cart_f32 with FSW_CART_SPLIT_W_LINES off and on, alternating."""
    import statistics
    L = _lib.lib()
    S, F, d = args.slices, args.freqs, 32
    weights = "uniform" if args.weights == "unit" else args.weights
    print("library %s: split form of general weights against the one-workgroup-per-line kernel, weights %s, S=%d F=%d, host threshold %d lines"
          % (_lib.LIB_PATH, weights, S, F, L.fsw_embed_cart_split_w_max_lines()), flush=True)
    torch.manual_seed(7)
    mod = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, collapse_freqs=True, enable_bias=False, freqs_init='spread', device=dev)
    fr = mod.freqs.detach().contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    cases = [[1000000]] + [[150000] * k for k in (1, 2, 4, 8, 16, 32) if k * S <= 512]
    only = [key for key in args.workload.split(",") if key != "splitw"]      # splitw,c150000x4: that case alone (for a profile)
    if only:
        cases = [c for c in cases if ("c%d" % c[0] if len(c) == 1 else "c%dx%d" % (c[0], len(c))) in only]
    for sizes in cases:
        gi = torch.cat([torch.full((m,), g, dtype=torch.int64) for g, m in enumerate(sizes)]).to(dev)
        nv = gi.numel()
        if weights == "uniform":
            w = torch.cat([torch.full((m,), 1.0 / m) for m in sizes]).to(dev)
        else:
            w = (0.05 + 0.95 * torch.rand(nv, generator=torch.Generator().manual_seed(8))).to(dev)
        graph = build_csr(gi.contiguous(), torch.arange(nv, device=dev), w, len(sizes), nv)
        x = torch.randn((nv, d), device=dev)
        with torch.no_grad():
            prepared = mod.prepare_cartesian(x, graph)
        Xp, ldp, st = prepared["Xp"], prepared["ldp"], prepared["stats"]
        query = mod._cart_tuned_args(graph, st, Xp, ldp, fr, S, None, None, 1.0, 0)
        nbytes = max(int(L.fsw_embed_cart_forward_scratch_bytes(ctypes.byref(query))), int(L.fsw_embed_cart_split_w_scratch_bytes(ctypes.byref(query))))
        lines = int(L.fsw_embed_cart_split_w_lines(ctypes.byref(query)))
        assert lines == len(sizes) * S and nbytes > 0
        sets = [(torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty((len(sizes), S * F), device=dev)) for _ in range(3)]
        turn = [0]

        def call(flag):
            scratch, out = sets[turn[0] % len(sets)]
            turn[0] += 1
            a = mod._cart_tuned_args(graph, st, Xp, ldp, fr, S, None, scratch, 1.0, 0, split_w=flag)
            a.out, a.ldo = out.data_ptr(), out.stride(0)
            _lib.check(L.fsw_embed_cart_f32(ctypes.byref(a), stream), "fsw_embed_cart_f32")
            return out

        off, on = call(False).clone(), call(True).clone()
        torch.cuda.synchronize(dev)
        err = float((on.double() - off.double()).norm() / off.double().norm())
        ms = {False: [], True: []}
        for flag in (False, True):
            for _ in range(args.warmup):
                call(flag)
        for _ in range(args.runs):
            for flag in (False, True):
                ms[flag].append(bench.timed_ms(lambda: call(flag), args.steps, dev))
        m_off, m_on = statistics.median(ms[False]), statistics.median(ms[True])
        print("%2d cloud(s) of %7d, %4d lines: one workgroup per line %8.3f ms (%.3f .. %.3f)   split %8.3f ms (%.3f .. %.3f)   ratio %.2f   "
              "split against one workgroup per line %.1e" % (len(sizes), sizes[0], lines, m_off, min(ms[False]), max(ms[False]), m_on,
                                                             min(ms[True]), max(ms[True]), m_off / m_on, err), flush=True)
        del graph, x, prepared, Xp, sets, gi, w


if args.giant and "splitw" in args.workload.split(","):
    split_w_leg()
    sys.exit(0)
if args.giant:
    giant_leg()
    sys.exit(0)
if args.hub:
    hub_leg()
    sys.exit(0)
if args.edge_keys:
    edge_keys_leg()
    sys.exit(0)
if args.conv and args.edge_features > 0:
    conv_edge_leg()
    sys.exit(0)
if args.conv:
    conv_leg()
    sys.exit(0)
if args.train:
    train_leg()
    sys.exit(0)
n, E, d = bench.N_NODES, bench.N_EDGES, bench.D_FEAT
S, F = args.slices, args.freqs
x, ei = bench.make_inputs(n, E, dev)
graph = build_csr(ei[1].contiguous(), ei[0].contiguous(), None, n, n)
graph.read_stats()
torch.manual_seed(7)
cart = FSW_embedding(d_in=d, nSlices=S, nFreqs=F, collapse_freqs=True, enable_bias=False, device=dev)
expd = FSW_embedding(d_in=d, d_out=S * F, enable_bias=False, device=dev)
head = FSW_embedding(d_in=d, d_out=S * F, enable_bias=False, device=dev)
with torch.no_grad():
    expd.projVecs.copy_(cart.projVecs.repeat_interleave(F, dim=0))
    expd.freqs.copy_(cart.freqs.repeat(S))
out = torch.empty((n, S * F), device=dev)
ref = torch.empty((n, S * F), device=dev)
L = _lib.lib()
stream = torch.cuda.current_stream(dev).cuda_stream


def projection_ms(nslices, ldp):
    Xp = torch.empty((n, ldp), device=dev)
    V = torch.randn((nslices, d), device=dev)
    return bench.timed_ms(lambda: _lib.check(L.fsw_project_f32(_lib.ptr(x), n, d, x.stride(0), _lib.ptr(V), nslices, d, _lib.ptr(Xp), ldp,
                                                               None, 0, None, stream), "fsw_project_f32"), args.reps, dev)


with torch.no_grad():
    cart.embed_cartesian_into(x, graph, out)
    if "b" in args.only:
        expd.embed_into(x, graph, ref)
        print("(a) vs (b): max difference %.2e of max |out|" % float((out - ref).abs().max() / ref.abs().max()))
    rows = [
        ("(a) Cartesian S=%d x F=%d" % (S, F), lambda: cart.embed_cartesian_into(x, graph, out), (S, (S + 31) // 32 * 32), S),
        ("(b) diagonal expansion, %d slices" % (S * F), lambda: expd.embed_into(x, graph, ref), (S * F, (S * F + 63) // 64 * 64), S * F),
        ("(c) diagonal d_out=%d headline" % (S * F), lambda: head.embed_into(x, graph, ref), (S * F, (S * F + 63) // 64 * 64), S * F),
    ]
    print("config 3: n=%d E=%d d_in=%d, max degree %d" % (n, E, d, graph.max_degree))
    for name, fn, proj_shape, lines in rows:
        if name[1] not in args.only:
            continue
        ms = bench.timed_ms(fn, args.reps, dev)
        proj = projection_ms(*proj_shape)
        kern = max(ms - proj, 1e-6)
        gb = (4.0 * E * lines + 4.0 * n * S * F + 4.0 * E) / 1e9
        print("%-36s %7.3f ms/forward  projection %6.3f ms  rest (neighbourhood kernel + table + stats read) %7.3f ms  %5.2f GB  "
              ">= %5.0f GB/s = %.2f of 8 TB/s"
              % (name, ms, proj, kern, gb, gb / kern * 1e3, gb / kern * 1e3 / bench.HBM_PEAK_GBS), flush=True)
