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
    rocprofv3 --kernel-trace --stats -d DIR -o conv -- python tools/exp_cartesian.py --conv --forms fused --runs 1"""
import argparse
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
ap.add_argument("--workload", default="graph,pc", help="--train: subset of graph, graph_w, pc")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--generic", action="store_true", help="--train: the generic Cartesian kernel for forward and backward")
ap.add_argument("--conv", action="store_true", help="time the FSW_conv layer (diagonal / Cartesian unfused / Cartesian fused)")
ap.add_argument("--forms", default="unfused,fused", help="--conv: forms to time, alternating over the runs (--train: diag, cart)")
ap.add_argument("--runs", type=int, default=5, help="--conv: runs of every form")
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
