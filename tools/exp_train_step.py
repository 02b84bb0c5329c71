"""Timing of one FSW_conv training step (forward + backward) -- not the headline metric.

    python tools/exp_train_step.py            BASELINE config 3 (ER multigraph, every row on the <= 32 register path)
    python tools/exp_train_step.py --rmat 20  RMAT graph with 2^20 vertices and 10M edges (hubs up to 41 300 neighbours)
    python tools/exp_train_step.py --rmat 22 --edges 64000000 --feat 256 --forward-only [--gcn]   BASELINE config 5's shape
    python tools/exp_train_step.py --edge-weights   learnable per-edge weights (FSW_conv.forward(edge_weight=)): the training step, and
                                                    the embedding's backward on the tuned kernels (csrc/embed_w_bwd.hip up to 24
                                                    neighbours, csrc/embed_w_sort_bwd.hip up to the library's class limit,
                                                    csrc/embed_w_long_bwd.hip for the rows above) against the generic kernel's for every row
                                                    (FSW_embedding.forward with a sparse COO W that requires grad), alternating;
                                                    also the share of the entries in each of the three classes
"""
import argparse, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from fsw_gnn_amd import FSW_conv, synth
ap = argparse.ArgumentParser()
ap.add_argument("--rmat", type=int, default=0)
ap.add_argument("--forward-only", action="store_true")
ap.add_argument("--edges", type=int, default=bench.N_EDGES)
ap.add_argument("--feat", type=int, default=128)
ap.add_argument("--gcn", action="store_true", help="edge_weighting='gcn': general edge weights (the (key, weight) kernels)")
ap.add_argument("--edge-weights", action="store_true", help="a learnable weight per edge; compares the two routes to its gradient")
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
n, E = bench.N_NODES, args.edges
if args.rmat:
    n = 1 << args.rmat
    ei = torch.from_numpy(synth.rmat_graph(args.rmat, E, 7)).to(dev)
    x = torch.from_numpy(synth.features(n, args.feat, 3)).to(dev)
else:
    x, ei = bench.make_inputs(n, E, dev)
    assert args.feat == 128
conv = FSW_conv(args.feat, 128, embed_dim=257, device=dev, edge_weighting='gcn' if args.gcn else 'unit')
with torch.no_grad():
    print("inference forward, %d nodes / %d edges / %d feat / 256 slices: %.2f ms (max in-degree %d)" % (
        n, E, args.feat, bench.timed_ms(lambda: conv(x, ei), 5, dev), int(torch.bincount(ei[1]).max())), flush=True)
if args.edge_weights:
    from fsw_gnn_amd.graph import build_csr_coalesced
    emb = conv.fsw_embed
    w = (0.25 + 0.75 * torch.rand(E, device=dev)).requires_grad_(True)

    def timed_backward(make_out):
        out = make_out()
        g = torch.ones_like(out)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out.backward(g)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def new_route():          # what FSW_conv.forward(edge_weight=w) runs for the embedding
        graph = build_csr_coalesced(ei[1], ei[0], w.detach(), None, n, n, want_slots=True)
        return emb.embed_autograd(x, graph, edge_weight=w)

    adj = torch.sparse_coo_tensor(ei.flip(0), w.detach(), (n, n)).coalesce()
    vals = adj.values().clone().requires_grad_(True)

    def generic_route():      # the only route to this gradient without the tuned kernels: _GenericEmbedFn
        return emb(x, W=torch.sparse_coo_tensor(adj.indices(), vals, (n, n), is_coalesced=True), graph_mode=True)

    from fsw_gnn_amd import _lib
    limit = int(_lib.lib().fsw_embed_backward_w_tuned_max_degree())
    deg = torch.bincount(adj.indices()[0], minlength=n)          # entries per recipient of the coalesced adjacency
    nnz = int(deg.sum())
    share = [int(deg[sel].sum()) / nnz for sel in (deg <= 24, (deg > 24) & (deg <= limit), deg > limit)]
    print("entries per class: <= 24 neighbours (register kernels) %.1f %%, 25 .. %d (wave-sort kernels) %.1f %%, above (scratch-line kernels) "
          "%.1f %% of %d; rows: %d / %d / %d" % (100 * share[0], limit, 100 * share[1], 100 * share[2], nnz, int((deg <= 24).sum()),
                                                 int(((deg > 24) & (deg <= limit)).sum()), int((deg > limit).sum())), flush=True)
    tuned = "tuned kernels (embed_w_bwd.hip, embed_w_sort_bwd.hip; embed_w_long_bwd.hip above %d)" % limit
    times = {tuned: [], "generic kernel": []}
    for i in range(args.runs + 1):                      # run 0 warms both up
        for name, fn in ((tuned, new_route), ("generic kernel", generic_route)):
            ms = timed_backward(fn)
            if i:
                times[name].append(ms)
    for name, v in times.items():
        print("embedding backward with dL/dW, %s: %.1f - %.1f ms over %d runs" % (name, min(v), max(v), len(v)), flush=True)
    a, b = times.values()
    print("ranges %s" % ("do not overlap: the tuned kernels are faster" if max(a) < min(b) else "overlap or the generic kernel is faster"))
    print("gkey buffer: %.2f GB" % (int(adj.values().numel()) * 256 * 4 / 1e9))

    def step_w():
        conv.zero_grad(set_to_none=True); w.grad = None
        conv(x, ei, edge_weight=w).square().mean().backward()
    step_w()
    steps = []
    for _ in range(args.runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        step_w()
        torch.cuda.synchronize(); steps.append((time.perf_counter() - t0) * 1e3)
    print("training step with learnable edge weights (fwd + bwd): %.1f - %.1f ms" % (min(steps), max(steps)))
elif not args.forward_only:
    x.requires_grad_(True)
    def step():
        conv.zero_grad(set_to_none=True); x.grad = None
        y = conv(x, ei)
        y.square().mean().backward()
    for _ in range(2): step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(5): step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 5
    print("training step (fwd + bwd): %.2f ms" % (dt * 1e3))
