"""Timing of the two CSR builds (fsw_graph_build: three LSD passes; fsw_graph_build_two_level: partition pass + bucket kernel).

    python tools/exp_csr.py                 BASELINE config 3's edge list (1M rows, 10M random edges)
    python tools/exp_csr.py --rmat 22 --edges 64000000
    python tools/exp_csr.py --from-csr [--parent-library PATH]
        the same graph held as CSR: import_csr (fsw_graph_import_csr, no sort) with int64 and with int32 indices next to the build
        of its edge list -- by the library at PATH (a build of the parent commit, loaded beside this one) when given, else by this
        library.  Five rounds that alternate between the candidates; the smallest and the largest round of each are printed, and the
        fraction of the import's byte model (int64: reads 8 (nnz + rows), writes 4 (nnz + 2 rows); the binning passes not counted)
        that the measured time achieves against 6.3 TB/s, the copy rate this GPU reaches.
"""
import argparse, ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from fsw_gnn_amd import _lib, build_csr, import_csr, synth
ap = argparse.ArgumentParser()
ap.add_argument("--rmat", type=int, default=0)
ap.add_argument("--edges", type=int, default=bench.N_EDGES)
ap.add_argument("--from-csr", action="store_true")
ap.add_argument("--parent-library", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
if args.rmat:
    n = 1 << args.rmat
    ei = torch.from_numpy(synth.rmat_graph(args.rmat, args.edges, 7)).to(dev)
else:
    n = bench.N_NODES
    _, ei = bench.make_inputs(n, args.edges, dev)


def parent_build(L, entry):
    """build_csr's allocations and call, on another build of the library (same entry points, same arguments)."""
    fn = getattr(L, entry)
    fn.restype, fn.argtypes = _lib._SIGNATURES[entry]
    L.fsw_graph_workspace_bytes.restype, L.fsw_graph_workspace_bytes.argtypes = _lib._SIGNATURES["fsw_graph_workspace_bytes"]
    rec, snd, E = ei[1].contiguous(), ei[0].contiguous(), ei.shape[1]

    def run():
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        invperm = torch.empty(n, dtype=torch.int32, device=dev)
        meta = torch.empty(_lib.NUM_STATS + _lib.NUM_BINS + 1, dtype=torch.int32, device=dev)
        ws_bytes = L.fsw_graph_workspace_bytes(n, E)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        rc = fn(_lib.ptr(rec), _lib.ptr(snd), None, E, n, n, 0, _lib.ptr(rowptr), _lib.ptr(col), None, _lib.ptr(perm), _lib.ptr(invperm),
                _lib.ptr(meta[_lib.NUM_STATS:]), _lib.ptr(meta[:_lib.NUM_STATS]), _lib.ptr(ws), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
    return run


if args.from_csr:
    ref = build_csr(ei[1], ei[0], None, n, n, algo="lsd")
    nnz = ei.shape[1]
    rp64, col64 = ref.rowptr.long(), ref.col[:nnz].long()
    rp32, col32 = ref.rowptr.clone(), ref.col[:nnz].clone()
    got = import_csr(rp64, col64, None, n, n, want_invperm=True)
    assert torch.equal(got.rowptr, ref.rowptr) and torch.equal(got.col[:nnz], ref.col[:nnz]) and got.stats()[:7] == ref.stats()[:7]
    if args.parent_library:
        P = ctypes.CDLL(os.path.abspath(args.parent_library))
        builds = {"build two_level (parent library)": parent_build(P, "fsw_graph_build_two_level"),
                  "build lsd (parent library)": parent_build(P, "fsw_graph_build")}
    else:
        builds = {"build two_level": lambda: build_csr(ei[1], ei[0], None, n, n, want_invperm=True, algo="two_level"),
                  "build lsd": lambda: build_csr(ei[1], ei[0], None, n, n, want_invperm=True, algo="lsd")}
    cands = dict(builds)
    cands["import_csr int64"] = lambda: import_csr(rp64, col64, None, n, n, want_invperm=True)
    cands["import_csr int32"] = lambda: import_csr(rp32, col32, None, n, n, want_invperm=True)
    times = {k: [] for k in cands}
    for _ in range(5):
        for k, fn in cands.items():
            times[k].append(bench.timed_ms(fn, 10, dev))
    model = {"import_csr int64": 8 * (nnz + n) + 4 * (nnz + 2 * n), "import_csr int32": 4 * (nnz + n) + 4 * (nnz + 2 * n)}
    for k, v in times.items():
        line = "%-34s %d rows / %d entries: min %.3f ms  max %.3f ms over 5 rounds" % (k, n, nnz, min(v), max(v))
        if k in model:
            line += "   byte model %.3f GB = %.3f ms at 6.3 TB/s: %.0f %% of it achieved" % (
                model[k] / 1e9, model[k] / 6.3e9, 100.0 * model[k] / 6.3e9 / min(v))
        print(line, flush=True)
    sys.exit(0)

for algo in ("lsd", "two_level", "lsd", "two_level"):
    ms = bench.timed_ms(lambda: build_csr(ei[1], ei[0], None, n, n, want_invperm=True, algo=algo), 10, dev)
    print("%-10s %d rows / %d edges: %.3f ms" % (algo, n, ei.shape[1], ms), flush=True)
