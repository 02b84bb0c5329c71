"""csrc/graph_build.hip against the numpy references of tests/graph_ref.py, one case per branch of the builds: the LSD passes (one
pass of 8 bits up to four passes, the sentinel key taking a bit of its own, edge counts around one 4096-edge tile), the two-level
build (staged / scattering / unstaged buckets, one and two partition passes, the thresholds of two_level_ok), the degree bins with
every cut, row chunks and the stats words, the weight flags, the coalescing build beyond the sizes at which its scan once overran
the block sums of the workspace, and fsw_graph_transpose / fsw_segment_sum_rows_f32.

Integer outputs are compared exactly and the weights of the non-coalescing builds bit for bit; perm is compared as a set per bin
(inside a bin its order depends on atomics).  The inputs of the coalescing build and of the exact segment-sum cases are dyadic
(weights k / 1024, features and rows k / 256, sums far below 2^24 units): every float32 and float64 sum is exact in any order, so
those outputs are compared exactly as well."""
import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests import cases
from tests import graph_ref as R
from tests.conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5
NB = R.NUM_BINS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_CACHE = {}


def cached(key, make):
    """Inputs and references are built once and shared by the cases that use them (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def t(a, dev, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.to(device=dev, dtype=dtype) if dtype is not None else x.to(dev)


def dyadic_weights(rng, n):
    return (rng.integers(1, 4096, n) / 1024.0).astype(np.float32)


def make_invalid(rec, snd, at, rows, cols):
    """The four kinds of out-of-range edge, in turn, at the positions `at`."""
    for i, p in enumerate(at):
        k = i % 4
        if k == 0:
            rec[p] = rows
        elif k == 1:
            rec[p] = -1
        elif k == 2:
            snd[p] = cols
        else:
            snd[p] = -5


def random_edges(seed, rows, cols, edges, hub=0, bad_at=()):
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, rows, edges).astype(np.int64)
    snd = rng.integers(0, cols, edges).astype(np.int64)
    if hub:
        rec[rng.choice(edges, hub, replace=False)] = min(12345, rows - 1)
    make_invalid(rec, snd, bad_at, rows, cols)
    return rec, snd, dyadic_weights(rng, edges)


def host(x):
    return x.cpu().numpy()


def check_bins(gr, bins, chunk_rows=0):
    """bin_start, the stats words, perm (per bin as a set) and invperm against ref_bins."""
    st = host(gr.stats_dev).tolist()
    bs = host(gr.bin_start).reshape(-1, NB + 1)
    perm = host(gr.perm)
    rows = bins["bin_of_row"].size
    assert bs.shape[0] == bins["num_chunks"] and bs[-1, -1] == rows, (bs.shape, bs[-1, -1], rows)
    assert np.array_equal(bs, bins["bin_start"]), np.argwhere(bs != bins["bin_start"])[:5]
    assert np.array_equal(bs[1:, 0], bs[:-1, -1])                        # the rows of consecutive chunks join
    for word, want in bins["stats"].items():
        assert st[word] == want, (word, st[word], want)
    assert gr.max_degree == bins["stats"][R.STAT_MAX_DEGREE]
    bad = R.perm_mismatch(perm, bins, chunk_rows)
    assert bad is None, bad
    if gr.invperm is not None:
        assert np.array_equal(host(gr.invperm)[perm], np.arange(rows))
    return st


def check_csr(gr, ref, weighted, chunk_rows=0, bins=None):
    st = host(gr.stats_dev).tolist()
    nnz = ref["nnz"]
    assert st[R.STAT_NNZ] == nnz, (st, nnz)
    assert st[R.STAT_FLAGS] == (ref["flags"] if weighted else ref["flags"] & R.FLAG_INDEX_RANGE), st
    assert gr.flags == st[R.STAT_FLAGS]
    assert np.array_equal(host(gr.rowptr), ref["rowptr"])
    assert np.array_equal(host(gr.col[:nnz]), ref["col"])
    if weighted:
        assert np.array_equal(host(gr.w[:nnz]).view(np.int32), ref["w"].view(np.int32))
    else:
        assert gr.w is None
    check_bins(gr, bins if bins is not None else R.ref_bins(ref["rowptr"], chunk_rows), chunk_rows)


def run_build(dev, data, rows, cols, weighted, algo, chunk_rows=0):
    from fsw_gnn_amd import build_csr
    rec, snd, w = data
    return build_csr(t(rec, dev), t(snd, dev), t(w, dev) if weighted else None, rows, cols, want_invperm=True, chunk_rows=chunk_rows, algo=algo)


def case_with_refs(key, make, rows, cols, chunk_rows=0):
    def build():
        data = make()
        ref = R.ref_csr(data[0], data[1], data[2], rows, cols)
        return data, ref, R.ref_bins(ref["rowptr"], chunk_rows)
    return cached(key, build)


# ---- LSD build ------------------------------------------------------------------------------------------------------------------
LSD_SHAPES = [
    (1, 1, "one_edge"),
    (1, 5000, "one_row_of_5000_two_tiles"),
    (255, 4095, "one_pass_of_8_bits_tile_minus_one"),
    (256, 4096, "sentinel_takes_bit_9_two_passes_of_5_exact_tile"),
    (256, 4097, "two_passes_of_5_tile_plus_one"),
    (65_535, 8193, "two_passes_of_8_two_tiles_plus_one"),
    (65_536, 20_000, "sentinel_takes_bit_17_three_passes_of_6"),
    ((1 << 24) - 1, 300_000, "three_passes_of_8"),
    (1 << 24, 300_000, "four_passes_of_7"),
]


def lsd_passes(rows):
    bits = R._key_bits(rows)
    npass = -(-bits // 8)
    return npass, -(-bits // npass)


def test_lsd_pass_counts_of_the_shapes():
    """What the ids of the LSD cases claim (radix_sort_pairs: ceil(bits / 8) passes of ceil(bits / passes) bits)."""
    assert [lsd_passes(r) for r, _, _ in LSD_SHAPES] == [(1, 1), (1, 1), (1, 8), (2, 5), (2, 5), (2, 8), (3, 6), (3, 8), (4, 7)]


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("rows,edges,name", LSD_SHAPES, ids=[s[2] for s in LSD_SHAPES])
def test_lsd_build_shapes(dev, rows, edges, name, weighted):
    data, ref, bins = case_with_refs(("lsd", rows, edges), lambda: random_edges(rows + edges, rows, rows, edges), rows, rows)
    assert ref["nnz"] == edges and ref["flags"] == 0
    check_csr(run_build(dev, data, rows, rows, weighted, "lsd"), ref, weighted, bins=bins)


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
def test_lsd_build_invalid_edges_in_first_middle_and_last_tile(dev, weighted):
    rows, edges = 3000, 3 * 4096 + 100                                     # four tiles, the last one partial
    at = (0, 5, 4095, 4096 + 17, 6000, 8191, 3 * 4096, edges - 50, edges - 1)
    data, ref, bins = case_with_refs("lsd_invalid9", lambda: random_edges(31, rows, rows, edges, bad_at=at), rows, rows)
    assert ref["nnz"] == edges - 9 and ref["flags"] == R.FLAG_INDEX_RANGE
    check_csr(run_build(dev, data, rows, rows, weighted, "lsd"), ref, weighted, bins=bins)


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
def test_lsd_build_every_edge_invalid(dev, weighted):
    rows, edges = 100, 5000
    data, ref, bins = case_with_refs("lsd_all_invalid", lambda: random_edges(32, rows, rows, edges, bad_at=range(edges)), rows, rows)
    assert ref["nnz"] == 0 and ref["flags"] == R.FLAG_INDEX_RANGE
    gr = run_build(dev, data, rows, rows, weighted, "lsd")
    check_csr(gr, ref, weighted, bins=bins)
    assert int(gr.rowptr.abs().max()) == 0
    bs = host(gr.bin_start)
    assert bs[0] == 0 and (bs[1:] == rows).all() and gr.max_degree == 0                      # all rows in bin 0


def rect_case(edge_senders):
    rows, cols, edges = 8, 100_000, 20_000

    def make():
        rec, snd, w = random_edges(33, rows, cols, edges)
        if edge_senders:
            snd[7], snd[4100] = cols - 1, cols                                                # the last valid sender, the first invalid one
        return rec, snd, w
    return (rows, cols, edges) + case_with_refs(("lsd_rect", edge_senders), make, rows, cols)


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("edge_senders", [False, True], ids=["random_senders", "senders_cols_minus_1_and_cols"])
def test_lsd_build_rectangular(dev, edge_senders, weighted):
    rows, cols, edges, data, ref, bins = rect_case(edge_senders)
    assert ref["nnz"] == edges - edge_senders and ref["col"].max() > rows
    if edge_senders:
        assert ref["col"].max() == cols - 1 and ref["flags"] == R.FLAG_INDEX_RANGE
    check_csr(run_build(dev, data, rows, cols, weighted, "lsd"), ref, weighted, bins=bins)


@pytest.mark.parametrize("algo", ["lsd", "two_level"])
def test_build_without_edges(dev, algo):
    rows = 5000
    z = np.zeros(0, dtype=np.int64)
    data = (z, z, np.zeros(0, dtype=np.float32))
    ref = R.ref_csr(z, z, data[2], rows, rows)
    for weighted in (False, True):
        check_csr(run_build(dev, data, rows, rows, weighted, algo), ref, weighted)


# ---- two-level build ------------------------------------------------------------------------------------------------------------
# id = the path bucket_plan and the bucket sizes of the inputs confirm; (rows, edges, weights, hub, invalid edges), plan = (two_level_ok,
# partition passes, stage_cap), buckets = which buckets fit the staging tile
TWO_LEVEL = [
    ("weights_staged_cap11136_hub_bucket_scatters", (200_000, 900_000, True, 5000, 0), (True, 1, 11_136), "all_but_hub"),
    ("weights_staged_sentinel_run_cut_in_last_bucket", (200_000, 900_000, True, 0, 11), (True, 1, 11_136), "all"),
    ("unit_staged_cap22272_hub_bucket_scatters", (200_000, 1_000_000, False, 15_000, 0), (True, 1, 22_272), "all_but_hub"),
    ("unit_no_staging_avg_bucket_30000", (40_000, 600_000, False, 0, 0), (True, 1, 0), "none"),
    ("weights_two_partition_passes_bucket_starts_staged", (1_100_000, 600_000, True, 0, 0), (True, 2, 11_136), "all"),
    ("unit_at_both_thresholds_staged", (32_768, 262_144, False, 0, 0), (True, 1, 22_272), "all"),
    ("below_row_threshold_lsd_fallback", (32_767, 262_144, False, 0, 0), (False, 1, 22_272), "fallback"),
    ("below_edge_threshold_lsd_fallback", (32_768, 262_143, False, 0, 0), (False, 1, 22_272), "fallback"),
    ("avg_bucket_above_65536_lsd_fallback", (40_000, 1_400_000, False, 0, 0), (False, 1, 0), "fallback"),
]


@pytest.mark.parametrize("name,shape,plan,buckets", TWO_LEVEL, ids=[c[0] for c in TWO_LEVEL])
def test_two_level_build_paths(dev, name, shape, plan, buckets):
    rows, edges, weighted, hub, bad = shape
    bad_at = tuple(int(p) for p in np.linspace(3, edges - 2, bad).astype(np.int64)) if bad else ()
    data, ref, bins = case_with_refs(("two_level", shape), lambda: random_edges(rows + edges + bad, rows, rows, edges, hub, bad_at), rows, rows)
    # the path first: a retuned constant must not let the case pass without reaching it
    p = R.bucket_plan(rows, edges, weighted)
    assert (p["two_level_ok"], p["passes"], p["stage_cap"]) == plan, "this shape no longer reaches the path %s: %r" % (name, p)
    key = np.where((data[0] >= 0) & (data[0] < rows) & (data[1] >= 0) & (data[1] < rows), data[0], rows)
    size = np.sort(np.bincount(key // p["bucket_rows"], minlength=p["buckets"]))
    cap = p["stage_cap"]
    if buckets == "all_but_hub":
        assert size[-1] > cap >= size[-2], "this shape no longer reaches the path %s: buckets %r, cap %d" % (name, size[-3:], cap)
    elif buckets == "all":
        assert 0 < size[-1] <= cap, "this shape no longer reaches the path %s: buckets %r, cap %d" % (name, size[-3:], cap)
    elif buckets == "none":
        assert cap == 0
    if bad:                                                                # the sentinel row shares the last bucket with valid rows
        assert ref["nnz"] == edges - bad and rows % p["bucket_rows"] != 0 and rows // p["bucket_rows"] == p["buckets"] - 1
    b = run_build(dev, data, rows, rows, weighted, "two_level")
    check_csr(b, ref, weighted, bins=bins)
    a = run_build(dev, data, rows, rows, weighted, "lsd")
    nnz = ref["nnz"]
    assert torch.equal(a.stats_dev, b.stats_dev) and torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col[:nnz], b.col[:nnz])
    assert torch.equal(a.bin_start, b.bin_start)
    if weighted:
        assert torch.equal(a.w[:nnz].view(torch.int32), b.w[:nnz].view(torch.int32))
    assert R.perm_mismatch(host(a.perm), bins) is None


# ---- bins, stats, chunks, flags -------------------------------------------------------------------------------------------------
CUT_DEGREES = list(range(34)) + [40, 41, 48, 49, 64, 65, 80, 81, 96, 97, 128, 129, 160, 161, 192, 193, 256, 257, 512, 513, 1024, 1025, 2048,
                                 2049, 4096, 4097, 8192, 8193, 16_384, 16_385, 32_768, 32_769]


def test_degree_bins_every_cut(dev):
    """One row of every degree at and just above each cut of the degree classes, the other rows of degree 0 .. 3, rows in shuffled
    order: every row's bin, bin_start, all the stats words, invperm."""
    rows = 4999

    def make():
        rng = np.random.default_rng(41)
        deg = rng.integers(0, 4, rows)
        deg[:len(CUT_DEGREES)] = CUT_DEGREES
        deg = deg[rng.permutation(rows)]
        rec = np.repeat(np.arange(rows, dtype=np.int64), deg)
        rec = rec[rng.permutation(rec.size)]
        return (rec, rng.integers(0, rows, rec.size).astype(np.int64), dyadic_weights(rng, rec.size)), deg
    (data, deg) = cached("cuts", make)
    ref = R.ref_csr(data[0], data[1], data[2], rows, rows)
    bins = R.ref_bins(ref["rowptr"])
    assert 135_000 < ref["nnz"] < 145_000 and np.array_equal(np.diff(ref["rowptr"]), deg)
    assert len(set(bins["bin_of_row"].tolist())) == NB                        # every bin is populated
    gr = run_build(dev, data, rows, rows, False, "lsd")
    check_csr(gr, ref, False, bins=bins)
    # once more by the definition, row by row, through invperm and the scalar degree_bin
    bs, inv, st = host(gr.bin_start), host(gr.invperm), gr.stats()
    for r in range(rows):
        b = R.degree_bin(int(deg[r]))
        assert bs[b] <= inv[r] < bs[b + 1], (r, deg[r], b)
    assert st[R.STAT_NUM_ZERO] == (deg == 0).sum() and st[R.STAT_NUM_REG] == ((deg >= 1) & (deg <= 32)).sum()
    assert st[R.STAT_NUM_LDS] == ((deg >= 33) & (deg <= 2048)).sum() == 24 and st[R.STAT_NUM_GLOBAL] == (deg > 2048).sum() == 9
    assert st[R.STAT_MAX_DEGREE] == 32_769 and st[R.STAT_NNZ] == deg.sum()


@pytest.mark.parametrize("rows,edges", [(5 * 2048 + 77, 40_000), (256 * 2048, 300_000)], ids=["six_chunks_last_partial", "256_chunks"])
@pytest.mark.parametrize("algo", ["lsd", "two_level"])
def test_row_chunks_against_the_reference(dev, rows, edges, algo):
    chunk_rows = 2048
    data, ref, bins = case_with_refs(("chunks", rows), lambda: random_edges(rows, rows, rows, edges, hub=300), rows, rows, chunk_rows)
    assert bins["num_chunks"] == -(-rows // 2048) and bins["bin_start"].shape == (bins["num_chunks"], NB + 1)
    gr = run_build(dev, data, rows, rows, True, algo, chunk_rows=chunk_rows)
    assert gr.num_chunks == bins["num_chunks"]
    check_csr(gr, ref, True, chunk_rows=chunk_rows, bins=bins)
    # chunk c's slice of perm holds exactly the rows of chunk c
    perm, bs = host(gr.perm), host(gr.bin_start)
    for c in (0, 1, bins["num_chunks"] // 2, bins["num_chunks"] - 1):
        got = np.sort(perm[bs[c, 0]:bs[c, NB]])
        assert np.array_equal(got, np.arange(c * chunk_rows, min((c + 1) * chunk_rows, rows)))


def raw_build(dev, data, rows, cols, chunk_rows=0, short=0, entry="fsw_graph_build"):
    """The C entry point itself (build_csr refuses some of these arguments before the library sees them).  -> (status, tensors)"""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    rec, snd, w = t(data[0], dev), t(data[1], dev), t(data[2], dev)
    E = rec.numel()
    chunks = max(1, -(-rows // chunk_rows)) if chunk_rows > 0 else 1
    out = dict(rowptr=torch.full((rows + 1,), -7, dtype=torch.int32, device=dev), col=torch.empty(max(E, 1), dtype=torch.int32, device=dev),
               w=torch.empty(max(E, 1), dtype=torch.float32, device=dev), perm=torch.empty(rows, dtype=torch.int32, device=dev),
               invperm=torch.empty(rows, dtype=torch.int32, device=dev),
               bin_start=torch.empty((chunks, NB + 1), dtype=torch.int32, device=dev), stats=torch.empty(_lib.NUM_STATS, dtype=torch.int32, device=dev))
    ws_bytes = int(L.fsw_graph_workspace_bytes(rows, E))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rc = getattr(L, entry)(_lib.ptr(rec), _lib.ptr(snd), _lib.ptr(w), E, rows, cols, chunk_rows, _lib.ptr(out["rowptr"]), _lib.ptr(out["col"]),
                           _lib.ptr(out["w"]), _lib.ptr(out["perm"]), _lib.ptr(out["invperm"]), _lib.ptr(out["bin_start"]), _lib.ptr(out["stats"]),
                           _lib.ptr(ws), ws_bytes - short, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("entry", ["fsw_graph_build", "fsw_graph_build_two_level"])
def test_refused_arguments_leave_the_next_build_intact(dev, entry):
    """257 row chunks, a chunk size that is no multiple of 2048 and a workspace one byte short are refused with a status, before any
    launch; a valid build right after each refusal gives the right tables."""
    from fsw_gnn_amd import _lib
    rows, edges = 256 * 2048 + 1, 300_000
    data, ref, bins = case_with_refs(("refuse", rows), lambda: random_edges(51, rows, rows, edges), rows, rows, 4096)
    for kw in (dict(chunk_rows=2048), dict(chunk_rows=1000), dict(chunk_rows=4096, short=1), dict(short=1)):
        rc, out = raw_build(dev, data, rows, rows, entry=entry, **kw)
        assert rc != 0 and _lib.lib().fsw_last_error(), kw
        assert int((out["rowptr"] != -7).sum()) == 0                      # nothing ran
        rc, out = raw_build(dev, data, rows, rows, chunk_rows=4096, entry=entry)
        assert rc == 0
        assert np.array_equal(host(out["rowptr"]), ref["rowptr"]) and np.array_equal(host(out["col"]), ref["col"])
        assert np.array_equal(host(out["w"]).view(np.int32), ref["w"].view(np.int32))
        assert np.array_equal(host(out["bin_start"]), bins["bin_start"])
        assert R.perm_mismatch(host(out["perm"]), bins, 4096) is None
        assert host(out["stats"])[R.STAT_NNZ] == edges


FLAG_CASES = [("plus_inf", (np.inf,), R.FLAG_W_NONFINITE), ("nan", (np.nan,), R.FLAG_W_NONFINITE), ("minus_one", (-1.0,), R.FLAG_W_NEGATIVE),
              ("minus_zero", (-0.0,), 0), ("minus_inf", (-np.inf,), R.FLAG_W_NONFINITE | R.FLAG_W_NEGATIVE),
              ("plus_inf_and_minus_one", (-1.0, np.inf), R.FLAG_W_NONFINITE | R.FLAG_W_NEGATIVE)]


@pytest.mark.parametrize("name,values,want", FLAG_CASES, ids=[c[0] for c in FLAG_CASES])
@pytest.mark.parametrize("build", ["lsd", "two_level", "coalesced"])
def test_weight_flags(dev, build, name, values, want):
    """The offending weight is the last edge of a partial tile (the last lanes that still read an edge)."""
    from fsw_gnn_amd.graph import build_csr_coalesced
    rows, edges = (32_768, 262_144 + 10) if build == "two_level" else (50, 4096 + 10)
    if build == "two_level":
        assert R.bucket_plan(rows, edges, True)["two_level_ok"]
    rec, snd, w = cached(("flags", rows), lambda: random_edges(61, rows, rows, edges))
    w = w.copy()
    w[edges - len(values):] = values
    assert R.ref_csr(rec, snd, w, rows, rows)["flags"] == want
    if build == "coalesced":
        gr = build_csr_coalesced(t(rec, dev), t(snd, dev), t(w, dev), None, rows, rows)
    else:
        gr = run_build(dev, (rec, snd, w), rows, rows, True, build)
    assert gr.flags == want
    assert gr.stats()[R.STAT_NNZ] == (edges if build != "coalesced" else R.ref_coalesced(rec, snd, None, None, rows, rows)["nnz"])


@pytest.mark.parametrize("value,message", [(np.inf, "All entries of W must be finite"), (np.nan, "All entries of W must be finite"),
                                           (-1.0, "All entries of W must be nonnegative"), (-0.0, None)],
                         ids=["plus_inf", "nan", "minus_one", "minus_zero"])
def test_weight_flags_raise_the_documented_assertions(dev, value, message):
    from fsw_gnn_amd import FSW_embedding
    n, d, S = 60, 5, 8
    rng = np.random.default_rng(62)
    key = np.unique(rng.integers(0, n * n, 500))
    w = dyadic_weights(rng, key.size)
    w[-1] = value
    W = torch.sparse_coo_tensor(t(np.stack([key // n, key % n]), dev), t(w, dev), (n, n)).coalesce()
    E = FSW_embedding(d_in=d, d_out=S, device=dev, enable_bias=False)
    X = t(rng.standard_normal((n, d)).astype(np.float32), dev)
    with torch.no_grad():
        if message is None:
            assert bool(torch.isfinite(E(X, W, graph_mode=True)).all())
        else:
            with pytest.raises(AssertionError, match=message):
                E(X, W, graph_mode=True)


# ---- coalescing build -----------------------------------------------------------------------------------------------------------
COALESCE_SHAPES = [
    (7, 1, "one_edge"),
    (300, 4096, "exact_tile"),
    (300, 4097, "tile_plus_one"),
    (20_000, 300_000, "74_scan_blocks_just_over_the_old_block_sums"),
    (20_000, 600_000, "147_scan_blocks_once_overwrote_bin_count"),
    (200_000, 1_400_000, "342_scan_blocks_200000_rows"),
]


def coalesce_case(rows, edges):
    """~10 % duplicate pairs; one pair repeated 5000 times (E >= 10000), most of the copies contiguous in the edge list across the
    border of the first tile and -- 5000 > 4096 -- across a tile border of the sorted order too; invalid edges of all four kinds
    interleaved with further copies of that pair, in the first tile and in the last one; cols != rows."""
    cols = rows + 37
    rng = np.random.default_rng(rows + edges)
    rec = rng.integers(0, rows, edges).astype(np.int64)
    snd = rng.integers(0, cols, edges).astype(np.int64)
    if edges >= 10:
        dup = rng.choice(edges, edges // 10, replace=False)
        src = rng.integers(0, edges, dup.size)
        rec[dup], snd[dup] = rec[src].copy(), snd[src].copy()
    pair = (rows // 2, cols - 1)
    blocks = [(1, 6), (edges - 13, 6)] if edges >= 10_000 else [(1, 8)] if edges >= 32 else []
    nbad = sum(cnt for _, cnt in blocks)
    run = min(5000, edges // 2) - nbad                                     # contiguous copies; nbad more are interleaved below
    if run > 0:
        start = max(2 * nbad + 1, min(4096 - run // 2, edges - run))
        rec[start:start + run], snd[start:start + run] = pair
    at = []
    for base, cnt in blocks:                                               # invalid edge, copy of the pair, invalid edge, ...
        for i in range(cnt):
            at.append(base + 2 * i)
            rec[base + 2 * i + 1], snd[base + 2 * i + 1] = pair
    make_invalid(rec, snd, at, rows, cols)
    w = dyadic_weights(rng, edges)
    ef = (rng.integers(-1024, 1025, (edges, 3)) / 256.0).astype(np.float32)
    return rec, snd, w, ef, cols, len(at)


@pytest.mark.parametrize("d_edge", [0, 1, 3])
@pytest.mark.parametrize("rows,edges,name", COALESCE_SHAPES, ids=[s[2] for s in COALESCE_SHAPES])
def test_coalescing_build(dev, rows, edges, name, d_edge):
    from fsw_gnn_amd.graph import build_csr_coalesced

    def make():
        rec, snd, w, ef, cols, nbad = coalesce_case(rows, edges)
        ref = R.ref_coalesced(rec, snd, w, ef, rows, cols)
        return (rec, snd, w, ef, cols, nbad), ref, R.ref_bins(ref["rowptr"])
    (rec, snd, w, ef, cols, nbad), ref, bins = cached(("coalesce", rows, edges), make)
    ok = (rec >= 0) & (rec < rows) & (snd >= 0) & (snd < cols)
    assert (~ok).sum() == nbad and (nbad == 0) == (edges < 32) and ref["flags"] == (R.FLAG_INDEX_RANGE if nbad else 0)
    if edges >= 10_000:
        runs = np.bincount(ref["slot"][ok])
        assert ref["nnz"] < 0.96 * edges and runs.max() == 5000
        assert -(-edges // 4096) > -(-512 * -(-edges // 4096) // 4096) + 1                         # more scan blocks than the radix passes need
    gr = build_csr_coalesced(t(rec, dev), t(snd, dev), t(w, dev), t(ef[:, :d_edge], dev) if d_edge else None, rows, cols, want_slots=True)
    # the symptom of the overrun first: the bin tables
    perm = host(gr.perm)
    assert np.array_equal(np.sort(perm), np.arange(rows)) and int(gr.bin_start[-1]) == rows
    st = host(gr.stats_dev).tolist()
    nnz = ref["nnz"]
    assert st[R.STAT_NNZ] == nnz and st[R.STAT_FLAGS] == ref["flags"]
    assert np.array_equal(host(gr.rowptr), ref["rowptr"]) and np.array_equal(host(gr.col[:nnz]), ref["col"])
    assert np.array_equal(host(gr.w[:nnz]), ref["w"])
    assert np.array_equal(host(gr.slot_of_edge[:edges]), ref["slot"])
    if d_edge:
        assert np.array_equal(host(gr.ef[:nnz]), ref["ef"][:, :d_edge])
    else:
        assert gr.ef is None
    check_bins(gr, bins)


def test_conv_with_edge_features_on_600000_edges(dev):
    """FSW_conv(edgefeat_dim = 2) forward on a graph whose coalescing build needs 147 scan blocks, against the oracle on 200 rows."""
    from fsw_gnn_amd import FSW_conv
    n, edges, d, de, out_ch, embed_dim = 20_000, 600_000, 4, 2, 3, 9
    rng = np.random.default_rng(71)
    rec, snd = rng.integers(0, n, edges), rng.integers(0, n, edges)
    dup = rng.choice(edges, edges // 10, replace=False)
    rec[dup], snd[dup] = rec[(dup + 1) % edges].copy(), snd[(dup + 1) % edges].copy()
    ef = (rng.integers(-1024, 1025, (edges, de)) / 256.0).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = cases.synth.unit_slices(embed_dim - 1, d + de, seed=72)
    fr = cases.synth.spread_freqs(embed_dim - 1)
    conv = FSW_conv(d, out_ch, edgefeat_dim=de, embed_dim=embed_dim, device=dev)
    with torch.no_grad():
        conv.fsw_embed.projVecs.copy_(t(V, dev))
        conv.fsw_embed.freqs.copy_(t(fr, dev))
        y = host(conv(t(X, dev), t(np.stack([snd, rec]), dev), edge_features=t(ef, dev)))
    ref = R.ref_coalesced(rec, snd, None, ef, n, n)
    assert ref["nnz"] < 0.95 * edges
    rows = np.sort(rng.choice(n, 200, replace=False))
    rp = ref["rowptr"].astype(np.int64)
    take = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows])
    sub_ptr = np.concatenate([[0], np.cumsum(rp[rows + 1] - rp[rows])])
    emb = O.fsw_embedding_forward(X, sub_ptr, ref["col"][take].astype(np.int64), ref["w"][take].astype(np.float64), V, fr, encode_total_mass=True,
                                  edge_feat=ref["ef"][take])
    want = O.conv_tail(emb, X[rows].astype(np.float64), linear_weight=host(conv.mlp[0].weight.detach()), linear_bias=host(conv.mlp[0].bias.detach()))
    assert relerr(y[rows], want) < TOL


# ---- transpose and segment sum --------------------------------------------------------------------------------------------------
def transpose(dev, col, num_cols):
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    nnz = col.size
    cd = t(col, dev) if nnz else torch.zeros(1, dtype=torch.int32, device=dev)
    cptr = torch.full((num_cols + 1,), -7, dtype=torch.int32, device=dev)
    order = torch.full((max(nnz, 1),), -7, dtype=torch.int32, device=dev)
    ws_bytes = int(L.fsw_graph_workspace_bytes(num_cols, nnz))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(L.fsw_graph_transpose(_lib.ptr(cd), nnz, num_cols, _lib.ptr(cptr), _lib.ptr(order), _lib.ptr(ws), ws_bytes,
                                     torch.cuda.current_stream(dev).cuda_stream), "fsw_graph_transpose")
    torch.cuda.synchronize()
    return host(cptr), host(order)


@pytest.mark.parametrize("num_cols,nnz,invalid", [(1, 1, 0), (1, 4097, 3), (255, 4096, 4), (256, 4097, 4), (256, 1, 1), (65_536, 300_000, 9),
                                                  (100_000, 4096, 5), (100_000, 300_000, 0), (256, 0, 0)])
def test_graph_transpose(dev, num_cols, nnz, invalid):
    """col entries equal to -1 and to num_cols sort last and belong to no sender."""
    rng = np.random.default_rng(num_cols + nnz)
    col = rng.integers(0, num_cols, nnz).astype(np.int32)
    if nnz > 2:
        col[1], col[nnz - 2] = num_cols - 1, 0
    at = rng.choice(nnz, invalid, replace=False) if invalid else np.zeros(0, dtype=np.int64)
    col[at[0::2]] = -1
    col[at[1::2]] = num_cols
    if invalid and nnz > 1:
        col[nnz - 1] = num_cols                                             # the last entry of a partial tile
        invalid = int(((col < 0) | (col >= num_cols)).sum())
    cptr_ref, order_ref = R.ref_transpose(col, num_cols)
    cptr, order = transpose(dev, col, num_cols)
    assert cptr_ref[-1] == nnz - invalid
    assert np.array_equal(cptr, cptr_ref)
    assert np.array_equal(order[:nnz - invalid], order_ref)


def test_graph_transpose_of_a_rectangular_graph(dev):
    """CSRGraph.sender_major on 8 rows x 100 000 columns."""
    rows, cols, edges, data, ref, _ = rect_case(True)
    gr = run_build(dev, data, rows, cols, False, "lsd")
    cptr, order = gr.sender_major()
    cptr_ref, order_ref = R.ref_transpose(ref["col"], cols)
    assert cptr.numel() == cols + 1 and np.array_equal(host(cptr), cptr_ref) and np.array_equal(host(order[:ref["nnz"]]), order_ref)


def segment_lists():
    """Lengths of the sender lists, in order; 256 entries per segment.  Empty senders at the start; a list that is exactly segment 0; two
    lists of which the second ends exactly at the end of segment 1; a run of empty senders at that segment edge; a list over segments
    2 .. 25 (24 segments, ending inside the last); short lists; a list that ends on a segment edge followed by empty senders up to the end."""
    rng = np.random.default_rng(81)
    lens = [0, 0, 0, 256, 100, 156, 0, 0, 0, 24 * 256 - 100]
    lens += rng.integers(0, 40, 300).tolist()
    lens += [256 - sum(lens) % 256, 0, 0]
    return np.array(lens, dtype=np.int64)


def segment_sum(dev, src, lds, ptr, order, num_out, nnz, S, ldo):
    from fsw_gnn_amd import _lib
    out = torch.full((num_out, ldo), 7.5, device=dev)
    out[:, :S] = 0.0                                                        # the caller zeroes what the kernel may add to
    _lib.check(_lib.lib().fsw_segment_sum_rows_f32(_lib.ptr(src), lds, _lib.ptr(ptr), _lib.ptr(order), num_out, nnz, S, _lib.ptr(out), ldo,
                                                   torch.cuda.current_stream(dev).cuda_stream), "fsw_segment_sum_rows_f32")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("S", [1, 64, 65, 256, 257, 600])
def test_segment_sum_rows_exact(dev, S):
    lens = segment_lists()
    assert sum(lens[:4]) == 256 and sum(lens[:6]) == 512 and lens[6:9].sum() == 0 and lens.sum() % 256 == 0 and lens[-2:].sum() == 0
    num_out, valid = lens.size, int(lens.sum())
    tail = 37                                                               # entries that belong to no sender
    nnz = valid + tail
    rng = np.random.default_rng(82 + S)
    lds, ldo = S + 3, S + 5
    src = np.full((valid + 5, lds), np.nan, dtype=np.float32)               # padding columns and the tail's rows must never be read
    src[:valid, :S] = rng.integers(-1024, 1025, (valid, S)) / 256.0
    order = np.concatenate([rng.permutation(valid), np.full(tail, valid + 2)]).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    out = segment_sum(dev, t(src, dev), lds, t(ptr, dev), t(order, dev), num_out, nnz, S, ldo)
    sender = np.repeat(np.arange(num_out), lens)
    want = torch.zeros(num_out, S, dtype=torch.float64, device=dev).index_add_(0, t(sender, dev), t(src[order[:valid], :S], dev).double())
    assert torch.equal(out[:, :S].double(), want)
    assert bool((out[:, S:] == 7.5).all())                                  # padding columns untouched


def test_segment_sum_rows_normal_values(dev):
    lens = segment_lists()
    num_out, nnz, S = lens.size, int(lens.sum()), 70
    rng = np.random.default_rng(83)
    src = rng.standard_normal((nnz, S)).astype(np.float32)
    order = rng.permutation(nnz).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    out = segment_sum(dev, t(src, dev), S, t(ptr, dev), t(order, dev), num_out, nnz, S, 128)
    want = torch.zeros(num_out, S, dtype=torch.float64, device=dev).index_add_(0, t(np.repeat(np.arange(num_out), lens), dev), t(src[order], dev).double())
    assert float((out[:, :S].double() - want).abs().max()) < 1e-4 * float(want.abs().max())
    assert bool((out[:, S:] == 7.5).all())
