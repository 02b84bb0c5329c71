"""The packed path of fsw_graph_build_two_level (csrc/graph_plan.h: unit weights, one partition pass, row bits of a bucket + sender
bits <= 32 -- one uint32 per edge, 8192-edge partition tiles, degree bins counted by the bucket kernel) against the numpy references
of tests/graph_ref.py and against the LSD build of the same input.

Every case first asserts its path through fsw_graph_build_plan (the host code the build itself runs), so a retuned constant cannot
let a case pass without reaching its branch.  All outputs are integers and are compared exactly; perm as a set per (chunk, bin)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import graph_ref as R
from tests.test_hip_graph_build import CUT_DEGREES, cached, case_with_refs, check_csr, host, random_edges, run_build

pytestmark = pytest.mark.gpu
NB = R.NUM_BINS
TILE = 8192            # csrc/graph_plan.h: kPackTile (asserted through the plan in every packed case)
CAP = 22_272           # entries of the staging tile for 4-byte values (tests/test_graph_ref_cpu.py: PLAN)
WORDS = ("two_level", "packed", "tile", "stage_cap", "passes", "row_bits", "sender_bits", "buckets")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def plan(rows, cols, edges, weighted=False):
    from fsw_gnn_amd import _lib
    out = (ctypes.c_int32 * len(WORDS))()
    assert _lib.lib().fsw_graph_build_plan(rows, cols, edges, int(weighted), out) == 0
    return dict(zip(WORDS, list(out)))


def expect_packed(rows, cols, edges, stage_cap=CAP):
    p = plan(rows, cols, edges)
    assert (p["two_level"], p["packed"], p["tile"], p["stage_cap"], p["passes"], p["row_bits"]) == (1, 1, TILE, stage_cap, 1, 11), p
    ref = R.bucket_plan(rows, edges, False)
    assert (ref["two_level_ok"], ref["stage_cap"], ref["buckets"], ref["passes"]) == (True, p["stage_cap"], p["buckets"], 1), (p, ref)
    return p


def bucket_sizes(data, rows, cols, p):
    rec, snd = data[0], data[1]
    key = np.where((rec >= 0) & (rec < rows) & (snd >= 0) & (snd < cols), rec, rows)
    return np.bincount(key >> p["row_bits"], minlength=p["buckets"])


def build_and_compare(dev, data, ref, bins, rows, cols, weighted=False, chunk_rows=0):
    """two_level against the references, then against the LSD build, entry for entry."""
    b = run_build(dev, data, rows, cols, weighted, "two_level", chunk_rows=chunk_rows)
    check_csr(b, ref, weighted, chunk_rows=chunk_rows, bins=bins)
    a = run_build(dev, data, rows, cols, weighted, "lsd", chunk_rows=chunk_rows)
    nnz = ref["nnz"]
    assert torch.equal(a.stats_dev, b.stats_dev) and torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col[:nnz], b.col[:nnz])
    assert torch.equal(a.bin_start, b.bin_start)
    if weighted:
        assert torch.equal(a.w[:nnz].view(torch.int32), b.w[:nnz].view(torch.int32))
    assert R.perm_mismatch(host(a.perm), bins, chunk_rows) is None
    return b


# ---- thresholds of two_level_ok and of the packed word ------------------------------------------------------------------------
def rect_edges(seed, rows, cols, edges):
    rec, snd, w = random_edges(seed, rows, cols, edges)
    snd[3], snd[edges // 2], snd[edges - 1] = 0, cols - 1, cols - 1        # the smallest and the largest sender
    return rec, snd, w


THRESHOLDS = [
    ("square_packed", 32_768, (1, 1, TILE, 15)),
    ("cols_2p21_row_bits_plus_sender_bits_32_packed", 1 << 21, (1, 1, TILE, 21)),
    ("cols_2p21_plus_1_pair_path", (1 << 21) + 1, (1, 0, 4096, 22)),
]


@pytest.mark.parametrize("name,cols,want", THRESHOLDS, ids=[c[0] for c in THRESHOLDS])
def test_packed_at_both_thresholds_of_two_level_ok(dev, name, cols, want):
    rows, edges = 32_768, 262_144
    p = plan(rows, cols, edges)
    assert (p["two_level"], p["packed"], p["tile"], p["sender_bits"]) == want and p["stage_cap"] == CAP and p["row_bits"] == 11, p
    assert plan(rows - 1, cols, edges)["two_level"] == 0 and plan(rows, cols, edges - 1)["two_level"] == 0
    data, ref, bins = case_with_refs(("packed_thr", cols), lambda: rect_edges(61, rows, cols, edges), rows, cols)
    assert ref["nnz"] == edges and ref["col"].min() == 0 and ref["col"].max() == cols - 1
    build_and_compare(dev, data, ref, bins, rows, cols)


# ---- partial tiles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", [33 * TILE - 1, 33 * TILE, 33 * TILE + 1], ids=["33_tiles_minus_1", "33_tiles", "33_tiles_plus_1"])
def test_packed_partial_tiles(dev, edges):
    rows = 40_000
    expect_packed(rows, rows, edges)
    data, ref, bins = case_with_refs(("packed_tiles", edges), lambda: random_edges(62 + edges, rows, rows, edges), rows, rows)
    assert ref["nnz"] == edges
    build_and_compare(dev, data, ref, bins, rows, rows)


def test_one_packed_tile_plus_one_edge_takes_the_lsd_passes(dev):
    """8193 edges are below the edge threshold of two_level_ok: the two-level entry point runs the LSD passes, and says so."""
    rows, edges = 40_000, TILE + 1
    assert plan(rows, rows, edges) == dict.fromkeys(WORDS, 0)
    data, ref, bins = case_with_refs("packed_one_tile_plus_1", lambda: random_edges(63, rows, rows, edges), rows, rows)
    build_and_compare(dev, data, ref, bins, rows, rows)


# ---- invalid edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [32_768, 34_000], ids=["sentinel_row_opens_a_bucket_of_its_own", "sentinel_run_ends_a_staged_bucket"])
def test_packed_invalid_edges_in_first_middle_and_last_tile(dev, rows):
    edges = 33 * TILE + 100                                                  # 34 tiles, the last one partial
    at = (0, 5, 17, TILE - 1, 16 * TILE, 16 * TILE + 1, 17 * TILE - 1, 17 * TILE + 4000, 33 * TILE, edges - 50, edges - 2, edges - 1)
    p = expect_packed(rows, rows, edges)
    data, ref, bins = case_with_refs(("packed_invalid", rows), lambda: random_edges(64, rows, rows, edges, bad_at=at), rows, rows)
    assert ref["nnz"] == edges - len(at) and ref["flags"] == R.FLAG_INDEX_RANGE
    size = bucket_sizes(data, rows, rows, p)
    if rows % 2048 == 0:
        assert p["buckets"] == rows // 2048 + 1 and size[-1] == len(at)      # the last bucket holds the sentinel row alone
    else:
        assert p["buckets"] == rows // 2048 + 1 and len(at) < size[-1] <= CAP  # valid rows and the sentinel run share a staged bucket
    build_and_compare(dev, data, ref, bins, rows, rows)


def test_packed_every_edge_invalid(dev):
    rows, edges = 32_768, 262_144
    expect_packed(rows, rows, edges)
    data, ref, bins = case_with_refs("packed_all_invalid", lambda: random_edges(65, rows, rows, edges, bad_at=range(edges)), rows, rows)
    assert ref["nnz"] == 0 and ref["flags"] == R.FLAG_INDEX_RANGE
    gr = build_and_compare(dev, data, ref, bins, rows, rows)
    assert int(gr.rowptr.abs().max()) == 0 and gr.max_degree == 0
    bs = host(gr.bin_start)
    assert bs[0] == 0 and (bs[1:] == rows).all()                             # all rows in bin 0


# ---- oversized buckets ----------------------------------------------------------------------------------------------------------
def test_packed_every_edge_in_one_bucket_scatters(dev):
    rows, edges = 32_768, 262_144
    p = expect_packed(rows, rows, edges)

    def make():
        rec, snd, w = random_edges(66, rows, rows, edges)
        return rec % 2048, snd, w
    data, ref, bins = case_with_refs("packed_one_bucket", make, rows, rows)
    size = bucket_sizes(data, rows, rows, p)
    assert size[0] == edges > CAP and int(size[1:].sum()) == 0
    build_and_compare(dev, data, ref, bins, rows, rows)


def test_packed_hub_bucket_scatters_while_the_others_stage(dev):
    rows, edges = 200_000, 1_000_000
    p = expect_packed(rows, rows, edges)
    data, ref, bins = case_with_refs("packed_hub", lambda: random_edges(67, rows, rows, edges, hub=15_000), rows, rows)
    size = np.sort(bucket_sizes(data, rows, rows, p))
    assert size[-1] > CAP >= size[-2], size[-3:]
    assert bins["stats"][R.STAT_MAX_DEGREE] > 15_000
    build_and_compare(dev, data, ref, bins, rows, rows)


# ---- degree bins counted by the bucket kernel ---------------------------------------------------------------------------------------
BIN_ROWS = 40_000
BIN_CUTS = [d for d in CUT_DEGREES if d <= 2049] + [40_000]


def bin_case():
    """One row at and one above every degree cut from 0 to 2049 and a row of 40 000 neighbours, the other rows of degree 0 .. 15, rows
    in shuffled order."""
    def make():
        rng = np.random.default_rng(68)
        deg = rng.integers(0, 16, BIN_ROWS)
        deg[:len(BIN_CUTS)] = BIN_CUTS
        deg = deg[rng.permutation(BIN_ROWS)]
        rec = np.repeat(np.arange(BIN_ROWS, dtype=np.int64), deg)
        rec = rec[rng.permutation(rec.size)]
        return (rec, rng.integers(0, BIN_ROWS, rec.size).astype(np.int64), None), deg
    return cached("packed_bins", make)


@pytest.mark.parametrize("chunk_rows", [0, 2048, 4096], ids=["one_chunk", "chunks_of_2048_last_partial", "chunks_of_4096"])
def test_packed_degree_bins_every_cut_and_row_chunks(dev, chunk_rows):
    rows = BIN_ROWS
    data, deg = bin_case()
    edges = data[0].size
    expect_packed(rows, rows, edges)

    def refs():
        ref = R.ref_csr(data[0], data[1], None, rows, rows)
        return ref, R.ref_bins(ref["rowptr"], chunk_rows)
    ref, bins = cached(("packed_bins_ref", chunk_rows), refs)
    assert np.array_equal(np.diff(ref["rowptr"]), deg) and bins["num_chunks"] == (-(-rows // chunk_rows) if chunk_rows else 1)
    if chunk_rows:
        assert rows % chunk_rows != 0                                        # the last chunk is partial
    gr = build_and_compare(dev, data, ref, bins, rows, rows, chunk_rows=chunk_rows)
    # every stats word by the definition, and every row's bin through invperm and the scalar degree_bin
    st = gr.stats()
    assert st[R.STAT_NUM_ZERO] == (deg == 0).sum() and st[R.STAT_NUM_REG] == ((deg >= 1) & (deg <= 32)).sum()
    assert st[R.STAT_NUM_LDS] == ((deg >= 33) & (deg <= 2048)).sum() == 24 and st[R.STAT_NUM_GLOBAL] == (deg > 2048).sum() == 2
    assert st[R.STAT_MAX_DEGREE] == 40_000 and st[R.STAT_NNZ] == deg.sum() == edges and st[R.STAT_FLAGS] == 0
    bs, inv = host(gr.bin_start).reshape(-1, NB + 1), host(gr.invperm)
    cr = chunk_rows if chunk_rows else rows
    for r in np.flatnonzero(deg > 15).tolist() + list(range(0, rows, 997)):
        c, b = r // cr, R.degree_bin(int(deg[r]))
        assert bs[c, b] <= inv[r] < bs[c, b + 1], (r, deg[r], c, b)


# ---- weights: the pair kernels, as before -----------------------------------------------------------------------------------------
def test_weights_take_the_pair_path(dev):
    rows, edges = 40_000, 33 * TILE + 1
    p = plan(rows, rows, edges, weighted=True)
    # 8-byte values: the average bucket of 13 518 edges (+ 3 % + 256) no longer fits the staging tile of 11 136 entries
    assert (p["two_level"], p["packed"], p["tile"], p["stage_cap"]) == (1, 0, 4096, 0) and R.bucket_plan(rows, edges, True)["stage_cap"] == 0, p
    data, ref, bins = case_with_refs("packed_weights", lambda: random_edges(69, rows, rows, edges), rows, rows)
    build_and_compare(dev, data, ref, bins, rows, rows, weighted=True)


# ---- the upsweep's loads -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["both_aligned", "recipients_off_by_8", "senders_off_by_8", "both_off_by_8"])
def test_packed_endpoint_arrays_aligned_to_16_or_only_8_bytes(dev, skip):
    """The upsweep reads two edges per 16-byte load when both endpoint arrays are 16-byte aligned and one edge per load otherwise
    (a row of an odd-length edge_index): views that start one element into their buffers, invalid edges in the last, odd tile."""
    from fsw_gnn_amd import build_csr
    rows, edges = 40_000, 33 * TILE + 101
    at = (0, TILE, edges - 2, edges - 1)
    expect_packed(rows, rows, edges)
    data, ref, bins = case_with_refs("packed_align", lambda: random_edges(70, rows, rows, edges, bad_at=at), rows, rows)
    def view(a, off):                                                        # a starts `off` elements into a 16-byte aligned buffer
        buf = np.zeros(edges + 2, dtype=np.int64)
        buf[off:off + edges] = a
        return torch.from_numpy(buf).to(dev)[off:off + edges]
    rec, snd = view(data[0], 2 - skip[0]), view(data[1], 2 - skip[1])
    assert rec.numel() == snd.numel() == edges and rec.data_ptr() % 16 == 8 * skip[0] and snd.data_ptr() % 16 == 8 * skip[1]
    gr = build_csr(rec, snd, None, rows, rows, want_invperm=True, algo="two_level")
    check_csr(gr, ref, False, bins=bins)


def test_packed_count_table_scanned_by_one_or_three_launches():
    """The shapes above on either side of the one-workgroup scan (count table of digits x tiles <= 4096 entries)."""
    small, large = plan(32_768, 32_768, 262_144), plan(200_000, 200_000, 1_000_000)
    for p, rows, edges, one in ((small, 32_768, 262_144, True), (large, 200_000, 1_000_000, False)):
        digits = 1 << (R._key_bits(rows) - p["row_bits"])
        assert p["packed"] == 1 and (digits * -(-edges // p["tile"]) <= 4096) == one
