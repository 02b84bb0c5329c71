"""The numpy references of tests/graph_ref.py (what tests/test_hip_graph_build.py compares the CSR build with) against independent
forms -- the oracle's coalescing, torch's stable sort, the degree classes as tests/test_cart_scratch_cpu.py writes them -- the plan of
the two-level build for the shapes the GPU tests rely on, and the workspace layout of the build (csrc/graph_ws.h) swept on the CPU by
tests/native/test_graph_ws.cpp.  No GPU is needed."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import fsw_oracle as O
from tests import graph_ref as R
from tests.conftest import ROOT, golden
from tests.test_cart_scratch_cpu import degree_bin as scratch_degree_bin


def multigraph(seed, rows, cols, edges, bad=0):
    """Seeded multigraph with ~10 % duplicate pairs, dyadic weights (k / 1024) and features (k / 256): sums are exact in any order."""
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, rows, edges)
    snd = rng.integers(0, cols, edges)
    dup = rng.integers(0, edges, edges // 10)
    rec[dup], snd[dup] = rec[(dup * 7 + 3) % edges], snd[(dup * 7 + 3) % edges]
    if bad:
        at = rng.choice(edges, bad, replace=False)
        rec[at[0::4]] = rows
        rec[at[1::4]] = -1
        snd[at[2::4]] = cols
        snd[at[3::4]] = -5
    w = (rng.integers(1, 4096, edges) / 1024.0).astype(np.float32)
    ef = (rng.integers(-1024, 1025, (edges, 3)) / 256.0).astype(np.float32)
    return rec.astype(np.int64), snd.astype(np.int64), w, ef


def test_ref_coalesced_against_the_oracle():
    g, ge = golden("tiny_graph"), golden("edgefeat_tiny")
    ei, ef = g["edge_index"], ge["edge_features"].astype(np.float32)
    rowptr, col, w, _, efo, slot = O.coalesce_edge_index(ei, 64, edge_features=ef)
    got = R.ref_coalesced(ei[1], ei[0], None, ef, 64, 64)
    assert got["nnz"] == col.size < ei.shape[1] and got["flags"] == 0                       # the multigraph has parallel edges
    assert np.array_equal(got["rowptr"], rowptr) and np.array_equal(got["col"], col) and np.array_equal(got["slot"], slot)
    assert np.array_equal(got["w"], w.astype(np.float32))
    assert np.abs(got["ef"] - efo).max() <= 4 * np.finfo(np.float32).eps * np.abs(efo).max()   # float32 sums of up to a few terms
    for seed, n, edges in ((1, 50, 3000), (2, 700, 20000)):
        rec, snd, wv, ef = multigraph(seed, n, n, edges)
        rowptr, col, w, _, efo, slot = O.coalesce_edge_index(np.stack([snd, rec]), n, edge_values=wv, edge_features=ef)
        got = R.ref_coalesced(rec, snd, wv, ef, n, n)
        assert got["nnz"] == col.size < edges
        assert np.array_equal(got["rowptr"], rowptr) and np.array_equal(got["col"], col) and np.array_equal(got["slot"], slot)
        assert np.array_equal(got["w"], w.astype(np.float32)) and np.array_equal(got["ef"], efo.astype(np.float32))   # dyadic: exact


def test_ref_coalesced_drops_invalid_edges_and_handles_rectangles():
    rec, snd, wv, ef = multigraph(3, 40, 900, 5000, bad=12)
    ok = (rec >= 0) & (rec < 40) & (snd >= 0) & (snd < 900)
    assert (~ok).sum() == 12
    got = R.ref_coalesced(rec, snd, wv, ef, 40, 900)
    keep = R.ref_coalesced(rec[ok], snd[ok], wv[ok], ef[ok], 40, 900)
    assert got["flags"] == R.FLAG_INDEX_RANGE and keep["flags"] == 0
    for k in ("rowptr", "col", "w", "ef"):
        assert np.array_equal(got[k], keep[k]), k
    assert (got["slot"][~ok] == -1).all() and np.array_equal(got["slot"][ok], keep["slot"])
    # every edge's weight lands in its slot's sum
    back = np.zeros(got["nnz"])
    np.add.at(back, got["slot"][ok], wv[ok].astype(np.float64))
    assert np.array_equal(back.astype(np.float32), got["w"])
    assert got["col"].max() > 40                                                              # senders beyond the row range survive
    unit = R.ref_coalesced(rec, snd, None, None, 40, 900)
    assert unit["ef"] is None and np.array_equal(unit["w"], np.bincount(got["slot"][ok], minlength=got["nnz"]).astype(np.float32))


def test_ref_csr_against_a_torch_stable_sort():
    for seed, rows, cols, edges, bad in ((4, 1, 1, 50, 0), (5, 300, 300, 9000, 0), (6, 8, 5000, 4097, 9)):
        rec, snd, wv, _ = multigraph(seed, rows, cols, edges, bad)
        got = R.ref_csr(rec, snd, wv, rows, cols)
        tr, ts, tw = torch.from_numpy(rec), torch.from_numpy(snd), torch.from_numpy(wv)
        ok = (tr >= 0) & (tr < rows) & (ts >= 0) & (ts < cols)
        order = torch.sort(tr[ok], stable=True).indices
        assert got["nnz"] == int(ok.sum()) == edges - bad and got["flags"] == (R.FLAG_INDEX_RANGE if bad else 0)
        assert np.array_equal(got["col"], ts[ok][order].numpy()) and np.array_equal(got["w"].view(np.int32), tw[ok][order].numpy().view(np.int32))
        assert np.array_equal(got["rowptr"], np.concatenate([[0], torch.bincount(tr[ok], minlength=rows).cumsum(0).numpy()]))
        assert R.ref_csr(rec, snd, None, rows, cols)["w"] is None
    w = np.array([1.0, np.inf, 2.0], dtype=np.float32)
    z = np.zeros(3, dtype=np.int64)
    assert R.ref_csr(z, z, w, 1, 1)["flags"] == R.FLAG_W_NONFINITE
    assert R.ref_csr(z, z, np.array([1, np.nan, 2], dtype=np.float32), 1, 1)["flags"] == R.FLAG_W_NONFINITE
    assert R.ref_csr(z, z, np.array([1, -1, 2], dtype=np.float32), 1, 1)["flags"] == R.FLAG_W_NEGATIVE
    assert R.ref_csr(z, z, np.array([1, -0.0, 2], dtype=np.float32), 1, 1)["flags"] == 0
    assert R.ref_csr(z, z + 1, np.array([1, -np.inf, 2], dtype=np.float32), 1, 1)["flags"] == 7    # dropped edges are looked at too


def test_degree_bins_and_ref_bins():
    degs = np.arange(0, 40000)
    vec = R.degree_bins(degs)
    for d in degs:
        assert R.degree_bin(int(d)) == scratch_degree_bin(int(d)) == vec[d], d
    assert R.degree_bin(10 ** 6) == scratch_degree_bin(10 ** 6) == R.degree_bins([10 ** 6])[0] == R.NUM_BINS - 1
    assert len(set(vec.tolist())) == R.NUM_BINS
    # bins per chunk, by the definition: chunk 2 is partial
    rng = np.random.default_rng(9)
    deg = rng.choice([0, 1, 2, 33, 40, 41, 300, 5000], size=5000)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    for chunk_rows in (0, 2048):
        b = R.ref_bins(rowptr, chunk_rows)
        cr = chunk_rows or 5000
        assert b["num_chunks"] == -(-5000 // cr) and b["bin_start"][0, 0] == 0 and b["bin_start"][-1, -1] == 5000
        for c in range(b["num_chunks"]):
            for k in range(R.NUM_BINS):
                want = [r for r in range(c * cr, min((c + 1) * cr, 5000)) if R.degree_bin(int(deg[r])) == k]
                lo, hi = b["bin_start"][c, k], b["bin_start"][c, k + 1]
                assert b["perm"][lo:hi].tolist() == want
            if c:
                assert b["bin_start"][c, 0] == b["bin_start"][c - 1, -1]
        st = b["stats"]
        assert st[R.STAT_MAX_DEGREE] == 5000 and st[R.STAT_NNZ] == deg.sum() and st[R.STAT_NUM_ZERO] == (deg == 0).sum()
        assert st[R.STAT_NUM_REG] == ((deg >= 1) & (deg <= 32)).sum() and st[R.STAT_NUM_LDS] == ((deg > 32) & (deg <= 2048)).sum()
        assert st[R.STAT_NUM_GLOBAL] == (deg > 2048).sum()
        assert R.perm_mismatch(b["perm"], b, chunk_rows) is None
        shuffled = b["perm"].copy()
        lo, hi = b["bin_start"][0, 1], b["bin_start"][0, 2]
        shuffled[lo:hi] = shuffled[lo:hi][::-1]                         # another order inside a bin: still the same sets
        assert R.perm_mismatch(shuffled, b, chunk_rows) is None
        shuffled[[lo, hi]] = shuffled[[hi, lo]]                         # two rows swapped across a bin border
        assert R.perm_mismatch(shuffled, b, chunk_rows) is not None
        dup = b["perm"].copy()
        dup[5] = dup[6]
        assert "permutation" in R.perm_mismatch(dup, b, chunk_rows)


def test_ref_transpose():
    col = np.array([3, 0, -1, 3, 2, 5, 0, 3], dtype=np.int32)
    cptr, order = R.ref_transpose(col, 5)
    assert cptr.tolist() == [0, 2, 2, 3, 6, 6] and order.tolist() == [1, 6, 4, 0, 3, 7]


# rows, edges, weights -> two_level_ok, buckets, partition passes, stage_cap: the shapes of tests/test_hip_graph_build.py
PLAN = [
    (200_000, 900_000, True, True, 98, 1, 11_136),
    (200_000, 1_000_000, False, True, 98, 1, 22_272),
    (40_000, 600_000, False, True, 20, 1, 0),
    (1_100_000, 600_000, True, True, 538, 2, 11_136),
    (32_768, 262_144, False, True, 17, 1, 22_272),
    (32_767, 262_144, False, False, 16, 1, 22_272),
    (32_768, 262_143, False, False, 17, 1, 22_272),
    (40_000, 1_400_000, False, False, 20, 1, 0),
    # the shapes of tests/test_hip_parity.py::test_two_level_graph_build_equals_lsd_build: weighted ones never stage
    (65_535, 400_000, True, True, 32, 1, 0),
    (100_000, 600_000, True, True, 49, 1, 0),
    (70_001, 300_000, False, True, 35, 1, 22_272),
    (3_000_000, 2_000_000, False, True, 1465, 2, 22_272),
]


@pytest.mark.parametrize("rows,edges,weighted,ok,buckets,passes,cap", PLAN)
def test_bucket_plan(rows, edges, weighted, ok, buckets, passes, cap):
    p = R.bucket_plan(rows, edges, weighted)
    assert (p["two_level_ok"], p["buckets"], p["passes"], p["stage_cap"]) == (ok, buckets, passes, cap), p
    k = R.build_constants()
    assert (k["row_bits"], k["waves"], k["tile"], k["lds_kib"], k["pass_bits"]) == (11, 8, 4096, 160, 9)
    assert p["avg"] == -(-edges // buckets) and p["bucket_rows"] == 2048


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-g")], ids=["plain", "sanitized"])
def test_graph_ws_native(tmp_path, flags):
    """tests/native/test_graph_ws.cpp: the workspace layout of csrc/graph_ws.h for 6 x 10 (rows, edges) pairs -- block_sums holds the
    block totals of both scans, head | pos fit the idle value buffer, the regions are disjoint, aligned and inside the total -- as a
    plain executable and once more under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "fsw_test_graph_ws")
    src = os.path.join(ROOT, "tests", "native", "test_graph_ws.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", *flags, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


def test_workspace_query_matches_the_layout():
    """fsw_graph_workspace_bytes (every caller sizes its buffer with it) is the layout's total: a few hundred bytes above the
    radix-only sizing from 262 145 edges on, where the coalescing build's scan needs more block sums."""
    lib = os.path.join(ROOT, "fsw_gnn_amd", "libfsw_hip.so")
    if not os.path.isfile(lib):
        pytest.skip("libfsw_hip.so not built (run __graft_entry__.build())")
    from fsw_gnn_amd import _lib
    L = _lib.lib()

    def up(v):
        return -(-v // 256) * 256

    for rows in (1, 1000, 62_463, 62_464, 200_000, 1 << 24):
        for E in (0, 1, 4096, 4097, 262_144, 262_145, 524_289, 1_310_721, 5_000_000, (1 << 31) - 4097):
            En = max(E, 1)
            nt = -(-En // 4096)
            cap = max(-(-512 * nt // 4096), nt) + 1
            want = 2 * up(4 * En) + 2 * up(8 * En) + up(4 * 512 * nt) + up(4 * cap) + up(4 * ((rows >> 10) + 3)) + 2 * up(4 * 256 * R.NUM_BINS)
            assert int(L.fsw_graph_workspace_bytes(rows, E)) == want, (rows, E)
