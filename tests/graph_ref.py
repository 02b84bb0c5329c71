"""Plain numpy references for csrc/graph_build.hip: the CSR by recipient, the coalescing build, the degree bins with their stats
words, the sender-major transpose, and the plan of the two-level build (which path a shape takes).  Nothing here calls the library;
the cuts of the degree classes are written out as in tests/test_cart_scratch_cpu.py, the constants of the two-level build are read
from the source by regular expression, so that a retuned constant shows up as "this shape no longer reaches the path"."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fsw_gnn_amd", "csrc")

REG_MAX_DEG, LDS_MAX_DEG, HUB_MAX_DEG = 32, 2048, 32768
MID_SIZES = (40, 48, 64, 80, 96, 128, 160, 192, 256)
BIN_MID0 = REG_MAX_DEG + 1
BIN_LDS0 = BIN_MID0 + len(MID_SIZES)
BIN_HUB0 = BIN_LDS0 + 3
BIN_GLOBAL = BIN_HUB0 + 4
NUM_BINS = BIN_GLOBAL + 1
STAT_FLAGS, STAT_MAX_DEGREE, STAT_NUM_ZERO, STAT_NUM_REG, STAT_NUM_LDS, STAT_NUM_GLOBAL, STAT_NNZ = range(7)
FLAG_INDEX_RANGE, FLAG_W_NONFINITE, FLAG_W_NEGATIVE = 1, 2, 4
FLT_MAX = float(np.finfo(np.float32).max)


def degree_bin(deg):
    """csrc/fsw_common.h: degree_bin"""
    if deg <= REG_MAX_DEG:
        return deg
    if deg > HUB_MAX_DEG:
        return BIN_GLOBAL
    if deg > LDS_MAX_DEG:
        return BIN_HUB0 + (deg > 4096) + (deg > 8192) + (deg > 16384)
    if deg > MID_SIZES[-1]:
        return BIN_LDS0 + (deg > 512) + (deg > 1024)
    return BIN_MID0 + sum(deg > s for s in MID_SIZES[:-1])


# upper ends of the bins above the exact-degree bins, in bin order: bin = BIN_MID0 + number of ends below the degree
_UPPER_ENDS = np.array(MID_SIZES + (512, 1024, 2048, 4096, 8192, 16384, 32768), dtype=np.int64)


def degree_bins(deg):
    """degree_bin over an array (checked against the scalar form in tests/test_graph_ref_cpu.py)."""
    deg = np.asarray(deg, dtype=np.int64)
    upper = BIN_MID0 + np.searchsorted(_UPPER_ENDS, deg, side="left")
    return np.where(deg <= REG_MAX_DEG, deg, upper).astype(np.int16)


def _valid(rec, snd, rows, cols):
    return (rec >= 0) & (rec < rows) & (snd >= 0) & (snd < cols)


def _flags(ok, w):
    """Every edge's weight is looked at, dropped edges included (the first pass validates as it reads)."""
    fl = 0 if bool(ok.all()) else FLAG_INDEX_RANGE
    if w is not None and w.size:
        w = np.asarray(w, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            if not bool((np.abs(w) <= np.float32(FLT_MAX)).all()):
                fl |= FLAG_W_NONFINITE
            if bool((w < 0).any()):
                fl |= FLAG_W_NEGATIVE
    return fl


def _rowptr(row, rows):
    return np.concatenate([[0], np.cumsum(np.bincount(row, minlength=rows))]).astype(np.int32)


def ref_csr(rec, snd, w, rows, cols):
    """Edges with an endpoint out of range dropped, the rest sorted by recipient, stably (senders keep edge-list order).
    -> dict(rowptr int32[rows + 1], col int32[nnz], w float32[nnz] or None (gathered: bit-identical), nnz, flags)."""
    rec, snd = np.asarray(rec, dtype=np.int64), np.asarray(snd, dtype=np.int64)
    ok = _valid(rec, snd, rows, cols)
    r = rec[ok]
    order = np.argsort(r, kind="stable")
    wk = None if w is None else np.asarray(w, dtype=np.float32)[ok][order]
    return dict(rowptr=_rowptr(r, rows), col=snd[ok][order].astype(np.int32), w=wk, nnz=int(r.size), flags=_flags(ok, w))


def _run_sums(seg, first, vals, nnz):
    """out[seg[i]] += vals[i] for i = 0, 1, ... in this order, in the precision of vals (runs are contiguous and start where `first`).
    Step k adds the k-th element of every run that has one: at most one addend per run and step, so a vector add keeps the order."""
    out = np.zeros((nnz,) + vals.shape[1:], dtype=vals.dtype)
    if not vals.shape[0]:
        return out
    pos = np.arange(seg.size)
    rank = pos - np.maximum.accumulate(np.where(first, pos, 0))
    by_rank = np.argsort(rank, kind="stable")
    cuts = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2))
    for k in range(cuts.size - 1):
        sel = by_rank[cuts[k]:cuts[k + 1]]
        out[seg[sel]] += vals[sel]
    return out


def ref_coalesced(rec, snd, w, ef, rows, cols):
    """Entries in (recipient, sender) order, one per distinct pair; the weights of a run (1 per edge without w) summed in float64 and
    rounded to float32, the feature vectors summed in float32 in edge-list order.
    -> dict(rowptr, col, w float32[nnz], ef float32[nnz, d] or None, slot int32[E] (-1: dropped edge), nnz, flags)."""
    rec, snd = np.asarray(rec, dtype=np.int64), np.asarray(snd, dtype=np.int64)
    ok = _valid(rec, snd, rows, cols)
    idx = np.flatnonzero(ok)
    key = rec[idx] * np.int64(cols) + snd[idx]
    order = np.argsort(key, kind="stable")
    key = key[order]
    first = np.ones(key.size, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    seg = np.cumsum(first) - 1
    ukey = key[first]
    nnz = int(ukey.size)
    wv = np.ones(idx.size, dtype=np.float64) if w is None else np.asarray(w, dtype=np.float32)[idx][order].astype(np.float64)
    wsum = _run_sums(seg, first, wv, nnz)
    efs = None
    if ef is not None:
        efs = _run_sums(seg, first, np.asarray(ef, dtype=np.float32)[idx][order], nnz)
    slot = np.full(rec.size, -1, dtype=np.int32)
    slot[idx[order]] = seg
    return dict(rowptr=_rowptr(ukey // cols, rows), col=(ukey % cols).astype(np.int32), w=wsum.astype(np.float32), ef=efs, slot=slot,
                nnz=nnz, flags=_flags(ok, w))


def ref_bins(rowptr, chunk_rows=0):
    """Degree bins of a CSR, per chunk of chunk_rows consecutive rows (0: one chunk).
    -> dict(bin_of_row int16[rows], bin_start int32[chunks, NUM_BINS + 1] (offsets into perm, running on from chunk to chunk),
            perm int32[rows] (chunk by chunk, bin by bin, every bin's rows ascending: ONE representative -- inside a bin the library's
            order depends on atomics, compare with perm_mismatch), stats {stat word: value}, num_chunks)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    rows = rowptr.size - 1
    deg = np.diff(rowptr)
    b = degree_bins(deg)
    cr = chunk_rows if chunk_rows else max(rows, 1)
    num_chunks = -(-rows // cr)
    chunk = (np.arange(rows, dtype=np.int64) // cr)
    seg = (chunk * NUM_BINS + b).astype(np.int16 if num_chunks * NUM_BINS < 2 ** 15 else np.int64)
    counts = np.bincount(seg, minlength=num_chunks * NUM_BINS).reshape(num_chunks, NUM_BINS)
    ends = np.cumsum(counts.reshape(-1)).reshape(num_chunks, NUM_BINS)
    bin_start = np.empty((num_chunks, NUM_BINS + 1), dtype=np.int32)
    bin_start[:, 1:] = ends
    bin_start[0, 0] = 0
    bin_start[1:, 0] = ends[:-1, -1]
    tot = counts.sum(axis=0)
    stats = {STAT_MAX_DEGREE: int(deg.max()) if rows else 0, STAT_NUM_ZERO: int(tot[0]), STAT_NUM_REG: int(tot[1:REG_MAX_DEG + 1].sum()),
             STAT_NUM_LDS: int(tot[BIN_MID0:BIN_HUB0].sum()), STAT_NUM_GLOBAL: int(tot[BIN_HUB0:].sum()), STAT_NNZ: int(rowptr[-1])}
    return dict(bin_of_row=b, bin_start=bin_start, perm=np.argsort(seg, kind="stable").astype(np.int32), stats=stats, num_chunks=num_chunks)


def perm_mismatch(perm, bins, chunk_rows=0):
    """None when `perm` lists, in every (chunk, bin) slice of bins['bin_start'], exactly the rows ref_bins puts there (as a set);
    a description of the first difference otherwise.  Equivalent to comparing every slice sorted: perm is a permutation of the
    rows, and every position holds a row of the position's chunk and bin."""
    perm = np.asarray(perm).astype(np.int64)
    rows = bins["bin_of_row"].size
    if perm.size != rows:
        return "perm has %d entries for %d rows" % (perm.size, rows)
    if rows == 0:
        return None
    if perm.min() < 0 or perm.max() >= rows:
        return "perm holds a row outside [0, %d): min %d max %d" % (rows, perm.min(), perm.max())
    if not bool((np.bincount(perm, minlength=rows) == 1).all()):
        return "perm is not a permutation of the rows"
    bs = bins["bin_start"].reshape(-1, NUM_BINS + 1).astype(np.int64)
    cnt = np.diff(bs, axis=1).reshape(-1)
    want_seg = np.repeat(np.arange(cnt.size, dtype=np.int64), cnt)       # (chunk, bin) of every position
    cr = chunk_rows if chunk_rows else rows
    got_seg = (perm // cr) * NUM_BINS + bins["bin_of_row"][perm]
    bad = np.flatnonzero(want_seg != got_seg)
    if bad.size:
        p = int(bad[0])
        return "position %d (chunk %d bin %d) holds row %d of chunk %d bin %d; %d positions differ" % (
            p, want_seg[p] // NUM_BINS, want_seg[p] % NUM_BINS, perm[p], got_seg[p] // NUM_BINS, got_seg[p] % NUM_BINS, bad.size)
    return None


def ref_transpose(col, num_cols):
    """Sender-major view: cptr int32[num_cols + 1], order = the entries sorted by column, stably; entries whose column is out of range
    sort last and belong to no sender (only order[:cptr[num_cols]] is defined)."""
    col = np.asarray(col, dtype=np.int64)
    ok = (col >= 0) & (col < num_cols)
    key = np.where(ok, col, num_cols)
    order = np.argsort(key, kind="stable")
    return _rowptr(col[ok], num_cols), order[:int(ok.sum())].astype(np.int32)


def _key_bits(n):
    b = 1
    while (1 << b) <= n:
        b += 1
    return b


def _constant(src, pattern, what):
    m = re.search(pattern, src)
    assert m, "graph_build.hip / graph_ws.h no longer match %r (%s): update tests/graph_ref.py:bucket_plan" % (pattern, what)
    return int(m.group(1))


def build_constants():
    src = open(os.path.join(CSRC, "graph_build.hip")).read() + open(os.path.join(CSRC, "graph_ws.h")).read()
    two = src[src.index("static bool two_level_ok"):]
    two = two[:two.index("\n}\n")]
    return dict(
        row_bits=_constant(src, r"#define FSW_BUCKET_ROW_BITS (\d+)", "rows per bucket"),
        row_bits_used=bool(re.search(r"constexpr int kBucketMaxRowBits = FSW_BUCKET_ROW_BITS;", src)),
        waves=_constant(src, r"constexpr int kBucketWaves = (\d+);", "wavefronts per bucket"),
        tile=_constant(src, r"constexpr int kRsTile = (\d+);", "edges per tile"),
        lds_kib=_constant(src, r"const size_t room = \(size_t\)(\d+) \* 1024 - 1024 - tables;", "LDS of a workgroup"),
        pass_bits=_constant(src, r"stream, rb, (\d+), &bits\)", "bits of a partition pass"),
        min_rows=1 << _constant(two, r"num_rows < \(1 << (\d+)\)", "two_level_ok rows"),
        min_edges=1 << _constant(two, r"num_edges < \(1 << (\d+)\)", "two_level_ok edges"),
        max_avg=1 << _constant(two, r"num_edges / nbuckets <= \(1 << (\d+)\)", "two_level_ok bucket"),
    )


def bucket_plan(rows, edges, weighted):
    """What fsw_graph_build_two_level does with a shape (sort_and_finish_two_level, recomputed):
    two_level_ok, buckets, passes (partition passes over the upper row bits), stage_cap (entries of the LDS staging tile; 0: none),
    avg (edges per bucket), tiles."""
    k = build_constants()
    assert k["row_bits_used"]
    full = -(-(rows + 1) // (1 << k["row_bits"]))
    ok = rows >= k["min_rows"] and edges >= k["min_edges"] and edges // full <= k["max_avg"]
    rb = min(k["row_bits"], _key_bits(rows))
    buckets = -(-(rows + 1) // (1 << rb))
    upper = _key_bits(rows) - rb
    passes = -(-upper // k["pass_bits"]) if upper > 0 else 0
    tables = 4 * (k["waves"] + 1) * (1 << rb)
    room = k["lds_kib"] * 1024 - 1024 - tables
    size = 8 if weighted else 4
    avg = -(-edges // buckets)
    want = avg + avg // 32 + 256
    return dict(two_level_ok=ok, buckets=buckets, passes=passes, stage_cap=room // size if want * size <= room else 0, avg=avg,
                tiles=-(-edges // k["tile"]), bucket_rows=1 << rb)
