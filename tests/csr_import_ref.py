"""Plain numpy restatement of fsw_graph_import_csr (include/fsw_hip.h, csrc/graph_import.hip): the entries, weights and slots of the
imported graph, its flags and the empty-graph rule.  Nothing here calls the library.  tests/test_csr_import_cpu.py pins it to
graph_ref.ref_csr / ref_coalesced of the corresponding edge lists, tests/test_hip_csr_import.py compares the library to it."""
import numpy as np

from tests import graph_ref as R

FLAG_INDEX_RANGE, FLAG_W_NONFINITE, FLAG_W_NEGATIVE = R.FLAG_INDEX_RANGE, R.FLAG_W_NONFINITE, R.FLAG_W_NEGATIVE
FLAG_CSR_MALFORMED, FLAG_CSR_COL_ORDER, FLAG_W_NONUNIT = 16, 32, 64
BAD = FLAG_CSR_MALFORMED | FLAG_INDEX_RANGE | FLAG_CSR_COL_ORDER        # any of these: the imported graph is empty
FLT_MAX = R.FLT_MAX


def edges_to_csr(rec, snd, w, rows):
    """Stable sort by recipient: the CSR a user would hold for the edge list.  -> (rowptr int64, col int64, w or None, order)"""
    rec = np.asarray(rec, dtype=np.int64)
    order = np.argsort(rec, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rec, minlength=rows))]).astype(np.int64)
    return rowptr, np.asarray(snd, dtype=np.int64)[order], None if w is None else np.asarray(w, dtype=np.float32)[order], order


def weight_flags(w):
    w = np.asarray(w, dtype=np.float32)
    fl = 0
    with np.errstate(invalid="ignore"):
        if w.size and not bool((np.abs(w) <= np.float32(FLT_MAX)).all()):
            fl |= FLAG_W_NONFINITE
        if w.size and bool((w < 0).any()):
            fl |= FLAG_W_NEGATIVE
    return fl


def structure_flags(rowptr, col, rows, cols, nnz, strict):
    """MALFORMED / INDEX_RANGE / COL_ORDER.  COL_ORDER is only defined for a well-formed rowptr (rows are not known otherwise)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    fl = 0
    if rowptr[0] != 0 or rowptr[rows] != nnz or bool((rowptr < 0).any()) or bool((np.diff(rowptr) < 0).any()):
        fl |= FLAG_CSR_MALFORMED
    if col is not None:
        col = np.asarray(col, dtype=np.int64)
        if bool(((col < 0) | (col >= cols)).any()):
            fl |= FLAG_INDEX_RANGE
        if strict and not fl & FLAG_CSR_MALFORMED and nnz > 1:
            row = np.repeat(np.arange(rows), np.diff(rowptr))
            if bool(((row[1:] == row[:-1]) & (col[1:] <= col[:-1])).any()):
                fl |= FLAG_CSR_COL_ORDER
    return fl


def ref_import(rowptr, col, w, rows, cols, self_loop_weight=0.0, gcn=False, strict=False):
    """-> dict(rowptr int32[rows + 1], col int32[nnz_out], w float32[nnz_out] or None (unit result), w64 float64 (the 'gcn' weights
    before rounding; None without gcn), slot int32[nnz_in], nnz, flags).  col None: the identity (nnz_in = cols)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nnz = int(cols) if col is None else int(np.asarray(col).size)
    fl = structure_flags(rowptr, col, rows, cols, nnz, strict)
    if w is not None and bool((np.asarray(w, dtype=np.float32) != np.float32(1)).any()):
        fl |= FLAG_W_NONUNIT
    if fl & BAD:
        return dict(rowptr=np.zeros(rows + 1, dtype=np.int32), col=np.zeros(0, dtype=np.int32), w=None, w64=None,
                    slot=None, nnz=0, flags=fl)
    c = np.arange(nnz, dtype=np.int64) if col is None else np.asarray(col, dtype=np.int64)
    sl = np.float32(self_loop_weight)
    loops = float(sl) != 0.0
    weighted = w is not None or loops or gcn
    wv = np.ones(nnz, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    deg_in = np.diff(rowptr)
    row = np.repeat(np.arange(rows, dtype=np.int64), deg_in)
    e = np.arange(nnz, dtype=np.int64)
    if not loops:
        out_ptr, slot, oc, ow = rowptr, e, c, wv
    elif not strict:
        out_ptr = rowptr + np.arange(rows + 1)
        slot = e + row
        oc = np.empty(nnz + rows, dtype=np.int64)
        ow = np.empty(nnz + rows, dtype=np.float32)
        oc[slot], ow[slot] = c, wv
        at = rowptr[1:] + np.arange(rows)                       # the last entry of every row
        oc[at], ow[at] = np.arange(rows), sl
    else:
        is_diag = c == row
        has = np.bincount(row[is_diag], minlength=rows) > 0
        ins = (~has).astype(np.int64)
        shift = np.concatenate([[0], np.cumsum(ins)])
        out_ptr = rowptr + shift
        slot = e + shift[row] + ((c > row) & ~has[row])
        total = nnz + int(ins.sum())
        oc = np.empty(total, dtype=np.int64)
        ow = np.empty(total, dtype=np.float32)
        oc[slot] = c
        ow[slot] = np.where(is_diag, (wv.astype(np.float64) + np.float64(sl)).astype(np.float32), wv)
        below = np.bincount(row[c < row], minlength=rows)       # entries in front of the inserted loop
        at = (out_ptr[:-1] + below)[~has]
        oc[at], ow[at] = np.arange(rows)[~has], sl
    w64 = None
    if gcn:
        orow = np.repeat(np.arange(rows, dtype=np.int64), np.diff(out_ptr))
        deg = np.bincount(orow, weights=ow.astype(np.float64), minlength=rows)
        with np.errstate(divide="ignore", invalid="ignore"):
            w64 = ow.astype(np.float64) / np.sqrt(deg[orow]) / np.sqrt(deg[oc])
            ow = w64.astype(np.float32)
    if weighted:
        fl |= weight_flags(ow)
    return dict(rowptr=out_ptr.astype(np.int32), col=oc.astype(np.int32), w=ow if weighted else None, w64=w64,
                slot=slot.astype(np.int32), nnz=int(out_ptr[-1]), flags=fl)
