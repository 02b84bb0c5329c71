"""Tensor layouts under which callers hand arguments to the public layers (tests/test_hip_layouts.py), made once on the host.

layout_view(array, name) takes a contiguous numpy array and returns (base, view): CPU torch tensors, `view` a view of `base` that
equals the array.  Every element of `base` outside the view is POISON: NaN for floats, for index tensors an in-range value (0 <=
value < hi) different from both of its neighbours in memory.  Poison is always a value a kernel may read without leaving its
buffers: a mishandled stride shows as a wrong number or as the layers' "NaNs or infs" assertion, never as a fault.

on_device(base, view, device) moves the pair to a device and keeps the geometry (sizes, strides, storage offset); a fresh device
allocation is aligned to 512 bytes, so data_ptr() % 16 of the view is the view's byte offset % 16.

| name       | construction                               | what it breaks if mishandled                                   |
| contig     | the array itself (control)                 | -                                                              |
| colslice   | base[..., 3:3 + d], base 5 columns wider   | row stride != d, pointer 3 elements off 16-byte alignment      |
| rowstep    | base[::2]                                  | stride 2 rows on the first axis                                |
| transposed | baseT.transpose(-1, -2)                    | inner stride != 1 (an [E, 2] index tensor seen as [2, E])      |
| offset1    | contiguous view 1 element into a flat buf  | is_contiguous() true, pointer one element off 16-byte alignment |
| oddslice   | base[3:3 + n] of a longer 1-D tensor       | contiguous, pointer 3 elements off (index vectors, int32 too)  |
| expanded   | x1.expand(B, ...)                          | stride 0 on the first axis                                     |
| batchslice | N-D base[..., :d], base 3 columns wider    | reshape(B * n, d) stays a view                                 |
| widerows   | wide[:, 1:1 + E] with an even row length   | rows of an int64 [2, E] tensor 8- but not 16-byte aligned      |
"""
import numpy as np
import torch

LAYOUTS = ("contig", "colslice", "rowstep", "transposed", "offset1", "oddslice", "expanded", "batchslice", "widerows")
COPIED = ("colslice", "rowstep", "transposed", "expanded", "batchslice", "widerows")    # not is_contiguous(): the layer must copy
COLSLICE_LEFT, COLSLICE_EXTRA, BATCHSLICE_EXTRA, ODD_OFFSET = 3, 5, 3, 3


def _poisoned(shape, dtype, hi):
    """A buffer of poison: NaN, or for integers the in-range sequence (7 i + 1) mod hi (repaired by _finish)."""
    if np.issubdtype(dtype, np.floating):
        return np.full(shape, np.nan, dtype=dtype)
    assert hi is not None and hi >= 3, "index poison needs a range of at least three values"
    return ((np.arange(int(np.prod(shape)), dtype=np.int64) * 7 + 1) % hi).astype(dtype).reshape(shape)


def _finish(base, inside, hi):
    """Index poison differs from both neighbours in memory: bump the entries that do not (at most two bumps each, hi >= 3)."""
    if np.issubdtype(base.dtype, np.floating):
        return base
    flat, keep = base.reshape(-1), inside.reshape(-1)
    for i in np.nonzero(~keep)[0]:
        near = {int(flat[j]) for j in (i - 1, i + 1) if 0 <= j < flat.size}
        while int(flat[i]) in near:
            flat[i] = (int(flat[i]) + 1) % hi
    return base


def layout_view(array, name, hi=None, batch=None):
    """(base, view) of `array` in layout `name`.  hi: index tensors hold values in [0, hi).  batch: the B of 'expanded', whose view
    equals the array repeated B times along a new first axis."""
    a = np.ascontiguousarray(array)
    assert name in LAYOUTS, name
    dt = a.dtype
    if name == "contig":
        base = a.copy()
        inside = np.ones(a.shape, dtype=bool)
        cut = lambda b: b
    elif name == "colslice":
        assert a.ndim >= 2
        base = _poisoned(a.shape[:-1] + (a.shape[-1] + COLSLICE_EXTRA,), dt, hi)
        cut = lambda b: b[..., COLSLICE_LEFT:COLSLICE_LEFT + a.shape[-1]]
    elif name == "rowstep":
        base = _poisoned((2 * a.shape[0],) + a.shape[1:], dt, hi)
        cut = lambda b: b[::2]
    elif name == "transposed":
        assert a.ndim >= 2
        base = _poisoned(a.shape[:-2] + (a.shape[-1], a.shape[-2]), dt, hi)
        cut = lambda b: b.swapaxes(-1, -2) if isinstance(b, np.ndarray) else b.transpose(-1, -2)
    elif name == "offset1":
        base = _poisoned((a.size + 4,), dt, hi)
        cut = lambda b: b[1:1 + a.size].reshape(a.shape)
    elif name == "oddslice":
        assert a.ndim == 1
        base = _poisoned((a.size + 2 * ODD_OFFSET,), dt, hi)
        cut = lambda b: b[ODD_OFFSET:ODD_OFFSET + a.size]
    elif name == "expanded":
        assert batch is not None and batch >= 2
        base = a.copy()                          # every element is in the view, B times
        cut = lambda b: (np.broadcast_to(b, (batch,) + a.shape) if isinstance(b, np.ndarray) else b.expand((batch,) + a.shape))
    elif name == "batchslice":
        assert a.ndim >= 3
        base = _poisoned(a.shape[:-1] + (a.shape[-1] + BATCHSLICE_EXTRA,), dt, hi)
        cut = lambda b: b[..., :a.shape[-1]]
    else:  # widerows
        assert a.ndim == 2
        E = a.shape[1]
        base = _poisoned((a.shape[0], E + 2 + (E & 1)), dt, hi)       # even row length: row r starts r * width + 1 elements in
        cut = lambda b: b[:, 1:1 + E]
    if name not in ("contig", "expanded"):
        inside = np.zeros(base.shape, dtype=bool)
        cut(inside)[...] = True
        cut(base)[...] = a
        _finish(base, inside, hi)
    tb = torch.from_numpy(base)
    return tb, cut(tb)


def outside_mask(base, view):
    """Boolean tensor of the shape of `base`: True where an element of base is not an element of the view."""
    mask = torch.ones(base.shape, dtype=torch.bool, device=base.device)
    torch.as_strided(mask, view.shape, view.stride(), view.storage_offset()).fill_(False)
    return mask


def on_device(base, view, device, requires_grad=False):
    """The pair on `device` with the geometry kept.  requires_grad: base becomes a leaf that requires grad, view a differentiable view
    of it (base.grad then shows where the gradient of the view landed)."""
    b = (base.clone() if base.device == torch.device(device) else base.to(device)).requires_grad_(requires_grad)
    assert b.is_contiguous() and b.storage_offset() == 0
    return b, torch.as_strided(b, view.shape, view.stride(), view.storage_offset())


def bits(t):
    """The bytes of a tensor's elements (NaN payloads included) as a host array, for bit-for-bit comparisons of poisoned buffers."""
    return t.detach().contiguous().cpu().numpy().view(np.uint8).copy()


# ---- the inputs of tests/test_hip_layouts.py and tests/test_hip_streams.py ---------------------------------------------------------
N_VERT, D_INS, CLOUDS, CLOUD_POINTS, D_EDGE = 2200, (12, 7), 3, 300, 3
CUT_DEGREES = (0, 1, 2, 31, 32, 33, 256, 257, 2048, 2049)      # one row on each side of the register, mid, wave-sort and hub cuts
DENSE_ROWS = 64                                                 # recipients of the dense graph-mode W: the cut rows and 54 short ones
READOUT_SIZES = (0, 1, 40, 2100, 59)                            # graphs of the readout; they sum to N_VERT
_CACHE = {}


def graph(short=False):
    """The adjacency by recipient as CSR: rows 0..9 have the CUT_DEGREES, every other row r has r % 16 senders (short: every row r has
    r % 33, nothing above the register cut).  Distinct, increasing senders in every row.  Returns dict(rowptr, col, rec, deg)."""
    key = ("graph", short)
    if key not in _CACHE:
        rng = np.random.default_rng(41 + short)
        deg = np.arange(N_VERT) % (33 if short else 16)
        if not short:
            deg[:len(CUT_DEGREES)] = CUT_DEGREES
        col = np.concatenate([np.sort(rng.choice(N_VERT, size=k, replace=False)) for k in deg]).astype(np.int64)
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        _CACHE[key] = dict(rowptr=rowptr, col=col, rec=np.repeat(np.arange(N_VERT), deg).astype(np.int64), deg=deg)
    return _CACHE[key]


def _normal(seed, shape, dtype=np.float32):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


def _arguments():
    """name -> (array, layouts, hi, batch): every (layout, dtype, shape) the GPU tests use; tests/test_layout_cases_cpu.py checks each."""
    g, gs = graph(), graph(short=True)
    nnz = g["col"].size
    nd = int(g["rowptr"][DENSE_ROWS])                     # entries of the first DENSE_ROWS recipients
    rng = np.random.default_rng(43)
    w = (rng.random(nnz) + 0.25).astype(np.float32)
    plane = ("contig", "colslice", "rowstep", "transposed", "offset1")
    vec = ("contig", "rowstep", "offset1", "oddslice")
    args = {}
    for d in D_INS:
        args["X%d" % d] = (_normal(50 + d, (N_VERT, d)), plane, None, None)
        args["Xb%d" % d] = (_normal(60 + d, (CLOUDS, CLOUD_POINTS, d)), plane + ("batchslice",), None, None)
        args["x1_%d" % d] = (_normal(70 + d, (CLOUD_POINTS, d)), ("expanded",), None, CLOUDS)
        args["x1_%d_rep" % d] = (np.ascontiguousarray(np.broadcast_to(args["x1_%d" % d][0], (CLOUDS, CLOUD_POINTS, d))), ("contig",), None, None)
    args["X12_f64"] = (_normal(50 + 12, (N_VERT, 12)).astype(np.float64), plane, None, None)
    args["Wb"] = ((rng.random((CLOUDS, CLOUD_POINTS)) + 0.1).astype(np.float32), plane, None, None)
    args["w1"] = ((rng.random(CLOUD_POINTS) + 0.1).astype(np.float32), ("expanded",), None, CLOUDS)
    args["w1_rep"] = (np.ascontiguousarray(np.broadcast_to(args["w1"][0], (CLOUDS, CLOUD_POINTS))), ("contig",), None, None)
    Wd = np.zeros((DENSE_ROWS, N_VERT), dtype=np.float32)
    Wd[g["rec"][:nd], g["col"][:nd]] = w[:nd]
    args["Wdense"] = (Wd, plane, None, None)
    args["Wdense_f64"] = (Wd.astype(np.float64), plane, None, None)
    args["wvals"] = (w, vec, None, None)
    args["wvals_f64"] = (w.astype(np.float64), vec, None, None)
    ef = _normal(44, (nnz, D_EDGE))
    args["efvals"] = (ef, plane, None, None)
    Xe = np.zeros((DENSE_ROWS, N_VERT, D_EDGE), dtype=np.float32)
    Xe[g["rec"][:nd], g["col"][:nd]] = ef[:nd]
    args["Xedge_dense"] = (Xe, plane + ("batchslice",), None, None)
    for tag, gr in (("", g), ("_short", gs)):
        p = np.random.default_rng(45).permutation(gr["col"].size)
        ei = np.stack([gr["col"][p], gr["rec"][p]])                       # row 0 = sender, row 1 = recipient, shuffled
        args["edge_index" + tag] = (ei, plane + ("widerows",), N_VERT, None)
        args["perm" + tag] = (p, ("contig",), None, None)
    args["edge_features"] = (_normal(46, (nnz, D_EDGE)), plane, None, None)
    for it in (np.int32, np.int64):
        tag = "_i%d" % (8 * np.dtype(it).itemsize)
        args["rowptr" + tag] = (g["rowptr"].astype(it), vec, nnz + 1, None)
        args["col" + tag] = (g["col"].astype(it), vec, N_VERT, None)
        args["ptr" + tag] = (np.concatenate([[0], np.cumsum(READOUT_SIZES)]).astype(it), vec, N_VERT + 1, None)
    args["graph_index"] = (np.repeat(np.arange(len(READOUT_SIZES)), READOUT_SIZES).astype(np.int64), vec, len(READOUT_SIZES), None)
    assert sum(READOUT_SIZES) == N_VERT
    return args


def arguments():
    if "args" not in _CACHE:
        _CACHE["args"] = _arguments()
    return _CACHE["args"]


def array(name):
    """The contiguous array of an argument (for 'expanded': the one repeated element)."""
    return arguments()[name][0]


def layouts(name):
    return arguments()[name][1]


def case(name, layout):
    """(base, view) of argument `name` in `layout`, on the host."""
    a, allowed, hi, batch = arguments()[name]
    assert layout in allowed, (name, layout)
    made = _CACHE.setdefault("cases", {})
    if (name, layout) not in made:
        made[(name, layout)] = layout_view(a, layout, hi=hi, batch=batch)
    return made[(name, layout)]
