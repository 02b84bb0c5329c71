"""FSW_embedding: host-side mirror of the reference's FSW_embedding module (reference fsw_embedding.py:169-1144)
over the hand-written HIP kernels of libfsw_hip.so.

Same constructor arguments, parameter names (projVecs, freqs, bias, total_mass_encoding_scale -- state_dict
compatible, reference fsw_embedding.py:397-409), forward signature and assertion messages as the reference.
The computation is NOT the reference's chain of torch.sparse_coo operations: forward() builds a CSR adjacency
(graph.py), projects the points with fp32 MFMA (fsw_project_f32) and runs the fused per-neighbourhood
sort + cumulative-sum + Fourier readout kernels (fsw_embed_f32).  There is no CPU or pure-PyTorch fallback:
tensors must live on a HIP device and the native library must be present.

Autograd: forward under grad mode goes through _EmbedGraphFn (HIP backward kernels, csrc/embed_bwd.hip and
csrc/embed_wsort_bwd.hip) for every weight mode and degree class; gradients flow to X, projVecs, freqs, bias and the
total-mass scale (the weights W are constants).
Edge features (d_edge > 0) go through the coalescing CSR build and the general-weight kernels.
dtype=torch.float64 modules and gradients w.r.t. the weights W / sparse edge features run on the generic kernels
(csrc/embed_generic.hip: any degree, float64 arithmetic) through _GenericEmbedFn, which also serves Cartesian mode below (the same kernel).
The 'homog' / 'homog_alt' total-mass methods are one epilogue in torch (_homog_epilogue) on the kernels' 'plain' output: in place
for inference, out of place under autograd.  Nothing per call is kept on the module: what a call needs travels as arguments.

Cartesian mode, FSW_embedding(d_in, nSlices=S, nFreqs=F, collapse_freqs=...) (reference fsw_embedding.py:153-160, 241-259):
every slice is sorted once and read out at all F frequencies (csrc/embed_cart.hip); output (<batch>, [nR,] S, F), or
(<batch>, [nR,] S*F + mass_dim) collapsed, column s*F + f (after the mass column).  float32 calls run on the tuned kernels, under
autograd through _CartEmbedFn (backward kernels of csrc/embed_cart_bwd.hip, the key gradients summed sender by sender without
float atomics; gradients for X, projVecs, freqs, bias and the total-mass scale); float64 modules and calls whose W requires grad
run on the generic Cartesian kernel (_GenericEmbedFn).  Lines above 2048 elements have kernels of their own (csrc/embed_cart_hub*.hip:
forward, the line in the registers of 2 .. 16 wavefronts; backward, one wavefront per line in a scratch line).  Longer ones, of any
length, are sorted in blocks in a scratch line per workgroup in both directions (forward: csrc/embed_giant_cart.hip,
csrc/embed_giant_cart_w.hip; backward: csrc/embed_giant_cart_bwd.hip), so a float32 call with constant W runs the generic kernel
nowhere.  The library's table (csrc/embed_cart.h: kCartLong) says which rows go where, the host layer only asks it for the scratch
sizes (_cart_forward_scratch_bytes, _cart_backward_scratch_bytes).  One policy is the host's (_cart_split): a forward whose unit-weight
rows above 32768 neighbours make few (row, slice) lines -- one point cloud, one graph under FSW_readout -- asks for their split form
(csrc/embed_split_cart.hip: every phase a launch over (line, block), so one line fills the chip), and so does its backward
(_cart_split_backward, csrc/embed_split_cart_bwd.hip); general weights -- a weight tensor, W = 'uniform', total_mass_pad_thresh > 1 --
have split forms of their own in both directions (forward: _cart_split_w, csrc/embed_split_cart_w.hip; backward:
_cart_split_w_backward, csrc/embed_split_cart_w_bwd.hip).  It needs a HIP device at construction (this
package has no CPU path in any mode).  Edge features (d_edge > 0) in Cartesian mode are opt-in (cartesian_edge_features=True; the
constructor raises NotImplementedError without it, as it always did): the coalescing build as in diagonal mode, then
fsw_edge_keys_f32 (csrc/edge_keys.hip) stores the key of every CSR entry once, K[e, s] = Xp[col[e], s] + <ef[e], projVecs[s, d_in:]>
(prepare_cartesian / _edge_keys), and the same tuned kernels run on K with the identity as their column array in both directions
(_CartEdgeEmbedFn; every serialize_num_slices chunk forms its own K); float64 modules and calls whose W or X_edge requires grad give
the generic kernel the same keys (_GenericEmbedFn).  Two deliberate
differences from the reference: sparse-COO W works (same result as dense W), and collapsed + total mass +
bias works with the bias of shape (S*F + 1,) that generate_embedding_parameters creates.
"""
import ctypes
import numbers
import os
import struct

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .coherence import minimize_mutual_coherence
from .graph import CSRGraph, build_csr, build_csr_coalesced, import_csr

version = "0.1-mi355x"

# Same role as the reference's module flag (fsw_embedding.py:109): validate user input on every forward.
# The checks are fused into the HIP kernels (flags word read back once), not separate isnan/isinf scans.
fsw_embedding_basic_safety_checks = True

_MASS_FN = {"identity": 0, "sqrt": 1, "log": 2}


def _mass_f(fn, m):
    """f(m) of total_mass_encoding_function fn, the host-side twin of the kernels' mass_fn."""
    return m if fn == 'identity' else (2 * (m / (torch.sqrt(m + 1) + 1)) if fn == 'sqrt' else torch.log1p(m))


def _mass_df(fn, m):
    """f'(m)."""
    return torch.ones_like(m) if fn == 'identity' else (1 / torch.sqrt(m + 1) if fn == 'sqrt' else 1 / (1 + m))


def _round_up(v, m):
    return (v + m - 1) // m * m


def _grad_x(L, gXp, S, ldp, V, stream):
    """gX = gXp[:, :S] . V  ([n, S] x [S, d_in]).  The projection kernel (bf16x3 on the matrix cores, fp32-accurate) takes it as
    a projection of the rows of gXp onto the d_in "slices" V^T when the shapes suit it (S <= 256, 16-byte rows); hipBLASLt's
    fp32 GEMM otherwise (2.8 ms against 0.6 ms at 1M rows, S = 256, d_in = 128)."""
    n, d_in = gXp.shape[0], V.shape[1]
    if S % 4 == 0 and S <= 256 and ldp % 4 == 0 and d_in >= 1 and n >= 1:
        Vt = V.t().contiguous()                                   # [d_in, S]
        ldo = _round_up(d_in, 32)
        out = torch.empty((n, ldo), dtype=torch.float32, device=gXp.device)
        _lib.check(L.fsw_project_f32(_lib.ptr(gXp), n, S, ldp, _lib.ptr(Vt), d_in, S, _lib.ptr(out), ldo, None, 0, None, stream),
                   "fsw_project_f32")
        return out if ldo == d_in else out[:, :d_in].contiguous()
    return gXp[:, :S] @ V


GEMM_TN_MIN_ROWS = 1 << 16   # below this the BLAS GEMM is as good


def gemm_tn(A, B):
    """A^T . B for tall row-major A [K, M], B [K, N] (float32, unit inner stride): csrc/gemm_tn.hip when the result fits its 16 blocks
    of 64 x 64 and K is large (the weight-gradient shape: 1M rows x 256 x 128), the BLAS GEMM otherwise."""
    K, M = A.shape
    N = B.shape[1]
    blocks = -(-M // 64) * -(-N // 64)
    if (A.is_cuda and K >= GEMM_TN_MIN_ROWS and blocks <= 16 and not os.environ.get("FSW_GEMM_TN_OFF") and A.dtype == torch.float32 and B.dtype == torch.float32
            and A.stride(1) == 1 and B.stride(1) == 1 and B.shape[0] == K):
        L = _lib.lib()
        C = torch.empty((M, N), dtype=torch.float32, device=A.device)
        wsb = int(L.fsw_gemm_tn_workspace_bytes(M, N))
        ws = torch.empty(wsb, dtype=torch.uint8, device=A.device)
        _lib.check(L.fsw_gemm_tn_f32(_lib.ptr(A), A.stride(0), _lib.ptr(B), B.stride(0), K, M, N, _lib.ptr(C), N, 0.0, _lib.ptr(ws), wsb,
                                     torch.cuda.current_stream(A.device).cuda_stream), "fsw_gemm_tn_f32")
        return C
    return A.t() @ B


class LinearTallFn(torch.autograd.Function):
    """y = h . W^T + b like torch.nn.functional.linear, with the weight gradient gW = gy^T . h -- a reduction over the ROWS, a million
    of them in a training step at BASELINE config 3 -- on gemm_tn instead of the BLAS library's split-K (reference fsw_conv.py:361:
    the first Linear layer of the MLP applied to cat((emb, vertex_features)))."""

    @staticmethod
    def forward(ctx, h, W, b):
        ctx.save_for_backward(h, W)
        ctx.has_bias = b is not None
        return torch.addmm(b, h, W.t()) if b is not None else h @ W.t()

    @staticmethod
    def backward(ctx, gy):
        h, W = ctx.saved_tensors
        gy = gy.contiguous()
        gh = gy @ W if ctx.needs_input_grad[0] else None
        gW = gemm_tn(gy, h) if ctx.needs_input_grad[1] else None
        gb = gy.sum(dim=0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return gh, gW, gb


class LinearSplitTallFn(torch.autograd.Function):
    """y = [scale * emb | x] . W^T + b without building the concatenation (reference fsw_conv.py:357-361: torch.cat((mw * emb,
    vertex_features)) followed by mlp[0]): two GEMMs on the operands where they lie, weight gradient blocks on gemm_tn.  Saves the
    [n, embed_dim + in_channels] buffer, its copy kernel and the slicing copies of its backward (0.8 + 0.5 ms at config 3)."""

    @staticmethod
    def forward(ctx, emb, x, W, b, scale):
        E = emb.shape[1]
        ctx.save_for_backward(emb, x, W)
        ctx.scale, ctx.has_bias = float(scale), b is not None
        y = torch.addmm(b, x, W[:, E:].t()) if b is not None else x @ W[:, E:].t()
        return y.addmm_(emb, W[:, :E].t(), alpha=float(scale))

    @staticmethod
    def backward(ctx, gy):
        emb, x, W = ctx.saved_tensors
        E = emb.shape[1]
        gy = gy.contiguous()
        gemb = (gy @ W[:, :E]).mul_(ctx.scale) if ctx.needs_input_grad[0] else None
        gx = gy @ W[:, E:] if ctx.needs_input_grad[1] else None
        gW = None
        if ctx.needs_input_grad[2]:
            gW = torch.empty_like(W)
            gW[:, :E] = gemm_tn(gy, emb).mul_(ctx.scale)
            gW[:, E:] = gemm_tn(gy, x)
        gb = gy.sum(dim=0) if (ctx.has_bias and ctx.needs_input_grad[3]) else None
        return gemb, gx, gW, gb, None


class _EmbedGraphFn(torch.autograd.Function):
    """out = out_scale * E(X, graph) with gradients for X, projVecs, freqs, bias and the total-mass scale.

    Forward runs the same HIP kernels as inference (prepare + embed_into); backward runs csrc/embed_bwd.hip
    (neighbourhood ranks recomputed in registers, one wave-wide float atomic per neighbour into gXp) and two plain
    GEMMs.  Replaces the reference's chain of sparse autograd Functions (fsw_embedding.py:1232-2257).
    Every weight mode and degree class is supported (unit-weight register rows use the float64 coefficient tables, weighted
    rows and rows above 32 neighbours evaluate the coefficients in float64 on the fly); the weights themselves are
    constants (no gradient w.r.t. W); the 'homog' mass encodings are differentiated by embed_autograd on top of this.

    slice_range = (ka, kb): only slices ka..kb-1 (multi-GPU slice sharding, dist.py): the output is
    [mass column | slices ka..kb-1] and the parameter gradients are full-size tensors that are zero outside the block.
    With reduce_grads the block gradients of all ranks of `group` are summed by all_reduce inside backward, so that every rank ends with
    the gradients one GPU would compute (the mass column, replicated on every rank, is counted once).
    epilogue = False: 'homog' / 'homog_alt' -- embed_autograd asks for the 'plain' embedding without bias (`bias` is None) and
    applies the epilogue with differentiable torch ops on top of it.
    """

    @staticmethod
    def forward(ctx, X, projVecs, freqs, bias, mass_scale, edge_feat, module, graph, out_scale, slice_range, group, reduce_grads,
                epilogue):
        ka, kb = (0, module.nSlices) if slice_range is None else slice_range
        with torch.no_grad():
            prepared = module.prepare(X, graph, slice_range=slice_range)
            out = torch.empty((graph.num_rows, module.total_mass_encoding_dim + kb - ka), dtype=X.dtype, device=X.device)
            module.embed_into(X, graph, out, out_scale=out_scale, prepared=prepared, epilogue=epilogue)
        ctx.module, ctx.graph, ctx.prepared, ctx.out_scale = module, graph, prepared, float(out_scale)
        ctx.slice_range, ctx.group, ctx.reduce_grads = (ka, kb), group, bool(reduce_grads)
        ctx.num_edge_rows = 0 if edge_feat is None else edge_feat.shape[0]
        ctx.save_for_backward(X, projVecs, freqs)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        module, graph, prepared, out_scale = ctx.module, ctx.graph, ctx.prepared, ctx.out_scale
        X, Vfull, freqs_full = ctx.saved_tensors
        ka, kb = ctx.slice_range
        group = ctx.group
        sharded = ctx.reduce_grads        # group may be None = the default process group
        L = _lib.lib()
        S, has_mass = kb - ka, module.total_mass_encoding_dim
        V = Vfull.detach()[ka:kb]
        fr = freqs_full.detach()[ka:kb].contiguous()
        g = g.contiguous()
        stream = torch.cuda.current_stream(X.device).cuda_stream
        ldp, Xp, table, st = prepared["ldp"], prepared["Xp"], prepared["table"], prepared["stats"]
        gX = gV = gfreqs = gbias = gscale = None
        need_xp = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        gEf = None
        gVb = gfb = None          # block gradients (rows ka..kb-1 of projVecs, entries ka..kb-1 of freqs)
        has_ef = graph.ef is not None
        if S > 0 and (need_xp or ctx.needs_input_grad[2] or (has_ef and ctx.needs_input_grad[5])):
            nnz = st[_lib.STAT_NNZ]
            scratch = None
            if st[_lib.STAT_NUM_GLOBAL] > 0:
                scratch = torch.empty(int(L.fsw_embed_scratch_bytes(st[_lib.STAT_MAX_DEGREE])), dtype=torch.uint8, device=X.device)
            gf = torch.zeros(S, dtype=torch.float32, device=X.device)
            a = module.make_args(graph, st, Xp, ldp, fr, S, table, None, 0, None, out_scale, has_mass, scratch, slice_offset=ka)
            if has_ef:
                # edge features: the kernels store the gradient of every key; everything else is index_add + three GEMMs
                gkey = torch.zeros((max(nnz, 1), S), dtype=torch.float32, device=X.device)
                _lib.check(L.fsw_embed_backward_keys_f32(ctypes.byref(a), None, _lib.ptr(g), g.stride(0), _lib.ptr(gkey), S, _lib.ptr(gf),
                                                         stream), "fsw_embed_backward_keys_f32")
                gkey, ef = gkey[:nnz], graph.ef[:nnz]
                if need_xp:
                    gXp = torch.zeros((X.shape[0], S), dtype=torch.float32, device=X.device).index_add_(0, graph.col[:nnz].long(), gkey)
                    if ctx.needs_input_grad[0]:
                        gX = gXp @ V[:, :module.d_in]
                    if ctx.needs_input_grad[1]:
                        gVb = torch.cat([gXp.t() @ X.detach(), gkey.t() @ ef], dim=1)
                if ctx.needs_input_grad[5]:
                    slot = graph.slot_of_edge[:ctx.num_edge_rows].long()
                    gslots = gkey @ V[:, module.d_in:]
                    gEf = torch.where((slot >= 0)[:, None], gslots[slot.clamp(min=0)], torch.zeros((), device=X.device))
            else:
                gXp = torch.zeros((X.shape[0], ldp), dtype=torch.float32, device=X.device)
                dtable = None
                if prepared["unit_fast"]:
                    dtable = torch.empty_like(table)
                    _lib.check(L.fsw_unit_dcoeff_table(_lib.ptr(fr), S, _lib.REG_MAX_DEG, _lib.ptr(dtable), ldp, stream),
                               "fsw_unit_dcoeff_table")
                if prepared["unit_fast"] and need_xp and 0 < nnz * S * 4 <= module.store_sum_budget(X.device):
                    # store-and-sum: every neighbour's key gradient is stored once (plain stores), then summed sender by sender over
                    # the sender-major entry list -- no float atomics, reproducible gradients
                    gkey = torch.empty((nnz, S), dtype=torch.float32, device=X.device)
                    cptr, order = graph.sender_major()
                    _lib.check(L.fsw_embed_backward_keys_f32(ctypes.byref(a), _lib.ptr(dtable), _lib.ptr(g), g.stride(0), _lib.ptr(gkey), S,
                                                             _lib.ptr(gf), stream), "fsw_embed_backward_keys_f32")
                    _lib.check(L.fsw_segment_sum_rows_f32(_lib.ptr(gkey), S, _lib.ptr(cptr), _lib.ptr(order), graph.num_cols, nnz, S,
                                                          _lib.ptr(gXp), ldp, stream), "fsw_segment_sum_rows_f32")
                    del gkey
                else:
                    _lib.check(L.fsw_embed_backward_f32(ctypes.byref(a), _lib.ptr(dtable), _lib.ptr(g), g.stride(0), _lib.ptr(gXp), ldp,
                                                        _lib.ptr(gf), stream), "fsw_embed_backward_f32")
                if ctx.needs_input_grad[0]:
                    gX = _grad_x(L, gXp, S, ldp, V[:, :module.d_in], stream)
                if ctx.needs_input_grad[1]:
                    gVb = gemm_tn(gXp[:, :S], X.detach())
            if ctx.needs_input_grad[2]:
                gfb = gf
        # block gradients -> full-size parameter gradients (zero outside the block), summed over the ranks when sharded
        if ctx.needs_input_grad[0] and gX is None:
            gX = torch.zeros_like(X)
        if ctx.needs_input_grad[5] and gEf is None:
            gEf = torch.zeros((ctx.num_edge_rows, module.d_edge), dtype=X.dtype, device=X.device)
        if ctx.needs_input_grad[1]:
            gV = torch.zeros_like(Vfull)
            if gVb is not None:
                gV[ka:kb] = gVb
        if ctx.needs_input_grad[2]:
            gfreqs = torch.zeros_like(freqs_full)
            if gfb is not None:
                gfreqs[ka:kb] = gfb
        if ctx.needs_input_grad[3]:
            gbias = torch.zeros(has_mass + module.nSlices, dtype=g.dtype, device=g.device)
            gb = out_scale * g.sum(dim=0)
            if has_mass and ((not sharded) or dist.get_rank(group) == 0):
                gbias[0] = gb[0]                       # replicated column: counted once in the sum over the ranks
            gbias[has_mass + ka:has_mass + kb] = gb[has_mass:]
        if ctx.needs_input_grad[4]:
            deg = (graph.rowptr[1:] - graph.rowptr[:-1]).long()
            if graph.w is None:
                m = deg.to(torch.float32)                                  # unit weights: total mass = in-degree
            else:
                rows = torch.repeat_interleave(torch.arange(graph.num_rows, device=X.device), deg)
                m = torch.zeros(graph.num_rows, dtype=torch.float32, device=X.device).index_add_(0, rows, graph.w[:rows.numel()])
            fm = _mass_f(module.total_mass_encoding_function, m)
            gscale = (out_scale * (g[:, 0] * fm).sum()).reshape(())     # identical on every rank: no reduction
        if sharded:
            for t in (gX, gV, gfreqs, gbias, gEf):
                if t is not None:
                    dist.all_reduce(t, group=group)
        return gX, gV, gfreqs, gbias, gscale, gEf, None, None, None, None, None, None, None


class _EmbedGraphWFn(torch.autograd.Function):
    """out = out_scale * E(X, graph) with gradients for X, projVecs, freqs, bias, the total-mass scale AND the per-edge weights the
    graph was built from (float32, diagonal mode, no edge features, 'plain' mass encoding).

    graph: a coalescing build with want_slots=True (graph.slot_of_edge: the CSR entry of every input edge; the entry's weight is the
    sum of its edges' weights, so every edge receives its entry's gradient).  edge_w [num_input_edges]: the weights the graph was
    built from -- only the gradient is routed to it, the forward kernels read graph.w.  A float64 edge_w (FSW_conv: the self-loop
    and 'gcn' arithmetic in float64) gives the backward the entries' weights beyond float32: w_lo = sum of the entry's edge_w - graph.w
    (fsw_embed_backward_w_lo_f32), because d out / d w at frequency xi feels a weight's rounding times 2 pi xi.
    Forward: the tuned path of _EmbedGraphFn (prepare + embed_into).  Backward: fsw_embed_backward_w_f32 (rows of up to 24
    neighbours on the register kernels of csrc/embed_w_bwd.hip, rows of 25 .. fsw_embed_backward_w_tuned_max_degree() = 1024 on the
    wave-sort kernels of csrc/embed_w_sort_bwd.hip, one (row, slice) line per wavefront; longer rows on the scratch-line kernels of
    csrc/embed_w_long_bwd.hip, one wavefront per (row, fsw_embed_backward_w_long_slices() = 4 slices) on a line in the scratch buffer;
    every class reads w + w_lo) stores the key gradients per entry and accumulates gfreq and gw; gXp is their sum sender by sender
    (graph.sender_major + fsw_segment_sum_rows_f32).  The total-mass
    column depends on the weights through m: out_scale scale g[:, 0] f'(m) per recipient is added, as in _GenericEmbedFn.backward.
    Pad rule: as _GenericEmbedFn.key_grads -- without a deficient row (empty recipients included) the launch gets tau / 2."""

    @staticmethod
    def forward(ctx, X, projVecs, freqs, bias, mass_scale, edge_w, module, graph, out_scale):
        assert graph.w is not None and graph.ef is None and graph.slot_of_edge is not None, \
            'the gradient of the edge weights needs a coalesced graph built with want_slots=True and without edge features'
        with torch.no_grad():
            prepared = module.prepare(X, graph)
            out = torch.empty((graph.num_rows, module.total_mass_encoding_dim + module.nSlices), dtype=X.dtype, device=X.device)
            module.embed_into(X, graph, out, out_scale=out_scale, prepared=prepared)
        ctx.module, ctx.graph, ctx.prepared, ctx.out_scale = module, graph, prepared, float(out_scale)
        ctx.num_edges, ctx.w_dtype = edge_w.shape[0], edge_w.dtype
        ctx.save_for_backward(X, projVecs, freqs, edge_w if edge_w.dtype == torch.float64 else X.new_zeros(0))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        module, graph, prepared, out_scale = ctx.module, ctx.graph, ctx.prepared, ctx.out_scale
        X, V, freqs, w64 = ctx.saved_tensors
        V, fr = V.detach(), freqs.detach().contiguous()
        L = _lib.lib()
        dev = X.device
        S, has_mass = module.nSlices, module.total_mass_encoding_dim
        need = ctx.needs_input_grad
        g = g.contiguous()
        stream = torch.cuda.current_stream(dev).cuda_stream
        ldp, Xp, st = prepared["ldp"], prepared["Xp"], prepared["stats"]
        nnz, max_deg = st[_lib.STAT_NNZ], st[_lib.STAT_MAX_DEGREE]
        tau = float(module.total_mass_pad_thresh)
        deg = (graph.rowptr[1:] - graph.rowptr[:-1]).long()
        rows = torch.repeat_interleave(torch.arange(graph.num_rows, device=dev), deg)
        slot = graph.slot_of_edge[:ctx.num_edges].long()
        wd, w_lo = graph.w[:nnz].double(), None
        if ctx.w_dtype == torch.float64 and nnz:      # the entries' weights in float64 = graph.w + w_lo
            kept = slot >= 0
            wd = torch.zeros(nnz, dtype=torch.float64, device=dev).index_add_(0, slot[kept], w64.detach()[kept])
            w_lo = (wd - graph.w[:nnz].double()).to(torch.float32)
        m = torch.zeros(graph.num_rows, dtype=torch.float64, device=dev).index_add_(0, rows, wd)
        gX = gV = gfreqs = gbias = gscale = gWe = None
        gw = torch.zeros(max(nnz, 1), dtype=torch.float32, device=dev)
        if nnz and S:
            a = module.make_args(graph, st, Xp, ldp, fr, S, None, None, 0, None, out_scale, has_mass)
            if not bool((m < tau).any()):
                a.tau = 0.5 * tau                      # no row is padded: _GenericEmbedFn.key_grads explains
            # scratch: the lines of the rows that need one, above fsw_embed_backward_w_tuned_max_degree() (the query is an upper bound)
            nbytes = int(L.fsw_embed_backward_w_scratch_bytes(max_deg, graph.num_rows)) if max_deg > L.fsw_embed_backward_w_tuned_max_degree() else 0
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
            gkey = torch.empty((nnz, S), dtype=torch.float32, device=dev)
            gf = torch.zeros(S, dtype=torch.float32, device=dev)
            _lib.check(L.fsw_embed_backward_w_lo_f32(ctypes.byref(a), _lib.ptr(w_lo), max_deg, _lib.ptr(g), g.stride(0), _lib.ptr(gkey), S,
                                                     _lib.ptr(gf), _lib.ptr(gw), _lib.ptr(scratch), nbytes, stream),
                       "fsw_embed_backward_w_lo_f32")
            if need[0] or need[1]:
                gXp = torch.zeros((X.shape[0], ldp), dtype=torch.float32, device=dev)
                cptr, order = graph.sender_major()
                _lib.check(L.fsw_segment_sum_rows_f32(_lib.ptr(gkey), S, _lib.ptr(cptr), _lib.ptr(order), graph.num_cols, nnz, S,
                                                      _lib.ptr(gXp), ldp, stream), "fsw_segment_sum_rows_f32")
                if need[0]:
                    gX = _grad_x(L, gXp, S, ldp, V[:, :module.d_in], stream)
                if need[1]:
                    gV = gemm_tn(gXp[:, :S], X.detach())
            del gkey
            gfreqs = gf
        if need[0] and gX is None:
            gX = torch.zeros_like(X)
        if need[1] and gV is None:
            gV = torch.zeros_like(V)
        if need[2] and gfreqs is None:
            gfreqs = torch.zeros_like(freqs)
        if need[3]:
            gbias = out_scale * g.sum(dim=0)
        fn = module.total_mass_encoding_function
        m32 = m.to(torch.float32)
        if need[4]:
            gscale = (out_scale * (g[:, 0] * _mass_f(fn, m32)).sum()).reshape(())
        if need[5]:
            if has_mass and nnz:      # the total-mass column depends on the weights through m
                gw[:nnz] += (out_scale * module._mass_scale_read(st) * g[:, 0] * _mass_df(fn, m32))[rows]
            gWe = torch.where(slot >= 0, gw[slot.clamp(min=0)], torch.zeros((), dtype=torch.float32, device=dev)).to(ctx.w_dtype)
        return gX, gV, gfreqs if need[2] else None, gbias, gscale, gWe, None, None, None


def _flat_batch_index(idx, batch_dims):
    """Row-major position in the flattened batch of every entry of a COO index matrix idx [len(batch_dims) + ..., nnz]."""
    strides = torch.tensor(list(np.cumprod((batch_dims + (1,))[::-1])[::-1][1:]), device=idx.device, dtype=torch.int64)
    return (idx[:len(batch_dims)] * strides[:, None]).sum(0)


def _check_finite_nonnegative(Xf, wvals):
    """Input validation of the generic paths (reference fsw_embedding.py:652-703); the tuned kernels check inside (_checked_stats)."""
    if fsw_embedding_basic_safety_checks:
        assert bool(torch.isfinite(Xf).all()), "The entries of X cannot contain NaNs or infs"
        if wvals is not None:
            assert bool(torch.isfinite(wvals).all()), "All entries of W must be finite"
            assert bool((wvals >= 0).all()), "All entries of W must be nonnegative"


def _csr_rec_snd(csr, num_rows):
    """(rec, snd) int64 of the entries of a CSR adjacency (crow_indices, col_indices), for the generic kernels."""
    crow, col = csr[0].long(), csr[1].long()
    rec = torch.repeat_interleave(torch.arange(num_rows, device=crow.device, dtype=torch.int64), crow[1:] - crow[:-1])
    assert rec.numel() == col.numel(), CSR_MALFORMED_MESSAGE
    return rec.contiguous(), col.contiguous()


def _import_csr_graph(csr, wvals, efvals, num_rows, num_cols):
    """The graph of a torch.sparse_csr W (float32): graph.import_csr; with edge features the columns must be strictly increasing in
    every row (the coalesced adjacency), and the feature rows are the entries' own (no self loops here: the positions are kept)."""
    graph = import_csr(csr[0], csr[1], wvals.detach().contiguous(), num_rows, num_cols, strict_cols=efvals is not None)
    if efvals is not None:
        graph.ef = efvals.detach().contiguous() if efvals.shape[0] else torch.zeros((1, efvals.shape[1]), dtype=efvals.dtype, device=efvals.device)
    return graph


CSR_MALFORMED_MESSAGE = "CSR adjacency is malformed (crow_indices must start at 0, be non-decreasing and end at nnz)"
CSR_COL_ORDER_MESSAGE = "with edge features the CSR adjacency must have strictly increasing column indices in every row"


class SimpleCSR:
    """Plain CSR adjacency for the generic kernels (csrc/embed_generic.hip): rowptr int32 [num_rows + 1], col int32 [nnz] with
    the entries in the order of the coalesced COO tensor they came from (row-major), max_degree on the host."""

    def __init__(self, rec, snd, num_rows, num_cols):
        dev = rec.device
        counts = torch.bincount(rec, minlength=num_rows) if rec.numel() else torch.zeros(num_rows, dtype=torch.int64, device=dev)
        self.rowptr = torch.zeros(num_rows + 1, dtype=torch.int32, device=dev)
        self.rowptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
        self.col = snd.to(torch.int32).contiguous()
        self.rec = rec
        self.num_rows, self.num_cols, self.nnz = num_rows, num_cols, int(rec.numel())
        self.max_degree = int(counts.max()) if num_rows > 0 and rec.numel() else 0
        if fsw_embedding_basic_safety_checks and rec.numel():
            assert bool((rec[1:] >= rec[:-1]).all()), 'adjacency entries must be sorted by recipient (coalesced COO order)'
            assert int(snd.min()) >= 0 and int(snd.max()) < num_cols and int(rec.min()) >= 0 and int(rec.max()) < num_rows, \
                "adjacency index out of range"


def _value_args(a, module, Xp, ldp, freqs, S, out_scale, has_mass, mass_scale):
    """The fields struct fsw_generic_args and struct fsw_cart_args have in common by name, for every entry point that takes one."""
    a.value_dtype = 1 if Xp.dtype == torch.float64 else 0
    a.S, a.has_mass = S, has_mass
    a.Xp, a.ldp, a.freqs = Xp.data_ptr(), ldp, freqs.data_ptr()
    a.tau, a.out_scale = float(module.total_mass_pad_thresh), float(out_scale)
    a.mass_fn, a.mass_scale = _MASS_FN[module.total_mass_encoding_function], float(mass_scale)
    return a


def _cart_args(module, Xp, ldp, freqs, S, out_scale, has_mass, mass_scale):
    """struct fsw_cart_args with the fields both Cartesian entry points share."""
    a = _value_args(_lib.CartArgs(), module, Xp, ldp, freqs, S, out_scale, has_mass, mass_scale)
    a.F = module.nFreqs
    return a


def _project(X, V, d_in, S, ldp):
    """Xp [n, ldp] = X . V[:, :d_in]^T in the dtype of X, without the by-products of the tuned forward (stats, copy of X)."""
    L = _lib.lib()
    stream = torch.cuda.current_stream(X.device).cuda_stream
    Xp = torch.empty((X.shape[0], ldp), dtype=X.dtype, device=X.device)
    if X.dtype == torch.float64:
        _lib.check(L.fsw_project_f64(_lib.ptr(X), X.shape[0], d_in, X.stride(0), _lib.ptr(V), S, V.stride(0), _lib.ptr(Xp), ldp,
                                     None, stream), "fsw_project_f64")
    else:
        _lib.check(L.fsw_project_f32(_lib.ptr(X), X.shape[0], d_in, X.stride(0), _lib.ptr(V), S, V.stride(0), _lib.ptr(Xp), ldp,
                                     None, 0, None, stream), "fsw_project_f32")
    return Xp


class _GenericEmbedFn(torch.autograd.Function):
    """out = out_scale * E(X, W) through the generic kernels (any degree, float32 or float64 storage, float64 arithmetic) with
    gradients for X, projVecs, freqs, bias, the total-mass scale, the WEIGHTS and the edge features.  module.cartesian_mode picks
    the entry point (`variant`); everything else is the same code for both:

      fsw_embed_generic (csrc/embed_generic.hip): out [num_rows, has_mass + S], slice s read out at frequency s.
      fsw_embed_cart_generic (the same kernel; arguments checked in csrc/embed_cart.hip): out [num_rows, has_mass + S F], column has_mass + s F + f = (slice s,
        frequency f); bias flattened, gkey one column per slice, gf one entry per frequency; edge features: the kernel has no edge term, so it
        runs on the keys of the entries, Xp[col] + Ke, with the identity as its col (forward()).

    Callers: every float64 module (the float64 build of the path, reference test_conv.py:24), float32 modules whose weights or
    sparse edge features require a gradient (the tuned float32 backward kernels treat W as a constant), and Cartesian mode under
    autograd.  Replaces the reference's sparse autograd chain incl. ag.div_sparse_dense.backward (fsw_embedding.py:1656),
    ag.cumsum_sparse.backward (:2160, the reverse segmented cumsum) and ag.permute_sparse.backward (:1286)."""

    @staticmethod
    def variant(module):
        """(args struct, entry point, rounding of the projection stride ldp)"""
        if module.cartesian_mode:
            return _lib.CartArgs, "fsw_embed_cart_generic", 32
        return _lib.GenericArgs, "fsw_embed_generic", 64

    @staticmethod
    def launch(module, csr, aux, freqs, out_scale, mass_scale, what="", **fields):
        """One call of the entry point: `fields` are out / ldo / bias (forward) or g / ldg / gkey / ldk / gfreq / gw (backward)."""
        L = _lib.lib()
        args_t, entry, _ = _GenericEmbedFn.variant(module)
        Xp, ldp, Ke, wv = aux
        scratch = torch.empty(int(getattr(L, entry + "_scratch_bytes")(csr.max_degree, max(csr.num_rows, 1))), dtype=torch.uint8,
                              device=Xp.device)
        a = _value_args(args_t(), module, Xp, ldp, freqs, module.nSlices, out_scale, module.total_mass_encoding_dim, mass_scale)
        if module.cartesian_mode:
            a.F = module.nFreqs
        else:
            a.Ke, a.ldke = (Ke.data_ptr(), Ke.stride(0)) if Ke is not None else (None, 0)
        a.rowptr, a.col = csr.rowptr.data_ptr(), csr.col.data_ptr() if csr.nnz else None
        a.w = wv.data_ptr() if wv is not None else None
        a.num_rows, a.max_degree = csr.num_rows, csr.max_degree
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        for name, value in fields.items():
            setattr(a, name, value)
        _lib.check(getattr(L, entry)(ctypes.byref(a), torch.cuda.current_stream(Xp.device).cuda_stream), entry + what)

    @staticmethod
    def forward(ctx, X, V, freqs, bias, mass_scale, wvals, efvals, module, csr, out_scale):
        S, d_in = module.nSlices, module.d_in
        with torch.no_grad():
            Xc, Vd, fr = X.detach().contiguous(), V.detach(), freqs.detach().contiguous()
            ldp = _round_up(S, _GenericEmbedFn.variant(module)[2])
            Xp = _project(Xc, Vd, d_in, S, ldp)
            Ke = None
            if efvals is not None:
                Ke = (efvals.detach() @ Vd[:, d_in:].t()).contiguous()        # [nnz, S], the reference's E x S edge term (:934-968)
            wv = wvals.detach().contiguous() if wvals is not None else None
            out = torch.empty((csr.num_rows, module.d_out), dtype=X.dtype, device=X.device)
            ms = float(mass_scale.detach()) if mass_scale is not None else 1.0
            b = bias.detach().contiguous() if bias is not None else None
            ctx.key_col = {}
            if module.cartesian_mode and Ke is not None:
                # fsw_embed_cart_generic has no edge term: it gets the key of every entry, K = Xp[col] + Ke [nnz, S], as its Xp and
                # the identity as its col (a launch field); gkey is then dL/dK and backward() below applies unchanged
                Xp, ldp, Ke = (Xp[csr.col.long(), :S] + Ke).contiguous(), S, None
                ctx.key_ident = torch.arange(max(csr.nnz, 1), dtype=torch.int32, device=X.device)
                ctx.key_col = {"col": ctx.key_ident.data_ptr()}
            ctx.aux = (Xp, ldp, Ke, wv)
            _GenericEmbedFn.launch(module, csr, ctx.aux, fr, out_scale, ms, out=out.data_ptr(), ldo=out.stride(0),
                                   bias=b.data_ptr() if b is not None else None, **ctx.key_col)
        ctx.module, ctx.csr, ctx.out_scale, ctx.mass_scale_value = module, csr, float(out_scale), ms
        ctx.has_ef, ctx.has_w = efvals is not None, wvals is not None
        ctx.save_for_backward(X, V, freqs, efvals if efvals is not None else X.new_zeros(0))
        return out

    @staticmethod
    def key_grads(ctx, g, gkey, gf, gw):
        """The entry point in backward mode: stores gkey [nnz, S], accumulates gf [nFreqs] and gw [nnz] (each nullable)."""
        freqs = ctx.saved_tensors[2]
        fields = dict(ctx.key_col)      # Cartesian mode with edge features: the identity col that goes with the key array (forward)
        if gw is not None:
            # The reference pads no row unless the mass of SOME row is below the threshold (`if (W_pad > 0).any()`, fsw_embedding.py:790):
            # without a deficient row there is no pad element and no clamp on the path of the weights, so a row with m == tau exactly
            # gets d out / d a_j = [R(rank_j) - sum_t H_t c_t] / m, without the kernel's [m <= tau] R(rank_pad) term.  Every m >= tau then,
            # and with tau / 2 in place of tau the kernel computes the same coefficients and takes that branch.
            csr, wv, tau = ctx.csr, ctx.aux[3], float(ctx.module.total_mass_pad_thresh)
            m = torch.zeros(csr.num_rows, dtype=torch.float64, device=wv.device).index_add_(0, csr.rec, wv.double())
            if not bool((m < tau).any()):
                fields["tau"] = 0.5 * tau
        _GenericEmbedFn.launch(ctx.module, ctx.csr, ctx.aux, freqs.detach().contiguous(), ctx.out_scale, ctx.mass_scale_value,
                               " (backward)", **fields, g=g.data_ptr(), ldg=g.stride(0),
                               gkey=gkey.data_ptr() if gkey is not None else None, ldk=gkey.shape[1] if gkey is not None else 0,
                               gfreq=gf.data_ptr() if gf is not None else None, gw=gw.data_ptr() if gw is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        """The kernel call key_grads, then the GEMMs of gX and gprojVecs, the bias, total-mass scale and weight gradients."""
        g = g.contiguous()
        module, csr, out_scale = ctx.module, ctx.csr, ctx.out_scale
        X, V, freqs, efvals = ctx.saved_tensors
        wv = ctx.aux[3]
        dev, dt = X.device, X.dtype
        S, d_in = module.nSlices, module.d_in
        need = ctx.needs_input_grad
        gX = gV = gfreqs = gbias = gscale = gW = gEf = None
        nnz = csr.nnz
        want_key = need[0] or need[1] or (ctx.has_ef and need[6])
        want_w = ctx.has_w and need[5]
        if nnz and S and (want_key or need[2] or want_w):
            gkey = torch.zeros((nnz, S), dtype=dt, device=dev) if want_key else None
            gf = torch.zeros(freqs.numel(), dtype=dt, device=dev) if need[2] else None
            gw = torch.zeros(nnz, dtype=dt, device=dev) if want_w else None
            _GenericEmbedFn.key_grads(ctx, g, gkey, gf, gw)
            Vd = V.detach()
            if need[0] or need[1]:
                gXp = torch.zeros((X.shape[0], S), dtype=dt, device=dev).index_add_(0, csr.col.long(), gkey)
                if need[0]:
                    gX = gXp @ Vd[:, :d_in]
                if need[1]:
                    gV = gXp.t() @ X.detach()
                    if ctx.has_ef:
                        gV = torch.cat([gV, gkey.t() @ efvals.detach()], dim=1)
            if ctx.has_ef and need[6]:
                gEf = gkey @ Vd[:, d_in:]
            gfreqs, gW = gf, gw
        if need[0] and gX is None:
            gX = torch.zeros_like(X)
        if need[1] and gV is None:
            gV = torch.zeros_like(V)
        if need[2] and gfreqs is None:
            gfreqs = torch.zeros_like(freqs)
        if ctx.has_ef and need[6] and gEf is None:
            gEf = torch.zeros_like(efvals)
        if need[3]:
            gbias = out_scale * g.sum(dim=0)
        if module.encode_total_mass and (need[4] or want_w):
            m = torch.zeros(csr.num_rows, dtype=dt, device=dev)
            if nnz:
                m.index_add_(0, csr.rec, wv if wv is not None else torch.ones(nnz, dtype=dt, device=dev))
            fn = module.total_mass_encoding_function
            if need[4]:
                gscale = (out_scale * (g[:, 0] * _mass_f(fn, m)).sum()).reshape(())
            if want_w:      # the total-mass column depends on the weights through m
                gW = (gW if gW is not None else torch.zeros(nnz, dtype=dt, device=dev)) + (
                    out_scale * ctx.mass_scale_value * g[:, 0] * _mass_df(fn, m))[csr.rec]
        if want_w and gW is None:
            gW = torch.zeros(nnz, dtype=dt, device=dev)
        return gX, gV, gfreqs, gbias, gscale, gW, gEf, None, None, None


class _CartEmbedFn(torch.autograd.Function):
    """Cartesian mode, float32: out = out_scale * E(X, graph) [num_rows, has_mass + S F] on the tuned kernels, with gradients for X,
    projVecs, freqs, bias and the total-mass scale (the weights are constants: a W that requires grad takes _GenericEmbedFn).

    Forward: one projection of all S slices (prepare_cartesian) + fsw_embed_cart_f32; the projection, the stats and the unit table
    stay on ctx.  Backward: fsw_embed_cart_backward_keys_f32 (csrc/embed_cart_bwd.hip, tuned kernels for rows of every length; its
    scratch, _cart_backward_scratch_bytes or what the split form of the longest rows needs (_cart_split_backward for unit weights,
    _cart_split_w_backward for general weights), is the
    forward's buffer where that is large enough, else a buffer of its own: _cart_scratch) stores the key gradient of every entry,
    [nnz, S], and accumulates the frequency gradients; the store-and-sum pair (graph.sender_major + fsw_segment_sum_rows_f32) sums
    the entries sender by sender without float atomics, then the two GEMMs of _EmbedGraphFn.  bias: None for 'homog' /
    'homog_alt' (the caller applies _homog_epilogue on the 'plain' output)."""

    @staticmethod
    def forward(ctx, X, projVecs, freqs, bias, mass_scale, module, graph, out_scale):
        with torch.no_grad():
            prepared = module.prepare_cartesian(X, graph)
            out = torch.empty((graph.num_rows, module.d_out), dtype=X.dtype, device=X.device)
            module.embed_cartesian_into(X, graph, out, bias.detach().reshape(-1) if bias is not None else None, out_scale=out_scale,
                                        prepared=prepared)
        ctx.module, ctx.graph, ctx.prepared, ctx.out_scale = module, graph, prepared, float(out_scale)
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.save_for_backward(X, projVecs, freqs)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        module, graph, prepared, out_scale = ctx.module, ctx.graph, ctx.prepared, ctx.out_scale
        X, V, freqs = ctx.saved_tensors
        L = _lib.lib()
        S, F, has_mass = module.nSlices, module.nFreqs, module.total_mass_encoding_dim
        g = g.contiguous()
        dev = X.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        st, ldp = prepared["stats"], prepared["ldp"]
        nnz = st[_lib.STAT_NNZ]
        need = ctx.needs_input_grad
        gX = gV = gfreqs = gbias = gscale = None
        if nnz > 0 and (need[0] or need[1] or need[2]):
            fr = freqs.detach().contiguous()
            table = prepared["table"]
            dtable = None
            if table is not None:
                dtable = torch.empty_like(table)
                _lib.check(L.fsw_unit_dcoeff_table(_lib.ptr(fr), F, _lib.REG_MAX_DEG, _lib.ptr(dtable), F, stream), "fsw_unit_dcoeff_table")
            gf = torch.zeros(F, dtype=torch.float32, device=dev)
            gkey = torch.empty((nnz, S), dtype=torch.float32, device=dev)      # every entry is stored
            split_bytes, split_w_bytes = module._cart_split_backward(graph, st), module._cart_split_w_backward(graph, st)    # one of them is 0
            scratch = module._cart_scratch(graph, st, backward=True, reuse=prepared["scratch"], split_bytes=split_bytes or split_w_bytes)
            a = module._cart_tuned_args(graph, st, prepared["Xp"], ldp, fr, S, table, scratch, out_scale, has_mass,
                                        split_backward=split_bytes > 0, split_w_backward=split_w_bytes > 0)
            a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g.data_ptr(), g.stride(0), gkey.data_ptr(), S, gf.data_ptr()
            _lib.check(L.fsw_embed_cart_backward_keys_f32(ctypes.byref(a), _lib.ptr(dtable), F, stream), "fsw_embed_cart_backward_keys_f32")
            if need[0] or need[1]:
                gXp = torch.zeros((X.shape[0], ldp), dtype=torch.float32, device=dev)
                cptr, order = graph.sender_major()
                _lib.check(L.fsw_segment_sum_rows_f32(_lib.ptr(gkey), S, _lib.ptr(cptr), _lib.ptr(order), graph.num_cols, nnz, S,
                                                      _lib.ptr(gXp), ldp, stream), "fsw_segment_sum_rows_f32")
                del gkey
                if need[0]:
                    gX = _grad_x(L, gXp, S, ldp, V.detach(), stream)
                if need[1]:
                    gV = gemm_tn(gXp[:, :S], X.detach())
            if need[2]:
                gfreqs = gf
        if need[0] and gX is None:
            gX = torch.zeros_like(X)
        if need[1] and gV is None:
            gV = torch.zeros_like(V)
        if need[2] and gfreqs is None:
            gfreqs = torch.zeros_like(freqs)
        if need[3]:
            gbias = (out_scale * g.sum(dim=0)).reshape(ctx.bias_shape)
        if need[4]:
            deg = (graph.rowptr[1:] - graph.rowptr[:-1]).long()
            if graph.w is None:
                m = deg.to(torch.float32)                                  # unit weights: total mass = in-degree
            else:
                rows = torch.repeat_interleave(torch.arange(graph.num_rows, device=dev), deg)
                m = torch.zeros(graph.num_rows, dtype=torch.float32, device=dev).index_add_(0, rows, graph.w[:rows.numel()])
            gscale = (out_scale * (g[:, 0] * _mass_f(module.total_mass_encoding_function, m)).sum()).reshape(())
        return gX, gV, gfreqs, gbias, gscale, None, None, None


class _CartEdgeEmbedFn(torch.autograd.Function):
    """_CartEmbedFn for a graph with edge features (d_edge > 0, the coalescing build): the same tuned kernels in both directions, run on
    the key of every CSR entry, K[e, s] = Xp[col[e], s] + <ef[e], projVecs[s, d_in:]> (prepare_cartesian: fsw_edge_keys_f32), with the
    identity as their column array.  The gkey [nnz, S] the backward kernels store is then dL/dK, and from it
      gXp = the rows of gkey summed by the graph's own col (the store-and-sum pair on graph.sender_major(), no float atomics),
      gX = gXp . V[:, :d_in],   gprojVecs = [gXp^T . X | gkey^T . ef],
      g edge_feat[i] = gkey[slot_of_edge[i]] . V[:, d_in:] (merged parallel edges each receive their slot's gradient, dropped edges 0),
    as _EmbedGraphFn does in diagonal mode.  gfreqs, gbias and the total-mass scale as in _CartEmbedFn.  edge_feat: the per-input-edge
    tensor the graph was coalesced from (needs graph.slot_of_edge when it requires grad), or None."""

    @staticmethod
    def forward(ctx, X, projVecs, freqs, bias, mass_scale, edge_feat, module, graph, out_scale):
        with torch.no_grad():
            prepared = module.prepare_cartesian(X, graph)
            out = torch.empty((graph.num_rows, module.d_out), dtype=X.dtype, device=X.device)
            module.embed_cartesian_into(X, graph, out, bias.detach().reshape(-1) if bias is not None else None, out_scale=out_scale,
                                        prepared=prepared)
        ctx.module, ctx.graph, ctx.prepared, ctx.out_scale = module, graph, prepared, float(out_scale)
        ctx.bias_shape = bias.shape if bias is not None else None
        ctx.num_edge_rows = 0 if edge_feat is None else edge_feat.shape[0]
        ctx.save_for_backward(X, projVecs, freqs)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        module, graph, prepared, out_scale = ctx.module, ctx.graph, ctx.prepared, ctx.out_scale
        X, V, freqs = ctx.saved_tensors
        L = _lib.lib()
        S, F, has_mass, d_in = module.nSlices, module.nFreqs, module.total_mass_encoding_dim, module.d_in
        g = g.contiguous()
        dev = X.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        st = prepared["stats"]
        nnz = st[_lib.STAT_NNZ]
        need = ctx.needs_input_grad
        gX = gV = gfreqs = gbias = gscale = gEf = None
        if nnz > 0 and (need[0] or need[1] or need[2] or need[5]):
            fr = freqs.detach().contiguous()
            Vd = V.detach()
            gf = torch.zeros(F, dtype=torch.float32, device=dev)
            gkey = torch.empty((nnz, S), dtype=torch.float32, device=dev)      # every entry is stored
            split_w_bytes = module._cart_split_w_backward(graph, st)          # a coalesced graph carries weights: general-weight kernels
            scratch = module._cart_scratch(graph, st, backward=True, reuse=prepared["scratch"], split_bytes=split_w_bytes)
            a = module._cart_tuned_args(graph, st, prepared["Xp"], prepared["ldp"], fr, S, None, scratch, out_scale, has_mass,
                                        split_w_backward=split_w_bytes > 0, col=prepared["col"])
            a.g, a.ldg, a.gkey, a.ldk, a.gfreq = g.data_ptr(), g.stride(0), gkey.data_ptr(), S, gf.data_ptr()
            _lib.check(L.fsw_embed_cart_backward_keys_f32(ctypes.byref(a), None, F, stream), "fsw_embed_cart_backward_keys_f32")
            if need[0] or need[1]:
                ldg = _round_up(S, 32)
                gXp = torch.zeros((X.shape[0], ldg), dtype=torch.float32, device=dev)
                cptr, order = graph.sender_major()
                _lib.check(L.fsw_segment_sum_rows_f32(_lib.ptr(gkey), S, _lib.ptr(cptr), _lib.ptr(order), graph.num_cols, nnz, S,
                                                      _lib.ptr(gXp), ldg, stream), "fsw_segment_sum_rows_f32")
                if need[0]:
                    gX = _grad_x(L, gXp, S, ldg, Vd[:, :d_in], stream)
                if need[1]:
                    gV = torch.cat([gemm_tn(gXp[:, :S], X.detach()), gkey.t() @ graph.ef[:nnz]], dim=1)
            if need[5]:
                assert graph.slot_of_edge is not None, 'the gradient of the edge features needs a graph built with want_slots=True'
                slot = graph.slot_of_edge[:ctx.num_edge_rows].long()
                gslots = gkey @ Vd[:, d_in:]
                gEf = torch.where((slot >= 0)[:, None], gslots[slot.clamp(min=0)], torch.zeros((), device=dev))
            if need[2]:
                gfreqs = gf
        if need[0] and gX is None:
            gX = torch.zeros_like(X)
        if need[1] and gV is None:
            gV = torch.zeros_like(V)
        if need[2] and gfreqs is None:
            gfreqs = torch.zeros_like(freqs)
        if need[5] and gEf is None:
            gEf = torch.zeros((ctx.num_edge_rows, module.d_edge), dtype=X.dtype, device=dev)
        if need[3]:
            gbias = (out_scale * g.sum(dim=0)).reshape(ctx.bias_shape)
        if need[4]:
            deg = (graph.rowptr[1:] - graph.rowptr[:-1]).long()
            rows = torch.repeat_interleave(torch.arange(graph.num_rows, device=dev), deg)
            m = torch.zeros(graph.num_rows, dtype=torch.float32, device=dev).index_add_(0, rows, graph.w[:rows.numel()])
            gscale = (out_scale * (g[:, 0] * _mass_f(module.total_mass_encoding_function, m)).sum()).reshape(())
        return gX, gV, gfreqs, gbias, gscale, gEf, None, None, None


class FSW_embedding(nn.Module):
    def __init__(self,
                 d_in, d_out=None, nSlices=None, nFreqs=None, collapse_freqs=False,
                 d_edge=0,
                 encode_total_mass=False,
                 total_mass_encoding_function='identity',
                 total_mass_encoding_scale=1.0,
                 total_mass_encoding_method='plain',
                 total_mass_pad_thresh=1.0,
                 learnable_slices=False, learnable_freqs=False, learnable_total_mass_encoding_scale=False,
                 freqs_init='random',
                 minimize_slice_coherence=False,
                 enable_bias=True,
                 device=None, dtype=torch.float32,
                 load_custom_cuda_lib=True,
                 report=False, user_warnings=True,
                 report_on_coherence_minimization=False,
                 cartesian_edge_features=False):
        super().__init__()
        self.user_warnings = user_warnings
        # reference fsw_embedding.py:195-206 loads its CUDA library here; this build cannot run without its
        # native library, so load_custom_cuda_lib=False is rejected instead of selecting a slow path.
        if not load_custom_cuda_lib:
            raise RuntimeError("fsw_gnn_amd has no pure-PyTorch path: load_custom_cuda_lib=False is not supported")
        _lib.lib()

        assert d_in >= 0, 'd_in must be nonnegative'
        assert d_edge >= 0, 'd_edge must be nonnegative'
        assert (d_out is None) or (d_out >= 0), 'd_out must be nonnegative or None'
        if d_out == 0:
            encode_total_mass = False
        self.d_in, self.d_edge = d_in, d_edge
        self.encode_total_mass = bool(encode_total_mass)
        self.total_mass_encoding_dim = 1 if self.encode_total_mass else 0
        self.total_mass_encoding_scale_init = total_mass_encoding_scale

        total_mass_pad_thresh = float(total_mass_pad_thresh)
        assert not np.isinf(total_mass_pad_thresh), 'total_mass_pad_thresh cannot be inf'
        assert not np.isnan(total_mass_pad_thresh), 'total_mass_pad_thresh cannot be NaN'
        assert total_mass_pad_thresh > 0, 'total_mass_pad_thresh must be positive'
        self.total_mass_pad_thresh = total_mass_pad_thresh
        assert total_mass_encoding_method in {'plain', 'homog', 'homog_alt'}, \
            "<total_mass_encoding_method> must be one of 'plain', 'homog', 'homog_alg'"
        self.total_mass_encoding_method = total_mass_encoding_method
        assert total_mass_encoding_function in {'identity', 'sqrt', 'log'}, \
            "<total_mass_encoding_function> must be one of 'identity', 'sqrt', 'log'"
        self.total_mass_encoding_function = total_mass_encoding_function

        # size logic: reference fsw_embedding.py:242-261
        if (d_out is not None) and (nSlices is None) and (nFreqs is None):
            self.cartesian_mode = False
            self.collapse_freqs = False
            self.d_out = d_out
            self.nSlices = d_out - self.total_mass_encoding_dim
            self.nFreqs = d_out - self.total_mass_encoding_dim
        elif (d_out is None) and (nSlices is not None) and (nFreqs is not None):
            assert collapse_freqs or (not encode_total_mass), 'Cartesian mode with collapse_freqs=False is not supported when encode_total_mass=True'
            self.cartesian_mode = True
            self.collapse_freqs = bool(collapse_freqs)
            self.nSlices = nSlices
            self.nFreqs = nFreqs
            self.d_out = nSlices * nFreqs + self.total_mass_encoding_dim
        else:
            assert False, "Expected exactly one of (d_out != None) or (nSlices != None and nFreqs != None)"
        assert self.d_out >= 0, 'd_out must be nonnegative'
        self.minimize_slice_coherence = minimize_slice_coherence
        self.learnable_slices = learnable_slices
        self.learnable_freqs = learnable_freqs
        self.learnable_total_mass_encoding_scale = learnable_total_mass_encoding_scale
        self.freqs_init = freqs_init
        self.enable_bias = enable_bias
        if device is None:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.device_new = torch.device(device)
        if self.cartesian_mode:
            # checked before any parameter exists: a module that cannot run is not built at all
            if self.device_new.type != 'cuda':
                raise NotImplementedError("fsw_gnn_amd: Cartesian mode needs a HIP device ('cuda'), got device=%s; this package has "
                                          "no CPU path in any mode" % self.device_new)
            # opt-in: without the keyword the constructor refuses as it always did (callers that rely on the refusal keep it; the
            # reference runs the combination through its dense-W path only and lists it as untested)
            if d_edge > 0 and not cartesian_edge_features:
                raise NotImplementedError("fsw_gnn_amd: Cartesian mode with edge features (d_edge > 0) is opt-in: pass "
                                          "cartesian_edge_features=True (the reference lists the combination as untested)")
        assert dtype.is_floating_point and (not dtype.is_complex), \
            'dtype must be real floating-point; instead got dtype=%s' % (dtype)
        if dtype not in (torch.float32, torch.float64):
            raise NotImplementedError("fsw_gnn_amd: the HIP kernels are built for float32 and float64 (got dtype=%s)" % dtype)
        self.dtype_new = dtype
        self.report = report
        self.report_on_coherence_minimization = report_on_coherence_minimization
        if report:
            print('Fourier Sliced-Wasserstein Embedding, MI355X-native build %s' % version)
            if self.cartesian_mode:
                print('Cartesian mode: %d slices x %d frequencies -> %s; device: %s    dtype: %s' % (
                    self.nSlices, self.nFreqs, ('R^%d' % self.d_out) if self.collapse_freqs else ('R^(%dx%d)' % (self.nSlices, self.nFreqs)),
                    self.device_new, dtype))
            else:
                print('Using %d (slice, frequency) pairs; device: %s    dtype: %s' % (self.nSlices, self.device_new, dtype))
        self.reset_parameters()

    # ------------------------------------------------------------------------------------------------
    def reset_parameters(self, freqs_init=None, minimize_slice_coherence=None, report=None,
                         report_on_coherence_minimization=None):
        """Reference fsw_embedding.py:343-414 / 445-559 (parameter semantics; RNG values differ)."""
        self.freqs_init = self.freqs_init if freqs_init is None else freqs_init
        if minimize_slice_coherence is not None:
            self.minimize_slice_coherence = minimize_slice_coherence
        if report is not None:
            self.report = report
        if hasattr(self, 'device_new'):
            device = self.device_new
            delattr(self, 'device_new')
        else:
            device = self.get_device()
        if hasattr(self, 'dtype_new'):
            dtype = self.dtype_new
            delattr(self, 'dtype_new')
        else:
            dtype = self.get_dtype()
        projVecs, freqs, bias, scale = FSW_embedding.generate_embedding_parameters(
            d_in=self.d_in + self.d_edge, nSlices=self.nSlices, nFreqs=self.nFreqs,
            total_mass_encoding_dim=self.total_mass_encoding_dim,
            total_mass_encoding_scale_init=self.total_mass_encoding_scale_init, freqs_init=self.freqs_init, device=device,
            minimize_slice_coherence=self.minimize_slice_coherence, report=self.report_on_coherence_minimization,
            cartesian_mode=self.cartesian_mode, collapse_freqs=self.collapse_freqs)
        self.projVecs = nn.Parameter(projVecs.to(dtype=dtype, device=device), requires_grad=self.learnable_slices)
        self.freqs = nn.Parameter(freqs.to(dtype=dtype, device=device), requires_grad=self.learnable_freqs)
        if self.enable_bias:
            self.bias = nn.Parameter(bias.to(dtype=dtype, device=device), requires_grad=self.learnable_slices)
        if self.encode_total_mass:
            self.total_mass_encoding_scale = nn.Parameter(scale.to(dtype=dtype), requires_grad=self.learnable_total_mass_encoding_scale)
        return self

    @staticmethod
    def generate_embedding_parameters(d_in, nSlices, nFreqs, total_mass_encoding_dim, total_mass_encoding_scale_init,
                                      freqs_init, device, minimize_slice_coherence=False, report=False, cartesian_mode=False,
                                      collapse_freqs=False):
        dt = torch.float64
        # A. random unit projection vectors (reference :448-456), optionally spread out by mutual-coherence
        #    minimisation (:464, :3045-3248 -> coherence.py)
        projVecs = torch.randn(size=(nSlices, d_in), dtype=dt, device=device)
        projVecs = nn.functional.normalize(projVecs, p=2.0, dim=1, eps=0)
        if minimize_slice_coherence and nSlices > 1 and d_in > 0:
            projVecs = minimize_mutual_coherence(projVecs, report=report)
        if nSlices > 0 and d_in > 0:
            assert not torch.isinf(projVecs).any(), "Found infs in projVecs"
            assert not torch.isnan(projVecs).any(), "Found nans in projVecs"
        # B. frequencies (reference :489-535)
        shape = (nFreqs,)
        if nFreqs == 0:
            freqs = torch.zeros(size=shape, dtype=dt, device=device)
        elif isinstance(freqs_init, numbers.Real):
            assert not np.isinf(freqs_init), 'freqs_init cannot be infinite'
            assert not np.isnan(freqs_init), 'freqs_init cannot be NaN'
            freqs = freqs_init * torch.ones(size=shape, dtype=dt, device=device)
        elif isinstance(freqs_init, tuple):
            assert (len(freqs_init) == 2), 'When freqs_init is a tuple, it must be of length 2'
            a, b = freqs_init
            assert not np.isinf(a) and not np.isinf(b), 'Received infinite value in freqs_init tuple'
            assert not np.isnan(a) and not np.isnan(b), 'Received NaN value in freqs_init tuple'
            assert a <= b, 'When freqs_init is a tuple, it is required to satisfy freqs_init[0] <= freqs_init[1]'
            if nFreqs == 1:
                freqs = a + (b - a) / 2 * torch.ones(size=shape, dtype=dt, device=device)
            else:
                freqs = a + (b - a) * (torch.arange(nFreqs, dtype=dt, device=device) / (nFreqs - 1))
        elif freqs_init == 'random':
            freqs = torch.rand(size=shape, dtype=dt, device=device)
            freqs, _ = torch.sort(freqs, dim=0)
            freqs = freqs / (1 - freqs)
        elif freqs_init == 'spread':
            freqs = (0.5 + torch.arange(nFreqs, dtype=dt, device=device)) / nFreqs
            freqs = freqs / (1 - freqs)
        else:
            raise RuntimeError("Invalid value for argument freqs_init; expected number, tuple (a,b) of numbers "
                               "denoting an interval, 'random' or 'spread'")
        if nFreqs > 0:
            assert not torch.isinf(freqs).any(), "Found infs in freqs"
            assert not torch.isnan(freqs).any(), "Found nans in freqs"
        # C. zero bias (reference :542-550) and the total-mass scale.  Cartesian mode: (nSlices, nFreqs), collapsed
        #    (nSlices * nFreqs + total_mass_encoding_dim,) -- with the total mass the reference's constructor then fails to
        #    reshape this to nSlices * nFreqs (:403-404); here the mass column keeps its bias entry
        if cartesian_mode and not collapse_freqs:
            bias_shape = (nSlices, nFreqs)
        elif cartesian_mode:
            bias_shape = (nSlices * nFreqs + total_mass_encoding_dim,)
        else:
            bias_shape = (nSlices + total_mass_encoding_dim,)
        bias = torch.zeros(size=bias_shape, dtype=dt, device=device)
        scale = torch.tensor(total_mass_encoding_scale_init, device=device, dtype=dt) if total_mass_encoding_dim > 0 else None
        return projVecs, freqs, bias, scale

    def spread_freqs_at_interval(self, center, radius):
        """Reference fsw_embedding.py:567-582."""
        assert radius >= 0
        if (self.nFreqs == 1) or (radius == 0):
            freqs_new = center * torch.ones_like(self.freqs)
        else:
            spread = 2 * (0.5 + torch.arange(self.nFreqs, dtype=self.get_dtype(), device=self.get_device())) / self.nFreqs - 1
            spread = spread * 1 / (1 - 1 / self.nFreqs)
            freqs_new = center + radius * spread
        sd = self.state_dict()
        sd['freqs'] = freqs_new
        self.load_state_dict(sd)
        return self

    def _check_csr_arguments(self, X, W, X_edge, graph_mode):
        """Host-side checks of a call whose W (or X_edge) has a compressed sparse layout; nothing here touches a device."""
        supported = ("Supported sparse layouts: torch.sparse_coo (coalesced), and torch.sparse_csr with graph_mode=True, a 2-D W "
                     "[nRecipients, n] without batch dimensions and X [n, d_in]")
        assert torch.is_tensor(W) and W.layout == torch.sparse_csr, \
            "Sparse W has an unsupported sparsity layout '%s'. %s." % (getattr(W, 'layout', type(W)), supported)
        assert graph_mode, "A torch.sparse_csr W needs graph_mode=True. %s." % supported
        assert W.dim() == 2 and X.dim() == 2 and W.dense_dim() == 0, \
            "A torch.sparse_csr W must be 2-D [nRecipients, n] with X [n, d_in]: batch dimensions are not supported. %s." % supported
        assert W.shape[1] == X.shape[0], "Shape mismatch between X and W: a torch.sparse_csr W [nRecipients, n] needs X [n, d_in]"
        if self.d_edge > 0:
            assert torch.is_tensor(X_edge) and X_edge.layout == torch.sparse_csr, \
                "With a torch.sparse_csr W, X_edge must be torch.sparse_csr too (values [nnz, d_edge], or [nnz] when d_edge == 1)"
            assert tuple(X_edge.shape[:2]) == tuple(W.shape), "X_edge must have the sparse shape of W"
        if W.requires_grad or (torch.is_tensor(X_edge) and X_edge.requires_grad):
            raise NotImplementedError("fsw_gnn_amd: gradients of a torch.sparse_csr W or X_edge are not implemented; pass them in the "
                                      "COO layout (torch.sparse_coo), which the generic kernels differentiate")

    def get_device(self):
        return self.projVecs.device

    def get_dtype(self):
        return self.projVecs.dtype

    # ------------------------------------------------------------------------------------------------
    def forward(self, X, W='unit', X_edge=None, graph_mode=False, serialize_num_slices=None):
        """Same contract as the reference forward (fsw_embedding.py:587-890).

        X (<batch>, n, d_in); W (<batch>, n) | 'unit' | 'uniform'; graph_mode: W (<batch>, nRecipients, n) dense or
        coalesced torch.sparse_coo, X shared by the recipients.  Returns (<batch>, [nRecipients,] d_out).

        Beyond the reference, graph_mode also takes a 2-D torch.sparse_csr W [nRecipients, n] (X [n, d_in], no batch dimensions):
        the adjacency is imported as it is, without the sort of the other layouts (graph.import_csr).  With d_edge > 0, X_edge is
        then torch.sparse_csr with the indices of W and values [nnz, d_edge], and every row's columns must be strictly increasing.
        Gradients of a CSR W / X_edge are not implemented (NotImplementedError: use the COO layout).
        """
        assert self.total_mass_pad_thresh > 0, 'total_mass_pad_thresh must be positive'
        if self.d_edge > 0:
            assert graph_mode, 'd_edge > 0 (given at initialization) necessitates graph_mode=True on forward call'
            assert X_edge is not None, 'X_edge must be provided since d_edge > 0'
            assert torch.is_tensor(W), 'When X_edge is provided, W must be provided explicitly'
            assert X_edge.device == self.get_device() and X_edge.dtype == self.get_dtype(), 'X_edge has the wrong device or dtype'
            assert X_edge.is_sparse == W.is_sparse, 'X_edge and W must either both or neither be sparse'
        else:
            assert (X_edge is None) or (X_edge.numel() == 0), 'X_edge should be None or empty since d_edge == 0'
        assert torch.is_tensor(X), 'X must be a pytorch tensor. Instead got type %s' % (type(X))
        assert torch.is_tensor(W) or W in {'unit', 'uniform'}, "W must be a pytorch tensor, 'unit' or 'uniform'"
        csr_in = torch.is_tensor(W) and W.layout not in (torch.strided, torch.sparse_coo)
        if csr_in or (torch.is_tensor(X_edge) and X_edge.layout not in (torch.strided, torch.sparse_coo)):
            self._check_csr_arguments(X, W, X_edge, graph_mode)     # host-side only: raises before any device is touched
        assert X.dtype == self.get_dtype(), ("X has the wrong dtype. Expected %s, got %s" % (self.get_dtype(), X.dtype))
        assert X.device == self.get_device(), ("X is on the wrong device. Expected %s, got %s" % (self.get_device(), X.device))
        if X.device.type != 'cuda':
            raise RuntimeError("fsw_gnn_amd: forward needs tensors on a HIP device ('cuda'); there is no CPU path")
        needs_grad = torch.is_grad_enabled() and (X.requires_grad or any(p.requires_grad for p in self.parameters()))
        # float64 modules, and float32 calls that ask for gradients of the weights or of sparse edge features, run on the
        # generic kernels (csrc/embed_generic.hip); everything else on the tuned float32 kernels
        generic = self.get_dtype() == torch.float64 or (torch.is_grad_enabled() and (
            (torch.is_tensor(W) and W.requires_grad) or (X_edge is not None and torch.is_tensor(X_edge) and X_edge.requires_grad)))
        if torch.is_tensor(W):
            assert W.dtype == self.get_dtype(), ("W has the wrong dtype. Expected %s, got %s" % (self.get_dtype(), W.dtype))
            assert W.device == self.get_device(), ("W is on the wrong device. Expected %s, got %s" % (self.get_device(), W.device))
            if W.is_sparse:
                assert W.is_coalesced(), 'Sparse W must be coalesced'
                assert W.dense_dim() == 0, 'W.dense_dim() must be zero'
        assert len(X.shape) >= 2, "X must be a tensor of order at least 2"
        assert X.shape[-1] == self.d_in, "The last dimension of X must equal d_in=%d. Instead got %d" % (self.d_in, X.shape[-1])

        d = self.d_in
        efvals = None
        if not graph_mode:
            batch_dims = tuple(X.shape[0:-2])
            n = X.shape[-2]
            B = int(np.prod(batch_dims)) if batch_dims else 1
            if torch.is_tensor(W):
                assert (len(W.shape) == len(X.shape) - 1) and (tuple(W.shape) == tuple(X.shape[0:-1])), \
                    "Shape mismatch between X and W: If X.shape = (b1,b2,...,bk,n,d_in) then W.shape should be (b1,b2,...,bk,n) (unless graph_mode=True)"
                wvals = None if W.is_sparse else W.reshape(-1)
            elif W == 'unit':
                wvals = None
            else:  # 'uniform'
                wvals = torch.full((B * n,), 1.0 / n, dtype=self.get_dtype(), device=X.device)
            if torch.is_tensor(W) and W.is_sparse:
                # coalesced COO weights (reference fsw_embedding.py:664-668 accepts them in both modes): entry (b.., j)
                # is element j of multiset b; absent entries are absent elements (weight 0)
                idx, wvals = W.indices(), W.values()
                if batch_dims:
                    rec = _flat_batch_index(idx, batch_dims)
                else:
                    rec = torch.zeros(idx.shape[1], device=X.device, dtype=torch.int64)
                snd = (rec * n + idx[-1]).contiguous()
                rec = rec.contiguous()
            else:
                rec = torch.arange(B, device=X.device, dtype=torch.int64).repeat_interleave(n)
                snd = torch.arange(B * n, device=X.device, dtype=torch.int64)
            Xf = X.reshape(B * n, d)
            num_rows, out_shape = B, batch_dims
        else:
            assert torch.is_tensor(W), 'W must be explicitly provided when graph_mode=True'
            batch_dims = tuple(W.shape[0:-2])
            nR, n = W.shape[-2], W.shape[-1]
            assert (len(W.shape) == len(X.shape)) and (W.shape[-1] == X.shape[-2]) and (tuple(W.shape[0:-2]) == tuple(X.shape[0:-2])), \
                "Shape mismatch between X and W: When graph_mode=True, if W.shape = (b1,b2,...,bk,nRecipients,n) then X.shape should be (b1,b2,...,bk,n,d_in)"
            B = int(np.prod(batch_dims)) if batch_dims else 1
            efvals = None
            if csr_in:
                # the adjacency by recipient as the caller holds it: imported without a sort (graph.import_csr); rec / snd are only
                # made for the generic kernels (float64 modules), with torch ops
                idx = None
                csr = (W.crow_indices(), W.col_indices())
                wvals = W.values()
                if self.d_edge > 0:
                    assert X_edge.values().shape[0] == wvals.shape[0], 'Sparse X_edge must have the same number of values() as W'
                    if fsw_embedding_basic_safety_checks:
                        assert torch.equal(X_edge.crow_indices(), csr[0]) and torch.equal(X_edge.col_indices(), csr[1]), \
                            'Sparse X_edge must have the same nonzero pattern as W'
                    efvals = X_edge.values().reshape(wvals.shape[0], -1)
            elif W.is_sparse:
                idx, wvals = W.indices(), W.values()
                if self.d_edge > 0:
                    assert X_edge.is_coalesced() and X_edge.values().shape[0] == wvals.shape[0], \
                        'Sparse X_edge must have the same number of values() as W'
                    if fsw_embedding_basic_safety_checks:
                        assert (X_edge.indices() == idx).all(), 'Sparse X_edge must have the same nonzero pattern as W'
                    efvals = X_edge.values().reshape(wvals.shape[0], -1)
            else:
                idx = W.nonzero(as_tuple=False).t().contiguous()
                wvals = W[tuple(idx)]
                if self.d_edge > 0:
                    efvals = X_edge[tuple(idx)].reshape(wvals.shape[0], -1)
            if self.d_edge > 0:
                assert efvals.shape[1] == self.d_edge, 'X_edge must carry d_edge features per edge'
            if csr_in:
                rec = snd = None
            else:
                b = _flat_batch_index(idx, batch_dims) if batch_dims else 0
                rec = (b * nR + idx[-2]).contiguous()
                snd = (b * n + idx[-1]).contiguous()
            Xf = X.reshape(B * n, d)
            num_rows, out_shape = B * nR, batch_dims + (nR,)
        if not (graph_mode and csr_in):
            csr = None

        if self.cartesian_mode:
            # float32 calls run on the tuned kernels, under autograd with their own backward; the generic kernel keeps float64
            # modules and gradients of the weights or of X_edge (a W or X_edge that requires grad selects it, whatever else does: the
            # rule of the diagonal mode above)
            generic = self.get_dtype() == torch.float64 or (torch.is_grad_enabled() and (
                (torch.is_tensor(W) and W.requires_grad) or (self.d_edge > 0 and X_edge.requires_grad)))
            out = self._forward_cartesian(Xf, rec, snd, wvals, num_rows, generic, needs_grad, serialize_num_slices, efvals, csr)
            return out.reshape(out_shape + ((self.d_out,) if self.collapse_freqs else (self.nSlices, self.nFreqs)))
        if generic and num_rows > 0 and Xf.shape[0] > 0:
            if self.d_out == 0:
                return torch.zeros(out_shape + (0,), dtype=X.dtype, device=X.device)
            if self.nSlices == 0:
                raise NotImplementedError("fsw_gnn_amd: nSlices == 0 with encode_total_mass is not supported")
            bias = self.bias if self.enable_bias else None
            if csr is not None:
                rec, snd = _csr_rec_snd(csr, num_rows)
            return self._forward_generic(Xf.contiguous(), rec, snd, wvals, efvals, num_rows, bias).reshape(out_shape + (self.d_out,))
        if num_rows == 0 or Xf.shape[0] == 0:
            # nothing to embed / empty multisets only: the reference returns an empty tensor, resp. the embedding of the
            # pad element alone; the kernels need at least one row and one point
            if num_rows == 0:
                return torch.zeros(out_shape + (self.d_out,), dtype=X.dtype, device=X.device)
            Xf = torch.zeros((1, d), dtype=X.dtype, device=X.device)
        if csr is not None:
            graph = _import_csr_graph(csr, wvals, efvals, num_rows, Xf.shape[0])
        elif self.d_edge > 0:
            graph = build_csr_coalesced(rec, snd, wvals.contiguous(), efvals.contiguous(), num_rows, Xf.shape[0])
        else:
            graph = build_csr(rec, snd, wvals, num_rows, Xf.shape[0])
        if needs_grad:
            out = self.embed_autograd(Xf.contiguous(), graph)
        else:
            out = torch.empty((num_rows, self.d_out), dtype=X.dtype, device=X.device)
            # a view (a column slice, every other row, a transpose) is copied here, as on the three sibling paths; embed_into and
            # prepare keep their contiguity contract
            self.embed_into(Xf.contiguous(), graph, out, out_scale=1.0, serialize_num_slices=serialize_num_slices)
        return out.reshape(out_shape + (self.d_out,))

    def _forward_generic(self, Xf, rec, snd, wvals, efvals, num_rows, bias):
        """The generic-kernel path (float64 modules; float32 with gradients of W / X_edge, in Cartesian mode too):
        differentiable in everything.  bias (flattened): in the kernel for the 'plain' method, in the torch epilogue otherwise."""
        _check_finite_nonnegative(Xf, wvals)
        csr = SimpleCSR(rec, snd, num_rows, Xf.shape[0])
        scale = self.total_mass_encoding_scale if self.encode_total_mass else None
        plain = self.plain_mass
        P = _GenericEmbedFn.apply(Xf, self.projVecs, self.freqs, bias if plain else None, scale, wvals, efvals, self, csr, 1.0)
        return P if plain else self._homog_epilogue(P, 1.0, bias)

    def _forward_cartesian(self, Xf, rec, snd, wvals, num_rows, generic, train, serialize_num_slices, efvals=None, csr=None):
        """Cartesian mode: [num_rows, has_mass + S F], column has_mass + s F + f = (slice s, frequency f).  generic: the generic
        kernel (float64 modules, gradients of W or X_edge); otherwise the tuned float32 kernels (csrc/embed_cart.hip), under autograd
        (train) with their backward (_CartEmbedFn, csrc/embed_cart_bwd.hip).  efvals [nnz, d_edge]: the edge features of the entries
        (d_edge > 0): the coalescing build, as in diagonal mode, and the kernels on the key of every entry (_edge_keys)."""
        dev, dt = Xf.device, Xf.dtype
        S, F = self.nSlices, self.nFreqs
        if num_rows == 0 or self.d_out == 0:
            return torch.zeros((num_rows, self.d_out), dtype=dt, device=dev)
        if S * F == 0:
            raise NotImplementedError("fsw_gnn_amd: Cartesian mode with nSlices * nFreqs == 0 and encode_total_mass is not supported")
        bias = self.bias.reshape(-1) if self.enable_bias else None
        plain = self.plain_mass
        if Xf.shape[0] == 0:
            # empty multisets only: the embedding of the pad element alone is 0 and so is f(0) for every mass encoding and method,
            # which leaves the bias (any dtype; differentiable in the bias)
            Z = torch.zeros((num_rows, self.d_out), dtype=dt, device=dev)
            return Z + bias if bias is not None else Z
        if generic:
            if csr is not None:
                rec, snd = _csr_rec_snd(csr, num_rows)
            return self._forward_generic(Xf.contiguous(), rec, snd, wvals, efvals, num_rows, bias)
        if csr is not None:     # a torch.sparse_csr W: (crow_indices, col_indices), imported without a sort
            graph = _import_csr_graph(csr, wvals, efvals, num_rows, Xf.shape[0])
        elif self.d_edge > 0:
            graph = build_csr_coalesced(rec, snd, wvals.detach().contiguous(), efvals.detach().contiguous(), num_rows, Xf.shape[0])
        else:
            graph = build_csr(rec, snd, wvals.detach().contiguous() if wvals is not None else None, num_rows, Xf.shape[0])
        if train:
            return self.embed_cartesian_autograd(Xf.contiguous(), graph)
        with torch.no_grad():
            out = torch.empty((num_rows, self.d_out), dtype=dt, device=dev)
            self.embed_cartesian_into(Xf.contiguous(), graph, out, bias.detach() if (bias is not None and plain) else None,
                                      serialize_num_slices)
            return out if plain else self._homog_epilogue(out, 1.0, bias.detach() if bias is not None else None)

    def embed_cartesian_autograd(self, X, graph, out_scale=1.0, edge_feat=None):
        """Differentiable float32 Cartesian embedding of a CSR graph, [num_rows, d_out] collapsed (training path of forward() and of
        FSW_conv / FSW_readout with embed_slices / embed_freqs): see _CartEmbedFn.  'homog' / 'homog_alt': the 'plain' embedding
        without bias from the kernels, then the epilogue out of place so that autograd differentiates it (as embed_autograd does).
        A graph with edge features (d_edge > 0, the coalescing build) goes through _CartEdgeEmbedFn; edge_feat: the per-input-edge
        feature tensor the graph was coalesced from (its gradient is routed back through graph.slot_of_edge), or None."""
        scale = self.total_mass_encoding_scale if self.encode_total_mass else None
        plain = self.plain_mass
        if graph.ef is not None:
            P = _CartEdgeEmbedFn.apply(X, self.projVecs, self.freqs, self.bias if (plain and self.enable_bias) else None, scale, edge_feat,
                                       self, graph, out_scale)
            return P if plain else self._homog_epilogue(P, out_scale, self.bias.reshape(-1) if self.enable_bias else None)
        P = _CartEmbedFn.apply(X, self.projVecs, self.freqs, self.bias if (plain and self.enable_bias) else None, scale, self, graph,
                               out_scale)
        return P if plain else self._homog_epilogue(P, out_scale, self.bias.reshape(-1) if self.enable_bias else None)

    def _cart_unit_table(self, graph, fr):
        """Unit coefficient table [rows, F] of the F frequencies (unit weights with tau <= 1), else None."""
        if not self._unit_fast(graph):
            return None
        L = _lib.lib()
        table = torch.empty((int(L.fsw_unit_table_rows(_lib.REG_MAX_DEG)), self.nFreqs), dtype=torch.float32, device=fr.device)
        _lib.check(L.fsw_unit_coeff_table(_lib.ptr(fr), self.nFreqs, _lib.REG_MAX_DEG, _lib.ptr(table), self.nFreqs,
                                          torch.cuda.current_stream(fr.device).cuda_stream), "fsw_unit_coeff_table")
        return table

    def _cart_scratch_bytes(self, graph, st, backward):
        """Bytes of scratch the tuned Cartesian forward (backward: its backward) needs on this graph, 0 for none: the library's answer
        from the host copy of the degree bins, the longest row, the weight mode and the number of slices.  No device is touched."""
        a = _lib.CartArgs()
        a.S, a.tau, a.max_degree = self.nSlices, self.total_mass_pad_thresh, st[_lib.STAT_MAX_DEGREE]
        a.w = graph.w.data_ptr() if graph.w is not None else None
        a.bin_start_host = graph.bin_start_host[0].ctypes.data
        return int(_lib.lib().fsw_embed_cart_scratch_bytes(ctypes.byref(a), int(backward)))

    def _cart_forward_scratch_bytes(self, graph, st):
        """Bytes of scratch the tuned Cartesian forward uses on this graph, 0 for none: one scratch line per workgroup of the longest rows'
        kernels (fsw_embed_cart_forward_scratch_bytes), from the same host values as _cart_scratch_bytes."""
        a = _lib.CartArgs()
        a.S, a.tau, a.max_degree = self.nSlices, self.total_mass_pad_thresh, st[_lib.STAT_MAX_DEGREE]
        a.w = graph.w.data_ptr() if graph.w is not None else None
        a.bin_start_host = graph.bin_start_host[0].ctypes.data
        return int(_lib.lib().fsw_embed_cart_forward_scratch_bytes(ctypes.byref(a)))

    def _cart_backward_scratch_bytes(self, graph, st):
        """Bytes of scratch the tuned Cartesian backward uses on this graph, 0 for none: one scratch line per wavefront or workgroup of
        its long-row kernels (fsw_embed_cart_backward_keys_scratch_bytes), from the same host values as _cart_scratch_bytes."""
        a = _lib.CartArgs()
        a.S, a.tau, a.max_degree = self.nSlices, self.total_mass_pad_thresh, st[_lib.STAT_MAX_DEGREE]
        a.w = graph.w.data_ptr() if graph.w is not None else None
        a.bin_start_host = graph.bin_start_host[0].ctypes.data
        return int(_lib.lib().fsw_embed_cart_backward_keys_scratch_bytes(ctypes.byref(a)))

    # form -> (unit weights?, the library's queries of the form's lines, its largest measured line count and its scratch bytes)
    _CART_SPLIT_FORMS = {
        "forward": (True, "fsw_embed_cart_split_lines", "fsw_embed_cart_split_max_lines", "fsw_embed_cart_split_scratch_bytes"),
        "forward_w": (False, "fsw_embed_cart_split_w_lines", "fsw_embed_cart_split_w_max_lines", "fsw_embed_cart_split_w_scratch_bytes"),
        "backward": (True, "fsw_embed_cart_split_backward_lines", "fsw_embed_cart_split_backward_max_lines",
                     "fsw_embed_cart_split_backward_scratch_bytes"),
        "backward_w": (False, "fsw_embed_cart_split_w_backward_lines", "fsw_embed_cart_split_w_backward_max_lines",
                       "fsw_embed_cart_split_w_backward_scratch_bytes"),
    }

    def _cart_split_bytes(self, graph, st, form):
        """The policy of the split forms of the longest rows (csrc/embed_split_cart*.hip), decided ONCE per forward or backward on the
        module's nSlices, so that every serialize_num_slices chunk takes the same form: bytes of scratch the split form needs, or 0 for
        the one-workgroup-per-line kernel -- the other weight mode (a weight tensor, W='uniform' or total_mass_pad_thresh > 1 are general
        weights; it leaves before the query), no such row, or more lines than the form's largest measured count, which fill the chip by
        themselves.  Host values only.  Called through the class by the four methods below, which tests run on stand-in modules."""
        unit, lines_fn, max_lines_fn, bytes_fn = FSW_embedding._CART_SPLIT_FORMS[form]
        if (graph.w is None and self.total_mass_pad_thresh <= 1.0) != unit:
            return 0
        a = _lib.CartArgs()
        a.S, a.F, a.tau, a.max_degree = self.nSlices, self.nFreqs, self.total_mass_pad_thresh, st[_lib.STAT_MAX_DEGREE]
        a.w = graph.w.data_ptr() if graph.w is not None else None
        a.bin_start_host = graph.bin_start_host[0].ctypes.data
        L = _lib.lib()
        lines = int(getattr(L, lines_fn)(ctypes.byref(a)))
        if not (0 < lines <= int(getattr(L, max_lines_fn)())):
            return 0
        return int(getattr(L, bytes_fn)(ctypes.byref(a)))

    def _cart_split(self, graph, st):
        """_cart_split_bytes of the forward with unit weights (csrc/embed_split_cart.hip)."""
        return FSW_embedding._cart_split_bytes(self, graph, st, "forward")

    def _cart_split_w(self, graph, st):
        """_cart_split_bytes of the forward with general weights (csrc/embed_split_cart_w.hip)."""
        return FSW_embedding._cart_split_bytes(self, graph, st, "forward_w")

    def _cart_split_backward(self, graph, st):
        """_cart_split_bytes of the backward with unit weights (csrc/embed_split_cart_bwd.hip)."""
        return FSW_embedding._cart_split_bytes(self, graph, st, "backward")

    def _cart_split_w_backward(self, graph, st):
        """_cart_split_bytes of the backward with general weights (csrc/embed_split_cart_w_bwd.hip)."""
        return FSW_embedding._cart_split_bytes(self, graph, st, "backward_w")

    def _cart_scratch(self, graph, st, backward=False, reuse=None, split_bytes=0):
        """The scratch buffer of the forward (_cart_forward_scratch_bytes) or of the backward (_cart_backward_scratch_bytes), or of
        split_bytes (_cart_split / _cart_split_w / _cart_split_backward / _cart_split_w_backward) if larger; None for 0 bytes; reuse (the forward's buffer) when it is large enough."""
        nbytes = max(self._cart_backward_scratch_bytes(graph, st) if backward else self._cart_forward_scratch_bytes(graph, st), split_bytes)
        if reuse is not None and reuse.numel() >= nbytes:
            return reuse
        return torch.empty(nbytes, dtype=torch.uint8, device=graph.rowptr.device) if nbytes else None

    def _cart_tuned_args(self, graph, st, Xp, ldp, fr, S, table, scratch, out_scale, has_mass, split=False, split_backward=False, split_w=False,
                         split_w_backward=False, col=None):
        """struct fsw_cart_args of the tuned entry points (fsw_embed_cart_f32, fsw_embed_cart_backward_keys_f32) without the
        output / gradient fields.  split: FSW_CART_SPLIT_LINES, for the forward call only (_cart_split); split_w: FSW_CART_SPLIT_W_LINES,
        for the forward call only (_cart_split_w); split_backward: FSW_CART_SPLIT_BWD_LINES, for the backward call only
        (_cart_split_backward); split_w_backward: FSW_CART_SPLIT_W_BWD_LINES, for the backward call only (_cart_split_w_backward).
        col: the column array the kernels gather Xp by, the graph's by default; with edge features Xp is the key array of _edge_keys
        (one row per CSR entry) and col the identity (_identity_col) -- everything else still comes from the graph."""
        a = _cart_args(self, Xp, ldp, fr, S, out_scale, has_mass, self._mass_scale_read(st))
        a.flags = ((_lib.CART_SPLIT_LINES if split else 0) | (_lib.CART_SPLIT_BWD_LINES if split_backward else 0) |
                   (_lib.CART_SPLIT_W_LINES if split_w else 0) | (_lib.CART_SPLIT_W_BWD_LINES if split_w_backward else 0))
        a.rowptr, a.col = graph.rowptr.data_ptr(), (col if col is not None else graph.col).data_ptr()
        a.w = graph.w.data_ptr() if graph.w is not None else None
        a.perm, a.bin_start, a.bin_start_host = graph.perm.data_ptr(), graph.bin_start.data_ptr(), graph.bin_start_host[0].ctypes.data
        a.num_rows, a.max_degree = graph.num_rows, st[_lib.STAT_MAX_DEGREE]
        a.unit_table, a.ldt = (table.data_ptr(), self.nFreqs) if table is not None else (None, 0)
        if scratch is not None:
            a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
        return a

    def prepare_cartesian(self, X, graph: CSRGraph):
        """What the tuned Cartesian forward needs and its backward needs again: ONE projection of all S slices at
        ldp = round_up(S, 32) -- the call the generic path makes (_project), so both sort bit-identical keys --, the one
        device->host stats read of the forward (input validation as in prepare()), the unit coefficient table, the form the longest
        unit-weight rows take ("split": _cart_split), the form the longest general-weight rows take ("split_w": _cart_split_w) and the
        scratch of the longest rows."""
        L = _lib.lib()
        S = self.nSlices
        assert X.is_contiguous() and X.dtype == torch.float32 and graph.num_chunks == 1
        ldp = _round_up(S, 32)      # fsw_project_f32 takes its wavefront-per-tile kernel for <= 64 columns at this stride
        Xp = torch.empty((X.shape[0], ldp), dtype=torch.float32, device=X.device)
        V = self.projVecs.detach()
        _lib.check(L.fsw_project_f32(_lib.ptr(X), X.shape[0], self.d_in, X.stride(0), _lib.ptr(V), S, V.stride(0), _lib.ptr(Xp), ldp,
                                     None, 0, _lib.ptr(graph.stats_dev), torch.cuda.current_stream(X.device).cuda_stream),
                   "fsw_project_f32")
        st = self._checked_stats(graph)   # one device->host read per forward (flags + degree bins)
        split_bytes, split_w_bytes = self._cart_split(graph, st), self._cart_split_w(graph, st)    # one of them is 0
        col = None
        assert (graph.ef is None) == (self.d_edge == 0), 'edge features must be given exactly when d_edge > 0'
        if graph.ef is not None:
            # edge features: the sort kernels run on the key of every CSR entry, K [nnz, ldk], gathered by the identity; the backward
            # reads the same K, so both directions see bit-identical keys
            Xp, ldp = self._edge_keys(graph, st, Xp, ldp, 0, S)
            col = self._identity_col(graph, st)
        return {"Xp": Xp, "ldp": ldp, "col": col, "stats": st, "table": self._cart_unit_table(graph, self.freqs.detach().contiguous()),
                "scratch": self._cart_scratch(graph, st, split_bytes=max(split_bytes, split_w_bytes)), "split": split_bytes > 0,
                "split_w": split_w_bytes > 0}

    def _edge_keys(self, graph, st, Xp, ldp, k0, k1, K=None):
        """(K, ldk): K[e, s] = Xp[col[e], s] + <ef[e], projVecs[k0 + s, d_in:]> for the st[STAT_NNZ] entries of a coalesced graph with edge
        features and the slices k0 .. k1 - 1 whose projection Xp holds (fsw_edge_keys_f32, csrc/edge_keys.hip: the float32 fma chain of
        the diagonal edge-feature kernels).  ldk = the slices rounded up to 4 floats: the Cartesian kernels ask ldp >= S of their key
        array and nothing else (cart_check_common), and rows of whole 16 bytes give the key kernel its 16-byte accesses.  Called after
        the stats read, which has validated the column indices the kernel trusts.  K: a buffer to fill again (chunks of slices)."""
        S, nnz = k1 - k0, st[_lib.STAT_NNZ]
        ldk = _round_up(S, 4)
        if K is None:
            K = torch.empty((max(nnz, 1), ldk), dtype=torch.float32, device=Xp.device)
        assert K.shape == (max(nnz, 1), ldk) and 0 <= nnz <= graph.col.numel() and graph.ef.shape[1] == self.d_edge
        V = self.projVecs.detach()
        _lib.check(_lib.lib().fsw_edge_keys_f32(_lib.ptr(graph.col), nnz, _lib.ptr(Xp), ldp, _lib.ptr(graph.ef), self.d_edge,
                                                V.data_ptr() + 4 * (k0 * V.stride(0) + self.d_in), V.stride(0), S, _lib.ptr(K), ldk,
                                                torch.cuda.current_stream(Xp.device).cuda_stream), "fsw_edge_keys_f32")
        return K, ldk

    @staticmethod
    def _identity_col(graph, st):
        """int32 0 .. nnz - 1, the column array that goes with the key array of _edge_keys; kept on the graph."""
        ident = getattr(graph, "_identity_col", None)
        n = max(st[_lib.STAT_NNZ], 1)
        if ident is None or ident.numel() < n:
            ident = graph._identity_col = torch.arange(n, dtype=torch.int32, device=graph.col.device)
        return ident

    def embed_cartesian_into(self, X, graph: CSRGraph, out, bias=None, serialize_num_slices=None, out_scale=1.0, prepared=None):
        """Tuned float32 Cartesian forward (fsw_embed_cart_f32) of a CSR graph into out [num_rows, d_out] (unit inner stride): the
        'plain' embedding, plus bias [has_mass + S F] when given.  serialize_num_slices chunks the slices; every chunk covers all
        frequencies (reference fsw_embedding.py:848).  prepared: the result of prepare_cartesian() (all slices in one chunk), which
        the caller keeps for the backward."""
        L = _lib.lib()
        dev = X.device
        S, F = self.nSlices, self.nFreqs
        has_mass = self.total_mass_encoding_dim
        assert X.is_contiguous() and X.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] == graph.num_rows
        assert out.shape[1] >= has_mass + S * F and graph.num_chunks == 1
        step = S if (prepared is not None or serialize_num_slices is None or serialize_num_slices >= S) else int(serialize_num_slices)
        assert step >= 1, 'serialize_num_slices must be None or a positive integer'
        stream = torch.cuda.current_stream(dev).cuda_stream
        fr = self.freqs.detach().contiguous()
        if prepared is None and step == S:
            prepared = self.prepare_cartesian(X, graph)
        if prepared is not None:
            Xp, ldp, st, table, scratch = (prepared[k] for k in ("Xp", "ldp", "stats", "table", "scratch"))
            split, split_w = prepared.get("split", False), prepared.get("split_w", False)
            keys, ldk, col = Xp, ldp, prepared.get("col")
        else:       # chunks of slices: Xp once per forward, refilled by every chunk
            ldp = _round_up(step, 32)
            Xp = torch.empty((X.shape[0], ldp), dtype=torch.float32, device=dev)
            V = self.projVecs.detach()
            table = self._cart_unit_table(graph, fr)
            st = scratch = None
            split = split_w = False
            keys, ldk, col = Xp, ldp, None
            assert (graph.ef is None) == (self.d_edge == 0), 'edge features must be given exactly when d_edge > 0'
        for k0 in range(0, S, step):
            k1 = min(S, k0 + step)
            if prepared is None:
                Vc = V[k0:k1]
                _lib.check(L.fsw_project_f32(_lib.ptr(X), X.shape[0], self.d_in, X.stride(0), _lib.ptr(Vc), k1 - k0, Vc.stride(0),
                                             _lib.ptr(Xp), ldp, None, 0, _lib.ptr(graph.stats_dev) if k0 == 0 else None, stream),
                           "fsw_project_f32")
                if st is None:
                    st = self._checked_stats(graph)   # one device->host read per forward (flags + degree bins)
                    split_bytes, split_w_bytes = self._cart_split(graph, st), self._cart_split_w(graph, st)    # on all nSlices: every chunk takes the same form
                    split, split_w = split_bytes > 0, split_w_bytes > 0
                    scratch = self._cart_scratch(graph, st, split_bytes=max(split_bytes, split_w_bytes))
                if graph.ef is not None:      # every chunk forms its own keys from its own Xp and its rows of projVecs[:, d_in:]
                    refill = keys if (keys is not Xp and keys.shape[1] == _round_up(k1 - k0, 4)) else None
                    keys, ldk = self._edge_keys(graph, st, Xp, ldp, k0, k1, K=refill)
                    col = self._identity_col(graph, st)
            first = k0 == 0
            col0 = 0 if first else has_mass + k0 * F
            a = self._cart_tuned_args(graph, st, keys, ldk, fr, k1 - k0, table, scratch, out_scale, has_mass if first else 0, split=split,
                                      split_w=split_w, col=col)
            a.out, a.ldo = out.data_ptr() + 4 * col0, out.stride(0)
            a.bias = (bias.data_ptr() + 4 * col0) if bias is not None else None
            _lib.check(L.fsw_embed_cart_f32(ctypes.byref(a), stream), "fsw_embed_cart_f32")
        return out

    def _homog_epilogue(self, P, out_scale, bias, in_place=False):
        """'homog' / 'homog_alt' (reference fsw_embedding.py:874-882, 1136-1144) on the 'plain' embedding without bias that the
        kernels wrote into the left d_out columns of P = [f(m) scale | emb]: rarely used epilogues, done with elementwise torch ops.
        Out of place (autograd differentiates it), or in_place on P without a full-size temporary (inference)."""
        emb = P[:, 1:self.d_out]
        tm = P[:, 0:1] / out_scale
        norm = emb.abs().mean(dim=-1, keepdim=True) / out_scale
        if self.total_mass_encoding_method == 'homog':
            col0, factor = out_scale * tm * norm, None
        else:
            col0 = out_scale * torch.where(tm <= 1, tm * (2 - tm), torch.ones_like(tm)) * norm
            factor = torch.where(tm <= 1, tm.square(), 2 * tm - 1)      # one per row
        if in_place:
            P[:, 0:1] = col0
            if factor is not None:
                emb.mul_(factor)
            out = P[:, :self.d_out]
        else:
            out = torch.cat([col0, emb if factor is None else emb * factor], dim=1)
        if bias is not None:
            out = out.add_(out_scale * bias) if in_place else out + out_scale * bias
        return P if in_place else out

    def embed_autograd(self, X, graph, out_scale=1.0, edge_feat=None, slice_range=None, group=None, reduce_grads=False,
                       edge_weight=None):
        """Differentiable embedding of a CSR graph (training path): see _EmbedGraphFn.  edge_feat: the per-input-edge
        feature tensor the graph was coalesced from (its gradient is routed back through graph.slot_of_edge).
        slice_range / group: this rank's block of slices under slice sharding (dist.py).
        edge_weight: the per-input-edge weights [num_input_edges] a coalesced graph (want_slots=True, no edge features) was built
        from; the embedding is then differentiable in them too (_EmbedGraphWFn; 'plain' mass encoding, no slice sharding): rows of up
        to 24 neighbours on csrc/embed_w_bwd.hip, 25 .. 1024 on csrc/embed_w_sort_bwd.hip, longer ones on csrc/embed_w_long_bwd.hip."""
        bias = self.bias if self.enable_bias else None
        scale = self.total_mass_encoding_scale if self.encode_total_mass else None
        if edge_weight is not None:
            if not self.plain_mass or edge_feat is not None or slice_range is not None or self.cartesian_mode:
                raise NotImplementedError("fsw_gnn_amd: gradients of the edge weights need total_mass_encoding_method='plain', diagonal "
                                          "mode, no edge features and no slice sharding")
            return _EmbedGraphWFn.apply(X, self.projVecs, self.freqs, bias, scale, edge_weight, self, graph, out_scale)
        if self.plain_mass:
            return _EmbedGraphFn.apply(X, self.projVecs, self.freqs, bias, scale, edge_feat, self, graph, out_scale, slice_range, group,
                                       reduce_grads, True)
        if slice_range is not None:
            raise NotImplementedError("slice sharding supports total_mass_encoding_method='plain' only")
        # 'homog' / 'homog_alt' (reference fsw_embedding.py:874-882, 1136-1144): the 'plain' embedding without bias from the
        # kernels, then the same epilogue as embed_into(), out of place so that autograd differentiates it
        P = _EmbedGraphFn.apply(X, self.projVecs, self.freqs, None, scale, edge_feat, self, graph, out_scale, None, None, False, False)
        return self._homog_epilogue(P, out_scale, bias)

    # ------------------------------------------------------------------------------------------------
    # backward of unit-weight graphs: store the key gradients ([nnz, nSlices] float32) and sum them sender by sender instead of
    # float atomics, as long as that buffer stays below this size (10.2 GB at 10M edges x 256 slices); 0 = always atomics
    store_sum_backward_max_bytes = 32 << 30
    store_sum_free_memory_fraction = 0.25   # ... and below this share of the device memory that is free right now

    def store_sum_budget(self, device):
        """Bytes the transient [nnz, nSlices] key-gradient buffer of the store-and-sum backward may take: the fixed ceiling,
        capped by a quarter of the currently free device memory (free in the driver's sense + what torch's caching allocator
        holds unused), so that a training run that fits with the atomic backward never runs out of memory inside backward."""
        cap = int(self.store_sum_backward_max_bytes)
        if cap <= 0:
            return 0
        try:
            free, _ = torch.cuda.mem_get_info(device)
            cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
            cap = min(cap, int((free + max(cached, 0)) * self.store_sum_free_memory_fraction))
        except Exception:   # noqa: BLE001 -- no query, keep the fixed ceiling
            pass
        return cap

    @property
    def plain_mass(self):
        """The kernels' output is final: no total-mass column, or the 'plain' method (no 'homog' / 'homog_alt' epilogue)."""
        return (not self.encode_total_mass) or self.total_mass_encoding_method == 'plain'

    def _unit_fast(self, graph):
        """Unit weights and no padding above one element: the coefficients depend on the degree alone (unit coefficient table)."""
        return graph.w is None and self.total_mass_pad_thresh <= 1.0

    def _mass_scale_read(self, st):
        """The total-mass scale as _checked_stats parked it in the stats words st (float32 bits in an int)."""
        return struct.unpack('f', struct.pack('i', st[_lib.STAT_USER]))[0] if self.encode_total_mass else 1.0

    def prepare(self, X, graph: CSRGraph, x_copy=None, linear2=None, slice_range=None):
        """Projection of a block of slices (default: all) + (unit weights) coefficient table + the one device->host stats
        read of the forward.

        linear2 = (W2 [H2, d_in] contiguous, b2 [H2] or None, Y2 [n, H2]): the projection GEMM also writes
        Y2[graph.invperm[i]] = X[i] . W2^T + b2, the vertex-feature half of FSW_conv's first Linear layer in the
        row order of the degree bins (csrc/conv_fused.hip reads it back as contiguous runs).
        x_copy (optional [num_cols, d_in] view with unit inner stride): the projection kernel also stores X there
        (FSW_conv's concat buffer, reference fsw_conv.py:357-358).

        Returns a dict that embed_into(prepared=...) or FSW_conv's fused Linear path consume.  Input validation
        (reference fsw_embedding.py:652-703) happens here: the kernels set flag bits, the host reads them once.
        """
        ka, kb = (0, self.nSlices) if slice_range is None else slice_range
        assert 0 <= ka <= kb <= self.nSlices, 'bad slice_range'
        assert X.is_contiguous()
        unit_fast = self._unit_fast(graph)
        if kb == ka:      # a rank without slices (more ranks than slices): only the stats
            if x_copy is not None:
                x_copy.copy_(X)
            return {"Xp": None, "ldp": 0, "table": None, "stats": self._checked_stats(graph), "unit_fast": unit_fast,
                    "slice_range": (ka, kb)}
        ldp, Xp, table = self._projection_buffers(X, kb - ka, unit_fast)
        self._project_slices(X, graph, ka, kb, Xp, ldp, table, x_copy, linear2)
        st = self._checked_stats(graph)
        return {"Xp": Xp, "ldp": ldp, "table": table, "stats": st, "unit_fast": unit_fast, "slice_range": (ka, kb)}

    def _projection_buffers(self, X, width, unit_fast):
        """(ldp, Xp [num_cols, ldp], unit coefficient table [rows, ldp] or None) for projections of up to `width` slices at a time."""
        ldp = _round_up(width, 64)
        Xp = torch.empty((X.shape[0], ldp), dtype=torch.float32, device=X.device)
        table = None
        if unit_fast:
            table = torch.empty((int(_lib.lib().fsw_unit_table_rows(_lib.REG_MAX_DEG)), ldp), dtype=torch.float32, device=X.device)
        return ldp, Xp, table

    def _project_slices(self, X, graph, ka, kb, Xp, ldp, table, x_copy=None, linear2=None, first=True):
        """Xp[:, :kb - ka] = X . projVecs[ka:kb]^T and (table given) the unit coefficient table of freqs[ka:kb].  The by-products
        -- the input flags into graph.stats_dev, the copy of X into x_copy -- belong to the `first` projection of a forward."""
        L = _lib.lib()
        stream = torch.cuda.current_stream(X.device).cuda_stream
        S = kb - ka
        V = self.projVecs.detach()[ka:kb]
        stats = _lib.ptr(graph.stats_dev) if first else None
        if linear2 is not None:
            W2, b2, Y2 = linear2
            assert x_copy is None and W2.is_contiguous() and W2.shape[1] == self.d_in and Y2.stride(1) == 1
            rc = L.fsw_project_linear_f32(_lib.ptr(X), X.shape[0], self.d_in, X.stride(0), _lib.ptr(V), S, V.stride(0),
                                          _lib.ptr(Xp), ldp, _lib.ptr(W2), W2.shape[0], W2.stride(0), _lib.ptr(b2),
                                          _lib.ptr(Y2), Y2.stride(0), _lib.ptr(graph.invperm), stats, stream)
        else:
            rc = L.fsw_project_f32(_lib.ptr(X), X.shape[0], self.d_in, X.stride(0), _lib.ptr(V), S, V.stride(0), _lib.ptr(Xp),
                                   ldp, _lib.ptr(x_copy) if first else None, x_copy.stride(0) if x_copy is not None else 0,
                                   stats, stream)
        _lib.check(rc, "fsw_project_f32")
        if table is not None:
            fr = self.freqs.detach()[ka:kb]
            rc = L.fsw_unit_coeff_table(_lib.ptr(fr), S, _lib.REG_MAX_DEG, _lib.ptr(table), ldp, stream)
            _lib.check(rc, "fsw_unit_coeff_table")

    def _checked_stats(self, graph):
        """The one device->host copy of a forward: validation flags, degree-class counts and -- parked in the spare stats
        word right before the copy -- the current value of the total-mass scale (read from the parameter every time: no
        host-side cache that an in-place edit of .data could outdate)."""
        if self.encode_total_mass:
            graph.stats_dev[_lib.STAT_USER:_lib.STAT_USER + 1].view(torch.float32).copy_(
                self.total_mass_encoding_scale.detach().reshape(1).to(torch.float32))
        st = graph.read_stats()
        if fsw_embedding_basic_safety_checks:
            fl = st[_lib.STAT_FLAGS]
            assert not (fl & _lib.FLAG_CSR_MALFORMED), CSR_MALFORMED_MESSAGE
            assert not (fl & _lib.FLAG_CSR_COL_ORDER), CSR_COL_ORDER_MESSAGE
            assert not (fl & _lib.FLAG_INDEX_RANGE), "adjacency index out of range"
            assert not (fl & _lib.FLAG_X_NONFINITE), "The entries of X cannot contain NaNs or infs"
            assert not (fl & _lib.FLAG_W_NONFINITE), "All entries of W must be finite"
            assert not (fl & _lib.FLAG_W_NEGATIVE), "All entries of W must be nonnegative"
        return st

    def make_args(self, graph, st, Xp, ldp, freqs, S, table, out_ptr, ldo, bias_ptr, out_scale, has_mass, scratch=None,
                  slice_offset=0, chunk=None):
        """struct fsw_embed_args for one call.  chunk = c restricts the call to the recipients of row chunk c of a graph
        built with chunk_rows > 0 (graph.py)."""
        a = _lib.EmbedArgs()
        a.rowptr, a.col = graph.rowptr.data_ptr(), graph.col.data_ptr()
        a.w = graph.w.data_ptr() if graph.w is not None else None
        a.perm = graph.perm.data_ptr()
        if chunk is None:
            assert graph.num_chunks == 1, 'a graph with row chunks is consumed chunk by chunk'
            a.bin_start, rows = graph.bin_start.data_ptr(), graph.num_rows
        else:
            a.bin_start = graph.bin_start.view(-1, _lib.NUM_BINS + 1)[chunk].data_ptr()
            rows = min(graph.chunk_rows, graph.num_rows - chunk * graph.chunk_rows) if graph.chunk_rows else graph.num_rows
        a.num_rows = rows
        bsh = getattr(graph, "bin_start_host", None)     # host copy of the bin table (read with the stats): exact grids
        if bsh is not None:
            a.bin_start_host = bsh[0 if chunk is None else chunk].ctypes.data
        a.Xp, a.ldp, a.freqs, a.S, a.tau = Xp.data_ptr(), ldp, freqs.data_ptr(), S, float(self.total_mass_pad_thresh)
        a.unit_table, a.ldt = (table.data_ptr() if table is not None else None), ldp
        a.out, a.ldo, a.bias = out_ptr, ldo, bias_ptr
        a.out_scale, a.has_mass = float(out_scale), has_mass
        a.mass_fn = _MASS_FN[self.total_mass_encoding_function]
        a.mass_scale = self._mass_scale_read(st)
        a.num_reg_rows, a.num_lds_rows = min(st[_lib.STAT_NUM_REG], rows), min(st[_lib.STAT_NUM_LDS], rows)
        a.num_global_rows, a.num_zero_rows = min(st[_lib.STAT_NUM_GLOBAL], rows), min(st[_lib.STAT_NUM_ZERO], rows)
        a.max_degree = st[_lib.STAT_MAX_DEGREE]
        a.scratch = scratch.data_ptr() if scratch is not None else None
        a.scratch_bytes = scratch.numel() if scratch is not None else 0
        if graph.ef is not None:            # edge features: Ve = projVecs[:, d_in:], read in place (row stride d_in + d_edge)
            V = self.projVecs.detach()
            a.efeat, a.d_edge = graph.ef.data_ptr(), self.d_edge
            a.Ve, a.ldve = V.data_ptr() + 4 * (slice_offset * V.stride(0) + self.d_in), V.stride(0)
        return a

    def embed_into(self, X, graph: CSRGraph, out, out_scale=1.0, serialize_num_slices=None, slice_range=None, x_copy=None,
                   prepared=None, chunks=None, long_rows_only=False, epilogue=True):
        """Writes out_scale * E(X, graph) into the left columns of `out` (row stride out.stride(0)).

        X [num_cols, d_in] float32 contiguous; out [num_rows, >= width] float32 with unit inner stride, where
        width = d_out, or total_mass_dim + (kb - ka) when slice_range = (ka, kb) restricts the call to a block of
        slices (multi-GPU slice sharding, dist.py: column 0 is still the total-mass column, then slices ka..kb-1).
        x_copy (optional [num_cols, d_in] view with unit inner stride): the projection kernel also stores X there
        (FSW_conv's concat buffer, reference fsw_conv.py:357-358).
        prepared: the result of prepare() (its slice_range is used); chunks: row chunks to process (default all).
        long_rows_only: write only the rows of more than REG_MAX_DEG neighbours (the other rows of `out` are not touched).
        epilogue = False: stop at what the kernels write for the 'homog' / 'homog_alt' methods, the 'plain' embedding without bias
        (embed_autograd applies the epilogue out of place); no difference for the 'plain' method.
        This is the hot path: projection (MFMA) -> coefficient table -> fused neighbourhood kernels.
        """
        L = _lib.lib()
        dev = X.device
        has_mass = self.total_mass_encoding_dim
        if x_copy is not None:
            assert x_copy.shape == X.shape and x_copy.stride(1) == 1 and x_copy.dtype == X.dtype
        if prepared is not None:
            assert slice_range is None or tuple(slice_range) == tuple(prepared["slice_range"])
            slice_range = prepared["slice_range"]
        ka, kb = (0, self.nSlices) if slice_range is None else slice_range
        assert 0 <= ka < kb <= self.nSlices or self.d_out == 0, 'bad slice_range'
        S = kb - ka
        partial = (ka, kb) != (0, self.nSlices)
        assert X.is_contiguous() and out.stride(1) == 1 and out.shape[0] == graph.num_rows and out.shape[1] >= has_mass + S
        stream = torch.cuda.current_stream(dev).cuda_stream
        if self.d_out == 0:
            return out
        if self.nSlices == 0:
            raise NotImplementedError("fsw_gnn_amd: nSlices == 0 with encode_total_mass is not supported")
        homog = epilogue and not self.plain_mass      # the 'homog' / 'homog_alt' epilogue follows the kernels and adds the bias
        if partial and homog:
            raise NotImplementedError("slice sharding supports total_mass_encoding_method='plain' only")
        bias = self.bias.detach() if (self.enable_bias and epilogue and not homog) else None
        if bias is not None and partial:
            bias = torch.cat([bias[:has_mass], bias[has_mass + ka:has_mass + kb]])

        step = S if (serialize_num_slices is None or serialize_num_slices >= S) else int(serialize_num_slices)
        assert step >= 1, 'serialize_num_slices must be None or a positive integer'
        if prepared is not None:
            assert step == S, 'a prepared projection covers its slices in one chunk'
            ldp, Xp, table, st = prepared["ldp"], prepared["Xp"], prepared["table"], prepared["stats"]
        else:       # Xp and the table once per forward, refilled by every chunk of slices
            ldp, Xp, table = self._projection_buffers(X, step, self._unit_fast(graph))
            st = None
        freqs = self.freqs.detach()[ka:kb]
        scratch = None
        assert (graph.ef is None) == (self.d_edge == 0), 'edge features must be given exactly when d_edge > 0'
        if chunks is None:
            chunks = [None] if graph.num_chunks == 1 and not graph.chunk_rows else range(graph.num_chunks)
        for k0 in range(0, S, step):
            k1 = min(S, k0 + step)
            Sc = k1 - k0
            fc = freqs[k0:k1]
            if prepared is None:
                self._project_slices(X, graph, ka + k0, ka + k1, Xp, ldp, table, x_copy, first=(k0 == 0))
            if st is None:
                st = self._checked_stats(graph)   # one device->host read per forward (flags + degree classes)
            if scratch is None and st[_lib.STAT_NUM_GLOBAL] > 0:
                scratch = torch.empty(int(L.fsw_embed_scratch_bytes(st[_lib.STAT_MAX_DEGREE])), dtype=torch.uint8, device=dev)
            first = (k0 == 0)
            hm = has_mass if first else 0          # the first chunk also writes the total-mass column
            col0 = 0 if first else has_mass + k0   # first destination column of this chunk
            for c in chunks:
                a = self.make_args(graph, st, Xp, ldp, fc, Sc, table, out.data_ptr() + 4 * col0, out.stride(0),
                                   (bias.data_ptr() + 4 * col0) if bias is not None else None, out_scale, hm, scratch,
                                   slice_offset=ka + k0, chunk=c)
                if long_rows_only:      # rows above REG_MAX_DEG only (FSW_conv: the fused kernel did the others)
                    a.num_reg_rows, a.num_zero_rows = 0, 0
                rc = L.fsw_embed_f32(ctypes.byref(a), stream)
                _lib.check(rc, "fsw_embed_f32")

        if homog:      # the kernels wrote f(m) * scale into column 0
            self._homog_epilogue(out, out_scale, self.bias.detach() if self.enable_bias else None, in_place=True)
        return out


# ----------------------------------------------------------------------------------------------------
# segmented cumulative sum: public signature of the reference (fsw_embedding.py:2795)
# ----------------------------------------------------------------------------------------------------
def segcumsum(values, segment_ids, max_seg_size=None, in_place=False, thorough_verify_input=False,
              always_use_pure_torch=False, reverse=False):
    """Inclusive scan of `values` restarted wherever consecutive `segment_ids` differ (HIP, stream-ordered).

    Keeps the reference signature; max_seg_size is accepted and unused (the scan is single-level), and
    always_use_pure_torch=True is rejected because this build has no PyTorch path.
    """
    assert values.dim() == 1, 'values must be a 1-dimensional tensor'
    assert segment_ids.dim() == 1, 'segment_ids must be a 1-dimensional tensor'
    assert segment_ids.numel() == values.numel(), 'values and segment_ids must contain the same number of elements'
    assert segment_ids.dtype in (torch.int32, torch.int64), 'segment_ids must have int32 or int64 dtype'
    assert values.device == segment_ids.device, 'values and segment_ids must be on the same device'
    assert not segment_ids.is_sparse, 'segment_ids cannot be sparse'
    assert segment_ids.is_contiguous(), 'segment_ids must be in contiguous format'
    assert not values.is_sparse, 'values cannot be sparse'
    assert (not in_place) or values.is_contiguous(), 'when in_place==True, values must be in contiguous format'
    if max_seg_size is not None:
        assert isinstance(max_seg_size, numbers.Number)
        assert max_seg_size >= 1
    if always_use_pure_torch:
        raise RuntimeError("fsw_gnn_amd has no pure-PyTorch path: always_use_pure_torch=True is not supported")
    if values.device.type != 'cuda':
        raise RuntimeError("fsw_gnn_amd.segcumsum: tensors must live on a HIP device (no CPU path)")
    if values.dtype == torch.float32:
        dtype_num = 0
    elif values.dtype == torch.float64:
        dtype_num = 1
    else:
        raise RuntimeError("Unsupported input_tensor dtype ''%s''" % (str(values.dtype)))
    if thorough_verify_input:
        _, cc = torch.unique_consecutive(segment_ids, return_counts=True)
        _, ct = torch.unique(segment_ids, return_counts=True)
        assert cc.numel() == ct.numel(), 'repeated segment IDs detected'
        assert not torch.isinf(values).any(), "Found infs in ''values''"
        assert not torch.isnan(values).any(), "Found nans in ''values''"
    L = _lib.lib()
    src = values.contiguous()
    out = src if in_place else torch.empty_like(src)
    n = src.numel()
    if n == 0:
        return out
    ws_bytes = int(L.fsw_segcumsum_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=values.device)
    stream = torch.cuda.current_stream(values.device).cuda_stream
    rc = L.fsw_segcumsum(dtype_num, _lib.ptr(src), _lib.ptr(out), _lib.ptr(segment_ids), segment_ids.element_size(), n,
                         1 if reverse else 0, _lib.ptr(ws), ws_bytes, stream)
    _lib.check(rc, "fsw_segcumsum")
    return out
