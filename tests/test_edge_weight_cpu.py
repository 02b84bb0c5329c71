"""FSW_conv(edge_weight=) and the weight gradient of csrc/embed_w_bwd.hip, the parts that need no GPU.

(a) The rank-free form of d out / d w the kernel evaluates (tests/edge_weight_cases.py: rank_free_weight_grad), in numpy, per entry
    and per slice against weight_grad_reference(...)["gW_s"] (autograd of the forward, tests/weight_grad_ref.py): rows of every
    degree 1 .. 32, keys on the grid of 1/8 with the pad key 0 (ties inside the rows and with the pad element), weights from
    {0, 1/4, 1/2, 1}, rows of total mass below tau, tau exactly and above tau, tau 1 and 3; and the case without a deficient row,
    where the reference pads nothing and the form is evaluated at tau / 2 (_GenericEmbedFn.key_grads).  Bound: 1e-12 of the row
    maximum (both sides are float64; the reference's own error against the reference implementation is 1e-13,
    tests/test_weight_grad_ref_cpu.py).
    Measured: tau 1: 1.8e-14, tau 3: 2.3e-14, no deficient row: tau 1: 2.7e-14, tau 3: 1.6e-14 of the row maximum.
(b) The new entry points are declared in include/fsw_hip.h, bound in _lib and exported by the built library; the ABI version is 6.
(c) FSW_conv on the CPU device raises AssertionError for a wrong shape or dtype of edge_weight and for edge_weight next to a
    torch.sparse_csr adjacency, before the "no CPU path" error.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import edge_weight_cases as C
from tests import weight_grad_ref as R

BOUND = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fsw_embed_backward_w_scratch_bytes", "fsw_embed_backward_w_f32", "fsw_embed_backward_w_lo_f32")


def block_ratio(got, ref, rowptr):
    """Per row the largest |got - ref| over the row's [D, S] block, relative to the block's largest |ref|."""
    out = []
    for a, b in zip(rowptr[:-1], rowptr[1:]):
        top = np.abs(ref[a:b]).max()
        out.append(np.abs(got[a:b] - ref[a:b]).max() / (top if top > 0 else 1.0))
    return np.array(out)


@pytest.mark.parametrize("nopad", [False, True], ids=["padded", "no_deficient_row"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_rank_free_form_against_the_autograd_reference(tau, nopad):
    c = C.cpu_rows(tau, nopad)
    deg = np.diff(c["rowptr"])
    kinds = set(c["kinds"])
    # (without a deficient row a row of D neighbours needs m >= tau, and m <= D)
    assert kinds == ({"eq", "gt"} if nopad else {"lt", "eq", "gt"}) and set(deg) == set(range(int(tau) if nopad else 1, 33))
    m = np.array([c["w"][a:b].sum(dtype=np.float64) for a, b in zip(c["rowptr"][:-1], c["rowptr"][1:])])
    assert (m == tau).any() and (m > tau).any() and ((m < tau).any() != nopad) and (c["w"] == 0).any() and (c["K"] == 0).any()
    fr = C.FREQS8.astype(np.float64)
    ref = R.weight_grad_reference(c["rowptr"], None, c["w"], c["K"], fr, tau, c["G"])
    got = C.rank_free_weight_grad(c["rowptr"], c["w"], c["K"], fr, 0.5 * tau if nopad else tau, c["G"])
    ratio = block_ratio(got, ref["gW_s"], c["rowptr"])
    worst = int(ratio.argmax())
    print("tau %g %s: rank-free form against gW_s, per entry and slice / row maximum: %.2e (D = %d, %s)" % (
        tau, "no deficient row" if nopad else "padded", ratio.max(), deg[worst], c["kinds"][worst]))
    assert np.abs(ref["gW_s"]).max() > 0.1 and ratio.max() <= BOUND, (deg[worst], c["kinds"][worst], float(ratio.max()))
    if nopad:      # the clamp rule at tau itself is NOT what the reference computes on the rows of m == tau: tau / 2 is needed
        wrong = block_ratio(C.rank_free_weight_grad(c["rowptr"], c["w"], c["K"], fr, tau, c["G"]), ref["gW_s"], c["rowptr"])
        assert wrong[np.array(c["kinds"]) == "eq"].max() > 1e-3


def test_new_entry_points_are_declared_bound_and_exported():
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert re.search(r"#define\s+FSW_ABI_VERSION\s+6\b", header) and _lib.FSW_ABI_VERSION == 6
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    restype, argtypes = _lib._SIGNATURES["fsw_embed_backward_w_f32"]
    assert restype is _lib.ctypes.c_int and len(argtypes) == 11 and argtypes[1] is _lib.c_i64 and argtypes[9] is _lib.c_sz
    assert _lib._SIGNATURES["fsw_embed_backward_w_scratch_bytes"] == (_lib.c_sz, [_lib.c_i64, _lib.c_i64])
    L = _lib.lib()                                    # the built library: every bound symbol resolves, same ABI version
    assert L.fsw_abi_version() == 6
    assert L.fsw_embed_backward_w_scratch_bytes(8, 100) == 0
    assert L.fsw_embed_backward_w_scratch_bytes(300, 100) == L.fsw_embed_generic_scratch_bytes(300, 100) > 0


def test_edge_weight_argument_checks_come_before_the_device_check():
    from fsw_gnn_amd import FSW_conv
    conv = FSW_conv(4, 3, embed_dim=9, device="cpu")
    n, E = 6, 10
    x = torch.zeros((n, 4))
    ei = torch.stack([torch.arange(E) % n, (torch.arange(E) * 5 + 1) % n])
    for bad in (torch.ones(E + 1), torch.ones((E, 1)), torch.ones(E, dtype=torch.float64), torch.ones(E, dtype=torch.int64)):
        with pytest.raises(AssertionError, match="edge_weight"):
            conv(x, ei, edge_weight=bad)
    adj = torch.sparse_coo_tensor(ei.flip(0), torch.ones(E), (n, n)).coalesce().to_sparse_csr()
    with pytest.raises(AssertionError, match="sparse_csr"):
        conv(x, adj, edge_weight=torch.ones(adj.values().numel()))
    with pytest.raises(AssertionError, match="edge_weight"):          # the tuple form: one weight per entry
        conv(x, (adj.crow_indices(), adj.col_indices()), edge_weight=torch.ones(E + 3))
    with pytest.raises(RuntimeError, match="no CPU path"):            # a well-formed call reaches the device check
        conv(x, ei, edge_weight=torch.ones(E))
