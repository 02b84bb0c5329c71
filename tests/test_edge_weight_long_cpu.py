"""The weight gradient of rows above 24 neighbours (csrc/embed_w_sort_bwd.hip), the parts that need no GPU.

(a) The sorted, lane-blocked form the kernel evaluates (tests/edge_weight_long_cases.py: lane_blocked_weight_grad -- M ranks per lane,
    the lane's running cumulative weight on an exclusive scan of the lanes, in-lane suffix of q, reverse scan of the lanes' sums, the
    pad element's R picked at its rank), in numpy, per entry and per slice against weight_grad_reference (autograd of the forward,
    tests/weight_grad_ref.py) on the inputs of the GPU test: one recipient per degree 0, 24 .. 2049 at both sides of every instance,
    keys distinct or tied on the grid of 1/8 with the pad key, weights from {0, 1/4, 1/2, 1} with the kind (mass below tau / tau
    exactly / above tau) cycling over the rows, tau 1 and 3, the BASE = 9 base slices.  Bound: 1e-12 of the row maximum, the bound of
    tests/test_edge_weight_cpu.py (both sides are float64).
    Measured: tau 1 distinct 8.5e-13 (the row of 2048), tied 5.8e-13; tau 3 distinct 4.6e-13, tied 1.1e-13 of the row maximum.
(b) The condition of the GPU test of w_lo: with weights w + w_lo (float64) as the truth, the same form evaluated on w alone misses the
    GPU test's per-entry bound on at least one entry of EVERY row above 24 neighbours, for every S of that test -- a kernel that
    dropped w_lo on any of these rows would fail there.
    Measured: the smallest over the rows of the largest err / bound per row is 1.8 (tau 3, tied keys, S = 70, the row of 2048, which the
    generic kernel's A = S = 70 adds bound loosely; 139 and more at S = 3 and 8); the form on w + w_lo stands at 1.2e-12 of the row maximum
    against its reference (LO_BOUND below says why that is not 1e-12).
(c) fsw_embed_backward_w_tuned_max_degree is declared, bound and exported and returns the class limit; the scratch query returns
    what it returned before (an upper bound now); the ABI version is 6.
"""
import os
import re

import numpy as np
import pytest

from tests import edge_weight_long_cases as LC
from tests.test_edge_weight_cpu import BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_SCALE = 0.7
LO_BOUND = 1e-11
BASE_ZEROS = LC.BASE                                                          # more zero readouts than the zero row's


def block_ratio(got, ref, rowptr):
    """test_edge_weight_cpu.block_ratio with empty rows (0): per row the largest |got - ref| over the row's [D, S] block, relative to
    the block's largest |ref|."""
    out = []
    for a, b in zip(rowptr[:-1], rowptr[1:]):
        top = np.abs(ref[a:b]).max() if b > a else 0.0
        out.append(np.abs(got[a:b] - ref[a:b]).max() / (top if top > 0 else 1.0) if b > a else 0.0)
    return np.array(out)


def test_the_inputs_cover_every_instance_and_kind():
    deg = np.array(LC.DEGREES)
    assert deg.sum() < 13000 and LC.DEGREES[LC.ZERO_ROW] > LC.REG_MAX
    for lo in (24, 32, 192, 256, 512, 1024, 2048):                            # both sides of every hand-over
        assert lo in LC.DEGREES and lo + 1 in LC.DEGREES
    assert {LC.ranks_per_lane(int(d)) for d in deg if LC.REG_MAX < d <= LC.TUNED_MAX} == {4, 8, 16, 32}
    assert [LC.slices_per_group(M) for M in (4, 8, 16, 32)] == [48, 24, 12, 4]
    # S = 3: fewer slices than wavefronts; S = 70: more slice groups than y-blocks for the longest instance
    assert min(LC.S_VALUES) < 4 and -(-max(LC.S_VALUES) // LC.slices_per_group(32)) > 4
    assert LC.float32_adds(24, 70) == 2 and LC.float32_adds(25, 70) == 2 and LC.float32_adds(1024, 70) == 4 and LC.float32_adds(1025, 70) == 70
    for tau in (1.0, 3.0):
        k = LC.kernel_inputs(tau, True)
        long_kinds = {kind for kind, d in zip(k["kinds"], deg) if d > LC.REG_MAX}
        assert long_kinds == {"lt", "eq", "gt"} and (k["w"] == 0).sum() > 1000 and (k["K"] == 0).any() and (k["w_lo"] < 0).any()
        assert not k["G"][LC.ZERO_ROW].any() and (k["G"][:, 1:] == 0).sum() > BASE_ZEROS


@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_lane_blocked_form_against_the_autograd_reference(tau, tied):
    k = LC.kernel_inputs(tau, tied)
    rowptr, deg = k["rowptr"], k["degrees"]
    ref = LC.base_reference(tau, tied, OUT_SCALE)
    G = OUT_SCALE * k["G"][:, 1:].astype(np.float64)
    got = LC.lane_blocked_weight_grad(rowptr, k["w"], k["K"], LC.base_freqs(), tau, G)
    long_rows = deg > LC.REG_MAX
    ratio = block_ratio(got, ref["gW_s"], rowptr)
    worst = int(np.where(long_rows, ratio, 0.0).argmax())
    print("tau %g %s: lane-blocked form against gW_s, per entry and slice / row maximum: %.2e (D = %d, %s)" % (
        tau, "tied" if tied else "distinct", ratio[long_rows].max(), deg[worst], k["kinds"][worst]))
    assert np.abs(ref["gW_s"]).max() > 0.1
    assert ratio[long_rows].max() <= BOUND, (int(deg[worst]), k["kinds"][worst], float(ratio[worst]))
    assert not got[rowptr[LC.ZERO_ROW]:rowptr[LC.ZERO_ROW + 1]].any() and not ref["gW_s"][rowptr[LC.ZERO_ROW]:rowptr[LC.ZERO_ROW + 1]].any()


@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_dropping_w_lo_exceeds_the_gpu_bound_on_every_long_row(tau, tied):
    """(b) of the module docstring."""
    k = LC.kernel_inputs(tau, tied)
    rowptr, deg = k["rowptr"], k["degrees"]
    G = OUT_SCALE * k["G"][:, 1:].astype(np.float64)
    dropped_base = LC.lane_blocked_weight_grad(rowptr, k["w"], k["K"], LC.base_freqs(), tau, G)
    kept_base = LC.lane_blocked_weight_grad(rowptr, k["w64"], k["K"], LC.base_freqs(), tau, G)
    ref_base = LC.base_reference(tau, tied, OUT_SCALE, lo=True)["gW_s"]
    long_rows = deg > LC.REG_MAX
    # the form itself follows w + w_lo.  LO_BOUND, not BOUND: off the grid of 1/4 the reference's own cumulative sums round (it divides
    # every weight by m first: up to 2049 terms of relative rounding 2^-53 each, times the phase factor 2 pi xi <= 28: 6.4e-12 at most)
    kept = block_ratio(kept_base, ref_base, rowptr)[long_rows].max()
    print("tau %g %s: lane-blocked form on w + w_lo against its reference: %.2e of the row maximum" % (tau, "tied" if tied else "distinct", kept))
    assert kept <= LO_BOUND
    for S in LC.S_VALUES:
        ref = LC.reference(tau, tied, OUT_SCALE, S, lo=True)
        sel, sg = np.arange(S) % LC.BASE, LC.sigma(S)
        dropped = (dropped_base[:, sel] * sg[None, :]).sum(axis=1)
        adds = np.repeat([LC.float32_adds(int(d), S) for d in deg], deg)
        bound = LC.gw_bound(ref, rowptr, S, adds)
        ratio = np.abs(dropped - ref["gW"]) / np.where(bound > 0, bound, 1.0)
        per_row = np.array([ratio[a:b].max() if b > a else 0.0 for a, b in zip(rowptr[:-1], rowptr[1:])])
        sensitive = long_rows & (np.arange(deg.size) != LC.ZERO_ROW)               # the zero row has no gradient to lose
        worst = int(np.where(sensitive, per_row, np.inf).argmin())
        print("tau %g %s S %d: w_lo dropped, smallest over the long rows of the largest err / bound: %.1f (D = %d)" % (
            tau, "tied" if tied else "distinct", S, per_row[worst], deg[worst]))
        assert per_row[sensitive].min() > 1.0, (S, int(deg[worst]), float(per_row[worst]))


def test_tuned_max_degree_is_declared_bound_and_exported():
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert re.search(r"#define\s+FSW_ABI_VERSION\s+6\b", header) and _lib.FSW_ABI_VERSION == 6
    assert re.search(r"\bint\s+fsw_embed_backward_w_tuned_max_degree\s*\(\s*void\s*\)", header)
    assert "fsw_embed_backward_w_tuned_max_degree" in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["fsw_embed_backward_w_tuned_max_degree"] == (_lib.ctypes.c_int, [])
    L = _lib.lib()
    assert L.fsw_abi_version() == 6
    limit = L.fsw_embed_backward_w_tuned_max_degree()
    assert limit == LC.TUNED_MAX and 1024 <= limit <= 2048
    for maxdeg in (24, 25, 300, 1024, 1025, 5000):                                 # the query is unchanged: an upper bound now
        want = 0 if maxdeg <= 24 else L.fsw_embed_generic_scratch_bytes(maxdeg, 100)
        assert L.fsw_embed_backward_w_scratch_bytes(maxdeg, 100) == want and (maxdeg <= 24 or want > 0)
