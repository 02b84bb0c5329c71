"""The weight gradient of rows above 1024 neighbours (csrc/embed_w_long_bwd.hip), the parts that need no GPU.

(a) The chunked total-minus-prefix form the kernel evaluates (tests/edge_weight_hub_cases.py: chunked_weight_grad -- chunks of 64 M
    ranks with the carries of cum, P and h from chunk to chunk, e_t = h(c1_t) key_t - P_t, the three cases of K', and the float64
    accumulator acc[j] + Ksum over a group of G slices), in numpy, per entry and per slice against weight_grad_reference (autograd of
    the forward, tests/weight_grad_ref.py) on the inputs of the GPU test: one recipient per degree 0, 1024 .. 32769, keys distinct or
    tied on the grid of 1/8 with the pad key, weights from {0, 1/4, 1/2, 1} with the kind cycling over the rows, tau 1 and 3, the
    BASE = 9 base slices; with M = 16, the shipped chunk of 1024 words.
    Bound: 1e-12 of the row maximum, the bound of tests/test_edge_weight_cpu.py (both sides are float64).  The longest rows need
    more, and it is the reference's: it divides every weight by max(m, tau) first and runs one sequential cumulative sum over the
    D + 1 elements, every step rounding by up to 2^-53 of a running sum <= 1, so its cumulative weights carry up to (D + 2) 2^-53, and
    h = 2 (1 + xi) cos(2 pi xi c) feels that times 2 pi |xi| (the derivation of LO_BOUND in tests/test_edge_weight_long_cpu.py; the
    form under test sums the raw weights, multiples of 1/4, exactly).  Per row: max(1e-12, (D + 2) 2^-53 2 pi max |xi|) -- 1.0e-10 for
    the row of 32769 at max |xi| = 4.5, 1e-12 up to 3183 neighbours.
    Measured (per entry and slice / row maximum, the row closest to its bound): tau 1 distinct 6.3e-12 (D = 32768, allowed
    1.0e-10), tied 6.7e-13 (2049, allowed 6.4e-12); tau 3 distinct 4.2e-13 (4097, allowed 1.3e-11), tied 6.7e-12 (32768); the rows
    up to 2049 stand at 9.5e-14 .. 6.7e-13, inside 1e-12.  The grouped values (G = 4) against the reference's sums over the group
    (allowed G times as much): 8.3e-12 at most.  (M = 32, chunks of 2048, gave the same figures within 2 % when it was tried.)
(b) The condition of the GPU test of w_lo: with weights w + w_lo (float64) as the truth, the same form evaluated on w alone misses
    the GPU test's per-entry bound (with ceil(S / G) float32 adds) on at least one entry of EVERY row above 1024 neighbours, for
    every S of that test -- a kernel that dropped w_lo on any of these rows would fail there.
    Measured: the smallest over the rows of the largest err / bound per row is 77 (tau 3, distinct keys, S = 70, the row of 4097;
    4170 and more at S = 3 and 8); the form on w + w_lo stands at 7.1e-12 of the row maximum against its reference.
(c) fsw_embed_backward_w_long_slices is declared, bound and exported and returns G >= 1; the ABI version (6), the tuned limit (1024)
    and the scratch query are unchanged; 20 bytes per element of the largest padded line fit the query's result for one row and for
    the case's row count.  Fails on the parent commit: the symbol is missing.
"""
import os
import re

import numpy as np
import pytest

from tests import edge_weight_hub_cases as HC
from tests.test_edge_weight_cpu import BOUND
from tests.test_edge_weight_long_cpu import block_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_SCALE = 0.7
GROUP = 4                                                                     # the accumulator of (a); (c) pins the library's G


@pytest.fixture(scope="module", autouse=True)
def release_the_cached_cases():
    """The inputs and references of this module (some 200 MB of float64 arrays) are not kept for the rest of the session."""
    yield
    HC.base_reference.cache_clear()
    HC.kernel_inputs.cache_clear()


def row_bounds(deg):
    """(a) of the module docstring, per row."""
    xi = np.abs(HC.base_freqs().astype(np.float64)).max()
    return np.maximum(BOUND, (deg + 2) * 2.0 ** -53 * 2 * np.pi * xi)


def test_the_inputs_cover_every_bin_level_and_kind():
    deg = np.array(HC.DEGREES)
    assert deg.sum() < 150000 and HC.DEGREES[HC.ZERO_ROW] > HC.TUNED_MAX and tuple(sorted(HC.DEGREES)) == HC.DEGREES
    for edge in (1024, 2048, 4096, 8192, 16384, 32768):                       # both sides of the hand-over and of every bin edge
        assert edge in HC.DEGREES and edge + 1 in HC.DEGREES
    for M in (16, 32):                                                        # D + 1 at one chunk, two chunks, every power of two
        assert {HC.pow2ceil(d + 1) // (64 * M) for d in deg if d > HC.TUNED_MAX} >= {2 ** i for i in range(1, 6)}
        assert any((d + 1) % (64 * M) not in (0, 1) and d + 1 > 2 * 64 * M for d in deg)      # a partly filled last chunk
    assert 2047 in HC.DEGREES and 4095 in HC.DEGREES                          # D + 1 fills its chunks exactly
    assert min(HC.S_VALUES) < GROUP and max(HC.S_VALUES) % GROUP and -(-max(HC.S_VALUES) // GROUP) >= 2
    for tau in (1.0, 3.0):
        k = HC.kernel_inputs(tau, True)
        long_kinds = {kind for kind, d in zip(k["kinds"], deg) if d > HC.TUNED_MAX}
        assert long_kinds == {"lt", "eq", "gt"} and (k["w"] == 0).sum() > 1000 and (k["K"] == 0).any() and (k["w_lo"] < 0).any()
        assert not k["G"][HC.ZERO_ROW].any() and (k["G"][:, 1:] == 0).sum() > HC.BASE


@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_chunked_form_against_the_autograd_reference(tau, tied):
    """(a) of the module docstring."""
    k = HC.kernel_inputs(tau, tied)
    rowptr, deg = k["rowptr"], k["degrees"]
    ref = HC.base_reference(tau, tied, OUT_SCALE)
    G = OUT_SCALE * k["G"][:, 1:].astype(np.float64)
    long_rows = deg > HC.TUNED_MAX
    bound = row_bounds(deg)
    assert np.abs(ref["gW_s"]).max() > 0.1
    for M in (HC.RANKS,):
        got = HC.chunked_weight_grad(rowptr, k["w"], k["K"], HC.base_freqs(), tau, G, M=M)
        ratio = block_ratio(got, ref["gW_s"], rowptr)
        worst = int(np.where(long_rows, ratio / bound, 0.0).argmax())
        print("tau %g %s M %d: chunked form against gW_s, per entry and slice / row maximum: %.2e (D = %d, %s, allowed %.2e); rows <= 2049: %.2e"
              % (tau, "tied" if tied else "distinct", M, ratio[worst], deg[worst], k["kinds"][worst], bound[worst],
                 ratio[long_rows & (deg <= 2049)].max()))
        assert (ratio[long_rows] <= bound[long_rows]).all(), (M, int(deg[worst]), k["kinds"][worst], float(ratio[worst]))
        zr = slice(rowptr[HC.ZERO_ROW], rowptr[HC.ZERO_ROW + 1])
        assert not got[zr].any() and not ref["gW_s"][zr].any()
    # the float64 accumulator over a group of slices: acc[j] + Ksum against the reference's sum over the group
    grouped = HC.chunked_weight_grad(rowptr, k["w"], k["K"], HC.base_freqs(), tau, G, group=GROUP)
    ntask = -(-HC.BASE // GROUP)
    want = np.stack([ref["gW_s"][:, g * GROUP:(g + 1) * GROUP].sum(axis=1) for g in range(ntask)], axis=1)
    ratio = block_ratio(grouped, want, rowptr)
    print("tau %g %s: grouped values (G = %d) against the reference's sums: %.2e" % (tau, "tied" if tied else "distinct", GROUP,
                                                                                     ratio[long_rows].max()))
    assert grouped.shape == (k["w"].size, ntask) and (ratio[long_rows] <= GROUP * bound[long_rows]).all()


@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("tau", [1.0, 3.0])
def test_dropping_w_lo_exceeds_the_gpu_bound_on_every_hub_row(tau, tied):
    """(b) of the module docstring."""
    k = HC.kernel_inputs(tau, tied)
    rowptr, deg = k["rowptr"], k["degrees"]
    G = OUT_SCALE * k["G"][:, 1:].astype(np.float64)
    dropped_base = HC.chunked_weight_grad(rowptr, k["w"], k["K"], HC.base_freqs(), tau, G)
    kept_base = HC.chunked_weight_grad(rowptr, k["w64"], k["K"], HC.base_freqs(), tau, G)
    ref_base = HC.base_reference(tau, tied, OUT_SCALE, lo=True)["gW_s"]
    long_rows = deg > HC.TUNED_MAX
    kept = block_ratio(kept_base, ref_base, rowptr)
    print("tau %g %s: chunked form on w + w_lo against its reference: %.2e of the row maximum" % (tau, "tied" if tied else "distinct",
                                                                                                 kept[long_rows].max()))
    assert (kept[long_rows] <= row_bounds(deg)[long_rows]).all()                   # the form itself follows w + w_lo
    for S in HC.S_VALUES:
        ref = HC.reference(tau, tied, OUT_SCALE, S, lo=True)
        sel, sg = np.arange(S) % HC.BASE, HC.sigma(S)
        dropped = (dropped_base[:, sel] * sg[None, :]).sum(axis=1)
        adds = np.repeat([HC.float32_adds(int(d), S) for d in deg], deg)
        bound = HC.gw_bound(ref, rowptr, S, adds)
        ratio = np.abs(dropped - ref["gW"]) / np.where(bound > 0, bound, 1.0)
        per_row = np.array([ratio[a:b].max() if b > a else 0.0 for a, b in zip(rowptr[:-1], rowptr[1:])])
        sensitive = long_rows & (np.arange(deg.size) != HC.ZERO_ROW)               # the zero row has no gradient to lose
        worst = int(np.where(sensitive, per_row, np.inf).argmin())
        print("tau %g %s S %d: w_lo dropped, smallest over the hub rows of the largest err / bound: %.1f (D = %d)" % (
            tau, "tied" if tied else "distinct", S, per_row[worst], deg[worst]))
        assert per_row[sensitive].min() > 1.0, (S, int(deg[worst]), float(per_row[worst]))


def test_long_slices_is_declared_bound_and_exported_and_the_rest_is_unchanged():
    """(c) of the module docstring."""
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert re.search(r"#define\s+FSW_ABI_VERSION\s+6\b", header) and _lib.FSW_ABI_VERSION == 6
    assert re.search(r"\bint\s+fsw_embed_backward_w_long_slices\s*\(\s*void\s*\)", header)
    assert "fsw_embed_backward_w_long_slices" in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["fsw_embed_backward_w_long_slices"] == (_lib.ctypes.c_int, [])
    L = _lib.lib()
    G = L.fsw_embed_backward_w_long_slices()
    assert G >= 1 and G == HC.slices_per_task()
    assert max(HC.S_VALUES) > G, "add an S that gives at least two groups"
    assert HC.float32_adds(1024, 70) == 4 and HC.float32_adds(1025, 70) == -(-70 // G) and HC.float32_adds(32769, 3) == -(-3 // G)
    assert L.fsw_abi_version() == 6 and L.fsw_embed_backward_w_tuned_max_degree() == HC.TUNED_MAX == 1024
    for maxdeg in (24, 25, 300, 1024, 1025, 5000, 32769):                          # the query is unchanged
        want = 0 if maxdeg <= 24 else L.fsw_embed_generic_scratch_bytes(maxdeg, 100)
        assert L.fsw_embed_backward_w_scratch_bytes(maxdeg, 100) == want and (maxdeg <= 24 or want > 0)
    line = HC.BYTES_PER_ELEM * HC.pow2ceil(max(HC.DEGREES) + 1)                    # one wavefront's line of the largest bin
    assert line == 20 * 65536
    for rows in (1, len(HC.DEGREES)):
        assert L.fsw_embed_backward_w_scratch_bytes(max(HC.DEGREES), rows) >= line
    for maxdeg in (1025, 2048, 2049, 41300, 1 << 20):                              # whatever the graph: 36 bytes per element, one line at least
        assert L.fsw_embed_backward_w_scratch_bytes(maxdeg, 1) >= HC.BYTES_PER_ELEM * HC.pow2ceil(maxdeg + 1)
