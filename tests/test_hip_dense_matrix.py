"""The dense matrix kernels, called through the C ABI and checked per entry (tests/dense_matrix_cases.py holds the cases, the float64
references, the bounds and the check functions):
  1. fsw_gemm_tn_f32 (csrc/gemm_tn.hip), bf16 x 3: integer inputs (exact, every k split and block count), probe rows (exact, all 24
     significand bits, the edges of the workgroups' k ranges), random inputs within the derived bound, beta and ldc, the workspace,
     the refusals, power-of-two scaling, non-finite input, the Python wrapper gemm_tn();
  2. the generic fp32 projection kernel k_project (csrc/project.hip) and fsw_project_f64 (csrc/embed_generic.hip);
  3. the kernels behind FSW_GEMM_TN_EXACT_FP32=1 and FSW_PROJECT_EXACT_FP32=1 (k_gemm_tn_partial, k_project_bs) in a child process
     of their own: both switches are read once per process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dense_matrix_cases as D
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
PLANES = 6                 # the default number format: six products of bf16 planes


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert not os.environ.get("FSW_GEMM_TN_EXACT_FP32") and not os.environ.get("FSW_PROJECT_EXACT_FP32"), \
        "run this file without FSW_GEMM_TN_EXACT_FP32 / FSW_PROJECT_EXACT_FP32: it checks the bf16 x 3 kernels in this process"
    return torch.device("cuda:0")


# ---- 1. fsw_gemm_tn_f32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", D.TN_INT_CASES)
def test_gemm_tn_integer_inputs_exact(dev, K, M, N):
    """(a) K on both sides of one k step (16), of one split piece (512) and of the grid sizes 1 -> 2 (1024) and 8 (4097), G = 128 and
    512, K = 262 145 (pieces of 528 rows, 15 workgroups without rows); 1 .. 16 blocks of 64 x 64, 8 | 9 blocks = one | two per
    wavefront.  A row dropped, read twice or given to the wrong workgroup, or a wrong C/D map, is an exact mismatch."""
    D.check_tn_integer(dev, K, M, N)


def test_gemm_tn_k_ranges():
    """The k split that the probe rows rely on, at the values worked out by hand from csrc/gemm_tn.hip."""
    assert [D.tn_grid(K) for K in (1, 511, 1023, 1024, 1025, 4097, 65_537, 262_144, 262_145)] == [1, 1, 1, 2, 2, 8, 128, 512, 512]
    assert D.tn_ranges(1025) == [(0, 528), (528, 1025)] and D.tn_ranges(1024) == [(0, 512), (512, 1024)]
    assert D.tn_ranges(4097)[-1] == (3696, 4097) and D.tn_piece(4097) == 528
    assert D.tn_piece(262_144) == 512 and D.tn_piece(262_145) == 528 and D.tn_ranges(262_145)[497] == (262_145, 262_145)
    # the exact-fp32 form (k_gemm_tn_partial): per = (ceil(K / G) + 1) & ~1
    assert D.tn_piece(1025, planes=1) == 514 and D.tn_piece(262_145, planes=1) == 514 and D.tn_piece(1024, planes=1) == 512
    assert D.tn_ranges(1025, planes=1) == [(0, 514), (514, 1025)]
    assert D.tn_piece(4097, planes=1) == 514 and D.tn_ranges(4097, planes=1)[6:] == [(3084, 3598), (3598, 4097)]
    assert D.tn_ranges(262_145, planes=1)[509:] == [(261_626, 262_140), (262_140, 262_145), (262_145, 262_145)]
    assert [D.tn_blocks(M, N) for M, N in ((512, 64), (513, 64), (256, 256), (128, 385), (1025, 64), (257, 256), (65, 1024))] == [8, 9, 16, 14, 17, 20, 32]


@pytest.mark.parametrize("exchanged", [False, True])
@pytest.mark.parametrize("K,M,N", D.TN_PROBE_CASES)
def test_gemm_tn_probe_rows_exact(dev, K, M, N, exchanged):
    """(b) the rule of test_project_linear_exact_cases: one-hot probe rows times full 24-bit significands come back bit for bit.
    1024 probes at K = 4097 (8 ranges of 528 rows), 33 at K = 262 145, where the last range that has rows is partly filled."""
    assert D.check_tn_probes(dev, K, M, N, exchanged) == M


def test_gemm_tn_plane_product_exact(dev):
    D.check_tn_plane_product(dev)


@pytest.mark.parametrize("K,M,N", D.TN_RANDOM_CASES)
def test_gemm_tn_random_per_entry(dev, K, M, N):
    """(c) standard normal inputs: every entry within dense_matrix_cases.tn_bound of the float64 product."""
    D.check_tn_random(dev, K, M, N, PLANES)


@pytest.mark.parametrize("beta", D.TN_BETAS)
def test_gemm_tn_beta_and_ldc(dev, beta):
    """(d) C == beta C0 + A^T B: exact on the integer case, within the bound on the random one; with beta = 0 the NaN that C holds
    is not read.  ldc = N + 3 in every call of this file, the padding must stay NaN."""
    D.check_tn_integer(dev, *D.TN_BETA_INT_CASE, beta=beta)
    D.check_tn_random(dev, *D.TN_BETA_RANDOM_CASE, PLANES, beta=beta)


@pytest.mark.parametrize("K,M,N", D.TN_WORKSPACE_CASES)
def test_gemm_tn_workspace(dev, K, M, N):
    """(e)"""
    D.check_tn_workspace(dev, K, M, N, PLANES)


@pytest.mark.parametrize("name", list(D.TN_REFUSALS))
def test_gemm_tn_refusals(dev, name):
    """(f) non-zero status, a message, C untouched."""
    D.check_tn_refusal(dev, name)


def test_gemm_tn_power_of_two_scaling(dev):
    """(g)"""
    D.check_tn_scaling(dev)


def test_gemm_tn_nonfinite_input(dev):
    """(h)"""
    D.check_tn_nonfinite(dev, PLANES)


@pytest.fixture()
def kernel_calls(monkeypatch):
    """Counts the calls of fsw_gemm_tn_f32 that gemm_tn() makes."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    real, calls = L.fsw_gemm_tn_f32, []

    def counted(*args):
        calls.append(args[4:7])
        return real(*args)

    monkeypatch.setattr(L, "fsw_gemm_tn_f32", counted)
    return calls


@pytest.mark.parametrize("why", ["few rows", "B strided", "20 blocks"])
def test_gemm_tn_wrapper_falls_back(dev, kernel_calls, why):
    """(i) K below GEMM_TN_MIN_ROWS, a B with stride(1) != 1 and more than 16 blocks take the BLAS product, which lies within the
    bound of the kernel."""
    from fsw_gnn_amd.fsw_embedding import GEMM_TN_MIN_ROWS, gemm_tn
    K, M, N = {"few rows": (GEMM_TN_MIN_ROWS - 1, 40, 17), "B strided": (GEMM_TN_MIN_ROWS, 40, 17), "20 blocks": (GEMM_TN_MIN_ROWS, 257, 256)}[why]
    A, B, _ = D.tn_random_inputs(K, M, N)
    Ad = D.t(A, dev)
    Bd = D.t(B.T, dev).t() if why == "B strided" else D.t(B, dev)
    assert (Bd.stride(1) != 1) == (why == "B strided") and tuple(Bd.shape) == (K, N)
    C = gemm_tn(Ad, Bd).cpu().numpy()
    assert kernel_calls == []
    D.check_tn_entries(C, A, B, PLANES, what="wrapper, " + why, normwise=False)


def test_gemm_tn_wrapper_strided_a(dev, kernel_calls):
    """(i) A with stride(0) > M at K >= 65 536 takes the kernel; bitwise reproducible."""
    from fsw_gnn_amd.fsw_embedding import GEMM_TN_MIN_ROWS, gemm_tn
    K, M, N = GEMM_TN_MIN_ROWS, 40, 17
    A, B, _ = D.tn_random_inputs(K, M, N)
    Ad, Bd = D.t(D.padded(A, 7), dev)[:, :M], D.t(B, dev)
    assert Ad.stride(0) == M + 7
    C = gemm_tn(Ad, Bd)
    assert kernel_calls == [(K, M, N)]
    D.check_tn_entries(C.cpu().numpy(), A, B, PLANES, what="wrapper, A strided")
    assert torch.equal(C, gemm_tn(Ad, Bd))


# ---- 2. k_project, fsw_project_f64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,S,H2,mapped,with_b2,with_copy,form", D.GENERIC_CASES)
def test_project_generic_kernel(dev, n, d, S, H2, mapped, with_b2, with_copy, form):
    """The rules of test_project_linear_random_cases on the shapes that only k_project serves: d % 4 != 0, d > 256, rows that are not
    16-byte aligned.  This kernel writes nothing from column S on."""
    D.check_project_generic(dev, n, d, S, H2, mapped, with_b2, with_copy, form)


@pytest.mark.parametrize("case", [2, 4, 6, 8])
def test_project_generic_nonfinite_flag(dev, case):
    """An Inf in the last row and last k column -- one entry, staged by one thread in the last k step -- raises the flag."""
    n, d = D.GENERIC_CASES[case][:2]
    assert D.check_project_generic(dev, *D.GENERIC_CASES[case], bad=(n - 1, d - 1)) & D.FLAG_X_NONFINITE


@pytest.mark.parametrize("d", D.F64_D)
def test_project_f64_per_entry(dev, d):
    """fsw_project_f64 at every n and S around its 16 x 16 tile and its four tiles per workgroup."""
    worst = max(D.check_project_f64(dev, n, d, S) for n in D.F64_N for S in D.F64_S)
    print("project_f64 d %d: largest |err| / bound %.4f" % (d, worst))


def test_project_f64_integer_inputs_exact_and_flag(dev):
    rng = np.random.default_rng(11)
    n, d, S = 65, 13, 33
    X, V = rng.integers(-1000, 1001, (n, d)).astype(np.float64), rng.integers(-1000, 1001, (S, d)).astype(np.float64)
    Xp, flags = D.run_project_f64(dev, X, V)
    assert flags == 0 and np.array_equal(Xp, X @ V.T)
    for bad in (np.inf, np.nan):
        X2 = X.copy()
        X2[n - 1, d - 1] = bad
        Xp2, flags = D.run_project_f64(dev, X2, V)
        assert flags & D.FLAG_X_NONFINITE
        assert np.array_equal(Xp2[:n - 1], Xp[:n - 1]) and not np.isfinite(Xp2[n - 1]).any()


# ---- 3. the exact-fp32 kernels --------------------------------------------------------------------------------------------------------
def test_exact_fp32_kernels_in_a_child_process(dev, tmp_path):
    """One child with both switches set runs parts 1 (a) - (e), (g), (h) -- the probe rows of (b) on the fp32 form's own k
    ranges, pieces of 514 rows at K = 4097 and 262 145 -- and the k_project_bs cases of dense_matrix_cases.main
    with the bounds of one fp32 chain.  Its marker outputs differ in their bits from what this process's bf16 x 3 kernels give on
    the same inputs (the switches took effect), and the d = 192 case, which the projection switch does not cover, does not."""
    out = tmp_path / "markers.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("FSW_GEMM_TN_EXACT_FP32", "FSW_PROJECT_EXACT_FP32")}
    env.update(FSW_GEMM_TN_EXACT_FP32="1", FSW_PROJECT_EXACT_FP32="1")
    r = subprocess.run([sys.executable, "-m", "tests.dense_matrix_cases", str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "exact-fp32 checks done" in r.stdout
    child = np.load(out)
    mine = D.marker_outputs(dev, PLANES)
    assert set(child.files) == set(mine)
    for name in ("gemm", "project_xp", "project_y2"):
        assert child[name].shape == mine[name].shape
        assert not np.array_equal(D.bits(child[name]), D.bits(mine[name])), name + ": the switch changed nothing"
    for name in ("wide_xp", "wide_y2"):
        assert np.array_equal(child[name].view(np.uint32), mine[name].view(np.uint32)), name + ": the switch reaches d > 128"
