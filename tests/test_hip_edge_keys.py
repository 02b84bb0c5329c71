"""fsw_edge_keys_f32 (csrc/edge_keys.hip) alone: K[e, s] = Xp[col[e], s], then fmaf(ef[e, q], Ve[s, q], key) for q = 0 .. d_edge - 1.

Exact cases.  On the dyadic grids of tests/edge_feature_cases.py (Xp multiples of 2^-6 up to 512, ef multiples of 1/4 in [-2, 2], Ve
multiples of 1/8 in [-1, 1], d_edge <= 5) nothing rounds, so EC.keys_float32 describes the kernel bit for bit, in either order of q
(asserted: reverse=True gives the same array).  Shapes: nnz 1 / 63 / 64 / 65 / 1000 (one entry, both sides of a wavefront, several
workgroups' worth of groups), S 1 / 3 / 13 / 64 / 65 (one lane, partial groups, a whole wavefront per entry, the loop over s), d_edge
1 / 5; a random col with repeats, ldp > S, ldk > S with the pad columns of K pre-filled and required untouched, Ve read in place from
a [S, d_in + d_edge] matrix.  S = 64 with 16-byte strides takes the four-floats-per-lane kernel, S = 64 at an odd stride and every other
S the one-float kernel; S * d_edge > 8192 reads Ve from global memory instead of LDS.

One inexact case: d_edge = 33, random floats, S = 7, against float64 within d_edge 2^-24 (|Xp| + sum_q |ef Ve|) per entry: each of the
d_edge fused multiply-adds rounds once, by at most 2^-24 of its result, and every partial result is at most |Xp| + sum_q |ef Ve| in
size (up to the factor (1 + 2^-24)^33 - 1 = 2e-6 of earlier roundings, which only a chain whose every step rounds by a full half
ulp of that largest possible value could use).  Derived, not measured; the kernel's largest error on an MI355X is 0.12 of it."""
import numpy as np
import pytest
import torch

from tests import edge_feature_cases as EC

pytestmark = pytest.mark.gpu

D_IN = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def run_kernel(dev, col, Xp, ef, Vfull, d_in, S, ldk, fill=np.nan):
    """K [nnz, ldk] (pre-filled with `fill`) from Xp [n, ldp], ef [nnz, d_edge] and Ve = Vfull[:, d_in:] read in place."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    nnz, d_edge = ef.shape
    Xp_d, ef_d, V_d, col_d = t(Xp, dev), t(ef, dev), t(Vfull, dev), t(col, dev, torch.int32)
    K = torch.full((nnz, ldk), fill, dtype=torch.float32, device=dev)
    rc = L.fsw_edge_keys_f32(_lib.ptr(col_d), nnz, _lib.ptr(Xp_d), Xp_d.stride(0), _lib.ptr(ef_d), d_edge, V_d.data_ptr() + 4 * d_in,
                             V_d.stride(0), S, _lib.ptr(K), ldk, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "fsw_edge_keys_f32")
    torch.cuda.synchronize()
    return K.cpu().numpy()


def exact_inputs(nnz, S, d_edge, n, seed):
    rng = np.random.default_rng(seed)
    col = rng.integers(0, n, size=nnz)                               # not the identity; repeats as soon as nnz > n
    xp = (rng.integers(-512 * 64, 512 * 64 + 1, size=(n, S)) * EC.XP_STEP).astype(np.float32)
    ef = (rng.integers(-8, 9, size=(nnz, d_edge)) / 4.0).astype(np.float32)
    Ve = EC.slice_vectors(S, d_edge, seed=seed + 1)
    return col, xp, ef, Ve


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("d_edge", [1, 5])
@pytest.mark.parametrize("S", [1, 3, 13, 64, 65])
@pytest.mark.parametrize("nnz", [1, 63, 64, 65, 1000])
def test_exact_keys_bit_for_bit(dev, nnz, S, d_edge):
    n = max(1, nnz // 2)                                             # every sender about twice
    col, xp, ef, Ve = exact_inputs(nnz, S, d_edge, n, seed=1000 * d_edge + 10 * S + nnz % 7)
    want = EC.keys_float32(xp[col], ef, Ve)
    assert np.array_equal(bits(want), bits(EC.keys_float32(xp[col], ef, Ve, reverse=True)))
    Vfull = np.full((S, D_IN + d_edge), np.nan, dtype=np.float32)    # the columns of X in front of Ve are never read
    Vfull[:, D_IN:] = Ve
    # ldp > S, ldk > S: a 16-byte stride (the four-float kernel when S % 4 == 0) and an odd one
    for ldp, ldk in ((S + 4 - S % 4, S + 8 - S % 4), (S + 3, S + 1)):
        Xp = np.full((n, ldp), np.nan, dtype=np.float32)
        Xp[:, :S] = xp
        K = run_kernel(dev, col, Xp, ef, Vfull, D_IN, S, ldk, fill=-7.5)
        assert np.array_equal(bits(K[:, :S]), bits(want)), (nnz, S, d_edge, ldp, ldk)
        assert (K[:, S:] == -7.5).all(), "pad columns of K were written"


def test_contiguous_rows_and_identity_col(dev):
    """ldp == ldk == S (the module's layout for S % 4 == 0) with the identity as col."""
    nnz, S, d_edge = 777, 16, 4
    _, xp, ef, Ve = exact_inputs(nnz, S, d_edge, nnz, seed=5)
    K = run_kernel(dev, np.arange(nnz), xp, ef, Ve, 0, S, S)
    assert np.array_equal(bits(K), bits(EC.keys_float32(xp, ef, Ve)))


@pytest.mark.parametrize("S,d_edge", [(2052, 4), (1643, 5)])
def test_ve_from_global_memory(dev, S, d_edge):
    """S * d_edge above the LDS stage (8192 floats): Ve is read in place, by the four-float kernel (S % 4 == 0) and the one-float one."""
    nnz = 70
    col, xp, ef, Ve = exact_inputs(nnz, S, d_edge, 31, seed=9)
    assert S * d_edge > 8192
    ld = S + (4 - S % 4) % 4
    Xp = np.zeros((31, ld), dtype=np.float32)
    Xp[:, :S] = xp
    K = run_kernel(dev, col, Xp, ef, Ve, 0, S, ld, fill=3.25)
    assert np.array_equal(bits(K[:, :S]), bits(EC.keys_float32(xp[col], ef, Ve))) and (K[:, S:] == 3.25).all()


def test_inexact_chain_within_its_rounding_bound(dev):
    nnz, S, d_edge, n = 500, 7, 33, 200
    rng = np.random.default_rng(77)
    col = rng.integers(0, n, size=nnz)
    xp = rng.standard_normal((n, S)).astype(np.float32)
    ef = rng.standard_normal((nnz, d_edge)).astype(np.float32)
    Ve = rng.standard_normal((S, d_edge)).astype(np.float32)
    K = run_kernel(dev, col, xp, ef, Ve, 0, S, S + 1)[:, :S].astype(np.float64)
    ef64, Ve64, x64 = ef.astype(np.float64), Ve.astype(np.float64), xp[col].astype(np.float64)
    want = x64 + ef64 @ Ve64.T
    bound = d_edge * 2.0 ** -24 * (np.abs(x64) + np.abs(ef64) @ np.abs(Ve64).T)
    ratio = np.abs(K - want) / bound
    print("d_edge 33: largest |K - float64| / bound %.3f" % ratio.max())
    assert np.isfinite(K).all() and ratio.max() <= 1.0
