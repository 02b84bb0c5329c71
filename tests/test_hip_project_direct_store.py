"""fsw_project_linear_f32 and fsw_project_f32 at the shapes where storing C straight from the transposed accumulators
(csrc/project.hip: k_project_bf3, k_project_narrow) can go wrong, with the rules of
tests/test_hip_conv_fused.py::test_project_linear_random_cases: outputs pre-filled with NaN, every entry within
conv_fused_ref.project_bound of the float64 product, the columns S .. slab_end of Xp hold 0.0 or NaN only, everything from
slab_end on and the padding of Y2 keep their NaN, and every Y2 row is written exactly once, where row_map says.

The shapes: workgroups that run three or four tiles (A-buffer parity, the look-ahead of the per-lane row map) with a partial
last tile, on the straight-line store path and on the general one; 1, 31 and 33 rows; slab counts and widths at the column
edges, with 16-byte aligned and unaligned Y2 rows; the d <= 256 kernel (which keeps its staging tile); the wavefront-per-tile
kernel with one and with several tiles per wavefront, with aligned and unaligned Xp rows; x_copy; a non-finite entry of X."""
import numpy as np
import pytest
import torch

from tests import conv_fused_ref as R
from tests.conftest import relerr
from tests.test_hip_conv_fused import TOL, last_error, run_project_linear, stream_of, t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def check_project_linear(dev, n, d, S, H2, mapped, with_b2, aligned, seed=0):
    rng = np.random.default_rng(seed + n + 7 * d + 11 * S + 13 * H2)
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = (rng.standard_normal((S, d)) / np.sqrt(d)).astype(np.float32)
    W2 = (rng.standard_normal((H2, d)) / np.sqrt(d)).astype(np.float32)
    b2 = rng.standard_normal(H2).astype(np.float32) if with_b2 else None
    row_map = rng.permutation(n).astype(np.int32) if mapped else None
    slab_end = 32 * ((S + 31) // 32)
    ldp = slab_end + 4
    ldy2 = 4 * ((H2 + 3) // 4) if aligned else H2 + 3
    Xp, Y2, flags = run_project_linear(dev, X, V, S, W2, b2, row_map, ldp, ldy2)
    assert flags == 0
    X64 = X.astype(np.float64)
    ref1, bound1 = X64 @ V.astype(np.float64).T, R.project_bound(X, V)
    ref2 = X64 @ W2.astype(np.float64).T + (b2.astype(np.float64) if with_b2 else 0.0)
    bound2 = R.project_bound(X, W2, b2)
    assert np.isfinite(Xp[:, :S]).all() and np.isfinite(Y2[:, :H2]).all()
    pad = Xp[:, S:slab_end]
    assert (np.isnan(pad) | (pad == 0.0)).all()
    assert np.isnan(Xp[:, slab_end:]).all() and np.isnan(Y2[:, H2:]).all()
    got2 = Y2[row_map, :H2] if mapped else Y2[:, :H2]
    e1, e2 = np.abs(Xp[:, :S] - ref1), np.abs(got2 - ref2)
    print("n %d d %d S %d H2 %d ldy2 %d: largest |err| / bound: Xp %.3f, Y2 %.3f"
          % (n, d, S, H2, ldy2, (e1 / bound1).max(), (e2 / bound2).max()))
    assert (e1 <= bound1).all(), ("Xp", np.unravel_index((e1 / bound1).argmax(), e1.shape))
    assert (e2 <= bound2).all(), ("Y2", np.unravel_index((e2 / bound2).argmax(), e2.shape))
    assert relerr(Xp[:, :S], ref1) < TOL and relerr(got2, ref2) < TOL
    return X, V, W2, b2, row_map, ldp, ldy2


@pytest.mark.parametrize("S,H2", [(256, 128), (64, 100)])
def test_tile_loop(dev, S, H2):
    """24 743 rows, the last tile has 7.  S = 256, H2 = 128: 773 whole tiles over 256 workgroups, three or four each, on the
    straight-line store path, and the last 7 rows in a launch of the general kernel.  S = 64, H2 = 100 (six slab wavefronts and
    two that only move X, a partial last Y2 slab): all 774 tiles in the general kernel."""
    check_project_linear(dev, 3 * 8192 + 167, 128, S, H2, True, True, True)


@pytest.mark.parametrize("n", [1, 31, 33])
def test_row_edges(dev, n):
    check_project_linear(dev, n, 128, 256, 128, True, True, True)


@pytest.mark.parametrize("S", [1, 33, 65, 257])
def test_slice_column_edges(dev, S):
    """ldp = 32 ceil(S / 32) + 4; S = 257 with H2 = 128 is 13 slabs = two column groups of seven wavefronts."""
    check_project_linear(dev, 65, 128, S, 128, True, True, True)


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("H2", [1, 30, 33])
def test_second_block_column_edges(dev, H2, aligned):
    """ldy2 = H2 + 3 (rows not 16-byte aligned: scalar stores) and ldy2 rounded up to 4 (16-byte stores, scalar in the last quad)."""
    check_project_linear(dev, 65, 128, 256, H2, True, True, aligned)
    check_project_linear(dev, 33, 128, 256, H2, False, False, aligned, seed=1)


@pytest.mark.parametrize("d", [192, 256])
def test_wide_rows_template(dev, d):
    """d <= 256 (k_project_bf3_staged): four slab wavefronts per workgroup, 7 slabs in two column groups; 258 tiles over 256
    workgroups."""
    check_project_linear(dev, 8192 + 45, d, 64, 160, True, True, True)


def run_project(dev, X, V, ldp, with_copy=False):
    """fsw_project_f32 on host arrays: (Xp [n, ldp], x_copy [n, d + 4] or None, flags), outputs pre-filled with NaN."""
    from fsw_gnn_amd import _lib
    L = _lib.lib()
    n, d = X.shape
    S = V.shape[0]
    Xd = t(np.concatenate([X, np.full((n, 4), 333.0, dtype=np.float32)], axis=1), dev)
    Vd = t(np.concatenate([V, np.full((S, 4), 333.0, dtype=np.float32)], axis=1), dev)
    Xp = torch.full((n, ldp), float("nan"), device=dev)
    xc = torch.full((n, d + 4), float("nan"), device=dev) if with_copy else None
    stats = torch.zeros(_lib.NUM_STATS, dtype=torch.int32, device=dev)
    rc = L.fsw_project_f32(_lib.ptr(Xd), n, d, Xd.stride(0), _lib.ptr(Vd), S, Vd.stride(0), _lib.ptr(Xp), ldp, _lib.ptr(xc),
                           d + 4 if with_copy else 0, _lib.ptr(stats), stream_of(dev))
    assert rc == 0, last_error()
    return Xp.cpu().numpy(), xc.cpu().numpy() if with_copy else None, int(stats.cpu()[_lib.STAT_FLAGS])


def check_project(Xp, X, V, slab_end):
    S = V.shape[0]
    ref, bound = X.astype(np.float64) @ V.astype(np.float64).T, R.project_bound(X, V)
    assert np.isfinite(Xp[:, :S]).all()
    pad = Xp[:, S:slab_end]
    assert (np.isnan(pad) | (pad == 0.0)).all()
    assert np.isnan(Xp[:, slab_end:]).all()
    e = np.abs(Xp[:, :S] - ref)
    print("n %d d %d S %d: largest |err| / bound %.3f" % (X.shape[0], X.shape[1], S, (e / bound).max()))
    assert (e <= bound).all(), np.unravel_index((e / bound).argmax(), e.shape)
    assert relerr(Xp[:, :S], ref) < TOL


@pytest.mark.parametrize("n", [33, 4 * 512 * 32 + 5])
@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("S", [16, 64])
def test_narrow_kernel(dev, S, d, n):
    """The wavefront-per-tile kernel (S <= 64, no second block, no copy): 65 541 rows = 2049 tiles over 2048 wavefronts, so
    one wavefront runs a second, partial tile.  At 33 rows also with rows of Xp that are not 16-byte aligned (scalar stores)."""
    rng = np.random.default_rng(n + 7 * d + 11 * S)
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = (rng.standard_normal((S, d)) / np.sqrt(d)).astype(np.float32)
    slab_end = 32 * ((S + 31) // 32)
    for ldp in [slab_end + 4] + ([slab_end + 3] if n == 33 else []):
        Xp, _, flags = run_project(dev, X, V, ldp)
        assert flags == 0
        check_project(Xp, X, V, slab_end)


def test_x_copy_is_bit_exact(dev):
    """Without linear2 the kernel also writes a copy of X: bit for bit, its padding untouched."""
    rng = np.random.default_rng(5)
    n, d, S = 8192 + 45, 128, 256
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[3, 5], X[n - 1, d - 1] = -0.0, np.float32(1e-42)
    V = (rng.standard_normal((S, d)) / np.sqrt(d)).astype(np.float32)
    Xp, xc, flags = run_project(dev, X, V, S + 4, with_copy=True)
    assert flags == 0
    check_project(Xp, X, V, S)
    assert np.array_equal(xc[:, :d].view(np.uint32), X.view(np.uint32))
    assert np.isnan(xc[:, d:]).all()


def test_nonfinite_input_sets_the_flag(dev):
    from fsw_gnn_amd import _lib
    rng = np.random.default_rng(6)
    n, d = 8192 + 45, 128
    X = rng.standard_normal((n, d)).astype(np.float32)
    V = (rng.standard_normal((256, d)) / np.sqrt(d)).astype(np.float32)
    W2 = (rng.standard_normal((128, d)) / np.sqrt(d)).astype(np.float32)
    for bad in (np.inf, np.nan):
        X2 = X.copy()
        X2[n - 3, 77] = bad                       # in a workgroup's second tile
        _, _, flags = run_project_linear(dev, X2, V, 256, W2, None, None, 260, 128)
        assert flags & _lib.FLAG_X_NONFINITE
        _, _, flags = run_project(dev, X2, V[:64], 68)          # the wavefront-per-tile kernel
        assert flags & _lib.FLAG_X_NONFINITE
    _, _, flags = run_project(dev, X, V[:64], 68)
    assert flags == 0
