"""The checks of tests/dense_matrix_cases.py for fsw_gemm_tn_f32 against a numpy model of csrc/gemm_tn.hip, without a GPU: the k split
over the workgroups, the three bf16 planes of both operands, the six plane products per piece (summed in float64 and rounded once
-- more exact than the kernel's float32 accumulator, the same on the exact cases), the sum of the partial results in float32 and
beta.  The model passes every check; with one workgroup's first row shifted by one, without the clamp of the last piece at K, with
the two off-diagonal 32 x 32 tiles of every 64 x 64 block exchanged in the store, or without one plane product, the exact check that
is meant to notice it fails (tests/test_conv_fused_ref_cpu.py does the same for the fused layer's bound)."""
import numpy as np
import pytest

from tests import dense_matrix_cases as D

PAIRS = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]          # x_i y_j with i + j <= 2 (planes from 0), smallest first


def bf16(x):
    """float32 rounded to the nearest bf16 (ties to even), as float32; finite values only."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def planes(x):
    p1 = bf16(x)
    r = (x - p1).astype(np.float32)
    p2 = bf16(r)
    return [p1.astype(np.float64), p2.astype(np.float64), bf16((r - p2).astype(np.float32)).astype(np.float64)]


def model(broken=None):
    def run(dev, A, B, beta=0.0, C0=None, pads=(3, 2, 3), ws_fill=None, ws_bytes=None, edit=None):
        (K, M), N = A.shape, B.shape[1]
        per = D.tn_piece(K)
        past = np.ones((per, 1), dtype=np.float32)                  # what lies behind the operands is not zero
        Ax, Bx = np.concatenate([A, past * np.ones((1, M), np.float32)]), np.concatenate([B, past * np.ones((1, N), np.float32)])
        pairs = [p for p in PAIRS if not (broken == "plane" and p == (1, 1))]
        s = np.zeros((M, N), dtype=np.float32)
        for g in range(D.tn_grid(K)):
            k0 = g * per + (1 if broken == "k0" and g == 1 else 0)
            k1 = (g + 1) * per if broken == "clamp" and g * per < K else min((g + 1) * per, K)
            if k1 <= k0:
                continue
            ap, bp = planes(Ax[k0:k1]), planes(Bx[k0:k1])
            s = s + sum(ap[i].T @ bp[j] for i, j in pairs).astype(np.float32)
        if broken == "store":
            full = np.zeros((64 * -(-M // 64), 64 * -(-N // 64)), dtype=np.float32)
            full[:M, :N] = s
            t = full.reshape(full.shape[0] // 64, 2, 32, full.shape[1] // 64, 2, 32).copy()
            t[:, 0, :, :, 1, :], t[:, 1, :, :, 0, :] = t[:, 1, :, :, 0, :].copy(), t[:, 0, :, :, 1, :].copy()
            s = t.reshape(full.shape)[:M, :N]
        C = np.full((M, N + pads[2]), np.nan, dtype=np.float32)
        C[:, :N] = np.float32(beta) * C0 + s if beta != 0.0 else s
        return 0, C
    return run


def exact_checks():
    return {
        "integer": lambda: [D.check_tn_integer(None, K, M, N) for K, M, N in ((1025, 33, 17), (1025, 65, 64), (4097, 33, 17))],
        "probes": lambda: [D.check_tn_probes(None, 4097, 64, 17, exchanged) for exchanged in (False, True)],
        "plane product": lambda: D.check_tn_plane_product(None),
    }


def test_the_model_passes_every_check(monkeypatch):
    monkeypatch.setattr(D, "run_gemm_tn", model())
    for check in exact_checks().values():
        check()
    for beta in D.TN_BETAS:
        D.check_tn_integer(None, *D.TN_BETA_INT_CASE, beta=beta)
        D.check_tn_random(None, *D.TN_BETA_RANDOM_CASE, 6, beta=beta)
    D.check_tn_scaling(None)


@pytest.mark.parametrize("broken,noticed_by", [("k0", ("integer", "probes")), ("clamp", ("integer", "probes")),
                                               ("store", ("integer", "probes", "plane product")), ("plane", ("plane product",))])
def test_a_broken_model_fails_its_exact_check(monkeypatch, broken, noticed_by):
    monkeypatch.setattr(D, "run_gemm_tn", model(broken))
    checks = exact_checks()
    for name in noticed_by:
        with pytest.raises(AssertionError):
            checks[name]()
