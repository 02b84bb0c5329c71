"""tests/layout_cases.py on the host: every (argument, layout) the GPU tests use has the property it is named for, equals its
contiguous array, and is surrounded by poison a kernel can read safely."""
import numpy as np
import pytest
import torch

from tests import layout_cases as LC

CASES = [(name, layout) for name, (_, allowed, _, _) in LC.arguments().items() for layout in allowed]


def test_every_layout_is_used_and_known():
    used = {layout for _, layout in CASES}
    assert used == set(LC.LAYOUTS)
    g = LC.graph()
    assert g["deg"][:10].tolist() == list(LC.CUT_DEGREES) and set(g["deg"][10:].tolist()) == set(range(16))
    assert int(LC.graph(short=True)["deg"].max()) == 32
    for gr in (g, LC.graph(short=True)):
        for a, b in zip(gr["rowptr"][:-1], gr["rowptr"][1:]):
            assert bool((np.diff(gr["col"][a:b]) > 0).all())


@pytest.mark.parametrize("name,layout", CASES, ids=["%s-%s" % c for c in CASES])
def test_layout_has_its_property(name, layout):
    a, _, hi, batch = LC.arguments()[name]
    base, view = LC.case(name, layout)
    item = a.dtype.itemsize
    want = np.broadcast_to(a, (batch,) + a.shape) if layout == "expanded" else a
    # values
    assert tuple(view.shape) == want.shape and view.dtype == torch.from_numpy(a).dtype
    assert np.array_equal(view.numpy(), want, equal_nan=False)
    assert base.is_contiguous() and base.storage_offset() == 0
    # geometry; byte offset of the view relative to the base = data_ptr() % 16 on a device, where a base is 512-byte aligned
    off = (view.data_ptr() - base.data_ptr())
    assert off == view.storage_offset() * item
    d = a.shape[-1] if a.ndim else 1
    if layout == "contig":
        assert view.is_contiguous() and off == 0 and base.shape == view.shape
    elif layout == "colslice":
        assert not view.is_contiguous() and view.stride(-1) == 1 and view.stride(-2) == d + LC.COLSLICE_EXTRA
        assert off == LC.COLSLICE_LEFT * item and off % 16 != 0
    elif layout == "rowstep":
        assert not view.is_contiguous() and off == 0 and view.stride(0) == 2 * int(np.prod(a.shape[1:], dtype=np.int64))
        assert a.ndim == 1 or view.stride(-1) == 1
    elif layout == "transposed":
        assert not view.is_contiguous() and view.stride(-1) == a.shape[-2] and view.stride(-2) == 1 and off == 0
    elif layout == "offset1":
        assert view.is_contiguous() and off == item and off % 16 == item
    elif layout == "oddslice":
        assert view.is_contiguous() and off == LC.ODD_OFFSET * item and off % 16 in (8, 12)
    elif layout == "expanded":
        assert not view.is_contiguous() and view.stride(0) == 0 and view[0].is_contiguous()
    elif layout == "batchslice":
        assert not view.is_contiguous() and view.stride(-2) == d + LC.BATCHSLICE_EXTRA and off == 0
        flat = view.reshape(-1, d)
        assert flat.data_ptr() == view.data_ptr() and not flat.is_contiguous()          # reshape keeps the view
    else:  # widerows
        assert not view.is_contiguous() and view.stride(0) % 2 == 0 and item == 8
        assert all((off + r * view.stride(0) * item) % 16 == 8 for r in range(view.shape[0]))
    if layout in LC.COPIED:
        assert not view.is_contiguous()
    # poison outside the view
    mask = LC.outside_mask(base, view).numpy()
    assert int((~mask).sum()) == (a.size if layout != "expanded" else a.size)
    out = base.numpy()[mask]
    if np.issubdtype(a.dtype, np.floating):
        assert bool(np.isnan(out).all()) and bool(np.isfinite(base.numpy()[~mask]).all())
    else:
        assert out.size == 0 or (int(out.min()) >= 0 and int(out.max()) < hi)
        flat, m = base.numpy().reshape(-1), mask.reshape(-1)
        idx = np.nonzero(m)[0]
        left, right = idx[idx > 0], idx[idx < flat.size - 1]
        assert bool((flat[left] != flat[left - 1]).all()) and bool((flat[right] != flat[right + 1]).all())


def test_on_device_keeps_the_geometry_on_the_host_device():
    base, view = LC.case("X12", "colslice")
    b, v = LC.on_device(base, view, torch.device("cpu"), requires_grad=True)
    assert v.stride() == view.stride() and v.storage_offset() == view.storage_offset() and torch.equal(v, view)
    (v * 2).sum().backward()
    mask = LC.outside_mask(base, view)
    assert bool((b.grad[mask] == 0).all()) and bool((b.grad[~mask] == 2).all())
    assert np.array_equal(LC.bits(b), LC.bits(base))
