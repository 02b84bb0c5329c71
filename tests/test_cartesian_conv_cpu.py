"""FSW_conv / FSW_readout with a Cartesian embedding (embed_slices x embed_freqs), the part that needs no GPU: the constructor's
argument checks, the two new entry points of the native library and the ABI that has to stay as it was."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fsw_gnn_amd", "libfsw_hip.so")

pytestmark = pytest.mark.skipif(not os.path.isfile(LIB), reason="libfsw_hip.so not built (run __graft_entry__.build())")


@pytest.mark.parametrize("cls_name", ["FSW_conv", "FSW_readout"])
def test_cartesian_layer_on_cpu_raises_not_implemented(cls_name):
    import fsw_gnn_amd
    cls = getattr(fsw_gnn_amd, cls_name)
    with pytest.raises(NotImplementedError, match="Cartesian mode needs a HIP device"):
        cls(4, 4, embed_slices=2, embed_freqs=3, device="cpu")
    with pytest.raises(NotImplementedError, match="Cartesian mode needs a HIP device"):
        cls(4, 4, config={"embed_slices": 2, "embed_freqs": 3, "device": "cpu"})
    # the matching embed_dim is accepted: 2 * 3 + the mass column, or 2 * 3 without it
    with pytest.raises(NotImplementedError, match="Cartesian mode needs a HIP device"):
        cls(4, 4, embed_dim=7, embed_slices=2, embed_freqs=3, device="cpu")
    with pytest.raises(NotImplementedError, match="Cartesian mode needs a HIP device"):
        cls(4, 4, embed_dim=6, embed_slices=2, embed_freqs=3, encode_vertex_degrees=False, device="cpu")


def test_argument_errors_come_before_anything_else():
    from fsw_gnn_amd import FSW_conv
    with pytest.raises(AssertionError, match="given together"):
        FSW_conv(4, 4, embed_slices=2, device="cpu")
    with pytest.raises(AssertionError, match="given together"):
        FSW_conv(4, 4, embed_freqs=3, device="cpu")
    with pytest.raises(AssertionError, match="given together"):
        FSW_conv(4, 4, config={"embed_freqs": 3}, device="cpu")
    with pytest.raises(AssertionError, match="embed_dim must be None or"):
        FSW_conv(4, 4, embed_dim=8, embed_slices=2, embed_freqs=3, device="cpu")
    with pytest.raises(AssertionError, match="embed_dim must be None or"):      # 7 only with the mass column
        FSW_conv(4, 4, embed_dim=7, embed_slices=2, embed_freqs=3, encode_vertex_degrees=False, device="cpu")
    with pytest.raises(AssertionError, match="out_channels must equal 7"):
        FSW_conv(4, 4, embed_slices=2, embed_freqs=3, mlp_layers=0, concat_self=False, device="cpu")
    with pytest.raises(ValueError, match="Invalid argument 'embed_slice'"):
        FSW_conv(4, 4, config={"embed_slice": 2}, device="cpu")


def test_diagonal_layer_is_unchanged_by_the_new_arguments():
    from fsw_gnn_amd import FSW_conv
    conv = FSW_conv(4, 6, device="cpu")
    assert conv.embed_dim == 12 and not conv.fsw_embed.cartesian_mode
    assert tuple(conv.fsw_embed.projVecs.shape) == (11, 4) and tuple(conv.fsw_embed.freqs.shape) == (11,)


def test_new_entry_points_are_declared_and_bound():
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in ("fsw_conv_fused_cart_f32", "fsw_conv_fused_cart_lds_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES and hasattr(L, name)
    assert _lib._SIGNATURES["fsw_conv_fused_cart_f32"][1][0]._type_ is _lib.CartArgs
    assert _lib._SIGNATURES["fsw_conv_fused_cart_f32"][1][1:] == _lib._SIGNATURES["fsw_conv_fused_f32"][1][1:]
    # pure host function: H [32][ldh] floats + 32 node ids, ldh = (K rounded up to 8) | 1, at least the 132-float staging row
    q = L.fsw_conv_fused_cart_lds_bytes
    assert q(16, 16, 1) == 32 * 265 * 4 + 128 and q(3, 5, 0) == 32 * 132 * 4 + 128
    assert q(2, 70, 1) == q(70, 2, 1) == 32 * 145 * 4 + 128
    assert q(64, 16, 1) > 64 * 1024 >= q(16, 16, 1)


def test_abi_and_structs_are_unchanged():
    from fsw_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsw_hip.h")).read()
    assert int(re.search(r"#define FSW_ABI_VERSION (\d+)", header).group(1)) == 6 == _lib.FSW_ABI_VERSION
    assert _lib.lib().fsw_abi_version() == 6
    assert ctypes.sizeof(_lib.CartArgs) == 240 and len(_lib.CartArgs._fields_) == 33
    assert ctypes.sizeof(_lib.EmbedArgs) == 8 * 6 + 8 * 3 + 8 + 8 * 2 + 8 * 3 + 16 + 8 * 5 + 16 + 8 * 3 + 8 + 8
