"""CPU checks of the matrix-core packed-row grouped 3x3 at group widths 56 and 112 (ldn_grouped_wide_conv3x3_rows, k_grouped_wide_rows): the
shape query is host arithmetic and answers without a GPU; the entry point refuses bad arguments before any launch; the dispatch switch is off
by default, and with it on a prepared block holds the ONE packed copy that the image form and the row form share."""
import ctypes

import pytest

# conv b of every stage of RegNetY-8GF (group width 56) and RegNetY-16GF (112)
MODEL_SHAPES = [(224, 56), (448, 56), (896, 56), (2016, 56), (224, 112), (448, 112), (1232, 112), (3024, 112)]


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


def test_ok_takes_every_conv_b_of_both_models(lib):
    from laudnet_amd import ops
    for C, gw in MODEL_SHAPES:
        assert lib.ldn_grouped_wide_rows_ok(C, gw) == 1, (C, gw)
        assert ops.grouped_wide_rows_ok(C, gw) is True


def test_ok_takes_nothing_else(lib):
    from laudnet_amd import ops
    for gw in (8, 16, 24, 40):
        assert lib.ldn_grouped_wide_rows_ok(gw * 4, gw) == 0, gw
        assert lib.ldn_grouped_wide_rows_ok(gw * 14, gw) == 0, gw           # 112 / 224 / 336 / 560 channels at another width
    assert lib.ldn_grouped_wide_rows_ok(0, 56) == 0
    assert lib.ldn_grouped_wide_rows_ok(0, 112) == 0
    assert lib.ldn_grouped_wide_rows_ok(100, 56) == 0                       # C % gw != 0
    assert lib.ldn_grouped_wide_rows_ok(168, 112) == 0
    assert lib.ldn_grouped_wide_rows_ok(-56, 56) == 0
    assert ops.grouped_wide_rows_ok(168, 112) is False


def test_tiles_per_wave_plan(lib):
    """ldn_grouped_wide_rows_tiles: two pixel tiles per wave, one where groups x ceil(tiles / 2) < 3072 (fewer than 3 waves per SIMD at the cap);
    a function of m_cap and the shape only"""
    f = lib.ldn_grouped_wide_rows_tiles
    # batch 64: the stride-1 conv b of every stage of both models at 56^2 / 28^2 / 14^2 / 7^2
    got = [f(C, gw, 64 * S * S) for (C, gw), S in zip(MODEL_SHAPES, [56, 28, 14, 7] * 2)]
    assert got == [2, 2, 2, 1, 2, 2, 1, 1], got
    for C, gw in MODEL_SHAPES:
        G = C // gw
        tiles = 2 * ((3072 + G - 1) // G)                   # the smallest even tile count at which groups x tiles / 2 reaches 3072
        assert f(C, gw, 32 * tiles) == 2 and f(C, gw, 32 * (tiles - 1) + 1) == 2, (C, gw)
        assert f(C, gw, 32 * (tiles - 2)) == 1 and f(C, gw, 1) == 1, (C, gw)
    assert f(224, 56, 0) == 0 and f(224, 56, -5) == 0
    assert f(96, 24, 1 << 20) == 0 and f(100, 56, 1 << 20) == 0
    assert f(3024, 112, (1 << 31) - 1) == 2 and f(56, 56, (1 << 31) - 1) == 2      # no overflow at the largest row count


def test_entry_point_refuses_before_any_launch(lib):
    f = lib.ldn_grouped_wide_conv3x3_rows
    # (a, lda, nbr, m_count, m_cap, w_frag, C, gw, scale, shift, relu, out, ldo, stream)
    assert f(None, 112, None, None, 32, None, 112, 56, None, None, 1, None, 112, None) == -1
    assert b"null" in lib.ldn_last_error()
    d = ctypes.c_void_p(256)
    for hole in (0, 2, 5, 8, 9, 11):                                        # each required pointer in turn (m_count may be null)
        args = [d, 112, d, None, 32, d, 112, 56, d, d, 1, d, 112, None]
        args[hole] = None
        assert f(*args) == -1, hole
        assert b"null" in lib.ldn_last_error()
    for gw, C in ((24, 96), (16, 64), (8, 64), (40, 80), (56, 100), (112, 168), (56, 0)):      # shapes outside _ok
        assert f(d, 224, d, d, 32, d, C, gw, d, d, 1, d, 224, None) == -1, (gw, C)
        assert b"not built" in lib.ldn_last_error()
    assert f(d, 114, d, d, 32, d, 112, 56, d, d, 1, d, 112, None) == -1     # lda % 4
    assert b"strides" in lib.ldn_last_error()
    assert f(d, 112, d, d, 32, d, 112, 56, d, d, 1, d, 114, None) == -1     # ldo % 4
    assert b"strides" in lib.ldn_last_error()
    assert f(d, 220, d, d, 32, d, 224, 112, d, d, 1, d, 224, None) == -1    # lda < C
    assert b"strides" in lib.ldn_last_error()
    assert f(d, 224, d, d, 32, d, 224, 112, d, d, 1, d, 220, None) == -1    # ldo < C
    assert b"strides" in lib.ldn_last_error()
    assert f(d, 112, d, d, 32, d, 112, 56, d, d, 1, ctypes.c_void_p(260), 112, None) == -1
    assert b"aligned" in lib.ldn_last_error()
    # an empty problem is no error and no launch: the pointers are never touched
    assert f(d, 112, d, d, 0, d, 112, 56, d, d, 1, d, 112, None) == 0
    assert f(d, 112, d, d, -3, d, 112, 56, d, d, 1, d, 112, None) == 0
    assert f(d, 112, d, d, (1 << 31) - 1, d, 112, 56, d, d, 1, d, 112, None) == -1          # a row index of the last tile would leave int
    assert b"too many rows" in lib.ldn_last_error()


def test_python_op_refuses_other_widths_without_a_gpu():
    import torch
    from laudnet_amd import ops
    from laudnet_amd._lib import LdnError
    assert ops.grouped_wide_rows_ok(224, 56) and not ops.grouped_wide_rows_ok(96, 24)
    z = torch.zeros(4, 96)
    with pytest.raises(LdnError):                                           # CPU tensors are refused too: nothing here reaches a launch
        ops.grouped_wide_conv3x3_rows(z, torch.zeros(36, dtype=torch.int32), torch.zeros(4, 14, 64, 2, 8, dtype=torch.bfloat16), 24,
                                      torch.ones(96), torch.zeros(96), z.clone())


@pytest.mark.parametrize("gw,w_b", [(8, 24), (16, 32), (24, 48), (56, 112), (56, 224), (112, 224)])
def test_switch_is_off_by_default_and_gates_the_dispatch(gw, w_b, monkeypatch):
    """laud_regnet.grouped_wide_rows_on: the switch, USE_GROUPED_MFMA, bf16x3 mode and the shape; prepared() packs wb_frag_wide when either wide
    switch is on, only at widths 56 / 112, and the tensor is pack_grouped_wide_weights(p["wb"], gw): the image form's copy."""
    import torch
    from torch import nn
    from laudnet_amd import laud_regnet, ops
    assert laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS is False
    assert laud_regnet.USE_GROUPED_MFMA_WIDE is False
    wide = gw in (56, 112)

    def prepared():
        torch.manual_seed(0)
        return laud_regnet.BottleneckTransform(w_b, w_b, 1, nn.BatchNorm2d, nn.ReLU, gw, 1.0, 0.25, output_size=8, dyn_mode="spatial").eval().prepared("cpu")
    before = ops.get_math_mode()
    ops.set_math_mode("bf16x3")
    try:
        assert not laud_regnet.grouped_wide_rows_on(224, 56)
        assert not laud_regnet.grouped_wide_rows_on(w_b, gw)
        assert "wb_frag_wide" not in prepared()
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE_ROWS", True)
        assert laud_regnet.grouped_wide_rows_on(224, 56)
        assert laud_regnet.grouped_wide_rows_on(w_b, gw) == wide
        assert not laud_regnet.grouped_wide_rows_on(100, 56)
        p = prepared()
        assert ("wb_frag_wide" in p) == wide
        if wide:
            assert torch.equal(p["wb_frag_wide"], ops.pack_grouped_wide_weights(p["wb"], gw))
        # the other switches answer as before
        assert not laud_regnet.grouped_wide_on(w_b, gw, 8, 8, 1)
        assert not laud_regnet.grouped_mfma_widths_on(w_b, gw)
        assert "wb_frag_gw" not in p and ("wb_frag" in p) == (gw == 16)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", False)
        assert not laud_regnet.grouped_wide_rows_on(w_b, gw)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", True)
        ops.set_math_mode("fp32")
        assert not laud_regnet.grouped_wide_rows_on(w_b, gw)
    finally:
        ops.set_math_mode(before if before != ops.get_math_mode() else None)
        ops.set_math_mode(None)
