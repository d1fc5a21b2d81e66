"""CPU checks of the matrix-core channel-mode grouped 3x3 (ldn_grouped_chan_mfma_conv3x3_image): the fits query and the band count are
host arithmetic and answer without a GPU; the entry point refuses bad arguments before any launch."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


def test_ok_takes_the_three_widths_and_nothing_else(lib):
    assert lib.ldn_grouped_chan_mfma_ok(48, 24, 112, 112, 2) == 1       # RegNetY-1.6GF's first block: bands are required
    assert lib.ldn_grouped_chan_mfma_ok(64, 16, 56, 56, 1) == 1
    assert lib.ldn_grouped_chan_mfma_ok(440, 8, 7, 7, 1) == 1
    assert lib.ldn_grouped_chan_mfma_ok(448, 56, 14, 14, 1) == 0        # width 56
    assert lib.ldn_grouped_chan_mfma_ok(100, 8, 7, 7, 1) == 0           # C % gw != 0
    assert lib.ldn_grouped_chan_mfma_ok(40, 24, 7, 7, 1) == 0
    assert lib.ldn_grouped_chan_mfma_ok(64, 16, 56, 56, 3) == 0         # stride 3
    assert lib.ldn_grouped_chan_mfma_ok(0, 8, 7, 7, 1) == 0
    assert lib.ldn_grouped_chan_mfma_ok(64, 16, 0, 56, 1) == 0
    assert lib.ldn_grouped_chan_mfma_ok(24, 24, 8, 1 << 20, 1) == 0     # three rows of a map this wide do not fit: an answer, not a failed launch


def test_bands_is_zero_outside_ok_and_positive_inside(lib):
    for C, gw, Hi, Wi, s in [(48, 24, 112, 112, 2), (64, 16, 56, 56, 1), (440, 8, 7, 7, 1), (888, 24, 14, 14, 2), (8, 8, 5, 5, 1)]:
        assert lib.ldn_grouped_chan_mfma_ok(C, gw, Hi, Wi, s) == 1
        Ho = (Hi - 1) // s + 1
        nb = lib.ldn_grouped_chan_mfma_bands(C, gw, Hi, Wi, Ho, s)
        assert 1 <= nb <= Ho, (C, gw, Hi, Wi, s, nb)
        assert lib.ldn_grouped_chan_mfma_bands(C, gw, Hi, Wi, Ho + 1, s) == 0      # not this geometry's output height
    assert lib.ldn_grouped_chan_mfma_bands(440, 8, 7, 7, 7, 1) == 1                 # a small map is one band
    assert lib.ldn_grouped_chan_mfma_bands(48, 24, 112, 112, 56, 2) >= 2
    assert lib.ldn_grouped_chan_mfma_bands(448, 56, 14, 14, 14, 1) == 0
    assert lib.ldn_grouped_chan_mfma_bands(100, 8, 7, 7, 7, 1) == 0
    assert lib.ldn_grouped_chan_mfma_bands(64, 16, 56, 56, 19, 3) == 0


def test_entry_point_refuses_before_any_launch(lib):
    assert lib.ldn_grouped_chan_mfma_conv3x3_image(None, 64, 1, 7, 7, 1, 7, 7, None, 64, 16, None, None, None, None, 1, None, 64, None) == -1
    assert b"null" in lib.ldn_last_error()
    d = ctypes.c_void_p(256)
    # a channel list without its counts
    assert lib.ldn_grouped_chan_mfma_conv3x3_image(d, 64, 1, 7, 7, 1, 7, 7, d, 64, 16, d, None, d, d, 1, d, 64, None) == -1
    assert b"null" in lib.ldn_last_error()
    assert lib.ldn_grouped_chan_mfma_conv3x3_image(d, 64, 1, 7, 7, 1, 6, 7, d, 64, 16, d, d, d, d, 1, d, 64, None) == -1       # Ho of another geometry
    assert b"geometry" in lib.ldn_last_error()
    assert lib.ldn_grouped_chan_mfma_conv3x3_image(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, d, 112, None) == -1    # width 56
    assert b"not built" in lib.ldn_last_error()
    assert lib.ldn_grouped_chan_mfma_conv3x3_image(d, 66, 1, 7, 7, 1, 7, 7, d, 64, 16, d, d, d, d, 1, d, 64, None) == -1       # lda % 4
    assert b"strides" in lib.ldn_last_error()
    assert lib.ldn_grouped_chan_mfma_conv3x3_image(d, 64, 1, 7, 7, 1, 7, 7, d, 64, 16, d, d, d, d, 1, d, 66, None) == -1       # ldo % 4
    assert lib.ldn_grouped_chan_mfma_conv3x3_image(d, 64, 1, 7, 7, 1, 7, 7, d, 64, 16, d, d, d, d, 1, d, 60, None) == -1       # ldo < C
    assert lib.ldn_grouped_chan_mfma_conv3x3_image(d, 64, 1, 7, 7, 1, 7, 7, d, 64, 16, d, d, d, d, 1, ctypes.c_void_p(260), 64, None) == -1
    assert b"aligned" in lib.ldn_last_error()


@pytest.mark.parametrize("gw,w_b", [(8, 24), (16, 32), (24, 48), (56, 112)])
def test_switch_is_off_by_default_and_gates_the_dispatch(gw, w_b, monkeypatch):
    """laud_regnet.grouped_chan_mfma_on: the switch, USE_GROUPED_MFMA, bf16x3 mode and the shape; prepared() packs the fragments of widths 8
    and 24 when the switch is on (width 16 always has its own)."""
    import torch
    from torch import nn
    from laudnet_amd import laud_regnet, ops
    assert laud_regnet.USE_GROUPED_MFMA_CHANNEL is False

    def prepared():
        torch.manual_seed(0)
        return laud_regnet.BottleneckTransform(w_b, w_b, 1, nn.BatchNorm2d, nn.ReLU, gw, 1.0, 0.25, output_size=8, dyn_mode="channel").eval().prepared("cpu")
    before = ops.get_math_mode()
    ops.set_math_mode("bf16x3")
    try:
        assert not laud_regnet.grouped_chan_mfma_on(w_b, gw, 8, 8, 1)
        p = prepared()
        assert "wb_frag_gw" not in p and ("wb_frag" in p) == (gw == 16)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_CHANNEL", True)
        assert laud_regnet.grouped_chan_mfma_on(w_b, gw, 8, 8, 1) == (gw != 56)
        assert laud_regnet.grouped_chan_mfma_on(w_b, gw, 16, 16, 2) == (gw != 56)
        assert not laud_regnet.grouped_chan_mfma_on(w_b, gw, 8, 8, 3)
        p = prepared()
        assert ("wb_frag_gw" in p) == (gw in (8, 24)) and ("wb_frag" in p) == (gw == 16)
        if gw in (8, 24):
            assert torch.equal(p["wb_frag_gw"], ops.pack_grouped_mfma_weights(p["wb"], gw))
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", False)
        assert not laud_regnet.grouped_chan_mfma_on(w_b, gw, 8, 8, 1)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", True)
        ops.set_math_mode("fp32")
        assert not laud_regnet.grouped_chan_mfma_on(w_b, gw, 8, 8, 1)
    finally:
        ops.set_math_mode(before if before != ops.get_math_mode() else None)
        ops.set_math_mode(None)
