"""CPU checks of the matrix-core channel-mode grouped 3x3 at group widths 56 and 112 (ldn_grouped_wide_conv3x3_image, k_grouped_wide): the
plan (fits query, row bands, images per workgroup, fragment bytes) is host arithmetic and answers without a GPU; the entry point refuses
bad arguments before any launch; the dispatch switch is off by default and leaves the narrow-width switch and its fragments alone."""
import ctypes

import pytest

# conv b of every stage of RegNetY-8GF (group width 56) and RegNetY-16GF (112) at 224 px: the stride-2 first block and the stride-1 blocks
MODEL_SHAPES = [(224, 56, 112, 112, 2), (224, 56, 56, 56, 1), (448, 56, 56, 56, 2), (448, 56, 28, 28, 1), (896, 56, 28, 28, 2), (896, 56, 14, 14, 1),
                (2016, 56, 14, 14, 2), (2016, 56, 7, 7, 1),
                (224, 112, 112, 112, 2), (224, 112, 56, 56, 1), (448, 112, 56, 56, 2), (448, 112, 28, 28, 1), (1232, 112, 28, 28, 2),
                (1232, 112, 14, 14, 1), (3024, 112, 14, 14, 2), (3024, 112, 7, 7, 1)]


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


def test_ok_takes_every_conv_b_of_both_models(lib):
    for C, gw, Hi, Wi, s in MODEL_SHAPES:
        assert lib.ldn_grouped_wide_ok(C, gw, Hi, Wi, s) == 1, (C, gw, Hi, Wi, s)


def test_ok_takes_nothing_else(lib):
    for gw in (8, 16, 24, 40):
        assert lib.ldn_grouped_wide_ok(gw * 4, gw, 14, 14, 1) == 0, gw
    assert lib.ldn_grouped_wide_ok(100, 56, 7, 7, 1) == 0               # C % gw != 0
    assert lib.ldn_grouped_wide_ok(168, 112, 7, 7, 1) == 0
    assert lib.ldn_grouped_wide_ok(0, 56, 7, 7, 1) == 0
    assert lib.ldn_grouped_wide_ok(112, 56, 0, 7, 1) == 0
    assert lib.ldn_grouped_wide_ok(112, 56, 14, 14, 3) == 0             # stride 3
    assert lib.ldn_grouped_wide_ok(56, 56, 8, 1 << 20, 1) == 0          # a map this wide has no rectangle the plan tries that fits: an answer
    assert lib.ldn_grouped_wide_ok(112, 112, 8, 1 << 20, 2) == 0


def test_bands_and_images(lib):
    for C, gw, Hi, Wi, s in MODEL_SHAPES:
        Ho = (Hi - 1) // s + 1
        nb = lib.ldn_grouped_wide_bands(C, gw, Hi, Wi, Ho, s)
        assert 1 <= nb <= Ho, (C, gw, Hi, Wi, s, nb)
        assert lib.ldn_grouped_wide_bands(C, gw, Hi, Wi, Ho + 1, s) == 0            # not this geometry's output height
        ni = lib.ldn_grouped_wide_images(C, gw, Hi, Wi, s)
        assert 1 <= ni <= 8 and (ni == 1 or nb == 1), (C, gw, Hi, Wi, s, nb, ni)    # several images only as whole images
    assert lib.ldn_grouped_wide_bands(224, 56, 112, 112, 56, 2) >= 2
    assert lib.ldn_grouped_wide_bands(224, 112, 112, 112, 56, 2) >= 2
    assert lib.ldn_grouped_wide_bands(2016, 56, 7, 7, 7, 1) == 1                    # a small map is one band ...
    assert lib.ldn_grouped_wide_images(2016, 56, 7, 7, 1) >= 2                      # ... and shares its workgroup
    assert lib.ldn_grouped_wide_images(3024, 112, 7, 7, 1) >= 2
    for C, gw, Hi, Wi, s in [(96, 24, 14, 14, 1), (100, 56, 7, 7, 1), (0, 56, 7, 7, 1), (112, 56, 14, 14, 3), (56, 56, 8, 1 << 20, 1)]:
        assert lib.ldn_grouped_wide_ok(C, gw, Hi, Wi, s) == 0
        assert lib.ldn_grouped_wide_bands(C, gw, Hi, Wi, (Hi - 1) // s + 1, s) == 0
        assert lib.ldn_grouped_wide_images(C, gw, Hi, Wi, s) == 0


def test_weight_bytes_match_the_packed_tensor(lib):
    import torch
    from laudnet_amd import ops
    for gw, C, per_group in ((56, 112, 32 * 2 * 64 * 32), (112, 224, 63 * 4 * 64 * 32)):
        frag = ops.pack_grouped_wide_weights(torch.zeros(C, 9, gw), gw)
        assert frag.dtype == torch.bfloat16 and frag.is_contiguous()
        assert frag.numel() * 2 == lib.ldn_grouped_wide_weight_bytes(C, gw) == (C // gw) * per_group
    assert lib.ldn_grouped_wide_weight_bytes(96, 24) == 0 and lib.ldn_grouped_wide_weight_bytes(100, 56) == 0
    assert lib.ldn_grouped_wide_weight_bytes(0, 56) == 0


def test_entry_point_refuses_before_any_launch(lib):
    f = lib.ldn_grouped_wide_conv3x3_image
    assert f(None, 112, 1, 7, 7, 1, 7, 7, None, 112, 56, None, None, None, None, 1, None, 112, None) == -1
    assert b"null" in lib.ldn_last_error()
    d = ctypes.c_void_p(256)
    assert f(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, None, d, d, 1, d, 112, None) == -1        # a channel list without its counts
    assert b"null" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 1, 6, 7, d, 112, 56, d, d, d, d, 1, d, 112, None) == -1           # Ho of another geometry
    assert b"geometry" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 3, 3, 3, d, 112, 56, d, d, d, d, 1, d, 112, None) == -1           # stride 3
    assert b"not built" in lib.ldn_last_error()
    for gw, C in ((24, 96), (16, 64), (8, 64), (40, 80)):                                       # the other widths
        assert f(d, C, 1, 7, 7, 1, 7, 7, d, C, gw, d, d, d, d, 1, d, C, None) == -1
        assert b"not built" in lib.ldn_last_error()
    assert f(d, 114, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, d, 112, None) == -1           # lda % 4
    assert b"strides" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, d, 114, None) == -1           # ldo % 4
    assert f(d, 224, 1, 7, 7, 1, 7, 7, d, 224, 112, d, d, d, d, 1, d, 220, None) == -1          # ldo < C
    assert b"strides" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, ctypes.c_void_p(260), 112, None) == -1
    assert b"aligned" in lib.ldn_last_error()


@pytest.mark.parametrize("gw,w_b", [(8, 24), (16, 32), (24, 48), (56, 112), (112, 224)])
def test_switch_is_off_by_default_and_gates_the_dispatch(gw, w_b, monkeypatch):
    """laud_regnet.grouped_wide_on: the switch, USE_GROUPED_MFMA, bf16x3 mode and the shape; prepared() packs wb_frag_wide only with the
    switch on and only at widths 56 / 112; the narrow-width switch and its fragments do not move."""
    import torch
    from torch import nn
    from laudnet_amd import laud_regnet, ops
    assert laud_regnet.USE_GROUPED_MFMA_WIDE is False
    wide = gw in (56, 112)

    def prepared():
        torch.manual_seed(0)
        return laud_regnet.BottleneckTransform(w_b, w_b, 1, nn.BatchNorm2d, nn.ReLU, gw, 1.0, 0.25, output_size=8, dyn_mode="channel").eval().prepared("cpu")
    before = ops.get_math_mode()
    ops.set_math_mode("bf16x3")
    try:
        assert not laud_regnet.grouped_wide_on(w_b, gw, 8, 8, 1)
        assert "wb_frag_wide" not in prepared()
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE", True)
        assert laud_regnet.grouped_wide_on(w_b, gw, 8, 8, 1) == wide
        assert laud_regnet.grouped_wide_on(w_b, gw, 16, 16, 2) == wide
        assert not laud_regnet.grouped_wide_on(w_b, gw, 8, 8, 3)
        p = prepared()
        assert ("wb_frag_wide" in p) == wide
        if wide:
            assert torch.equal(p["wb_frag_wide"], ops.pack_grouped_wide_weights(p["wb"], gw))
        # the narrow-width entry points answer as before
        assert not laud_regnet.grouped_chan_mfma_on(112, 56, 8, 8, 1)
        assert "wb_frag_gw" not in p and ("wb_frag" in p) == (gw == 16)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", False)
        assert not laud_regnet.grouped_wide_on(w_b, gw, 8, 8, 1)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", True)
        ops.set_math_mode("fp32")
        assert not laud_regnet.grouped_wide_on(w_b, gw, 8, 8, 1)
    finally:
        ops.set_math_mode(before if before != ops.get_math_mode() else None)
        ops.set_math_mode(None)
