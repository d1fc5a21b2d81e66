"""CPU checks of the whole-image / SE-fused matrix-core grouped 3x3 at group widths 8 and 24 (ldn_grouped_mfma_conv3x3_images[_gap],
k_grouped_gw_img): the plan (fits query, bands per image) is host arithmetic and answers without a GPU for every conv b of RegNetY-400MF,
-1.6GF and -3.2GF; the entry points refuse bad arguments before any launch; the dispatch switch is off by default, and with it off the
row form keeps every call that LDN_GROUPED_MFMA_WIDTHS alone gives it."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


def _model_shapes():
    """(tag, C, gw, Hi, stride) of conv b of every stage at 224 px -- the stride-2 first block and the stride-1 blocks -- from laud_regnet._Y"""
    from laudnet_amd import laud_regnet
    shapes = []
    for tag in ("400mf", "1_6gf", "3_2gf"):
        params = laud_regnet.BlockParams.from_init_params(se_ratio=0.25, **laud_regnet._Y[tag])
        size = 112                                     # the stem halves 224
        for width, stride, depth, gw, mult in params._get_expanded_params():
            w_b = int(round(width * mult))
            assert stride == 2 and w_b % gw == 0 and gw in (8, 24)
            shapes.append((tag, w_b, gw, size, 2))
            size //= 2
            if depth > 1:
                shapes.append((tag, w_b, gw, size, 1))
        assert size == 7
    return shapes


def test_every_conv_b_of_the_three_models_fits(lib):
    shapes = _model_shapes()
    assert len(shapes) >= 22 and {s[2] for s in shapes} == {8, 24}
    for tag, C, gw, Hi, s in shapes:
        Ho = (Hi - 1) // s + 1
        assert lib.ldn_grouped_mfma_ok(C, gw) == 1
        ng = lib.ldn_grouped_mfma_images_fit(Hi, Hi, C, gw)
        nb = lib.ldn_grouped_mfma_images_bands(Hi, Hi, Ho, s, C, gw)
        assert 1 <= ng <= C // gw, (tag, C, gw, Hi, s, ng)
        assert 1 <= nb <= Ho, (tag, C, gw, Hi, s, nb)
        if Ho in (14, 7):
            assert nb == 1, (tag, C, gw, Hi, s, nb)      # the small maps are whole images
        if Hi == 112:
            assert nb >= 2, (tag, C, gw, Hi, s, nb)      # 112 x 112 -> 56 x 56 is banded
        assert lib.ldn_grouped_mfma_images_bands(Hi, Hi, Ho + 1, s, C, gw) == 0       # not this geometry's output height


def test_non_square_maps_are_planned(lib):
    assert lib.ldn_grouped_mfma_images_fit(6, 10, 24, 8) > 0 and lib.ldn_grouped_mfma_images_bands(6, 10, 6, 1, 24, 8) == 1
    assert lib.ldn_grouped_mfma_images_fit(20, 12, 72, 24) > 0 and lib.ldn_grouped_mfma_images_bands(20, 12, 10, 2, 72, 24) == 1
    assert lib.ldn_grouped_mfma_images_bands(7, 600, 7, 1, 8, 8) >= 2        # a wide, low map: banded although it has few rows


def test_refusals_answer_zero(lib):
    fit, bands, ok = lib.ldn_grouped_mfma_images_fit, lib.ldn_grouped_mfma_images_bands, lib.ldn_grouped_mfma_ok
    for gw in (16, 56, 40):                            # the other widths
        assert ok(gw * 4, gw) == 0 and fit(14, 14, gw * 4, gw) == 0 and bands(14, 14, 14, 1, gw * 4, gw) == 0, gw
    for C, gw in ((100, 8), (100, 24), (0, 8), (0, 24), (-24, 24)):      # C % gw != 0, C = 0
        assert ok(C, gw) == 0 and fit(14, 14, C, gw) == 0 and bands(14, 14, 14, 1, C, gw) == 0, (C, gw)
    for gw in (8, 24):
        C = 2 * gw
        assert ok(C, gw) == 1
        assert fit(0, 14, C, gw) == 0 and bands(0, 14, 0, 1, C, gw) == 0 and bands(0, 14, 1, 1, C, gw) == 0      # Hi = 0
        assert fit(14, 0, C, gw) == 0 and bands(14, 0, 14, 1, C, gw) == 0
        assert bands(14, 14, 5, 3, C, gw) == 0 and bands(14, 14, 14, 0, C, gw) == 0                              # stride 3, stride 0
        assert bands(14, 14, 13, 1, C, gw) == 0 and bands(14, 14, 14, 2, C, gw) == 0                             # a wrong Ho
        assert fit(8, 1 << 20, C, gw) == 0                                                                       # three rows do not fit: an answer
        assert bands(8, 1 << 20, 8, 1, C, gw) == 0 and bands(8, 1 << 20, 4, 2, C, gw) == 0
        assert fit(14, 14, C, gw) > 0 and bands(14, 14, 14, 1, C, gw) == 1 and bands(14, 14, 7, 2, C, gw) == 1   # ... and the map next to them is taken


def test_entry_points_refuse_before_any_launch(lib):
    d = ctypes.c_void_p(256)
    for name, extra in (("ldn_grouped_mfma_conv3x3_images", ()), ("ldn_grouped_mfma_conv3x3_images_gap", (d,))):
        f = getattr(lib, name)

        def call(a=d, lda=48, Hi=7, Wi=7, Ho=7, Wo=7, stride=1, C=48, gw=24, out=d, ldo=48, extra=extra):
            return f(a, lda, d, 2, Hi, Wi, Ho, Wo, stride, d, C, gw, d, d, 1, out, ldo, *extra, None)
        assert call(a=None) == -1 and b"null" in lib.ldn_last_error()
        if extra:
            assert call(extra=(None,)) == -1 and b"null" in lib.ldn_last_error()
        for gw, C in ((16, 64), (56, 112), (40, 80), (24, 100), (8, 0)):
            assert call(C=C, gw=gw, lda=112, ldo=112) == -1 and b"not built" in lib.ldn_last_error(), (gw, C)
        assert call(lda=50) == -1 and b"strides" in lib.ldn_last_error()
        assert call(ldo=50) == -1 and b"strides" in lib.ldn_last_error()
        assert call(ldo=44) == -1 and b"strides" in lib.ldn_last_error()                       # ldo < C
        assert call(out=ctypes.c_void_p(260)) == -1 and b"aligned" in lib.ldn_last_error()
        assert call(Ho=6) == -1 and b"geometry" in lib.ldn_last_error()
        assert call(stride=3, Ho=3, Wo=3) == -1 and b"geometry" in lib.ldn_last_error()
        assert call(Hi=8, Wi=1 << 20, Ho=8, Wo=1 << 20) == -1 and b"do not fit" in lib.ldn_last_error()


def test_signatures_follow_the_width_16_twins():
    """the argument order of ldn_grouped16_* with group_width after C"""
    from laudnet_amd import _lib
    S = _lib.SIGNATURES
    for new, twin, at in (("ldn_grouped_mfma_images_fit", "ldn_grouped16_images_fit", 3), ("ldn_grouped_mfma_images_bands", "ldn_grouped16_images_bands", 5),
                          ("ldn_grouped_mfma_conv3x3_images", "ldn_grouped16_conv3x3_images", 11),
                          ("ldn_grouped_mfma_conv3x3_images_gap", "ldn_grouped16_conv3x3_images_gap", 11)):
        args, ret = S[twin]
        assert S[new] == (args[:at] + [ctypes.c_int] + args[at:], ret), new


@pytest.mark.parametrize("gw,w_b", [(8, 24), (24, 48)])
def test_switch_is_off_by_default_and_gates_conv_b_rows(gw, w_b, monkeypatch):
    """With LDN_GROUPED_MFMA_WIDTHS alone, _conv_b_rows gives whole images to the row form (tests/test_hip_grouped_mfma.py counts on it); the
    image form needs both switches, a fitting map and the images argument.  Stubbed ops: no GPU."""
    from laudnet_amd import laud_regnet, ops
    assert laud_regnet.USE_GROUPED_MFMA_WIDTHS_IMAGES is False
    calls = []
    monkeypatch.setattr(ops, "grouped_mfma_conv3x3_rows", lambda *a, **k: calls.append("rows"))
    monkeypatch.setattr(ops, "grouped_mfma_conv3x3_images", lambda *a, **k: calls.append("images"))
    monkeypatch.setattr(ops, "grouped_conv3x3_rows", lambda *a, **k: calls.append("valu"))
    monkeypatch.setattr(ops, "pack_grouped_mfma_weights", lambda w, g: "frag")

    class F:
        group_width = gw

    class H:
        shape = (4 * 49, w_b)
    images = (4, 7, 7, 7, 7, 1)

    def run(images=images):
        del calls[:]
        laud_regnet._conv_b_rows({"wb": None, "sb": None, "tb": None}, F, None, None, H, object(), 4 * 49, images=images)
        return list(calls)
    before = ops.get_math_mode()
    ops.set_math_mode("bf16x3")
    try:
        assert run() == ["valu"]                                               # both switches off: today's dispatch
        assert not laud_regnet.grouped_mfma_images_on(w_b, gw, 7, 7, 1)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS_IMAGES", True)
        assert run() == ["valu"]                                               # the new switch alone does nothing
        assert not laud_regnet.grouped_mfma_images_on(w_b, gw, 7, 7, 1)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS_IMAGES", False)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS", True)
        assert run() == ["rows"]                                               # WIDTHS alone: the row form, never the new op
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS_IMAGES", True)
        assert laud_regnet.grouped_mfma_images_on(w_b, gw, 7, 7, 1) and laud_regnet.grouped_mfma_images_on(w_b, gw, 14, 14, 2)
        assert not laud_regnet.grouped_mfma_images_on(w_b, 16, 7, 7, 1) and not laud_regnet.grouped_mfma_images_on(w_b, gw, 8, 1 << 20, 1)
        assert run() == ["images"]
        assert run(images=None) == ["rows"]                                    # training and the gathered lists pass no images
        assert run(images=(1, 8, 1 << 20, 8, 1 << 20, 1)) == ["rows"]          # a map that does not fit
        ops.set_math_mode("fp32")
        assert run() == ["valu"]
    finally:
        ops.set_math_mode(before if before != ops.get_math_mode() else None)
        ops.set_math_mode(None)
