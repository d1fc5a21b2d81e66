"""CPU checks of group width 232 in the `wide` family of conv b (the width of lad_regnet_y_32gf): the shape predicates and plan queries of the
three entry points (host arithmetic: no GPU), the fragments of ops.pack_grouped_wide_weights unpacked by the documented index formula, the
chooser laud_regnet.conv_b_choice, and the factory lad_regnet_y_32gf."""
import pytest
import torch

from fill import seeded_randn

GW = 232
STEPS, MT = 131, 8
GROUP_BYTES = 2146304
MODEL_C = (232, 696, 1392, 3712)
# the eight conv b shapes of lad_regnet_y_32gf at 224 px: (w_b, input map, stride) of each stage's stride-2 first block and its stride-1 blocks
MODEL_MAPS = [(232, 112, 2), (232, 56, 1), (696, 56, 2), (696, 28, 1), (1392, 28, 2), (1392, 14, 1), (3712, 14, 2), (3712, 7, 1)]


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


def test_predicates_take_the_models_shapes_and_nothing_near_them(lib):
    for C in MODEL_C:
        assert lib.ldn_grouped_wide_rows_ok(C, GW) == 1 and lib.ldn_wgrad_grouped_wide_rows_ok(C, GW) == 1, C
        assert lib.ldn_grouped_wide_ok(C, GW, 7, 7, 1) == 1 and lib.ldn_grouped_wide_ok(C, GW, 14, 14, 2) == 1, C
        assert lib.ldn_grouped_wide_weight_bytes(C, GW) == (C // GW) * GROUP_BYTES
    assert GROUP_BYTES == STEPS * MT * 2048
    for C, gw in ((464, 116), (240, 232), (528, 264), (0, 232), (-232, 232)):
        assert lib.ldn_grouped_wide_rows_ok(C, gw) == 0, (C, gw)
        assert lib.ldn_grouped_wide_ok(C, gw, 7, 7, 1) == 0, (C, gw)
        assert lib.ldn_wgrad_grouped_wide_rows_ok(C, gw) == 0, (C, gw)
        assert lib.ldn_grouped_wide_weight_bytes(C, gw) == 0, (C, gw)
        assert lib.ldn_grouped_wide_rows_tiles(C, gw, 4096) == 0 and lib.ldn_wgrad_grouped_wide_rows_workspace_bytes(4096, C, gw) == 0
    assert lib.ldn_grouped_wide_rows_ok(4176, GW) == 1, "18 groups: the forward has no channel bound"
    assert lib.ldn_wgrad_grouped_wide_rows_ok(4176, GW) == 0, "C <= 4096 stays"
    assert lib.ldn_grouped_wide_ok(232, GW, 7, 7, 3) == 0


def test_image_plan_fits_the_model_and_refuses_what_does_not_fit(lib):
    for C, H, stride in MODEL_MAPS:
        Ho = (H - 1) // stride + 1
        assert lib.ldn_grouped_wide_ok(C, GW, H, H, stride) == 1, (C, H, stride)
        bands, strips, images = (lib.ldn_grouped_wide_bands(C, GW, H, H, Ho, stride), lib.ldn_grouped_wide_strips(C, GW, H, H, stride),
                                 lib.ldn_grouped_wide_images(C, GW, H, H, stride))
        assert bands >= 1 and strips >= 1 and images >= 1, (C, H, stride)
        assert images == 1 or bands == strips == 1, "several images share a workgroup only when the rectangle is the whole image"
        # the rectangle with its halo, 928 bytes a staged pixel, and the tables fit 150 KB
        R, Wc = -(-Ho // bands), -(-Ho // strips)
        staged = ((R - 1) * stride + 3) * ((Wc - 1) * stride + 3)
        assert images * staged * 928 + (images * GW + 20) * 4 + 32 <= 150 * 1024, (C, H, stride, bands, strips, images)
        assert lib.ldn_grouped_wide_bands(C, GW, H, H, Ho + 1, stride) == 0, "a wrong output height"
    assert lib.ldn_grouped_wide_images(3712, GW, 7, 7, 1) == 2, "two whole 7 x 7 maps with their halo: 2 x 81 staged pixels"
    big = (8, 1 << 20)
    assert lib.ldn_grouped_wide_ok(232, GW, *big, 1) == 0, "no rectangle of the plan's 32 x 32 cuts fits: 'does not fit', not a failed launch"
    assert lib.ldn_grouped_wide_bands(232, GW, *big, 8, 1) == 0 and lib.ldn_grouped_wide_strips(232, GW, *big, 1) == 0
    assert lib.ldn_grouped_wide_images(232, GW, *big, 1) == 0
    # the smallest cut maps of tests/test_hip_grouped_wide_232.py: 164 staged pixels is the most that fits
    assert lib.ldn_grouped_wide_bands(232, GW, 14, 8, 14, 1) == 1 and lib.ldn_grouped_wide_bands(232, GW, 15, 8, 15, 1) == 2
    assert lib.ldn_grouped_wide_strips(232, GW, 5, 21, 1) == 1 and lib.ldn_grouped_wide_strips(232, GW, 5, 22, 1) == 2


def test_rows_plan_and_workspace_are_functions_of_their_arguments(lib):
    tiles, work = lib.ldn_grouped_wide_rows_tiles, lib.ldn_wgrad_grouped_wide_rows_workspace_bytes
    for C in MODEL_C:
        last = 0
        for m_cap in (1, 31, 32, 127, 128, 255, 256, 784, 3136, 12544, 50176, 1 << 20, (1 << 31) - 1):
            assert tiles(C, GW, m_cap) == 1 and tiles(C, GW, m_cap) == 1, "one pixel tile per wave at this width, whatever the row count"
            if m_cap < (1 << 24):
                w = work(m_cap, C, GW)
                assert w == work(m_cap, C, GW) and w % (C * 9 * GW * 4) == 0 and w >= last, (C, m_cap)
                assert w // (C * 9 * GW * 4) <= max(1, m_cap // 128), "a split holds at least 128 rows of capacity"
                last = w
        assert tiles(C, GW, 0) == 0 and tiles(C, GW, -1) == 0 and work(-1, C, GW) == 0
        assert work(127, C, GW) == 0, "no split, no workspace"
    # training at batch 16 and 224 px: the four stages' stride-1 blocks (DESIGN.md 4zd states these)
    got = [work(16 * S * S, C, GW) for C, S in zip(MODEL_C, (56, 28, 14, 7))]
    assert got == [61 * 232 * 2088 * 4, 21 * 696 * 2088 * 4, 11 * 1392 * 2088 * 4, 4 * 3712 * 2088 * 4], got


def _unpack(frag):
    """-> (hi, lo [C, 9, 232] float32, number of pad elements, whether they are all zero), by the docstring's formula
    frag[g, s, m, l, p, e] = split_p(w[g gw + 32 m + (l & 31), q // Q, 8 (q % Q) + e]), q = 2 s + (l >> 5), Q = 29"""
    G, Q = frag.shape[0], GW // 8
    f = frag.float()
    assert tuple(f.shape) == (G, STEPS, MT, 64, 2, 8)
    hi, lo = torch.full((G * GW, 9, GW), float("nan")), torch.full((G * GW, 9, GW), float("nan"))
    pads, pads_zero = 0, True
    for s in range(STEPS):
        for m in range(MT):
            for l in range(64):
                q, i = 2 * s + (l >> 5), 32 * m + (l & 31)
                v = f[:, s, m, l]                       # [G, 2, 8]
                if i >= GW or q >= 9 * Q:
                    pads += v.numel()
                    pads_zero = pads_zero and bool((v == 0).all())
                    continue
                tap, o = q // Q, q % Q
                hi[i::GW, tap, 8 * o:8 * o + 8] = v[:, 0]
                lo[i::GW, tap, 8 * o:8 * o + 8] = v[:, 1]
    return hi, lo, pads, pads_zero


@pytest.mark.parametrize("C", [232, 464])
def test_fragments_by_the_index_formula(C):
    """every element, the pads included: 131 x 8 x 64 (step, row tile, lane) positions"""
    from laudnet_amd import ops
    w = seeded_randn((C, 9, GW), 900 + GW + C) * (2.0 / (9 * GW)) ** 0.5
    w[0, 0, 0] = 0.0
    w[1, 4, 5] = 1.0 + 2.0 ** -9                       # needs its lo part
    frag = ops.pack_grouped_wide_weights(w, GW)
    assert frag.dtype == torch.bfloat16 and frag.is_contiguous() and tuple(frag.shape) == (C // GW, STEPS, MT, 64, 2, 8)
    assert frag.numel() * 2 == (C // GW) * GROUP_BYTES
    hi, lo, pads, pads_zero = _unpack(frag)
    assert not torch.isnan(hi).any() and not torch.isnan(lo).any(), "the formula must reach every weight"
    assert torch.equal(hi, w.to(torch.bfloat16).float()), "hi is the bf16 rounding of w"
    assert torch.equal(lo, (w - hi).to(torch.bfloat16).float()), "lo is the bf16 rounding of w - hi"
    err = (w.double() - (hi.double() + lo.double())).abs()
    assert bool((err <= 2.0 ** -16 * w.double().abs()).all()), err.max().item()
    assert hi[1, 4, 5] == 1.0 and lo[1, 4, 5] == 2.0 ** -9
    assert pads_zero, "pad rows and the pad octet are zeros"
    assert pads == (C // GW) * 16 * (STEPS * MT * 64 - GW * 9 * GW // 8), "every element is a weight or a pad"
    # the pads by name: out channels 232-255 are lanes 8-31 of row tile 7; octet 261 is the upper lane half of step 130
    f = frag.float()
    assert bool((f[:, :, 7, 8:32] == 0).all()) and bool((f[:, :, 7, 40:64] == 0).all()) and bool((f[:, 130, :, 32:] == 0).all())
    assert bool((f[:, 130, :7, :32] != 0).any()) and bool((f[:, :130, 7, :8] != 0).any())


def test_packer_refuses_bad_shapes():
    from laudnet_amd import ops
    from laudnet_amd._lib import LdnError
    for shape, gw in [((464, 9, 116), 116), ((240, 9, 232), 232), ((232, 9, 112), 232), ((232, 8, 232), 232), ((0, 9, 232), 232), ((528, 9, 264), 264)]:
        with pytest.raises(LdnError):
            ops.pack_grouped_wide_weights(torch.zeros(*shape), gw)


def test_chooser_follows_the_rule_of_widths_56_and_112(monkeypatch):
    from laudnet_amd import laud_regnet, ops
    assert laud_regnet.USE_GROUPED_MFMA_WIDE is False and laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS is False
    assert laud_regnet.CONV_B["wide"].widths == (56, 112, 232) and laud_regnet._WIDTH_FAMILY[232] == "wide"
    assert ops._FRAG["wide"].widths == (56, 112, 232) and ops._FRAG["wide"].geometry[232] == (STEPS, MT)
    images = (2, 14, 14, 14, 14, 1)
    huge = (1, 8, 1 << 20, 8, 1 << 20, 1)
    before = ops.get_math_mode()
    ops.set_math_mode("bf16x3")
    try:
        def choices(C=464, gw=GW):
            return (laud_regnet.conv_b_choice("rows", C, gw), laud_regnet.conv_b_choice("rows", C, gw, images=images),
                    laud_regnet.conv_b_choice("image", C, gw, images=images))
        valu = (("valu", "rows"), ("valu", "rows"), ("valu", "image"))
        assert choices() == valu, "both switches off"
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE_ROWS", True)
        assert choices() == (("wide", "rows"), ("wide", "rows"), ("valu", "image"))
        assert choices(448, 112)[:2] == (("wide", "rows"), ("wide", "rows")), "the rule of width 112"
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE", True)
        assert choices() == (("wide", "rows"), ("wide", "rows"), ("wide", "image"))
        for C in MODEL_C:
            assert choices(C)[0] == ("wide", "rows") and choices(C)[2] == ("wide", "image")
        assert laud_regnet.conv_b_choice("image", 464, GW, images=huge) == ("valu", "image"), "the shape predicate: a map that does not fit"
        assert choices(240) == valu and choices(464, 116) == valu and choices(528, 264) == valu
        assert laud_regnet.conv_b_choice("rows", 464, GW, families=("gw",)) == ("valu", "rows")
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", False)
        assert choices() == valu
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", True)
        ops.set_math_mode("fp32")
        assert choices() == valu
    finally:
        ops.set_math_mode(before if before != ops.get_math_mode() else None)
        ops.set_math_mode(None)


def test_training_takes_the_width_through_the_librarys_predicate(monkeypatch):
    from laudnet_amd import training
    assert training.USE_WGRAD_GROUPED_WIDE is False
    assert not training._wgrad_grouped_wide_kernel(464, GW)
    monkeypatch.setattr(training, "USE_WGRAD_GROUPED_WIDE", True)
    for C in MODEL_C:
        assert training._wgrad_grouped_wide_kernel(C, GW)
    assert not training._wgrad_grouped_wide_kernel(4176, GW) and not training._wgrad_grouped_wide_kernel(464, 116)
    assert not training._wgrad_grouped_kernel(464, GW)
    monkeypatch.setattr(training, "USE_WGRAD_KERNEL", False)
    assert not training._wgrad_grouped_wide_kernel(464, GW)


def test_lad_regnet_y_32gf_factory():
    import laudnet_amd
    from laudnet_amd import laud_regnet
    assert "lad_regnet_y_32gf" in laud_regnet.__all__ and laudnet_amd.lad_regnet_y_32gf is laud_regnet.lad_regnet_y_32gf
    params = laud_regnet.BlockParams.from_init_params(se_ratio=0.25, **laud_regnet._Y["32gf"])
    assert laud_regnet._Y["32gf"] == dict(depth=20, w_0=232, w_a=115.89, w_m=2.53, group_width=232)
    assert list(params.depths) == [2, 5, 12, 1] and list(params.widths) == [232, 696, 1392, 3712]
    assert list(params.group_widths) == [232, 232, 232, 232]
    m32, m16 = laud_regnet.lad_regnet_y_32gf(), laud_regnet.lad_regnet_y_16gf()
    assert laud_regnet.lad_regnet_y_32gf.__name__ == "lad_regnet_y_32gf"
    blocks = [m for m in m32.modules() if isinstance(m, laud_regnet.ResBottleneckBlock)]
    assert len(blocks) == 20 and all(b.f.group_width == GW for b in blocks)
    assert [b.f.w_b for b in blocks] == [232] * 2 + [696] * 5 + [1392] * 12 + [3712]
    k32, k16 = list(m32.state_dict().keys()), list(m16.state_dict().keys())

    def pattern(keys):
        """the keys with the (stage, block) indices taken out: the same set of per-block names in both models"""
        import re
        return sorted({re.sub(r"block(\d+)-(\d+)", "blockS-B", re.sub(r"block(\d+)\.", "blockS.", k)) for k in keys})
    assert pattern(k32) == pattern(k16)
    assert len(k32) == len(set(k32)) and len(k32) > len(k16), "20 blocks against 18"
    assert m32.state_dict()["fc.weight"].shape == (1000, 3712)
