"""-m gpu: the SE squeeze in the epilogue of the matrix-core channel-mode grouped 3x3 at group widths 56, 112 and 232
(ops.grouped_wide_conv3x3_image_gap -> ldn_grouped_wide_conv3x3_image_gap, k_grouped_wide<GW, true>, bf16x3; ops.grouped_wide_gap_ok its fit
query, ops.grouped_wide_splits its rectangles per image), and the channel block that folds its SE block with it
(laud_regnet.USE_CHANNEL_SE_FUSED + USE_CHANNEL_SE_FUSED_WIDE).

1. conv b with sums, on the problems of tests/test_hip_grouped_wide.py and tests/test_hip_grouped_wide_232.py (imported, with their cached
   problems): one and many groups, the group counts of the models, ragged pixel tiles, runs of images sharing a workgroup with an empty
   image in the middle, row bands, column strips, both strides; plus workgroups that run MORE THAN ONE PASS over the fragments, so that an
   image's tile sums come from several passes and tile sets.  Granularity 1 and = width, with and without ReLU.
2. Refusals, both buffers untouched.
3. The channel block, folded against the five launches."""
import pytest
import torch
import torch.nn as nn

import test_hip_grouped_wide as G
import test_hip_grouped_wide_232 as G232
from fill import fill_state_dict, seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -7.0

# pixel tiles (of 32 output pixels) one pass of a workgroup holds: (8 / row tiles) tile sets x 4 resident tiles a wave
CAP = {56: 16, 112: 8, 232: 4}
# gw, C, B, Hi, Wi, stride: workgroups of MORE tiles than a pass holds (asserted below through the plan queries).
#   34 x 17: one image a workgroup, 578 pixels = 19 tiles (the last one ragged): passes of 16 and 3, so the second pass leaves 3 of the 4
#            tile sets with a tile and one without;
#   10 x 26: two images a workgroup, 9 tiles each (260 pixels) = 18: the second image's tiles lie in both passes; with B = 5 the runs are
#            (0, 1), (2, 3), (4): image 0 has no channel, so the first run has 9 tiles, the second 18, the ragged last one 9.
# At widths 112 and 232 the plan never gives a workgroup more tiles than one pass holds (8 / 4): its cost model charges a further pass
# over a group's fragments (504 KB / 2096 KB) more than the staging it saves.  test_no_second_pass_at_widths_112_and_232 asserts that over
# a grid of maps; the shared-workgroup problems of the imported modules fill a pass exactly (112: 7 of 8 tiles; 232: 4 of 4).
MULTIPASS = [(56, 112, 4, 34, 17, 1), (56, 112, 5, 10, 26, 1)]


@pytest.fixture(autouse=True)
def _bf16x3():
    from laudnet_amd import ops
    ops.set_math_mode("bf16x3")
    yield
    ops.set_math_mode("fp32")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()
    return _ops


def _plan(gw, C, B, Hi, Wi, stride):
    """-> (bands, strips, images a workgroup, pixel tiles of a workgroup with every image active)"""
    from laudnet_amd import _lib
    lib = _lib.load()
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    bands, strips = lib.ldn_grouped_wide_bands(C, gw, Hi, Wi, Ho, stride), lib.ldn_grouped_wide_strips(C, gw, Hi, Wi, stride)
    images = min(lib.ldn_grouped_wide_images(C, gw, Hi, Wi, stride), B)
    R, Wc = -(-Ho // bands), -(-Wo // strips)
    return bands, strips, images, images * -(-(R * Wc) // 32)


# ------------------------------------------------------------------------------------------------ 1. conv b with sums
def _check_gap(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    M = G232 if gw == 232 else G
    gran = gw if gran == "gw" else gran
    prob, frag = M._problem(gw, C, B, Hi, Wi, stride, gran), M._frag(gw, C, B, Hi, Wi, stride, gran)
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = prob
    Ho, Wo = y64.shape[2], y64.shape[3]
    bands, strips, images, tiles = _plan(gw, C, B, Hi, Wi, stride)
    splits = ops.grouped_wide_splits(C, gw, Hi, Wi, Ho, stride)
    assert splits == bands * strips >= 1 and ops.grouped_wide_gap_ok(C, gw, Hi, Wi, stride)
    if B >= 4:
        assert n[0] == 0 and n[1] == C          # an image without a channel, one with all; image 2 has a whole group inactive where C > gw
    want = M._run(ops, prob, frag, gw, stride, relu)
    sc, sh = scale.to(DEV), shift.to(DEV)
    runs = []
    for _ in range(2):
        out = torch.full_like(want, SENTINEL)
        gap = torch.full((B, splits, C), NAN, device=DEV)
        got = ops.grouped_wide_conv3x3_image_gap(a, frag, gw, idx, cnt, sc, sh, out, stride=stride, relu=relu, gap=gap)
        torch.cuda.synchronize()
        assert got is gap
        runs.append((out, gap))
    out, gap = runs[0]
    assert torch.equal(out, want), "out differs from the plain op's"
    assert torch.isfinite(gap).all(), "an element of gap_partial was not written"
    for b in range(B):
        assert bool((gap[b, :, n[b]:] == 0).all()), f"image {b}: sums behind the count must be exactly zero"
    assert torch.equal(runs[1][0], out) and torch.equal(runs[1][1], gap), "two launches differ"
    ref = out[..., :C].double().sum(dim=(1, 2)).cpu()                 # [B, C] float64 sums of the kernel's own output, packed-column order
    tot = gap.double().sum(dim=1).cpu()
    err, bound = (tot - ref).abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item())
    print(f"wide gap gw {gw} C {C} B {B} {Hi}x{Wi} stride {stride} gran {gran} relu {relu} splits {bands}x{strips} images {images} tiles {tiles}: "
          f"max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    if splits > 1:
        # a split holds its own rectangle: band rb of R rows x strip cb of Wc columns, index rb strips + cb
        R, Wc = -(-Ho // bands), -(-Wo // strips)
        for rb in range(bands):
            for cb in range(strips):
                part = out[:, rb * R:(rb + 1) * R, cb * Wc:(cb + 1) * Wc, :C].double().sum(dim=(1, 2)).cpu()
                e = (gap[:, rb * strips + cb].double().cpu() - part).abs().max().item()
                assert e < bound, f"split ({rb}, {cb}): {e:.3e}"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", [1, "gw"])
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", G.CASES + G232.CASES)
def test_conv_b_leaves_its_channel_sums_in_packed_order(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    assert _plan(gw, C, B, Hi, Wi, stride)[:2] == (1, 1)
    _check_gap(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", [1, "gw"])
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", G.SHARED + G232.SHARED)
def test_sums_of_images_that_share_a_workgroup(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    """one split however many images share the workgroup; B = 7 has an image without a channel in the middle of its run"""
    bands, strips, images, tiles = _plan(gw, C, B, Hi, Wi, stride)
    assert (bands, strips) == (1, 1) and images > 1 and tiles <= CAP[gw]
    _check_gap(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", [1, "gw"])
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", G.BANDED + G232.BANDED + G.STRIPS + G232.STRIPS)
def test_sums_per_row_band_and_column_strip(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    bands, strips, images, tiles = _plan(gw, C, B, Hi, Wi, stride)
    assert bands * strips >= 2 and images == 1
    assert (bands >= 2) if (gw, C, B, Hi, Wi, stride) in G.BANDED + G232.BANDED else (strips >= 2)
    _check_gap(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", [1, "gw"])
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", MULTIPASS)
def test_sums_across_passes_and_tile_sets(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    bands, strips, images, tiles = _plan(gw, C, B, Hi, Wi, stride)
    assert (bands, strips) == (1, 1) and CAP[gw] < tiles < 2 * CAP[gw], "a workgroup of two passes, the second one partial"
    assert (images, tiles) == ((1, 19) if Hi == 34 else (2, 18))
    _check_gap(ops, gw, C, B, Hi, Wi, stride, gran, relu)


def test_no_second_pass_at_widths_112_and_232():
    """(CPU arithmetic) the plan gives no workgroup of width 112 / 232 more tiles than one pass holds, so the multi-pass cases are width 56's"""
    for gw in (112, 232):
        most = 0
        for Hi in list(range(1, 41)) + [56, 112]:
            for Wi in list(range(1, 41)) + [56, 112]:
                for stride in (1, 2):
                    most = max(most, _plan(gw, gw, 8, Hi, Wi, stride)[3])
        assert most == CAP[gw], (gw, most)


def test_refusals(ops):
    from laudnet_amd._lib import LdnError
    gw, C, B, Hi, Wi, stride = G.SHARED[0]
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = G._problem(gw, C, B, Hi, Wi, stride, 1)
    frag, sc, sh = G._frag(gw, C, B, Hi, Wi, stride, 1), scale.to(DEV), shift.to(DEV)
    out = torch.full((B, Hi, Wi, C + 4), SENTINEL, device=DEV)
    gap = torch.full((B * C + 1,), SENTINEL, device=DEV)
    with pytest.raises(LdnError):                   # not 16-byte aligned
        ops.grouped_wide_conv3x3_image_gap(a, frag, gw, idx, cnt, sc, sh, out, gap=gap[1:].view(B, 1, C))
    with pytest.raises(LdnError):                   # another split count
        ops.grouped_wide_conv3x3_image_gap(a, frag, gw, idx, cnt, sc, sh, out, gap=torch.zeros(B, 2, C, device=DEV))
    with pytest.raises(LdnError, match="not built"):        # width 24
        ops.grouped_wide_conv3x3_image_gap(a, frag, 24, idx, cnt, sc, sh, out)
    assert not ops.grouped_wide_gap_ok(96, 24, 7, 7, 1)
    with pytest.raises(LdnError):                   # a channel list without its counts
        ops.grouped_wide_conv3x3_image_gap(a, frag, gw, idx, None, sc, sh, out, gap=gap[:B * C].view(B, 1, C))
    with pytest.raises(LdnError):                   # fragments of the other width
        ops.grouped_wide_conv3x3_image_gap(a, frag, 112, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # stride 3
        ops.grouped_wide_conv3x3_image_gap(a, frag, gw, idx, cnt, sc, sh, torch.full((B, 3, 3, C + 4), SENTINEL, device=DEV), stride=3)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((gap == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 3. the block
COUNTED = ("se_packed", "conv_image_gated", "grouped_wide_conv3x3_image_gap", "se_gate_image", "grouped_wide_conv3x3_image")


def _counted(ops, monkeypatch):
    calls = {n: 0 for n in COUNTED}
    for name in calls:
        real = getattr(ops, name)

        def counted(*a, _real=real, _n=name, **kw):
            calls[_n] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


def _block_run(ops, monkeypatch, gw, W, stride, Ho, inplace, se_on, wide_on, B=5):
    """one seeded channel-mode ResBottleneckBlock W -> W at group width gw, granularity 1, forced masks: image 0 without a channel, image 1
    with every channel, the last image with its first group wholly inactive -> (output, calls)"""
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE", True)
    monkeypatch.setattr(laud_regnet, "USE_CHANNEL_SE_FUSED", se_on)
    monkeypatch.setattr(laud_regnet, "USE_CHANNEL_SE_FUSED_WIDE", wide_on)
    blk = laud_regnet.ResBottleneckBlock(W, W, stride, lambda c: nn.BatchNorm2d(c, eps=1e-5, momentum=0.1), nn.ReLU, group_width=gw,
                                         bottleneck_multiplier=1.0, se_ratio=0.25, channel_dyn_granularity=1, output_size=Ho,
                                         mask_spatial_granularity=1, dyn_mode="channel", channel_masker="MLP", channel_masker_layers=1).eval()
    assert (blk.proj is not None) == (stride == 2) and blk.f.group_width == gw and blk.f.w_b == W
    blk.load_state_dict(fill_state_dict(blk.state_dict(), 277 + gw))
    blk = blk.to(DEV)
    assert blk.f.masker_channel.channel_dyn_group == W              # granularity 1
    cm = seeded_bernoulli((B, W), 0.5, 2500 + gw + stride + Ho)
    cm[0] = 0.0
    cm[1] = 1.0
    cm[B - 1, :gw] = 0.0
    blk.f.forced_channel_mask = cm.to(DEV)
    x = torch.relu(seeded_randn((B, W, Ho * stride, Ho * stride), 2700 + gw)).to(DEV).contiguous(memory_format=torch.channels_last)
    calls = _counted(ops, monkeypatch)
    with torch.no_grad():
        out, _ = blk.run_dynamic(x, inplace=inplace)
    torch.cuda.synchronize()
    if inplace and stride == 1:
        assert out.data_ptr() == x.data_ptr(), "the in-place identity block writes its input's rows"
    return out.clone(), dict(calls)


def _folded_vs_five(ops, monkeypatch, gw, W, stride, Ho, inplace, B=5):
    on, calls = _block_run(ops, monkeypatch, gw, W, stride, Ho, inplace, True, True, B)
    assert calls == dict(se_packed=0, conv_image_gated=1, grouped_wide_conv3x3_image_gap=1, se_gate_image=1,
                         grouped_wide_conv3x3_image=0), calls
    monkeypatch.undo()
    off, calls = _block_run(ops, monkeypatch, gw, W, stride, Ho, inplace, False, False, B)
    assert calls == dict(se_packed=1, conv_image_gated=0, grouped_wide_conv3x3_image_gap=0, se_gate_image=0,
                         grouped_wide_conv3x3_image=1), calls
    err, bound = (on - off).abs().max().item(), 1e-5 * max(1.0, off.abs().max().item())
    print(f"channel block gw {gw} W {W} {Ho}x{Ho} stride {stride} inplace {inplace}: folded vs five launches max |diff| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(on).all() and err < bound


@pytest.mark.parametrize("stride,inplace", [(1, False), (1, True), (2, False)])
@pytest.mark.parametrize("Ho", [7, 14])
@pytest.mark.parametrize("gw", [56, 112, 232])
def test_channel_block_with_folded_se_matches_the_five_launch_path(ops, monkeypatch, gw, Ho, stride, inplace):
    _folded_vs_five(ops, monkeypatch, gw, 2 * gw, stride, Ho, inplace)


def test_stage_4_block_at_full_width(ops, monkeypatch):
    """a stage-4 block of lad_regnet_y_8gf: 2016 channels in 36 groups of 56 on 7 x 7 maps, B = 2 (one image a workgroup short of the plan's run)"""
    _folded_vs_five(ops, monkeypatch, 56, 2016, 1, 7, False, B=2)


@pytest.mark.parametrize("se_on,wide_on", [(True, False), (False, True)])
def test_either_switch_off_runs_none_of_the_new_ops(ops, monkeypatch, se_on, wide_on):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_CHANNEL_SE_FUSED is False and laud_regnet.USE_CHANNEL_SE_FUSED_WIDE is False
    for gw in (56, 232):
        _, calls = _block_run(ops, monkeypatch, gw, 2 * gw, 1, 7, False, se_on, wide_on)
        assert calls == dict(se_packed=1, conv_image_gated=0, grouped_wide_conv3x3_image_gap=0, se_gate_image=0,
                             grouped_wide_conv3x3_image=1), (gw, calls)
        monkeypatch.undo()
