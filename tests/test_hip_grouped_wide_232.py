"""GPU tests of the matrix-core grouped 3x3 of LAD-RegNet's channel mode at group width 232, the width of lad_regnet_y_32gf
(ops.grouped_wide_conv3x3_image -> ldn_grouped_wide_conv3x3_image, k_grouped_wide<232>, bf16x3): the construction and the checks of
tests/test_hip_grouped_wide.py.

1. The op against F.conv2d(x * chan, w, padding 1, stride, groups = C / 232) in float64, then scale / shift / ReLU, read at each image's
   active channels; bound 1e-4 max(1, |want|max), the project's bound for its matrix-core grouped kernels.  Left-packed columns in and out,
   NaN in every input column at or past the image's count and in the pad columns of lda = C + 8, an output buffer ldo = C + 32 wide (wider
   than the 24 pad out channels 232-255 of the eighth row tile) whose sentinel must survive in the columns >= C, exact zeros in the columns
   behind the count, zero and negative scales, with and without ReLU, twice bit for bit.  Per image: none / all / a whole group inactive /
   one active granule in the last group / Bernoulli; granularities 1, 2, 8 and 232.
2. Several images per workgroup (asserted through ldn_grouped_wide_images), a ragged last run, an image without an active channel in the
   middle of a run; row bands and column strips (asserted through ldn_grouped_wide_bands / _strips), each at stride 1 and 2.
3. Refusals, the output untouched.
4. The dispatch on single blocks with w_b = 464: laud_regnet.USE_GROUPED_MFMA_WIDE on against off."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
NAN = float("nan")
PAD = 32

# gw, C, B, Hi, Wi, stride
CASES = [(232, 232, 4, 5, 5, 1),                          # one group
         (232, 464, 4, 9, 5, 2),                          # two groups; odd map, Ho = (Hi - 1) // 2 + 1
         (232, 3712, 2, 4, 4, 1),                         # the 16 groups of the model's stage 4
         (232, 232, 1, 6, 5, 1)]                          # ragged pixel tiles (Ho Wo = 30) with ONE image (Bernoulli channels)
# A staged pixel is 928 bytes, so 150 KB hold 164 staged pixels of one image less its tables.  Several images share a workgroup while they
# fit: a 4 x 4 map with its halo is 36 staged pixels (4 images a workgroup; B = 7 has an image without any active channel in the middle of
# its run, index 3), a 7 x 7 map 81 (2 images: runs 2, 2, 1).
SHARED = [(232, 464, 7, 4, 4, 1), (232, 464, 5, 7, 7, 1)]
# The plan stages a rectangle of output pixels WITH its zero halo: ((R - 1) stride + 3) x ((Wc - 1) stride + 3) staged pixels.  A whole
# 15 x 8 map is 17 x 10 = 170 staged pixels (14 x 8: 160, one band): the smallest tall map of that width that is banded; two bands of 8 and
# 7 rows, the second starts at output row 8 whose halo row 7 lies inside the image.  17 x 7 at stride 2 -> 9 x 4 is 19 x 9 = 171 staged
# pixels (16 x 7 -> 8 x 4: 17 x 9 = 153): two bands of 5 and 4 output rows, the second starts at output row 5 = input row 10, halo row 9.
BANDED = [(232, 232, 4, 15, 8, 1), (232, 232, 4, 17, 7, 2)]
# The same budget across: 5 x 22 is 7 x 24 = 168 staged pixels (5 x 21: 161, whole), 4 x 31 at stride 2 -> 2 x 16 is 5 x 33 = 165
# (4 x 30 -> 2 x 15: 5 x 31 = 155, whole); the plan cuts both into two column strips.
STRIPS = [(232, 232, 4, 5, 22, 1), (232, 232, 4, 4, 31, 2)]
GRANS = (1, 2, 8, "gw")


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


def _granule_mask(B, C, gw, gran, seed):
    """[B, C / gran]: image 0 nothing, image 1 everything, image 2 with group 0 wholly inactive, image 3 (image 4 when B = 7) with exactly
    one active granule, in its last group (and something elsewhere), image 3 of B = 7 nothing; Bernoulli draws for the other images -- and
    for every image of a batch smaller than 4."""
    gm = seeded_bernoulli((B, C // gran), 0.6, seed)
    per_group = gw // gran
    if B >= 4:
        one = 4 if B == 7 else 3
        gm[0] = 0.0
        gm[1] = 1.0
        if C > gw:
            gm[2, :per_group] = 0.0
            gm[2, per_group] = 1.0
        if B == 7:
            gm[3] = 0.0
        gm[one, -per_group:] = 0.0
        gm[one, -1 if per_group == 1 else -2] = 1.0
        if C > gw:
            gm[one, 0] = 1.0
    else:
        gm[0, 0] = 1.0
    return gm


@functools.lru_cache(maxsize=None)
def _problem(gw, C, B, Hi, Wi, stride, gran):
    """-> (a [B, Hi, Wi, C + 8] on the device, kernel-layout weights [C, 9, gw], scale, shift, idx, cnt, n per image, cidx, y64 [B, C, Ho, Wo] =
    scale conv + shift in float64); built once per case and granularity, shared by the ReLU / no-ReLU runs, never modified"""
    from laudnet_amd import ops
    seed = 9000 + 11 * gw + C + 3 * gran + stride + Hi
    gm = _granule_mask(B, C, gw, gran, seed)
    chan = gm.repeat_interleave(gran, dim=1) > 0.5                  # [B, C]
    n = chan.sum(dim=1).tolist()
    if B >= 4:
        one = 4 if B == 7 else 3
        per_group = chan.view(B, C // gw, gw).sum(dim=2)
        assert n[0] == 0 and n[1] == C and (B != 7 or n[3] == 0)
        assert C == gw or (per_group[2, 0] == 0 and n[2] > 0), "image 2: a whole group inactive"
        assert per_group[one, -1] == gran, "one active granule in the last group"
    x = seeded_randn((B, C, Hi, Wi), seed + 1)
    w = seeded_randn((C, gw, 3, 3), seed + 2) * (2.0 / (9 * gw)) ** 0.5
    scale = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 3))
    scale[0::5] = 0.0
    scale[1::5] = -scale[1::5]
    shift = 0.1 * seeded_randn((C,), seed + 4)
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, C // gran, gran, mask_in=gm.to(DEV))
    torch.cuda.synchronize()
    cidx = idx.cpu().long()
    assert cnt.cpu().tolist() == n
    a = torch.full((B, Hi, Wi, C + 8), NAN)                           # NaN behind every image's count and in the pad columns
    for b in range(B):
        assert torch.equal(cidx[b, :n[b]], torch.nonzero(chan[b]).reshape(-1))
        a[b, :, :, :n[b]] = x[b, cidx[b, :n[b]]].permute(1, 2, 0)
    xm = x.double() * chan.view(B, C, 1, 1)
    y64 = F.conv2d(xm, w.double(), padding=1, stride=stride, groups=C // gw) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return a.to(DEV), w.permute(0, 2, 3, 1).reshape(C, 9, gw).contiguous(), scale, shift, idx, cnt, n, cidx, y64


@functools.lru_cache(maxsize=None)
def _frag(gw, C, B, Hi, Wi, stride, gran):
    from laudnet_amd import ops
    return ops.pack_grouped_wide_weights(_problem(gw, C, B, Hi, Wi, stride, gran)[1].to(DEV), gw)


def _run(ops, prob, frag, gw, stride, relu):
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = prob
    C = wk.shape[0]
    out = torch.full((a.shape[0], y64.shape[2], y64.shape[3], C + PAD), SENTINEL, device=DEV)
    ops.grouped_wide_conv3x3_image(a, frag, gw, idx, cnt, scale.to(DEV), shift.to(DEV), out, stride=stride, relu=relu)
    torch.cuda.synchronize()
    return out


def _check(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    gran = gw if gran == "gw" else gran
    assert ops.grouped_wide_ok(C, gw, Hi, Wi, stride)
    prob, frag = _problem(gw, C, B, Hi, Wi, stride, gran), _frag(gw, C, B, Hi, Wi, stride, gran)
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = prob
    assert tuple(y64.shape[2:]) == ((Hi - 1) // stride + 1, (Wi - 1) // stride + 1) and a.shape[3] == C + 8
    out = _run(ops, prob, frag, gw, stride, relu)
    got = out.cpu()
    want = torch.relu(y64) if relu else y64
    bound = 1e-4 * max(1.0, want.abs().max().item())
    err = 0.0
    zero = scale == 0
    for b in range(B):
        g = got[b, :, :, :n[b]]
        assert torch.isfinite(g).all(), f"image {b}: a column at or past the count was read"
        wb = want[b, cidx[b, :n[b]]].permute(1, 2, 0)
        if n[b]:
            err = max(err, (g.double() - wb).abs().max().item())
        assert bool((got[b, :, :, n[b]:C] == 0).all()), f"image {b}: columns behind the count must be exactly zero"
        if not relu:
            zb = zero[cidx[b, :n[b]]]
            assert torch.equal(g[:, :, zb], shift[cidx[b, :n[b]]][zb].expand(g.shape[0], g.shape[1], -1)), "a zero scale leaves the shift"
    print(f"grouped_wide gw {gw} C {C} B {B} {Hi}x{Wi} stride {stride} gran {gran} relu {relu}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    assert bool((got[..., C:] == SENTINEL).all()), "columns >= C (where the pad out channels 232-255 of the last group would land) must not be written"
    if not relu:
        assert bool((got[..., :C] < 0).any())
    assert torch.equal(_run(ops, prob, frag, gw, stride, relu), out), "two runs differ"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", CASES)
def test_grouped_wide_232_vs_float64(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", SHARED)
def test_grouped_wide_232_images_share_a_workgroup(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    from laudnet_amd import _lib
    per = _lib.load().ldn_grouped_wide_images(C, gw, Hi, Wi, stride)
    assert per == (4 if Hi == 4 else 2) and B % per, "more than one image shares a workgroup here, and the last run is ragged"
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", (2, "gw"))
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", BANDED)
def test_grouped_wide_232_row_bands(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    from laudnet_amd import _lib
    lib = _lib.load()
    Ho = (Hi - 1) // stride + 1
    assert lib.ldn_grouped_wide_bands(C, gw, Hi, Wi, Ho, stride) == 2 and lib.ldn_grouped_wide_strips(C, gw, Hi, Wi, stride) == 1
    assert lib.ldn_grouped_wide_bands(C, gw, Hi - 1, Wi, (Hi - 2) // stride + 1, stride) == 1, "the smallest banded map of this width"
    R = (Ho + 1) // 2
    assert 0 < R * stride - 1 < Hi, "the second band's first halo row lies inside the image"
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", (2, "gw"))
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", STRIPS)
def test_grouped_wide_232_column_strips(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    from laudnet_amd import _lib
    lib = _lib.load()
    assert lib.ldn_grouped_wide_strips(C, gw, Hi, Wi, stride) == 2
    assert lib.ldn_grouped_wide_strips(C, gw, Hi, Wi - 1, stride) == 1, "the smallest strip-cut map of this height"
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


def test_refusals(ops):
    from laudnet_amd._lib import LdnError
    gw, C, B, Hi, Wi, stride = SHARED[1]
    prob = _problem(gw, C, B, Hi, Wi, stride, 2)
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = prob
    frag = _frag(gw, C, B, Hi, Wi, stride, 2)
    out = torch.full((B, Hi, Wi, C + PAD), SENTINEL, device=DEV)
    sc, sh = scale.to(DEV), shift.to(DEV)
    with pytest.raises(LdnError, match="not built"):        # width 116
        ops.grouped_wide_conv3x3_image(a, frag, 116, idx, cnt, sc, sh, out)
    assert not ops.grouped_wide_ok(464, 116, 7, 7, 1) and not ops.grouped_wide_ok(528, 264, 7, 7, 1) and not ops.grouped_wide_ok(240, 232, 7, 7, 1)
    with pytest.raises(LdnError):                   # fragments of another width of the family
        ops.grouped_wide_conv3x3_image(a, frag, 112, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # truncated by 16 bytes
        ops.grouped_wide_conv3x3_image(a, frag.reshape(-1)[:-8], gw, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # fp32 fragments
        ops.grouped_wide_conv3x3_image(a, frag.float(), gw, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # ldo no multiple of 4
        ops.grouped_wide_conv3x3_image(a, frag, gw, idx, cnt, sc, sh, torch.full((B, Hi, Wi, C + 2), SENTINEL, device=DEV))
    with pytest.raises(LdnError):                   # stride 3
        ops.grouped_wide_conv3x3_image(a, frag, gw, idx, cnt, sc, sh, torch.full((B, 3, 3, C + PAD), SENTINEL, device=DEV), stride=3)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ the dispatch switch
def _counted(ops, monkeypatch):
    """counting wrappers around the new op and the VALU op it replaces -> (calls of the new one, calls of the old one), group widths"""
    new, old = [], []
    real_new, real_old = ops.grouped_wide_conv3x3_image, ops.grouped_conv3x3_image

    def counted_new(a, w_frag, group_width, *args, **kwargs):
        new.append(group_width)
        return real_new(a, w_frag, group_width, *args, **kwargs)

    def counted_old(a, w, group_width, *args, **kwargs):
        old.append(group_width)
        return real_old(a, w, group_width, *args, **kwargs)
    monkeypatch.setattr(ops, "grouped_wide_conv3x3_image", counted_new)
    monkeypatch.setattr(ops, "grouped_conv3x3_image", counted_old)
    return new, old


def _block_out(gw, stride, dyn_mode, on, monkeypatch, ops):
    """one seeded ResBottleneckBlock 2 gw -> 2 gw (w_b = 464: two groups), output 7 x 7, forced masks -> (output, new calls, old calls)"""
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE", on)
    W = 2 * gw
    blk = laud_regnet.ResBottleneckBlock(W, W, stride, lambda c: nn.BatchNorm2d(c, eps=1e-5, momentum=0.1), nn.ReLU, group_width=gw,
                                         bottleneck_multiplier=1.0, se_ratio=0.25, channel_dyn_granularity=2, output_size=7,
                                         mask_spatial_granularity=1, dyn_mode=dyn_mode, channel_masker="MLP", channel_masker_layers=1).eval()
    assert (blk.proj is not None) == (stride == 2) and blk.f.group_width == gw and blk.f.w_b == W
    blk.load_state_dict(fill_state_dict(blk.state_dict(), 77 + gw))
    blk = blk.to(DEV)
    B = 4
    cm = seeded_bernoulli((B, W // 2), 0.6, 500 + gw + stride)
    cm[0, :gw // 2] = 0.0                           # image 0: its first group wholly inactive
    blk.f.forced_channel_mask = cm.to(DEV)
    if dyn_mode == "both":
        blk.f.forced_spatial_mask = seeded_bernoulli((B, 1, 7, 7), 0.5, 600 + gw + stride)
    x = torch.relu(seeded_randn((B, W, 7 * stride, 7 * stride), 700 + gw)).to(DEV)
    new, old = _counted(ops, monkeypatch)
    with torch.no_grad():
        out, stats = blk.run_dynamic(x)
    torch.cuda.synchronize()
    return out.clone(), list(new), list(old)


@pytest.mark.parametrize("dyn_mode", ["channel", "both"])
@pytest.mark.parametrize("stride", [1, 2])
def test_block_dispatch_at_width_232(ops, monkeypatch, stride, dyn_mode):
    from laudnet_amd import laud_regnet
    gw = 232
    assert laud_regnet.USE_GROUPED_MFMA_WIDE is False
    on, new, old = _block_out(gw, stride, dyn_mode, True, monkeypatch, ops)
    assert new == [gw] and old == [], (new, old)
    monkeypatch.undo()
    off, new, old = _block_out(gw, stride, dyn_mode, False, monkeypatch, ops)
    assert new == [] and old == [gw], (new, old)
    err, bound = (on - off).abs().max().item(), 1e-4 * max(1.0, off.abs().max().item())
    print(f"block gw {gw} stride {stride} {dyn_mode}: switch on vs off max |diff| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(on).all() and err < bound
