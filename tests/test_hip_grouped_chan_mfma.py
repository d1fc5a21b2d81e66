"""GPU tests of the matrix-core grouped 3x3 of LAD-RegNet's channel mode (ops.grouped_chan_mfma_conv3x3_image ->
ldn_grouped_chan_mfma_conv3x3_image, bf16x3, group widths 8 / 16 / 24; ops.grouped_chan_mfma_ok is its fits query).

1. The op against F.conv2d(x * chan, w, padding 1, stride, groups = C / gw) in float64, then scale / shift / ReLU, read at each image's
   active channels; bound 1e-4 max(1, |want|max), the project's bound for its matrix-core grouped kernels.  Left-packed columns in and out,
   NaN in every input column at or past the image's count and in the pad columns of lda = C + 8, an output buffer ldo = C + 4 wide whose
   sentinel must survive in the columns >= C, exact zeros in the columns behind the count, zero and negative scales (a zero scale without
   ReLU leaves the shift exactly), with and without ReLU, twice bit for bit.  Per image: none / all / a whole group inactive / one active
   granule in the last group / Bernoulli; granularities 1, 2 and gw.
2. Refusals, the output untouched.
3. The dispatch on regnet_tiny.pt (group width 8): with laud_regnet.USE_GROUPED_MFMA_CHANNEL on, the channel and both cases pass the
   injected-mask comparison of tests/test_hip_blocks.py on the new kernel; off (the default), the new op is never called.
4. The dispatch at widths 16 and 24 on single blocks: switch on against switch off (the fp32 VALU path tests/test_hip_regnet_ops.py pins)."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn
from helpers import assert_tuple_close, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
NAN = float("nan")

# gw, C, B, Hi, Wi, stride
CASES = [(8, 8, 4, 5, 5, 1),            # one group
         (8, 64, 5, 7, 7, 1),
         (8, 104, 4, 9, 5, 2),          # 13 groups; odd map, Ho = (Hi - 1) // 2 + 1
         (8, 440, 4, 7, 7, 1),          # 55 groups, past one workgroup's chunk
         (16, 64, 4, 9, 7, 2),
         (16, 128, 5, 7, 7, 1),
         (16, 320, 4, 14, 10, 2),
         (24, 24, 4, 5, 5, 1),
         (24, 144, 4, 7, 7, 1),
         (24, 120, 5, 9, 7, 2),         # 5 groups
         (24, 888, 4, 7, 7, 1),         # 37 groups
         # ragged pixel tiles (Wo = 5 / 9 / 11: no multiple of 16, nor Ho Wo of the 16- / 32-pixel tile) with ONE image (Bernoulli channels)
         (8, 16, 1, 6, 5, 1), (16, 32, 1, 7, 9, 1), (24, 48, 1, 5, 11, 1)]
# One case per width whose map takes several row bands (asserted through the library's own answer).  The plan stages whole images while one
# group's image fits 80 KB of LDS (two workgroups per CU): 1 560 pixels at width 8, 895 at width 16, 474 at width 24 -- so the narrow, tall
# maps below are the smallest kind that is banded; the stride-2 one at width 16 also has bands whose first input row is a halo row.
BANDED = [(8, 8, 4, 64, 26, 1), (16, 32, 4, 113, 8, 2), (24, 24, 4, 40, 16, 1)]
GRANS = (1, 2, "gw")


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
    """[B, C / gran]: image 0 nothing, image 1 everything, image 2 with group 0 wholly inactive, image 3 with exactly one active granule, in
    its last group (and something elsewhere); Bernoulli draws for the other images -- and for every image of a batch smaller than 4."""
    gm = seeded_bernoulli((B, C // gran), 0.6, seed)
    per_group = gw // gran
    if B >= 4:
        gm[0] = 0.0
        gm[1] = 1.0
        if C > gw:
            gm[2, :per_group] = 0.0
            gm[2, per_group] = 1.0
        gm[3, -per_group:] = 0.0
        gm[3, -1 if per_group == 1 else -2] = 1.0
        if C > gw:
            gm[3, 0] = 1.0
    else:
        gm[0, 0] = 1.0
    return gm


@functools.lru_cache(maxsize=None)
def _problem(gw, C, B, Hi, Wi, stride, gran):
    """-> (a [B, Hi, Wi, C + 8] on the device, kernel-layout weights [C, 9, gw], scale, shift, idx, cnt, n per image, cidx, y64 [B, C, Ho, Wo] =
    scale conv + shift in float64); built once per case and granularity, shared by the ReLU / no-ReLU runs, never modified"""
    from laudnet_amd import ops
    seed = 3000 + 11 * gw + C + 3 * gran + stride + Hi
    gm = _granule_mask(B, C, gw, gran, seed)
    chan = gm.repeat_interleave(gran, dim=1) > 0.5                  # [B, C]
    n = chan.sum(dim=1).tolist()
    if B >= 4:
        per_group = chan.view(B, C // gw, gw).sum(dim=2)
        assert n[0] == 0 and n[1] == C
        assert C == gw or (per_group[2, 0] == 0 and n[2] > 0), "image 2: a whole group inactive"
        assert per_group[3, -1] == gran, "image 3: one active granule in its last group"
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


def _pack(ops, wk, gw):
    return ops.pack_grouped16_weights(wk.to(DEV)) if gw == 16 else ops.pack_grouped_mfma_weights(wk.to(DEV), gw)


def _run(ops, prob, gw, stride, relu):
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = prob
    C = wk.shape[0]
    out = torch.full((a.shape[0], y64.shape[2], y64.shape[3], C + 4), SENTINEL, device=DEV)
    ops.grouped_chan_mfma_conv3x3_image(a, _pack(ops, wk, gw), gw, idx, cnt, scale.to(DEV), shift.to(DEV), out, stride=stride, relu=relu)
    torch.cuda.synchronize()
    return out


def _check(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    gran = gw if gran == "gw" else gran
    assert ops.grouped_chan_mfma_ok(C, gw, Hi, Wi, stride)
    prob = _problem(gw, C, B, Hi, Wi, stride, gran)
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = prob
    assert tuple(y64.shape[2:]) == ((Hi - 1) // stride + 1, (Wi - 1) // stride + 1) and a.shape[3] == C + 8
    out = _run(ops, prob, gw, stride, relu)
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
    print(f"grouped_chan_mfma gw {gw} C {C} {Hi}x{Wi} stride {stride} gran {gran} relu {relu}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    assert bool((got[..., C:] == SENTINEL).all()), "columns >= C must not be written"
    if not relu:
        assert bool((got[..., :C] < 0).any())
    assert torch.equal(_run(ops, prob, gw, stride, relu), out), "two runs differ"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", CASES)
def test_grouped_chan_mfma_vs_float64(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", BANDED)
def test_grouped_chan_mfma_row_bands(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    """Maps that one workgroup does not hold: 64 x 26 (width 8), 113 x 8 at stride 2 (width 16), 40 x 16 (width 24) -- tall maps just past
    the whole-image limit of the plan (1 560 / 895 / 474 staged pixels of one group in 80 KB)."""
    from laudnet_amd import _lib
    Ho = (Hi - 1) // stride + 1
    assert _lib.load().ldn_grouped_chan_mfma_bands(C, gw, Hi, Wi, Ho, stride) >= 2
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


def test_refusals(ops):
    from laudnet_amd._lib import LdnError
    gw, C, B, Hi, Wi, stride = CASES[1]
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = _problem(gw, C, B, Hi, Wi, stride, 2)
    frag = _pack(ops, wk, gw)
    out = torch.full((B, Hi, Wi, C + 4), SENTINEL, device=DEV)
    sc, sh = scale.to(DEV), shift.to(DEV)
    with pytest.raises(LdnError):                   # width 56
        ops.grouped_chan_mfma_conv3x3_image(a, frag, 56, idx, cnt, sc, sh, out)
    assert not ops.grouped_chan_mfma_ok(448, 56, 7, 7, 1)
    with pytest.raises(LdnError):                   # fragments of another width
        ops.grouped_chan_mfma_conv3x3_image(a, frag, 24, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):
        ops.grouped_chan_mfma_conv3x3_image(a, frag, 16, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # truncated by 16 bytes
        ops.grouped_chan_mfma_conv3x3_image(a, frag.reshape(-1)[:-8], gw, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # fp32 fragments
        ops.grouped_chan_mfma_conv3x3_image(a, frag.float(), gw, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # ldo no multiple of 4
        ops.grouped_chan_mfma_conv3x3_image(a, frag, gw, idx, cnt, sc, sh, torch.full((B, Hi, Wi, C + 2), SENTINEL, device=DEV))
    with pytest.raises(LdnError):                   # a channel list without its counts
        ops.grouped_chan_mfma_conv3x3_image(a, frag, gw, idx, None, sc, sh, out)
    with pytest.raises(LdnError):                   # stride 3
        ops.grouped_chan_mfma_conv3x3_image(a, frag, gw, idx, cnt, sc, sh, torch.full((B, 3, 3, C + 4), SENTINEL, device=DEV), stride=3)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ the dispatch switch
def _counted(ops, monkeypatch):
    """counting wrappers around the new op and the VALU op it replaces -> (calls of the new one, calls of the old one), group widths"""
    new, old = [], []
    real_new, real_old = ops.grouped_chan_mfma_conv3x3_image, ops.grouped_conv3x3_image

    def counted_new(a, w_frag, group_width, *args, **kwargs):
        new.append(group_width)
        return real_new(a, w_frag, group_width, *args, **kwargs)

    def counted_old(a, w, group_width, *args, **kwargs):
        old.append(group_width)
        return real_old(a, w, group_width, *args, **kwargs)
    monkeypatch.setattr(ops, "grouped_chan_mfma_conv3x3_image", counted_new)
    monkeypatch.setattr(ops, "grouped_conv3x3_image", counted_old)
    return new, old


REGNET = load_golden("regnet_tiny.pt")
TOL = 1e-3                     # tests/test_hip_blocks.py: TOL, LOGIT_SCALE_TOL / LOGIT_RTOL of bf16x3
LOGIT_SCALE_TOL, LOGIT_RTOL = 1e-5, 0.0


def _regnet_injected(case):
    import laudnet_amd
    fx = REGNET["cases"][case]
    model = laudnet_amd.LAD_RegNet(laudnet_amd.BlockParams(**REGNET["tiny_params"]), **fx["kw"]).eval()
    assert list(model.state_dict().keys()) == fx["keys"]
    model.load_state_dict(fill_state_dict(model.state_dict(), fx["seed"]))
    size = fx["kw"]["input_size"]
    model, x = model.to(DEV), seeded_randn((fx["batch"], 3, size, size), fx["x_seed"]).to(DEV)
    assert {blk.f.group_width for blk in model.blocks()} == {8}
    for i, blk in enumerate(model.blocks()):
        if blk.f.masker_spatial is not None:
            ms = blk.f.masker_spatial.mask_size
            blk.f.forced_spatial_mask = seeded_bernoulli((fx["batch"], 1, ms, ms), 0.5, fx["mask_seed"] + 2 * i)
        blk.f.forced_channel_mask = seeded_bernoulli((fx["batch"], blk.f.masker_channel.channel_dyn_group), 0.62, fx["mask_seed"] + 2 * i + 1).to(DEV)
    with torch.no_grad():
        got = model(x, 1.0)
    want = fx["injected_run"]
    assert_tuple_close(got[1:6], want[1:6], atol=1e-6, what=f"regnet {case} stats")
    assert_tuple_close(got[:1], want[:1], atol=TOL + LOGIT_SCALE_TOL * float(torch.as_tensor(want[0]).abs().max()), rtol=LOGIT_RTOL,
                       what=f"regnet {case} logits")
    assert_tuple_close(got[6:], want[6:], atol=0.0, rtol=1e-5, what=f"regnet {case} flops")


@pytest.mark.parametrize("case", ["channel_g2", "both"])
def test_regnet_tiny_on_the_new_kernel(ops, monkeypatch, case):
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_CHANNEL", True)
    new, old = _counted(ops, monkeypatch)
    _regnet_injected(case)
    assert new and set(new) == {8} and old == [], (new, old)


@pytest.mark.parametrize("case", ["channel_g2", "both"])
def test_switch_off_never_calls_the_new_kernel(ops, monkeypatch, case):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_GROUPED_MFMA_CHANNEL is False
    new, old = _counted(ops, monkeypatch)
    _regnet_injected(case)
    assert new == [] and old and set(old) == {8}, (new, old)


def _block_out(gw, stride, dyn_mode, on, monkeypatch, ops):
    """one seeded ResBottleneckBlock 96 -> 96 (w_b 96: 6 groups of 16, 4 of 24), output 7 x 7, forced masks -> (output, new calls, old calls)"""
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_CHANNEL", on)
    blk = laud_regnet.ResBottleneckBlock(96, 96, stride, lambda c: nn.BatchNorm2d(c, eps=1e-5, momentum=0.1), nn.ReLU, group_width=gw,
                                         bottleneck_multiplier=1.0, se_ratio=0.25, channel_dyn_granularity=2, output_size=7,
                                         mask_spatial_granularity=1, dyn_mode=dyn_mode, channel_masker="MLP", channel_masker_layers=1).eval()
    assert (blk.proj is not None) == (stride == 2) and blk.f.group_width == gw and blk.f.w_b == 96
    blk.load_state_dict(fill_state_dict(blk.state_dict(), 77 + gw))
    blk = blk.to(DEV)
    B = 4
    cm = seeded_bernoulli((B, 48), 0.6, 500 + gw + stride)
    cm[0, :gw // 2] = 0.0                           # image 0: its first group wholly inactive
    blk.f.forced_channel_mask = cm.to(DEV)
    if dyn_mode == "both":
        blk.f.forced_spatial_mask = seeded_bernoulli((B, 1, 7, 7), 0.5, 600 + gw + stride)
    x = torch.relu(seeded_randn((B, 96, 7 * stride, 7 * stride), 700 + gw)).to(DEV)
    new, old = _counted(ops, monkeypatch)
    with torch.no_grad():
        out, stats = blk.run_dynamic(x)
    torch.cuda.synchronize()
    return out.clone(), list(new), list(old)


@pytest.mark.parametrize("dyn_mode", ["channel", "both"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("gw", [16, 24])
def test_block_dispatch_at_widths_16_and_24(ops, monkeypatch, gw, stride, dyn_mode):
    on, new, old = _block_out(gw, stride, dyn_mode, True, monkeypatch, ops)
    assert new == [gw] and old == [], (new, old)
    monkeypatch.undo()
    off, new, old = _block_out(gw, stride, dyn_mode, False, monkeypatch, ops)
    assert new == [] and old == [gw], (new, old)
    err, bound = (on - off).abs().max().item(), 1e-4 * max(1.0, off.abs().max().item())
    print(f"block gw {gw} stride {stride} {dyn_mode}: switch on vs off max |diff| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(on).all() and err < bound
