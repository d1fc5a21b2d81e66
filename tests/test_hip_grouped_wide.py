"""GPU tests of the matrix-core grouped 3x3 of LAD-RegNet's channel mode at group widths 56 and 112 (ops.grouped_wide_conv3x3_image ->
ldn_grouped_wide_conv3x3_image, k_grouped_wide, bf16x3; ops.grouped_wide_ok is its fits query, ops.pack_grouped_wide_weights its fragments).

1. The op against F.conv2d(x * chan, w, padding 1, stride, groups = C / gw) in float64, then scale / shift / ReLU, read at each image's
   active channels; bound 1e-4 max(1, |want|max), the project's bound for its matrix-core grouped kernels.  Left-packed columns in and out,
   NaN in every input column at or past the image's count and in the pad columns of lda = C + 8, an output buffer ldo = C + 4 wide whose
   sentinel must survive in the columns >= C, exact zeros in the columns behind the count, zero and negative scales (a zero scale without
   ReLU leaves the shift exactly), with and without ReLU, twice bit for bit.  Per image: none / all / a whole group inactive / one active
   granule in the last group / Bernoulli; granularities 1, 2 and gw.
2. Several images per workgroup (asserted through ldn_grouped_wide_images), ragged last runs, an image without an active channel in the
   middle of a run; row bands and column strips (asserted through ldn_grouped_wide_bands / _strips).
3. Refusals, the output untouched.
4. The dispatch on single blocks: laud_regnet.USE_GROUPED_MFMA_WIDE on against off (the fp32 VALU path tests/test_hip_regnet_ops.py pins).
5. The LDN_DEBUG build: a clean call reports no violation and computes what the release build computes, bit for bit."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# gw, C, B, Hi, Wi, stride
CASES = [(56, 56, 4, 5, 5, 1), (112, 112, 4, 5, 5, 1),                          # one group
         (56, 168, 4, 9, 5, 2), (112, 336, 4, 9, 7, 2),                         # few groups; odd map, Ho = (Hi - 1) // 2 + 1
         (56, 2016, 2, 4, 4, 1), (112, 3024, 2, 4, 4, 1),                       # the group counts of RegNetY-8GF / 16GF (36 / 27)
         # ragged pixel tiles (Ho Wo = 30 / 63 / 55: no multiple of the 32-pixel tile) with ONE image (Bernoulli channels)
         (56, 112, 1, 6, 5, 1), (112, 224, 1, 7, 9, 1), (56, 56, 1, 5, 11, 1)]
# Several images share a workgroup (the plan stages up to 8 whole images while they fit: asserted); B = 7 has an image without any active
# channel in the middle of its run (index 3); 7 x 7 at stride 2 (width 112) and 14 x 14 (width 56) take 2 images a workgroup: runs 2, 2, 1.
SHARED = [(56, 112, 5, 7, 7, 1), (112, 224, 7, 4, 4, 1), (112, 224, 5, 7, 7, 2), (56, 112, 5, 14, 14, 1)]
# The plan stages a rectangle of output pixels WITH its zero halo: ((R - 1) stride + 3) x ((Wc - 1) stride + 3) staged pixels, at most 684
# (width 56) / 318 (width 112) in 150 KB.  A whole 67 x 8 map is 69 x 10 = 690 staged pixels (66 x 8: 680, one band), a 30 x 8 map 32 x 10 =
# 320 (29 x 8: 310): the smallest tall narrow maps that are banded.  41 x 7 at stride 2 -> 21 x 4 is 43 x 9 = 387 staged pixels: two bands,
# the second starts at output row 11 = input row 21, a halo row inside the image.
BANDED = [(56, 56, 4, 67, 8, 1), (112, 112, 4, 30, 8, 1), (112, 112, 4, 41, 7, 2)]
# Where three rows of the map do not fit either, the rows are cut into column strips: 5 x 120 at width 112 (3 x 122 = 366 staged pixels), and
# the plan prefers strips to bands for 71 x 9 at stride 2 (width 56).
STRIPS = [(112, 112, 4, 5, 120, 1), (56, 56, 4, 71, 9, 2)]
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
    seed = 5000 + 11 * gw + C + 3 * gran + stride + Hi
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
    out = torch.full((a.shape[0], y64.shape[2], y64.shape[3], C + 4), SENTINEL, device=DEV)
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
    assert bool((got[..., C:] == SENTINEL).all()), "columns >= C must not be written"
    if not relu:
        assert bool((got[..., :C] < 0).any())
    assert torch.equal(_run(ops, prob, frag, gw, stride, relu), out), "two runs differ"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", CASES)
def test_grouped_wide_vs_float64(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", SHARED)
def test_grouped_wide_images_share_a_workgroup(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    from laudnet_amd import _lib
    per = _lib.load().ldn_grouped_wide_images(C, gw, Hi, Wi, stride)
    assert min(per, B) > 1, "more than one image must share a workgroup here"
    if (Hi, stride) in ((14, 1), (7, 2)):
        assert per == 2 and B % per, "runs of 2, 2, 1: a ragged last run"
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", BANDED)
def test_grouped_wide_row_bands(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    from laudnet_amd import _lib
    Ho = (Hi - 1) // stride + 1
    assert _lib.load().ldn_grouped_wide_bands(C, gw, Hi, Wi, Ho, stride) >= 2
    assert _lib.load().ldn_grouped_wide_bands(C, gw, Hi - 1, Wi, (Hi - 2) // stride + 1, stride) == 1 or stride == 2, "the smallest banded map"
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", (2, "gw"))
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", STRIPS)
def test_grouped_wide_column_strips(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    from laudnet_amd import _lib
    assert _lib.load().ldn_grouped_wide_strips(C, gw, Hi, Wi, stride) >= 2
    _check(ops, gw, C, B, Hi, Wi, stride, gran, relu)


def test_refusals(ops):
    from laudnet_amd._lib import LdnError
    gw, C, B, Hi, Wi, stride = SHARED[0]
    prob = _problem(gw, C, B, Hi, Wi, stride, 2)
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = prob
    frag = _frag(gw, C, B, Hi, Wi, stride, 2)
    out = torch.full((B, Hi, Wi, C + 4), SENTINEL, device=DEV)
    sc, sh = scale.to(DEV), shift.to(DEV)
    with pytest.raises(LdnError):                   # width 24
        ops.grouped_wide_conv3x3_image(a, frag, 24, idx, cnt, sc, sh, out)
    assert not ops.grouped_wide_ok(96, 24, 7, 7, 1)
    with pytest.raises(LdnError):                   # fragments of the other width
        ops.grouped_wide_conv3x3_image(a, frag, 112, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # (and the narrow kernels' fragments)
        ops.grouped_wide_conv3x3_image(a, ops.pack_grouped_mfma_weights(torch.zeros(48, 9, 24, device=DEV), 24), gw, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # truncated by 16 bytes
        ops.grouped_wide_conv3x3_image(a, frag.reshape(-1)[:-8], gw, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # fp32 fragments
        ops.grouped_wide_conv3x3_image(a, frag.float(), gw, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # ldo no multiple of 4
        ops.grouped_wide_conv3x3_image(a, frag, gw, idx, cnt, sc, sh, torch.full((B, Hi, Wi, C + 2), SENTINEL, device=DEV))
    with pytest.raises(LdnError):                   # a channel list without its counts
        ops.grouped_wide_conv3x3_image(a, frag, gw, idx, None, sc, sh, out)
    with pytest.raises(LdnError):                   # stride 3
        ops.grouped_wide_conv3x3_image(a, frag, gw, idx, cnt, sc, sh, torch.full((B, 3, 3, C + 4), SENTINEL, device=DEV), stride=3)
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
    """one seeded ResBottleneckBlock 2 gw -> 2 gw (w_b = 2 gw: two groups), output 7 x 7, forced masks -> (output, new calls, old calls)"""
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
@pytest.mark.parametrize("gw", [56, 112])
def test_block_dispatch_at_widths_56_and_112(ops, monkeypatch, gw, stride, dyn_mode):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_GROUPED_MFMA_WIDE is False
    on, new, old = _block_out(gw, stride, dyn_mode, True, monkeypatch, ops)
    assert new == [gw] and old == [], (new, old)
    monkeypatch.undo()
    off, new, old = _block_out(gw, stride, dyn_mode, False, monkeypatch, ops)
    assert new == [] and old == [gw], (new, old)
    err, bound = (on - off).abs().max().item(), 1e-4 * max(1.0, off.abs().max().item())
    print(f"block gw {gw} stride {stride} {dyn_mode}: switch on vs off max |diff| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(on).all() and err < bound


# ------------------------------------------------------------------ the LDN_DEBUG build
DEBUG_SCRIPT = r"""
import ctypes, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests/golden")
import torch
from laudnet_amd import _lib, ops
from fill import seeded_bernoulli, seeded_randn
lib = _lib.load()
ops.set_math_mode("bf16x3")
def violations(reset=1):
    c, code = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.ldn_debug_violations(ctypes.byref(c), ctypes.byref(code), reset) == 0
    return c.value, code.value
res = {"initial": violations(), "sums": {}}
B, H = 3, 7
for gw, C in ((56, 168), (112, 224)):
    gm = seeded_bernoulli((B, C // 2), 0.6, 40 + gw)
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, C // 2, 2, mask_in=gm.cuda())
    a = torch.relu(seeded_randn((B, H, H, C), 41 + gw)).cuda()
    w = (seeded_randn((C, 9, gw), 42 + gw) * 0.1).cuda()
    frag = ops.pack_grouped_wide_weights(w, gw)
    out = torch.zeros(B, H, H, C).cuda()
    ops.grouped_wide_conv3x3_image(a, frag, gw, idx, cnt, torch.ones(C).cuda(), torch.zeros(C).cuda(), out)
    torch.cuda.synchronize()
    res["sums"][str(gw)] = out.double().abs().sum().item()
    res["clean_%%d" %% gw] = violations()
print("RESULT " + json.dumps(res))
"""


def _run_lib(lib):
    env = dict(os.environ, LDN_LIB_PATH=os.path.join(ROOT, "laudnet_amd", lib))
    p = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_debug_build_is_clean_and_bit_identical():
    """codes 421 (entry outside [0, C)), 422 (not ascending), 423 (count outside [0, C]) of k_grouped_wide stay silent on a clean call"""
    assert os.path.exists(os.path.join(ROOT, "laudnet_amd", "libldn_hip_debug.so")), "build it: python -m laudnet_amd.build --debug"
    dbg = _run_lib("libldn_hip_debug.so")
    rel = _run_lib("libldn_hip.so")
    assert rel["clean_56"][0] == -1, "the release build must say that its checks are compiled away"
    assert dbg["sums"] == rel["sums"] and all(v > 0 for v in rel["sums"].values()), "debug and release builds must compute identical results"
    assert dbg["initial"][0] == 0
    for gw in (56, 112):
        assert dbg[f"clean_{gw}"] == [0, 0], f"violations in a clean run at width {gw}: {dbg[f'clean_{gw}']}"
