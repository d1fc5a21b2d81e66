"""ldn_conv_packed with per-image row ranges and channel lists (dyn_mode 'both': laud_resnet.py:101-103), op by op against float64.

A1  The three launches of Bottleneck._run_both -- conv1 on the dilated pixel list with an output-channel list, the 3x3 through the
    neighbour table with both lists and the border-class shift table, conv3 with an input list scattered into the NHWC residual
    stream -- with EVERY intermediate tensor compared against the dense-emulation algebra of oracle.torch_ref.BottleneckRef in
    float64 (helpers.bottleneck_stages_f64).  The model-level checks see these kernels only through a global average pool.
A2  The options of the entry point that _run_both never combines, as literal-contract tests of include/ldn_hip.h:285-308,447-462.

`expected_variant` (tests/conv_plan.py) asks the library's own chooser, conv_plan() of csrc/ldn_conv_plan.h, through a host-only program;
the non-GPU test test_case_table_reaches_every_variant proves from it that the case table runs every tile shape, wave grid,
weight-staging mode and kernel a packed launch with channel lists can reach, in both arithmetic modes.

Bounds (the library's own direct tests of the same arithmetic, tests/test_hip_ops.py::test_conv_image_channel_subsets and
tests/test_hip_tail.py): conv1 1e-4 + 1e-4 |ref|, conv2 2e-4 + 1e-4 |ref|, conv3 after residual and ReLU 2e-4 + 1e-4 |ref|."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_plan
from conv_plan import expected_variant, expected_wave_rows
from fill import seeded_bernoulli, seeded_randn
from helpers import apply_math_mode  # noqa: F401  (autouse fixture: a test that takes math_mode runs in that mode)
from helpers import assert_close, bn_shift_f64, bottleneck_stages_f64, upsample_mask
from oracle import torch_ref as TR

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()  # raises if libldn_hip.so is missing -- no fallback
    return _ops


# (B, H, Wd, cin, width, channel granularity, stride, spatial mask groups)
CASES = [
    (4, 56, 56, 256, 64, 2, 1, 1),      # 6 x 2 tiles; conv3: the streaming kernel / 4 x 4 with a residual
    (4, 28, 28, 512, 128, 2, 1, 1),     # 4 x 4 without a residual (conv1, conv2)
    (5, 14, 14, 1024, 256, 2, 1, 1),    # 8 x 6: whole 14 x 14 images with an output list
    (4, 7, 7, 2048, 512, 2, 1, 1),      # 49 rows per image: 4 x 10 (fp32) / 2 x 10 (bf16x3); conv3 must NOT take the streaming kernel
    (4, 10, 10, 512, 256, 4, 1, 1),     # 100 rows: 4 x 10 in both modes, B_KN4 from granularity 4, streaming conv3 at its row minimum
    (4, 14, 14, 64, 16, 1, 1, 1),       # granularity 1: B_KN1, odd channel counts, zero columns up to the next multiple of 4
    (4, 28, 28, 256, 128, 2, 2, 1),     # stride 2 (projection shortcut): conv1 on the dilated list of the 28 x 28 input
    (4, 14, 14, 512, 256, 2, 2, 1),     # stride 2 onto a 7 x 7 map: conv1 8 x 6, conv2 / conv3 4 x 10 | 2 x 10
    (4, 12, 20, 256, 64, 2, 1, 2),      # non-square; two spatial mask groups: conv3 per column slice (ldo > cout), 4 x 4 with a residual
    (9, 14, 14, 256, 64, 2, 1, 1),      # a batch that is not a multiple of 8 (the grid is padded to the 8 XCDs)
    # staging mode x tile shape are separate template instantiations (PAIR and the B_KN1 column table scale with the tile): the rest of the cross product
    (4, 14, 14, 1024, 256, 4, 1, 1),    # 8 x 6 + B_KN4 (granularity 4 at stage 3)
    (4, 14, 14, 512, 128, 1, 1, 1),     # 4 x 4 + B_KN1
    (4, 14, 14, 1024, 256, 1, 1, 1),    # 8 x 6 + B_KN1
    (4, 7, 7, 1024, 256, 1, 1, 1),      # 4 x 10 (fp32) / 2 x 10 (bf16x3) + B_KN1
    (4, 10, 10, 1024, 256, 1, 1, 1),    # 4 x 10 + B_KN1 in both modes
    (4, 10, 10, 1024, 256, 2, 1, 1),    # 4 x 10 + B_KN2 in bf16x3
    (4, 14, 14, 512, 128, 4, 1, 1),     # 4 x 4 + B_KN4 WITHOUT a residual (conv2 at granularity 4): the 4 x 1 wave grid of that instantiation
]
MATHS = ("fp32", "bf16x3")


def block_launches(rows_in, rows_out, cin, width, gran, sg):
    """The conv_packed launches of _run_both (laud_resnet.py, Bottleneck._run_both) for a block: (name, expected_variant keywords).  rows_in / rows_out:
    pixels of the input / output map (the m_cap of conv1 / of conv2 and conv3)."""
    cout = 4 * width
    return [
        ("conv1", dict(packed=True, rows_per_image=rows_in, cin=cin, cout=width, taps=1, has_k=False, has_n=True, kgran=1,
                       shift_classes=1, residual=False, scale=True)),
        ("conv2", dict(packed=True, rows_per_image=rows_out, cin=width, cout=width, taps=9, has_k=True, has_n=True, kgran=gran,
                       shift_classes=16, residual=False, scale=True)),
        ("conv3", dict(packed=True, rows_per_image=rows_out, cin=width, cout=cout // sg, taps=1, has_k=True, has_n=False, kgran=gran,
                       shift_classes=1, residual=True, scale=False)),
    ]


def case_launches(case):
    B, H, Wd, cin, width, gran, stride, sg = case
    return block_launches(H * Wd, (H // stride) * (Wd // stride), cin, width, gran, sg)


def reachable_variants():
    """Every (kernel, MS, NS, BMODE, math, WM) the three launches of a `both` block can run, by ENUMERATION of the chooser over the blocks the
    library admits: widths that are multiples of 8 (an input list needs cin % 8, conv_list_ok) from 8 to 2048, maps from one pixel to 112 x 112 on
    both sides of every row threshold of the dispatch (64 | 96 | 128 | 256 rows), channel granularity 1 / 2 / 4, one / two / four spatial mask
    groups, stride 1 and 2, both arithmetic modes.  Nothing is excluded."""
    widths = sorted(set(range(8, 513, 8)) | {768, 1024, 2048})
    rows = [1, 31, 32, 33, 49, 63, 64, 65, 95, 96, 97, 100, 127, 128, 129, 196, 255, 256, 257, 784, 3136, 12544]
    found = set()
    for math in MATHS:      # one line of the CLI's grid form per (launch, width, stride, mask groups): the row counts and granularities as lists
        lines = []
        for width in widths:
            for stride in (1, 2):
                for sg in (1, 2, 4):
                    if (4 * width) % (4 * sg):
                        continue
                    for name, kw in block_launches(1, 1, 4 * width, width, (1, 2, 4), sg):
                        kw["rows_per_image"] = [r * stride * stride for r in rows] if name == "conv1" else rows
                        lines.append(conv_plan.shape_line(math=math, **kw))
        found |= {k[:4] + (math, k[4]) for k in conv_plan.reachable(lines)}
    return found


# What reachable_variants() must come to, written out so that a reader sees it: every tile shape x every staging mode (conv1: B_NK, conv2:
# B_KN<granularity>, conv3: B_KN4, conv_plan) in both modes, the 4 x 4 tile of bf16x3 on both wave grids (4 x 1: conv1 / conv2, 2 x 2: conv3 behind
# its residual), and the streaming kernel with an input list.  fp32 has no 2 x 10 tile and no streaming kernel.  16 + 22 instantiations; the last
# element is WM, the rows of k_conv_bf3's wave grid.
REACHABLE = {
    ("k_conv_image", 6, 2, "B_NK", "fp32", None), ("k_conv_image", 4, 4, "B_NK", "fp32", None), ("k_conv_image", 8, 6, "B_NK", "fp32", None),
    ("k_conv_image", 4, 10, "B_NK", "fp32", None),
    ("k_conv_image", 6, 2, "B_KN1", "fp32", None), ("k_conv_image", 4, 4, "B_KN1", "fp32", None), ("k_conv_image", 8, 6, "B_KN1", "fp32", None),
    ("k_conv_image", 4, 10, "B_KN1", "fp32", None),
    ("k_conv_image", 6, 2, "B_KN2", "fp32", None), ("k_conv_image", 4, 4, "B_KN2", "fp32", None), ("k_conv_image", 8, 6, "B_KN2", "fp32", None),
    ("k_conv_image", 4, 10, "B_KN2", "fp32", None),
    ("k_conv_image", 6, 2, "B_KN4", "fp32", None), ("k_conv_image", 4, 4, "B_KN4", "fp32", None), ("k_conv_image", 8, 6, "B_KN4", "fp32", None),
    ("k_conv_image", 4, 10, "B_KN4", "fp32", None),
    ("k_conv_bf3", 6, 2, "B_NK", "bf16x3", 2), ("k_conv_bf3", 4, 4, "B_NK", "bf16x3", 4), ("k_conv_bf3", 8, 6, "B_NK", "bf16x3", 4),
    ("k_conv_bf3", 4, 10, "B_NK", "bf16x3", 2), ("k_conv_bf3", 2, 10, "B_NK", "bf16x3", 2),
    ("k_conv_bf3", 6, 2, "B_KN1", "bf16x3", 2), ("k_conv_bf3", 4, 4, "B_KN1", "bf16x3", 4), ("k_conv_bf3", 8, 6, "B_KN1", "bf16x3", 4),
    ("k_conv_bf3", 4, 10, "B_KN1", "bf16x3", 2), ("k_conv_bf3", 2, 10, "B_KN1", "bf16x3", 2),
    ("k_conv_bf3", 6, 2, "B_KN2", "bf16x3", 2), ("k_conv_bf3", 4, 4, "B_KN2", "bf16x3", 4), ("k_conv_bf3", 8, 6, "B_KN2", "bf16x3", 4),
    ("k_conv_bf3", 4, 10, "B_KN2", "bf16x3", 2), ("k_conv_bf3", 2, 10, "B_KN2", "bf16x3", 2),
    ("k_conv_bf3", 6, 2, "B_KN4", "bf16x3", 2), ("k_conv_bf3", 4, 4, "B_KN4", "bf16x3", 4), ("k_conv_bf3", 4, 4, "B_KN4", "bf16x3", 2), ("k_conv_bf3", 8, 6, "B_KN4", "bf16x3", 4),
    ("k_conv_bf3", 4, 10, "B_KN4", "bf16x3", 2), ("k_conv_bf3", 2, 10, "B_KN4", "bf16x3", 2),
    ("k_conv1x1_stream", None, None, "B_KN4", "bf16x3", None),
}


def test_case_table_reaches_every_variant():
    """The set of variants the case table runs equals the set an enumeration of the dispatch rule over every admissible block finds
    (reachable_variants; REACHABLE is that set written out) -- and, branch by branch: every tile shape, every staging mode, 4 x 4 with and
    without a residual, the streaming kernel and the 49-row launch that must not take it."""
    assert reachable_variants() == REACHABLE and len(REACHABLE) == 16 + 22
    seen, detail = set(), {}
    conv_plan.plans([dict(kw, math=math) for case in CASES for math in MATHS for _, kw in case_launches(case)])      # (one run of the chooser for all)
    for case in CASES:
        for math in MATHS:
            for name, kw in case_launches(case):
                v = expected_variant(math=math, **kw)
                seen.add(v + (math, expected_wave_rows(math=math, **kw)))
                detail.setdefault((v, math, name, kw["residual"]), dict(kw, math=math))
    assert seen == REACHABLE, f"missing {sorted(map(str, REACHABLE - seen))}, unexpected {sorted(map(str, seen - REACHABLE))}"
    shapes = {m: {(k[0][1], k[0][2]) for k in detail if k[1] == m and k[0][1] is not None} for m in MATHS}
    assert shapes["fp32"] == {(6, 2), (4, 4), (8, 6), (4, 10)}                      # n-subtiles per block <= 2, <= 4, 6, 10
    assert shapes["bf16x3"] == {(6, 2), (4, 4), (8, 6), (4, 10), (2, 10)}           # ... and the 2 x 10 special case
    for math in MATHS:
        modes = {k[0][3] for k in detail if k[1] == math}
        assert modes == {"B_NK", "B_KN1", "B_KN2", "B_KN4"}, (math, modes)
        four = {k[3] for k in detail if k[1] == math and (k[0][1], k[0][2]) == (4, 4)}
        assert four == {False, True}, f"{math}: the 4 x 4 tile must run with and without a residual"
    waves = {expected_wave_rows(**kw) for k, kw in detail.items() if k[1] == "bf16x3" and (k[0][1], k[0][2]) == (4, 4)}
    assert waves == {4, 2}
    # the streaming kernel with an input list; the same launch at 49 rows per image must not take it
    conv3 = dict(case_launches(CASES[4])[2][1])
    assert conv3["rows_per_image"] == 100 and expected_variant(math="bf16x3", **conv3)[0] == "k_conv1x1_stream"
    assert expected_variant(math="bf16x3", **dict(conv3, rows_per_image=95))[0] == "k_conv_bf3"
    small = dict(case_launches(CASES[3])[2][1])
    assert small["rows_per_image"] == 49 and small["cout"] % 128 == 0 and small["cout"] >= 256 and small["cin"] <= 1024
    assert expected_variant(math="bf16x3", **small) == ("k_conv_bf3", 2, 10, "B_KN4")
    assert expected_variant(math="bf16x3", **dict(small, rows_per_image=196))[0] == "k_conv1x1_stream"
    assert all(expected_variant(math="fp32", **kw)[0] == "k_conv_image" for c in CASES for _, kw in case_launches(c))
    # strides and map shapes
    assert {c[6] for c in CASES} == {1, 2} and any(c[1] != c[2] for c in CASES) and any(c[7] == 2 for c in CASES)
    assert all(c[1] % c[6] == 0 and c[2] % c[6] == 0 for c in CASES)               # (_out_hw refuses an odd map before a stride-2 block)
    assert any(c[0] % 8 for c in CASES)


# ------------------------------------------------------------------ masks: forced by construction, asserted on the CPU
def _patch_edge(Ho):
    return 4 if Ho >= 56 else (2 if Ho >= 28 else 1)        # pixels per mask patch edge


def case_masks(case):
    """(group_mask [B,G], patch [B,sg,Sy,Sx]) of a case: image 0 no channel, image 1 all channels, image 2 no pixel (an empty row
    range in the MIDDLE of the batch), image 3 every pixel, Bernoulli draws elsewhere."""
    B, H, Wd, cin, width, gran, stride, sg = case
    i = CASES.index(case)
    Ho, Wo = H // stride, Wd // stride
    ps = _patch_edge(Ho)
    gm = seeded_bernoulli((B, width // gran), 0.6, 31 + i)
    gm[0] = 0.0
    gm[1] = 1.0
    patch = seeded_bernoulli((B, sg, Ho // ps, Wo // ps), 0.5, 41 + i)
    patch[2] = 0.0
    patch[3] = 1.0
    return gm, patch


def check_mask_preconditions(case, gm, patch):
    B = case[0]
    width, gran = case[4], case[5]
    n = gm.sum(dim=1) * gran
    assert n[0] == 0 and n[1] == width, "image 0 without a channel, image 1 with all of them"
    assert all(0 < n[b] < width for b in range(2, B)), "the other images' channel masks are real draws"
    kept = patch.flatten(2).sum(dim=2)          # [B, sg]
    full = patch[0, 0].numel()
    assert B >= 4 and bool((kept[2] == 0).all()) and bool((kept[3] == full).all()), "image 2 empty (mid-batch), image 3 full"
    for b in (0, 1, *range(4, B)):
        assert bool(((kept[b] > 0) & (kept[b] < full)).all()), f"image {b}: a real spatial draw in every group"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_case_masks_hold_their_preconditions(case):
    gm, patch = case_masks(case)
    check_mask_preconditions(case, gm, patch)


# ------------------------------------------------------------------ the float64 reference of a case
def _make_ref_block(case, seed=5):
    B, H, Wd, cin, width, gran, stride, sg = case
    cout = 4 * width
    down = None
    if stride != 1 or cin != cout:
        down = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride, bias=False), nn.BatchNorm2d(cout))
    blk = TR.BottleneckRef(cin, width, stride=stride, downsample=down, dyn_mode="both", channel_dyn_granularity=gran,
                           channel_masker="MLP", output_size=H // stride, spatial_mask_channel_group=sg).eval()
    TR.randomize_bn_(blk, seed)
    with torch.no_grad():
        convs = [blk.conv1, blk.conv2, blk.conv3] + ([down[0]] if down is not None else [])
        for j, m in enumerate(convs):
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.copy_(seeded_randn(tuple(m.weight.shape), 70 + j) * (2.0 / fan_in) ** 0.5)
    return blk


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """Inputs, masks and the float64 intermediates of a case (NHWC, flattened to [pixels, channels]); arithmetic-mode independent."""
    B, H, Wd, cin, width, gran, stride, sg = case
    Ho, Wo = H // stride, Wd // stride
    gm, patch = case_masks(case)
    check_mask_preconditions(case, gm, patch)
    blk = _make_ref_block(case)
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    x = F.relu(seeded_randn((B, cin, H, Wd), 32 + CASES.index(case)))
    m3 = upsample_mask(patch, Ho, Wo)                                         # [B, sg, Ho, Wo]
    blk64 = blk.double()
    h1, h2, y3, identity, out = bottleneck_stages_f64(blk64, x, gm, m3)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()
    return dict(state=state, has_ds=blk.downsample is not None, x=x, gm=gm, patch=patch, m3=m3, h1=flat(h1), h2=flat(h2), identity=flat(identity),
                out=flat(out), c1=torch.relu(bn_shift_f64(blk64.bn1)), c2=torch.relu(bn_shift_f64(blk64.bn2)))


def test_reference_helper_reproduces_the_oracle_block():
    """helpers.bottleneck_stages_f64 against BottleneckRef.forward itself (float64, forced masks, square map: the oracle's own mask
    interpolation) -- identity and projection shortcut, stride 1 and 2, one and two spatial mask groups."""
    for case in [(4, 8, 8, 32, 8, 2, 1, 1), (4, 8, 8, 16, 8, 1, 2, 2)]:
        B, H, Wd, cin, width, gran, stride, sg = case
        Ho = H // stride
        down = None
        if stride != 1 or cin != 4 * width:
            down = nn.Sequential(nn.Conv2d(cin, 4 * width, 1, stride=stride, bias=False), nn.BatchNorm2d(4 * width))
        blk = TR.BottleneckRef(cin, width, stride=stride, downsample=down, dyn_mode="both", channel_dyn_granularity=gran,
                               channel_masker="MLP", output_size=Ho, spatial_mask_channel_group=sg, mask_spatial_granularity=2).eval()
        TR.randomize_bn_(blk, 5)
        blk = blk.double()
        x = F.relu(seeded_randn((B, cin, H, Wd), 3)).double()
        gm = seeded_bernoulli((B, width // gran), 0.6, 4)
        gm[0], gm[1] = 0.0, 1.0
        patch = seeded_bernoulli((B, sg, Ho // 2, Ho // 2), 0.5, 6)
        blk.forced_channel_mask, blk.forced_spatial_mask = gm, patch
        with torch.no_grad():
            want = blk((x, None, None, None, None, None, torch.tensor(0.0, dtype=torch.float64)))[0]
        h1, h2, y3, identity, out = bottleneck_stages_f64(blk, x, gm, upsample_mask(patch, Ho, Ho))
        assert out.dtype == torch.float64 and torch.equal(out, want)
        # masked channels of h1 / h2 are the constants relu(shift): what post_sub removes on the HIP side
        c1 = torch.relu(bn_shift_f64(blk.bn1))
        dead = (TR.broadcast_channel_mask(gm, width) == 0).expand_as(h1)
        assert torch.allclose(h1[dead], c1.view(1, -1, 1, 1).expand_as(h1)[dead], atol=1e-12, rtol=0)


# ------------------------------------------------------------------ A1: the three launches of _run_both
def _hip_block(case, state):
    from laudnet_amd.laud_resnet import Bottleneck
    B, H, Wd, cin, width, gran, stride, sg = case
    cout = 4 * width
    down = None
    if stride != 1 or cin != cout:
        down = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride, bias=False), nn.BatchNorm2d(cout))
    hb = Bottleneck(cin, width, stride=stride, downsample=down, dyn_mode="both", channel_dyn_granularity=gran, channel_masker="MLP",
                    output_size=H // stride, spatial_mask_channel_group=sg).eval()
    hb.load_state_dict(state)
    return hb.to(DEV)


def _check_neighbour_table(nbr, idx3, idx1, n3, B, Hi, Wi, Ho, Wo, stride):
    """Every neighbour of every kept output pixel that lies inside the image is a row of the dilated list; -1 means outside, nothing else."""
    pix = idx3[:n3].long()
    b, rem = pix // (Ho * Wo), pix % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    tab = nbr[:n3 * 9].view(n3, 9).long()
    for t in range(9):
        iy, ix_ = oy * stride + t // 3 - 1, ox * stride + t % 3 - 1
        inside = (iy >= 0) & (iy < Hi) & (ix_ >= 0) & (ix_ < Wi)
        assert bool((tab[~inside, t] == -1).all()), f"tap {t}: a neighbour outside the image must be -1"
        assert bool((tab[inside, t] >= 0).all()), f"tap {t}: the dilated list misses a neighbour of a kept pixel"
        want = (b * Hi * Wi + iy * Wi + ix_)[inside]
        assert torch.equal(idx1.long()[tab[inside, t]], want), f"tap {t}: neighbour rows point at the wrong pixels"


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_both_mode_launches_every_intermediate(ops, case, math_mode):
    B, H, Wd, cin, width, gran, stride, sg = case
    Hi, Wi, Ho, Wo, W, cout = H, Wd, H // stride, Wd // stride, width, 4 * width
    ref = case_reference(case)
    hb = _hip_block(case, ref["state"])
    p = hb._prepare(torch.device(DEV))
    gm, patch = ref["gm"], ref["patch"]
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, W // gran, gran, mask_in=gm.to(DEV))
    union = patch[:, 0] if sg == 1 else patch.amax(dim=1)
    ix = ops.mask_to_index(union.contiguous().to(DEV), Ho, Wo, stride)
    torch.cuda.synchronize()
    # ---- the lists, on the CPU, before any convolution
    cidx, ccnt = idx.cpu().long(), cnt.cpu().tolist()
    pre1, pre3 = ix.pre1.cpu().tolist(), ix.pre3.cpu().tolist()
    idx1, idx3, nbr = ix.idx1.cpu(), ix.idx3.cpu(), ix.nbr.cpu()
    n1, n3 = pre1[B], pre3[B]
    assert ccnt[0] == 0 and ccnt[1] == W
    assert pre3[2] == pre3[3] and pre1[2] == pre1[3] and pre3[4] - pre3[3] == Ho * Wo and pre1[4] - pre1[3] == Hi * Wi
    m3u = upsample_mask(union, Ho, Wo).reshape(-1)
    assert torch.equal(idx3[:n3].long(), torch.nonzero(m3u > 0.5).reshape(-1))
    assert torch.equal(torch.bucketize(torch.arange(B + 1) * Hi * Wi, idx1[:n1].long().contiguous()), torch.tensor(pre1))
    _check_neighbour_table(nbr, idx3, idx1, n3, B, Hi, Wi, Ho, Wo, stride)

    xn = ref["x"].permute(0, 2, 3, 1).contiguous().to(DEV)
    x2d = xn.reshape(B * Hi * Wi, cin)
    geom = (Hi, Wi, Ho, Wo, stride)
    # ---- conv1 (laud_resnet.py:937-938)
    h1 = torch.full((ix.cap1, W), NAN, device=DEV)
    ops.conv_packed(x2d, p["w1"], p["s1"], p["t1"], h1, B=B, row_prefix=ix.pre1, m_cap=Hi * Wi, a_map=ix.idx1, taps=1,
                    n_idx=idx, n_cnt=cnt, post_sub=p["c1"], relu=1)
    # ---- conv2 (:940-942)
    h2 = torch.full((ix.cap3, W), NAN, device=DEV)
    ops.conv_packed(h1, p["w2"], p["s2"], p["t2_tab"], h2, B=B, row_prefix=ix.pre3, m_cap=Ho * Wo, a_map=ix.nbr, taps=9,
                    pix_map=ix.idx3, geom=geom, k_idx=idx, k_cnt=cnt, kgran=gran, n_idx=idx, n_cnt=cnt,
                    post_sub=p["c2"], relu=1)
    torch.cuda.synchronize()
    g1, g2 = h1.cpu(), h2.cpu()
    errs = {"h1": 0.0, "h2": 0.0}
    for name, got, want_all, pix, pre, sub, atol in (("h1", g1, ref["h1"], idx1[:n1].long(), pre1, ref["c1"], 1e-4),
                                                      ("h2", g2, ref["h2"], idx3[:n3].long(), pre3, ref["c2"], 2e-4)):
        for b in range(B):
            lo, hi, n = pre[b], pre[b + 1], ccnt[b]
            ch = cidx[b, :n]
            want = want_all[pix[lo:hi]][:, ch] - sub[ch]
            errs[name] = max(errs[name], assert_close(got[lo:hi, :n], want, atol, 1e-4, f"{name} image {b} ({hi - lo} rows, {n} channels)"))
            pad_hi = min((n + 3) // 4 * 4, W)
            assert bool((got[lo:hi, n:pad_hi] == 0).all()), f"{name} image {b}: columns {n}..{pad_hi - 1} must be exactly 0"
        assert bool(torch.isnan(got[pre[B]:]).all()), f"{name}: rows past the last image's range were written"

    # ---- conv3 (:944-972), in place and out of place
    keep_col = ref["m3"].permute(0, 2, 3, 1).reshape(B * Ho * Wo, sg).repeat_interleave(cout // sg, dim=1) > 0.5
    ident = ref["identity"].float()                                  # (the block input itself without a projection shortcut)
    resid0 = torch.where(keep_col, ident, torch.relu(ident))         # dropped (pixel, group): already ReLU-ed, as the shortcut launch leaves it
    if sg == 1:
        groups = [(ix, None, slice(0, cout), p["w3"], p["t3c"])]
    else:
        groups = []
        ar = torch.arange(ix.cap3, device=DEV, dtype=torch.int32)
        for g in range(sg):
            ig = ops.mask_to_index(patch[:, g].contiguous().to(DEV), Ho, Wo, stride)
            rows = torch.where(ar < ig.cnt[0], ix.pos3[ig.idx3.clamp(0, ix.cap3 - 1).long()], torch.full_like(ar, -1))
            cs = slice(g * (cout // sg), (g + 1) * (cout // sg))
            groups.append((ig, rows.contiguous(), cs, p["w3"][:, :, cs].contiguous(), p["t3c"][cs]))

    def conv3(out2d, resid):
        for ig, rows, cs, w3g, t3g in groups:
            before = out2d.clone()
            ops.conv_packed(h2, w3g, None, t3g, out2d[:, cs], B=B, row_prefix=ig.pre3, m_cap=Ho * Wo, a_map=rows, taps=1,
                            out_map=ig.idx3, k_idx=idx, k_cnt=cnt, kgran=gran, relu=1, residual2d=resid[:, cs])
            torch.cuda.synchronize()
            outside = torch.ones(cout, dtype=torch.bool, device=DEV)
            outside[cs] = False
            assert torch.equal(out2d[:, outside].view(torch.int32), before[:, outside].view(torch.int32)), "columns outside the slice were touched"
        return out2d

    inplace = resid0.clone().to(DEV)
    conv3(inplace, inplace)
    res = resid0.clone().to(DEV)
    outofplace = conv3(torch.relu(res), res)
    assert torch.equal(res.cpu(), resid0), "the out-of-place form must leave the residual alone"
    assert torch.equal(inplace, outofplace), "in-place and out-of-place conv3 differ"
    got = inplace.cpu()
    assert torch.equal(got[~keep_col].view(torch.int32), resid0[~keep_col].view(torch.int32)), "a dropped pixel must pass the identity through, bit for bit"
    errs["out"] = assert_close(got, ref["out"], 2e-4, 1e-4, "out (every pixel of the residual stream)")
    print(f"[packed A1] {case} {math_mode}: max |err| h1 {errs['h1']:.2e} h2 {errs['h2']:.2e} out {errs['out']:.2e}")


# ------------------------------------------------------------------ A2: the options _run_both never combines
def _affine(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1


def packed_reference(a, w, scale, shift, rows, *, a_map=None, out_map=None, cls=None, relu=1, relu_if_neg=None, post_sub=None, residual=None):
    """include/ldn_hip.h:288-297,448-454 for packed rows 0 .. rows-1 without channel lists, in float64.  w [cout, taps, cin] n-major.
    Returns (destination rows [rows], values [rows, cout])."""
    cout, taps, cin = w.shape
    a64, w64 = a.double(), w.double()
    acc = torch.zeros(rows, cout, dtype=torch.float64)
    for t in range(taps):
        src = torch.arange(rows) if a_map is None else a_map.view(-1, taps)[:rows, t].long()
        arow = torch.where((src >= 0).view(-1, 1), a64[src.clamp(min=0), :cin], torch.zeros((), dtype=torch.float64))
        acc += arow @ w64[:, t].t()
    v = acc * scale.double() if scale is not None else acc
    v = v + (shift.double() if shift.dim() == 1 else shift.double()[cls[:rows].long()])
    dst = torch.arange(rows) if out_map is None else out_map[:rows].long()
    if residual is not None:
        v = v + residual.double()[dst]
    if relu == 1:
        v = torch.relu(v)
    elif relu == 2:
        v = torch.where((relu_if_neg[:rows] < 0).view(-1, 1), torch.relu(v), v)
    if post_sub is not None:
        v = v - post_sub.double()
    return dst, v


def _d(t):
    return None if t is None else t.to(DEV)


@gpu
@pytest.mark.parametrize("cout", [64, 256])
def test_one_image_device_count_below_capacity(ops, cout, math_mode):
    """B == 1 without row_prefix: rows [0, *m_count); the rows between the count and m_cap of a NaN-filled output stay NaN."""
    cap, count, cin = 333, 201, 64
    a = seeded_randn((cap, cin), 1)
    w = seeded_randn((cout, 1, cin), 2) * (2.0 / cin) ** 0.5
    sc, sh = _affine(cout, 3)
    ps = seeded_randn((cout,), 4) * 0.1
    out = torch.full((cap, cout), NAN, device=DEV)
    ops.conv_packed(_d(a), _d(w), _d(sc), _d(sh), out, B=1, m_count=torch.tensor([count], dtype=torch.int32, device=DEV), m_cap=cap,
                    taps=1, post_sub=_d(ps), relu=1)
    torch.cuda.synchronize()
    _, want = packed_reference(a, w, sc, sh, count, post_sub=ps)
    assert_close(out[:count], want, 1e-4, 1e-4, "rows below the count")
    assert bool(torch.isnan(out[count:]).all()), "rows >= *m_count were written"


@gpu
@pytest.mark.parametrize("cout", [64, 256])
def test_conditional_relu(ops, cout, math_mode):
    """relu == 2: ReLU only where relu_if_neg[R] < 0 (include/ldn_hip.h:453-454)."""
    rows, cin = 300, 96
    a = seeded_randn((rows, cin), 5)
    w = seeded_randn((cout, 1, cin), 6) * (2.0 / cin) ** 0.5
    sc, sh = _affine(cout, 7)
    flag = torch.where(seeded_bernoulli((rows,), 0.5, 8) > 0.5, torch.tensor(-1), torch.tensor(0)).to(torch.int32)
    flag[::7] = 5
    out = torch.full((rows, cout), NAN, device=DEV)
    ops.conv_packed(_d(a), _d(w), _d(sc), _d(sh), out, B=1, m_cap=rows, taps=1, relu=2, relu_if_neg=_d(flag))
    torch.cuda.synchronize()
    _, want = packed_reference(a, w, sc, sh, rows, relu=2, relu_if_neg=flag)
    assert bool((want[flag >= 0] < 0).any()) and bool((want[flag < 0] == 0).any())
    assert_close(out, want, 2e-4, 1e-4, "relu == 2")


@gpu
@pytest.mark.parametrize("prescaled", [False, True], ids=["scale", "scale_null"])
@pytest.mark.parametrize("cout", [64, 256])
def test_scatter_with_residual(ops, cout, prescaled, math_mode):
    """out_map scatter + residual, aliased (in place) and not; scale == NULL with a residual starts the bf16x3 kernels' accumulators
    from the residual tile (include/ldn_hip.h:295-297) -- same result.  Rows the scatter does not name keep their contents."""
    rows, count, cin, dst_rows = 300, 257, 128, 420
    a = seeded_randn((rows, cin), 9)
    w = seeded_randn((cout, 1, cin), 10) * (2.0 / cin) ** 0.5
    sc, sh = _affine(cout, 11)
    g = torch.Generator().manual_seed(12)
    out_map = torch.randperm(dst_rows, generator=g)[:rows].to(torch.int32)
    ident = seeded_randn((dst_rows, cout), 13)
    wk, sk = (w * sc.view(-1, 1, 1), None) if prescaled else (w, sc)
    dst, val = packed_reference(a, wk, sk, sh, count, out_map=out_map, residual=ident, relu=1)
    want = ident.double().clone()
    want[dst] = val
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    alias = ident.clone().to(DEV)
    ops.conv_packed(_d(a), _d(wk), _d(sk), _d(sh), alias, B=1, m_count=cnt, m_cap=rows, taps=1, out_map=_d(out_map), relu=1, residual2d=alias)
    res = ident.clone().to(DEV)
    apart = torch.full((dst_rows, cout), NAN, device=DEV)
    ops.conv_packed(_d(a), _d(wk), _d(sk), _d(sh), apart, B=1, m_count=cnt, m_cap=rows, taps=1, out_map=_d(out_map), relu=1, residual2d=res)
    torch.cuda.synchronize()
    assert_close(alias, want, 2e-4, 1e-4, "aliased")
    untouched = torch.ones(dst_rows, dtype=torch.bool)
    untouched[dst] = False
    assert torch.equal(alias.cpu()[untouched], ident[untouched]) and bool(torch.isnan(apart.cpu()[untouched]).all())
    assert torch.equal(apart[_d(dst)], alias[_d(dst)]) and torch.equal(res.cpu(), ident)


def _neighbour_rows(B, Hi, Wi, Ho, Wo, stride):
    """[B*Ho*Wo, 9] flat input pixel of every tap (pad 1), -1 outside the image; and the 16-way border class of every output pixel."""
    b, oy, ox = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    b, oy, ox = b.reshape(-1), oy.reshape(-1), ox.reshape(-1)
    tab = torch.empty(B * Ho * Wo, 9, dtype=torch.int64)
    for t in range(9):
        iy, ix_ = oy * stride + t // 3 - 1, ox * stride + t % 3 - 1
        inside = (iy >= 0) & (iy < Hi) & (ix_ >= 0) & (ix_ < Wi)
        tab[:, t] = torch.where(inside, b * Hi * Wi + iy * Wi + ix_, torch.tensor(-1))
    top, bottom = (oy * stride - 1 < 0).long(), (oy * stride + 1 >= Hi).long()
    left, right = (ox * stride - 1 < 0).long(), (ox * stride + 1 >= Wi).long()
    return tab.to(torch.int32), (top | bottom << 1) * 4 + (left | right << 1)


@gpu
@pytest.mark.parametrize("taps", [1, 9])
def test_a_map_with_missing_rows(ops, taps, math_mode):
    """a_map entries of -1 read a zero row, for a 1-tap gather and through a 9-tap neighbour table (a random one: any row of `a` per tap)."""
    rows, src_rows, cin, cout = 260, 190, 64, 96
    a = seeded_randn((src_rows, cin), 14)
    w = seeded_randn((cout, taps, cin), 15) * (2.0 / (cin * taps)) ** 0.5
    sc, sh = _affine(cout, 16)
    g = torch.Generator().manual_seed(17)
    a_map = torch.randint(0, src_rows, (rows, taps), generator=g, dtype=torch.int32)
    a_map[torch.rand(rows, taps, generator=g) < 0.3] = -1
    a_map[5] = -1                                       # a row with no source at all: act(shift)
    a_map = a_map.reshape(-1).contiguous()
    out = torch.full((rows, cout), NAN, device=DEV)
    ops.conv_packed(_d(a), _d(w), _d(sc), _d(sh), out, B=1, m_cap=rows, a_map=_d(a_map), taps=taps, relu=1)
    torch.cuda.synchronize()
    _, want = packed_reference(a, w, sc, sh, rows, a_map=a_map)
    assert_close(out, want, 2e-4, 1e-4, f"{taps}-tap a_map with -1")
    assert_close(out[5], torch.relu(sh.double()), 1e-6, 0.0, "the all-missing row")


@gpu
@pytest.mark.parametrize("B,Hi,Wi,stride", [(2, 3, 3, 1), (1, 1, 7, 1), (2, 6, 6, 2), (1, 1, 1, 1)])
def test_border_class_shift_table(ops, B, Hi, Wi, stride, math_mode):
    """shift_classes == 16: row R takes shift[class(pix_map[R])], class = (top | bottom << 1) * 4 + (left | right << 1) of the taps that
    fall outside (include/ldn_hip.h:291-292,452).  On a 1 x N map every pixel is in the top AND the bottom class; on 3 x 3 the corners
    are in a row and a column class at once.  The packed rows list the pixels in a shuffled order, one row range per image."""
    Ho, Wo = Hi // stride, Wi // stride
    cin, cout = 32, 64
    a = seeded_randn((B * Hi * Wi, cin), 18)
    w = seeded_randn((cout, 9, cin), 19) * (2.0 / (9 * cin)) ** 0.5
    sc, _ = _affine(cout, 20)
    tab16 = seeded_randn((16, cout), 21)
    nbr, cls = _neighbour_rows(B, Hi, Wi, Ho, Wo, stride)
    if (Hi, Wi) == (1, 7):
        assert set(cls.tolist()) == {12 + 1, 12, 12 + 2}
    if (Hi, Wi) == (3, 3):
        assert set(cls.tolist()) == {0, 1, 2, 4, 5, 6, 8, 9, 10}
    if (Hi, Wi) == (1, 1):
        assert cls.tolist() == [15]
    g = torch.Generator().manual_seed(22)
    order = torch.cat([b * Ho * Wo + torch.randperm(Ho * Wo, generator=g) for b in range(B)])      # packed row R = output pixel order[R]
    a_map, pix_map = nbr[order].reshape(-1).contiguous(), order.to(torch.int32)
    prefix = (torch.arange(B + 1) * Ho * Wo).to(torch.int32)
    rows = B * Ho * Wo
    out = torch.full((rows, cout), NAN, device=DEV)
    ops.conv_packed(_d(a), _d(w), _d(sc), _d(tab16), out, B=B, row_prefix=_d(prefix), m_cap=Ho * Wo, a_map=_d(a_map), taps=9,
                    pix_map=_d(pix_map), geom=(Hi, Wi, Ho, Wo, stride), relu=0)
    torch.cuda.synchronize()
    _, want = packed_reference(a, w, sc, tab16, rows, a_map=a_map, cls=cls[order], relu=0)
    assert_close(out, want, 2e-4, 1e-4, "16-class shift table")


@gpu
def test_argument_checks_refuse_before_any_launch(ops):
    """The checks of ldn_conv_packed (csrc/ldn_conv_image.hip, ldn_conv_packed): an error code, and the output is not touched."""
    from laudnet_amd import LdnError
    rows, cin, cout, B = 64, 32, 32, 2
    a = torch.zeros(rows, cin, device=DEV)
    w = torch.zeros(cout, 1, cin, device=DEV)
    wk = torch.zeros(1, cin, cout, device=DEV)
    w9 = torch.zeros(cout, 9, cin, device=DEV)
    sh = torch.zeros(cout, device=DEV)
    out = torch.full((rows, cout), NAN, device=DEV)
    lists = torch.arange(cout, dtype=torch.int32, device=DEV).repeat(B, 1).contiguous()
    counts = torch.full((B,), cout, dtype=torch.int32, device=DEV)
    prefix = torch.tensor([0, 32, 64], dtype=torch.int32, device=DEV)
    nbr = torch.full((rows * 9,), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(LdnError):      # per-image channel lists without per-image row ranges
        ops.conv_packed(a, w, None, sh, out, B=1, m_cap=rows, n_idx=lists, n_cnt=counts)
    with pytest.raises(LdnError):
        ops.conv_packed(a, wk, None, sh, out, B=1, m_cap=rows, k_idx=lists, k_cnt=counts, kgran=1)
    with pytest.raises(LdnError):      # a residual with an output-channel list
        ops.conv_packed(a, w, None, sh, out, B=B, row_prefix=prefix, m_cap=32, n_idx=lists, n_cnt=counts, residual2d=out)
    with pytest.raises(LdnError):      # nine taps without a neighbour table
        ops.conv_packed(a, w9, None, sh, out, B=B, row_prefix=prefix, m_cap=32, taps=9)
    with pytest.raises(LdnError):      # a 16-class shift table without pix_map
        ops.conv_packed(a, w9, None, torch.zeros(16, cout, device=DEV), out, B=B, row_prefix=prefix, m_cap=32, a_map=nbr, taps=9,
                        geom=(8, 4, 8, 4, 1))
    with pytest.raises(LdnError):      # B > 1 without row ranges
        ops.conv_packed(a, w, None, sh, out, B=B, m_cap=32)
    with pytest.raises(LdnError):      # relu == 2 without its flags
        ops.conv_packed(a, w, None, sh, out, B=1, m_cap=rows, relu=2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call must not launch"
