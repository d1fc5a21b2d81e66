"""ldn_bottleneck_chain / ldn_bottleneck_chain_f32 called directly (ops.bottleneck_chain with tensors of the test's own), against its
parts and against float64.

The chained launch has three bodies (csrc/ldn_tail.hip: launch_chain): k_chain_ld<4|8> (bf16x3, widths 128 / 256, maps of at most 224
pixels: the loader / consumer form of csrc/ldn_chain_ld.h), k_chain<2|4|8> (bf16x3: width 64 on any map, widths 128 / 256 on maps of 225 to
256 pixels) and k_chain<2|4|8, F32>.  tests/test_hip_chain.py reaches them through whole 224-pixel models: 14 x 14 maps, bf16x3, logits.

`expected_chain_kernel` and `chain_fits` restate the dispatch and the LDS predicate in Python; non-GPU tests compare the predicate with the
library over a grid and prove that the case table runs all eight instantiations, both sides of the 224 / 225-pixel switch, the 65-pixel
minimum of ResNet._chain_len, non-square maps, one-layer maskers, granularity 4, runs of 1 / 2 / 5 blocks and 1 / 7 / 8 GAP splits.

Per case and arithmetic mode the GPU test requires
  * bit-identity of the run with ldn_channel_masker -> ldn_bottleneck_head -> ldn_bottleneck_tail block after block (include/ldn_hip.h:391):
    masks, counts, lists, every pixel of x_work, the final colsum;
  * every block's output within 2e-4 + 1e-4 |ref| of the float64 block (helpers.bottleneck_stages_f64) started from the kernel's own input
    and mask -- the bound of tests/test_hip_tail.py and tests/test_hip_packed.py for the same arithmetic;
  * the kernel's decisions equal to the float64 maskers' wherever the margin exceeds 1e-4 x max(max |logit|, 1) (the rule of
    tests/test_hip_ops.py::test_channel_masker), with at most 1 % of the decisions inside that margin.

Measured maximum |error| of the chain blocks per case and mode: docs/lab_notebook.md."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fill import seeded_randn
from helpers import apply_math_mode  # noqa: F401  (autouse fixture: a test that takes math_mode runs in that mode)
from helpers import assert_close, bottleneck_stages_f64
from oracle import index_ref as IR
from oracle import torch_ref as TR

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()  # raises if libldn_hip.so is missing -- no fallback
    return _ops


# ------------------------------------------------------------------ the dispatch rule and the LDS predicate, restated
T_KIDX_BYTES = 1280      # csrc/ldn_tail.hip:107
T_W2_SLOTS = 3           # :133
LDS_BYTES = 160 * 1024


def _round_up(a, b):
    return -(-a // b) * b


def chain_fits(H, Wd, C, width, hidden, G):
    """ldn_bottleneck_chain_fits (csrc/ldn_tail.hip:1734-1737) with chain_fits (:1655-1666): do the masker, conv1, conv2 and conv3 phases of a
    chained block fit the workgroup's 160 KiB of LDS, and the map the 72-piece slice pipeline?"""
    if H < 1 or Wd < 1 or H * Wd > 256 or C < 1 or G < 1 or hidden < 0 or width not in (64, 128, 256):
        return False
    NS = width // 32
    nr = H * Wd
    slice_bytes = _round_up((_round_up(nr, 8) + 1) * 128, 1024)
    lds2 = T_KIDX_BYTES + (1 if NS == 2 else 2) * slice_bytes + T_W2_SLOTS * 16 * NS * 256
    lds3 = T_KIDX_BYTES + 2 * (width // 2) * (32 if NS == 8 else 64) * 8 + 18 * width * 4 + 8 * 4096
    ldsm = (C + (hidden if hidden > 0 else 1) + 2 * G) * 4 + 64
    lds1 = T_KIDX_BYTES + 3 * width * 4 + 2 * (_round_up(nr, 32) + width) * 128
    return max(lds2, lds3, ldsm, lds1) <= LDS_BYTES and _round_up(nr, 8) // 8 <= 72


def expected_chain_kernel(H, Wd, width, f32):
    """The instantiation launch_chain runs (csrc/ldn_tail.hip:1668-1702, LDN_CHAIN_LD at its default): the loader / consumer form serves
    bf16x3 at widths 128 / 256 on maps that leave the eighth wave without pixels (at most 224), the plain body everything else."""
    NS = width // 32
    if not f32 and NS >= 4 and H * Wd <= 224:
        return f"k_chain_ld<{NS}>"
    return f"k_chain<{NS}, F32>" if f32 else f"k_chain<{NS}>"


ALL_KERNELS = {"k_chain_ld<4>", "k_chain_ld<8>", "k_chain<2>", "k_chain<4>", "k_chain<8>", "k_chain<2, F32>", "k_chain<4, F32>", "k_chain<8, F32>"}

# (B, H, Wd, width, channel granularity, masker layers, blocks in the run, splits of gap_in); C = 4 * width
CASES = [
    (8, 14, 14, 256, 2, 2, 5, 8),     # stage 3 of ResNet-101: k_chain_ld<8>, a run of five
    (3, 14, 14, 128, 2, 2, 2, 7),     # k_chain_ld<4>; an odd number of GAP splits
    (5, 14, 14, 64, 2, 1, 2, 1),      # k_chain<2>; one-layer masker; one GAP split; DOMINANT
    (2, 15, 15, 256, 2, 2, 2, 8),     # 225 pixels (a 240-pixel input): the plain k_chain<8> in bf16x3
    (9, 15, 15, 128, 4, 2, 1, 7),     # the plain k_chain<4>; granularity 4; a run of one; a batch that is not a multiple of 8
    (3, 15, 15, 64, 2, 2, 2, 1),
    (4, 16, 14, 256, 2, 1, 2, 8),     # 224 pixels: the last map of the loader / consumer form; one-layer masker; DOMINANT
    (1, 9, 20, 128, 2, 2, 2, 7),      # non-square, a single image
    (3, 12, 20, 256, 2, 2, 2, 1),     # non-square, 240 pixels: 163 072 of the 163 840 bytes of LDS in the conv2 phase
    (4, 5, 13, 128, 2, 2, 2, 8),      # 65 pixels: the smallest map ResNet._chain_len admits
    (3, 5, 13, 256, 4, 1, 1, 7),      # ... at width 256, granularity 4, one layer, a run of one
    (3, 16, 16, 128, 2, 2, 2, 8),     # 256 pixels: the largest map (does not fit at width 256)
    (2, 16, 16, 64, 4, 1, 5, 7),      # ... at width 64: a run of five, granularity 4, one layer
]
# one-layer cases in which a dedicated input channel, large in image 0 only, dominates the masker: image 0 keeps NO channel in block 0 and
# EVERY channel in block 1
DOMINANT = {CASES[2], CASES[6]}
DOM_CHANNEL, DOM_VALUE, DOM_WEIGHT = 5, 20.0, 8.0
MODES = ("fp32", "bf16x3")


def _hidden(case):
    width, gran, layers = case[3], case[4], case[5]
    return max((width // gran) // 16, 16) if layers == 2 else 0       # Masker_channel_MLP: max(groups // reduction, 16)


def test_chain_fits_restated_equals_the_library():
    """The transcription against ldn_bottleneck_chain_fits (the library loads without a GPU) over H, Wd in 1..20 and the thin maps, the three
    widths and a few (C, hidden, G) -- and the boundaries written out."""
    from laudnet_amd import ops
    maps = [(h, w) for h in range(1, 21) for w in range(1, 21)] + [(1, 65), (1, 256), (256, 1), (3, 75), (1, 257), (257, 1)]
    n_fit = n_not = 0
    for width in (64, 128, 256):
        shapes = [(4 * width, 16, width // 2), (4 * width, 0, width // 2), (4 * width, 16, width // 4), (4 * width, 0, width // 4),
                  (40000, 16, 128), (40960, 0, 128)]      # the last one: the masker's vectors alone exceed the LDS
        for H, Wd in maps:
            for C, hidden, G in shapes:
                want = chain_fits(H, Wd, C, width, hidden, G)
                assert ops.bottleneck_chain_fits(H, Wd, C, width, hidden, G) == want, (H, Wd, C, width, hidden, G)
                n_fit += want
                n_not += not want
    assert n_fit > 1000 and n_not > 1000
    fits = lambda H, Wd, width: ops.bottleneck_chain_fits(H, Wd, 4 * width, width, 16, width // 2)
    assert fits(16, 16, 64) and fits(16, 16, 128) and not fits(16, 16, 256)
    for width in (64, 128, 256):
        assert fits(15, 15, width) and fits(12, 20, width) and fits(16, 14, width) and fits(5, 13, width)
        assert not fits(1, 257, width) and not fits(257, 1, width)
        assert chain_fits(14, 14, 40000, width, 16, 128) and not chain_fits(14, 14, 40960, width, 0, 128)
    assert not ops.bottleneck_chain_fits(14, 14, 1024, 96, 16, 48)         # a width the kernels are not built for


def test_case_table_reaches_every_instantiation():
    """The case table runs all eight instantiations of launch_chain and both sides of every switch named in this file's header."""
    seen = {}
    for case in CASES:
        B, H, Wd, width, gran, layers, nblocks, splits = case
        assert chain_fits(H, Wd, 4 * width, width, _hidden(case), width // gran), case
        assert 64 < H * Wd <= 256 and B <= 9 and nblocks <= 6                     # what ResNet._chain_len admits; small enough for float64 on the CPU
        assert width % gran == 0 and gran % 2 == 0
        for mode in MODES:
            seen.setdefault(expected_chain_kernel(H, Wd, width, mode == "fp32"), []).append(case)
    assert set(seen) == ALL_KERNELS, f"missing {sorted(ALL_KERNELS - set(seen))}"
    px = lambda k: {c[1] * c[2] for c in seen[k]}
    assert 224 in px("k_chain_ld<8>")                                                 # the last map of the loader / consumer form
    for ns in (4, 8):
        assert max(px(f"k_chain_ld<{ns}>")) <= 224
        assert 225 in px(f"k_chain<{ns}>") and min(px(f"k_chain<{ns}>")) >= 225       # plain body in bf16x3: only past the switch
        assert 196 in px(f"k_chain_ld<{ns}>") and 65 in px(f"k_chain_ld<{ns}>")
    assert expected_chain_kernel(16, 14, 256, False) == "k_chain_ld<8>" and expected_chain_kernel(15, 15, 256, False) == "k_chain<8>"
    assert expected_chain_kernel(16, 14, 128, False) == "k_chain_ld<4>" and expected_chain_kernel(15, 15, 128, False) == "k_chain<4>"
    assert expected_chain_kernel(14, 14, 64, False) == "k_chain<2>" and expected_chain_kernel(14, 14, 256, True) == "k_chain<8, F32>"
    col = lambda i: {c[i] for c in CASES}
    for width in (64, 128, 256):
        assert {(14, 14), (15, 15)} <= {(c[1], c[2]) for c in CASES if c[3] == width}
    maps = {(c[1], c[2]) for c in CASES}
    assert {(16, 14), (9, 20), (12, 20), (5, 13)} <= maps and (16, 16, 128) in {(c[1], c[2], c[3]) for c in CASES}
    assert {1, 8, 9} <= col(0)                                                        # one image, the XCD count, not a multiple of it
    assert {1, 2} <= col(6) and max(col(6)) >= 5
    assert col(5) == {1, 2} and {2, 4} <= col(4)
    assert {1, 7, 8} <= col(7)
    for case in DOMINANT:
        assert case[5] == 1 and case[6] >= 2 and case[0] >= 3


# ------------------------------------------------------------------ the run: blocks, input, GAP partials (CPU, seeded)
def _case_seed(case):
    return 1000 + 37 * CASES.index(case)


@functools.lru_cache(maxsize=None)
def build_run(case):
    """-> (reference blocks [nblocks] (float32 BottleneckRef, channel mode), x [B,C,H,Wd], gap_in [B,splits,C]).  He-scaled seeded conv
    weights, TR.randomize_bn_ statistics, bn3.weight x 0.3 (the residual stream stays O(1) over the run, as in tests/test_hip_chain.py),
    seeded N(0,1) masker weights and N(0, 0.5) masker biases.  gap_in: sums of x over `splits` disjoint pixel sets covering the image
    (a seeded random assignment of pixels to sets; include/ldn_hip.h:396 admits any producer)."""
    B, H, Wd, width, gran, layers, nblocks, splits = case
    C, G = 4 * width, width // gran
    seed = _case_seed(case)
    blocks = []
    for i in range(nblocks):
        blk = TR.BottleneckRef(C, width, stride=1, downsample=None, dyn_mode="channel", channel_dyn_granularity=gran,
                               channel_masker="MLP", channel_masker_layers=layers, output_size=H).eval()
        TR.randomize_bn_(blk, seed + i)
        g = torch.Generator().manual_seed(seed + 100 + i)
        with torch.no_grad():
            for m in (blk.conv1, blk.conv2, blk.conv3):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            blk.bn3.weight.mul_(0.3)
            for prm in blk.masker_channel.parameters():
                prm.copy_(torch.randn(prm.shape, generator=g) * (1.0 if prm.dim() == 2 else 0.5))
            if case in DOMINANT and i < 2:
                sign = -1.0 if i == 0 else 1.0          # block 0: the channel votes every group out; block 1: every group in
                blk.masker_channel.conv.weight[:G, DOM_CHANNEL] = sign * DOM_WEIGHT
                blk.masker_channel.conv.weight[G:, DOM_CHANNEL] = -sign * DOM_WEIGHT
        blocks.append(blk)
    x = F.relu(seeded_randn((B, C, H, Wd), seed + 7))
    if case in DOMINANT:
        x[:, DOM_CHANNEL] = 0.0
        x[0, DOM_CHANNEL] = DOM_VALUE
    g = torch.Generator().manual_seed(seed + 9)
    assign = torch.randint(splits, (H * Wd,), generator=g)
    assign[:splits] = torch.arange(splits)                  # every set holds a pixel
    gap = torch.zeros(B, splits, C).index_add_(1, assign, x.permute(0, 2, 3, 1).reshape(B, H * Wd, C).contiguous())
    return blocks, x, gap


def masker_logits_f64(blk, mean):
    """Masker_channel_MLP's logits (models/utils.py:92-131) from the channel means [B,C], in float64: [B,2,G]."""
    with torch.no_grad():
        conv = blk.masker_channel.conv
        lin = (lambda l, v: v @ l.weight.double().t() + l.bias.double())
        z = lin(conv, mean) if isinstance(conv, torch.nn.Linear) else lin(conv[2], torch.relu(lin(conv[0], mean)))
    return z.reshape(mean.shape[0], 2, -1)


def decision_margin(logits):
    """(float64 decision [B,G], bool [B,G]: the margin is at most 1e-4 x max(max |logit|, 1) -- the decisions a float32 masker may take
    the other way, tests/test_hip_ops.py::test_channel_masker)."""
    scale = max(float(logits.abs().max()), 1.0)
    return (logits[:, 0] >= logits[:, 1]).double(), (logits[:, 0] - logits[:, 1]).abs() <= 1e-4 * scale


def block_f64(blk64, x, mask):
    B, _, H, Wd = x.shape
    return bottleneck_stages_f64(blk64, x, mask, torch.ones(B, 1, H, Wd, dtype=torch.float64))[4]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_reference_run_decides_for_real(case):
    """Preconditions of the GPU test, on the float64 reference alone (the whole run in float64, each block deciding for itself): at most 1 %
    of the (block, image, group) decisions lie inside the margin the GPU test leaves to the kernel, the mean keep rate lies in (0.3, 0.85),
    and in the DOMINANT cases image 0 keeps no channel in block 0 and every channel in block 1."""
    B, H, Wd, width, gran, layers, nblocks, splits = case
    blocks, x, gap = build_run(case)
    assert torch.allclose(gap.sum(1).double(), x.double().sum(dim=(2, 3)), rtol=1e-5, atol=1e-3) and gap.shape == (B, splits, 4 * width)
    xi = x.double()
    mean = gap.double().sum(1) / (H * Wd)
    near = kept = total = 0
    for i, blk in enumerate(blocks):
        blk64 = TR.BottleneckRef(4 * width, width, stride=1, downsample=None, dyn_mode="channel", channel_dyn_granularity=gran,
                                 channel_masker="MLP", channel_masker_layers=layers, output_size=H).eval().double()
        blk64.load_state_dict(blk.state_dict())
        mask, close = decision_margin(masker_logits_f64(blk64, mean))
        near += int(close.sum())
        kept += float(mask.sum())
        total += mask.numel()
        if case in DOMINANT and i == 0:
            assert float(mask[0].sum()) == 0 and float(mask[1:].sum()) > 0
        if case in DOMINANT and i == 1:
            assert float(mask[0].sum()) == mask.shape[1] and float(mask[1:].mean()) < 1
        xi = block_f64(blk64, xi, mask)
        mean = xi.mean(dim=(2, 3))
    assert near <= 0.01 * total, f"{near} of {total} decisions inside the margin"
    assert 0.3 < kept / total < 0.85, f"keep rate {kept / total:.3f}"
    assert float(xi.abs().max()) < 100 and float(xi.mean()) > 0.05          # the residual stream stays O(1)


# ------------------------------------------------------------------ GPU: the run against its parts and against float64
def _hip_blocks(case, blocks):
    from laudnet_amd.laud_resnet import Bottleneck
    B, H, Wd, width, gran, layers, nblocks, splits = case
    out = []
    for blk in blocks:
        hb = Bottleneck(4 * width, width, stride=1, downsample=None, dyn_mode="channel", channel_dyn_granularity=gran,
                        channel_masker="MLP", channel_masker_layers=layers, output_size=H).eval()
        hb.load_state_dict(blk.state_dict())
        out.append(hb.to(DEV))
    return out


def _table_rows(hbs):
    """The rows of ops.chain_table exactly as ResNet._run_chain builds them (laudnet_amd/laud_resnet.py: _run_chain), under the mode in force."""
    rows = []
    for hb in hbs:
        p = hb._prepare(torch.device(DEV))
        mw = hb.masker_channel._weights()
        w2p, w3p = hb.tail_weights(p)
        rows.append((p[hb._w1s_key()], p["s1"], p["t1"], p["c1"], w2p, w3p, p["s2"], p["t2_tab"], p["c2"], p["t3c"], mw[0], mw[1], mw[2], mw[3]))
    return rows


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_chain_equals_its_parts_and_float64(ops, case, math_mode):
    B, H, Wd, width, gran, layers, nblocks, splits = case
    C, G, HW = 4 * width, width // gran, H * Wd
    hidden = _hidden(case)
    f32 = math_mode == "fp32"
    kernel = expected_chain_kernel(H, Wd, width, f32)
    blocks, x, gap_cpu = build_run(case)
    hbs = _hip_blocks(case, blocks)
    rows = _table_rows(hbs)
    for r in rows:
        assert r[0].dtype == r[4].dtype == r[5].dtype == (torch.float32 if f32 else torch.bfloat16)     # the mode's own weight layouts
        assert (r[12] is None) == (r[13] is None) == (layers == 1)
        assert r[10].shape == ((2 * G, C) if layers == 1 else (hidden, C))
    table = ops.chain_table(rows, DEV)
    assert ops.bottleneck_chain_fits(H, Wd, C, width, hidden, G) and ops.bottleneck_tail_splits(H, Wd, width, 1) == 8
    xin = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    gap = gap_cpu.to(DEV)
    keep = xin.clone()
    ops.plan_timeouts(reset=True)

    # ---- the run, out of place (x_work starts as NaN), in place, and again
    work = torch.full_like(xin, NAN)
    masks, idx, cnt, colsum = ops.bottleneck_chain(xin, work, table, width, hidden, G, gran, gap, f32=f32)
    torch.cuda.synchronize()
    assert torch.equal(xin, keep), "x_in must stay intact when x_work is a separate tensor"
    assert tuple(masks.shape) == (nblocks, B, G) and tuple(idx.shape) == (nblocks, B, width) and tuple(cnt.shape) == (nblocks, B)
    assert tuple(colsum.shape) == (B, 8, C) and not bool(torch.isnan(work).any())
    inpl = keep.clone()
    masks_i, idx_i, cnt_i, colsum_i = ops.bottleneck_chain(inpl, inpl, table, width, hidden, G, gran, gap, f32=f32)
    work2 = torch.full_like(xin, NAN)
    masks_2, idx_2, cnt_2, colsum_2 = ops.bottleneck_chain(xin, work2, table, width, hidden, G, gran, gap, f32=f32)
    torch.cuda.synchronize()
    for what, got in (("in place", (inpl, masks_i, idx_i, cnt_i, colsum_i)), ("second run", (work2, masks_2, idx_2, cnt_2, colsum_2))):
        assert torch.equal(got[0], work), f"{what}: x_work differs"
        assert torch.equal(got[1], masks) and torch.equal(got[3], cnt) and torch.equal(got[4], colsum), f"{what}: masks / counts / colsum differ"
        for i in range(nblocks):
            for b in range(B):
                n = int(cnt[i, b])
                assert torch.equal(got[2][i, b, :n], idx[i, b, :n]), f"{what}: list of block {i}, image {b}"
    if "k_chain_ld" in kernel:
        assert ops.plan_timeouts() == 0, "a hand-off wait of the loader / consumer form ran into its bound"

    # ---- the same run block by block through the stand-alone entry points: bit-identical
    xs = [xin]                      # the float32 input of every block, then the run's output
    gap_i = gap
    for i, r in enumerate(rows):
        mk, ix, ct, _ = ops.channel_masker(None, r[10], r[11], r[12], r[13], G, gran, gap_partial=gap_i, hw=HW)
        assert torch.equal(mk, masks[i]), f"block {i}: the chain's mask differs from ldn_channel_masker's"
        assert torch.equal(ct, cnt[i]), f"block {i}: counts differ"
        for b in range(B):
            n = int(ct[b])
            assert torch.equal(ix[b, :n], idx[i, b, :n]), f"block {i}, image {b}: channel lists differ"
        h1 = torch.full((B, H, Wd, width), NAN, device=DEV)
        ops.bottleneck_head(xs[-1], r[0], ix, ct, r[1], r[2], r[3], h1)
        out = torch.full_like(xin, NAN)
        cs = torch.full((B, 8, C), NAN, device=DEV)
        ops.bottleneck_tail(h1, r[4], r[5], ix, ct, r[6], r[7], r[8], r[9], out, residual=xs[-1], colsum=cs)
        xs.append(out)
        gap_i = cs
    torch.cuda.synchronize()
    diff = (xs[-1] - work).abs().max().item()
    assert torch.equal(xs[-1], work), f"x_work after the run differs from the block-by-block execution (max {diff:.3e})"
    assert torch.equal(gap_i, colsum), "the final colsum differs from the last stand-alone tail's"

    # ---- every block against float64, from the kernel's own input and mask; the decisions against the float64 maskers
    masks_c, cnt_c, idx_c = masks.cpu(), cnt.cpu().numpy(), idx.cpu().numpy()
    near = total = 0
    worst = 0.0
    for i, blk in enumerate(blocks):
        blk64 = TR.BottleneckRef(C, width, stride=1, downsample=None, dyn_mode="channel", channel_dyn_granularity=gran,
                                 channel_masker="MLP", channel_masker_layers=layers, output_size=H).eval().double()
        blk64.load_state_dict(blk.state_dict())
        x_i = xs[i].cpu().permute(0, 3, 1, 2).double()
        mean = gap_cpu.double().sum(1) / HW if i == 0 else x_i.mean(dim=(2, 3))
        want_mask, close = decision_margin(masker_logits_f64(blk64, mean))
        wrong = (masks_c[i].double() != want_mask) & ~close
        assert not bool(wrong.any()), f"block {i}: {int(wrong.sum())} decisions differ from the float64 masker outside the margin"
        near += int(close.sum())
        total += close.numel()
        widx, wcnt = IR.channel_lists(masks_c[i].numpy(), width)
        assert np.array_equal(cnt_c[i], wcnt), f"block {i}: counts are not those of the mask"
        for b in range(B):
            assert np.array_equal(idx_c[i, b, :wcnt[b]], widx[b, :wcnt[b]]), f"block {i}, image {b}: the list is not that of the mask"
        want = block_f64(blk64, x_i, masks_c[i].double()).permute(0, 2, 3, 1)
        worst = max(worst, assert_close(xs[i + 1], want, 2e-4, 1e-4, f"block {i} of {kernel}"))
    assert near <= 0.01 * total, f"{near} of {total} decisions inside the margin"
    keep_rate = float(masks_c.mean())
    assert 0.3 < keep_rate < 0.85, f"keep rate {keep_rate:.3f}: the maskers must be making real decisions"
    if case in DOMINANT:
        assert int(cnt_c[0, 0]) == 0 and int(cnt_c[0, 1:].min()) > 0, "image 0 must keep no channel in block 0"
        assert int(cnt_c[1, 0]) == width and int(cnt_c[1, 1:].min()) < width, "image 0 must keep every channel in block 1"
    out64 = work.cpu().double()
    assert torch.allclose(colsum.sum(1).cpu().double(), out64.sum(dim=(1, 2)), atol=1e-2, rtol=1e-5)
    print(f"\n[chain] {'x'.join(map(str, case))} {math_mode:6s} {kernel:16s} keep {keep_rate:.3f} near {near}/{total} max|err| {worst:.2e}")
