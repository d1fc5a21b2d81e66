"""-m gpu: the fp32 VALU kernels of csrc/ldn_regnet.hip and the two small bookkeeping kernels, op by op against float64.

ldn_grouped_conv3x3_rows (k_grouped3x3_lds<8/16/24>, k_grouped3x3_rows<0>), ldn_grouped_conv3x3_image (k_grouped3x3_chan), ldn_se_packed
(k_rows_gap, k_se_head, k_rows_scale), ldn_forward_stats and ldn_coarsen_cell_means are otherwise reached only from inside a whole
LAD-RegNet / ResNet forward, whose logits average a border or last-column error away.  Every reference is plain PyTorch on the CPU in
float64, written from the operation's definition (include/ldn_hip.h:276-283,464-500; laud_regnet.py:119-123,157-217).

Bounds: fp32 VALU convolutions and the cell means 1e-4 + 1e-4 |ref| (as test_grouped16_conv3x3_* against float64); SE gate 1e-5
absolute, scaled rows 1e-4 max(1, |ref|max) (as tests/test_hip_se_fused.py); forward_stats 1e-6 relative on perc / st_out, 1e-5 on flops."""
import pytest
import torch
import torch.nn.functional as F

from fill import seeded_bernoulli, seeded_randn
from helpers import assert_close, se_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()  # raises if libldn_hip.so is missing -- no fallback
    return _ops


def _affine(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1


def _grouped_weight(C, gw, seed):
    """conv weight [C, gw, 3, 3] (He-normal) and its kernel layout [C, 9, gw]."""
    w = seeded_randn((C, gw, 3, 3), seed) * (2.0 / (9 * gw)) ** 0.5
    return w, w.permute(0, 2, 3, 1).reshape(C, 9, gw).contiguous()


# ------------------------------------------------------------------ grouped 3x3 over packed rows
def _rows_grid_caps_bite(m_cap, C, gw):
    """Does the launch of ldn_grouped_conv3x3_rows cap its grid (csrc/ldn_regnet.hip:313-314 generic, :321-324 LDS variants), so that
    every workgroup walks several row blocks?"""
    if gw in (8, 16, 24):
        rows_per_block = 256 // (gw // 4)
        return -(-m_cap // rows_per_block) > (256 * 16) // (C // gw) + 1
    return -(-(m_cap * (C // 4)) // 256) > 256 * 32


ROWS_CASES = [
    # gw, C, B, Ho, Wo, stride, keep
    (8, 8, 3, 14, 14, 1, 0.5), (8, 64, 3, 14, 10, 2, 0.5),           # k_grouped3x3_lds<8>: one group, many groups
    (16, 16, 3, 14, 14, 2, 0.5), (16, 64, 2, 28, 28, 1, 0.4),        # <16>
    (24, 24, 3, 14, 14, 1, 0.5), (24, 144, 3, 9, 14, 2, 0.6),        # <24>: 6 channel quads, 252 of 256 threads
    (4, 4, 3, 14, 14, 1, 0.5), (4, 32, 3, 14, 14, 2, 0.5),           # the generic kernel
    (12, 12, 3, 7, 7, 1, 0.5), (12, 48, 3, 14, 14, 2, 0.5),
    (56, 56, 3, 14, 14, 1, 0.5), (56, 448, 2, 14, 14, 2, 0.5),       # RegNetY-8GF
    # row counts past the grid caps
    (8, 128, 12, 56, 56, 1, 0.8), (16, 256, 6, 56, 56, 1, 0.8), (24, 384, 4, 56, 56, 1, 0.8), (56, 448, 6, 56, 56, 1, 0.85),
]


@pytest.mark.parametrize("gw,C,B,Ho,Wo,stride,keep", ROWS_CASES)
def test_grouped_conv3x3_rows(ops, gw, C, B, Ho, Wo, stride, keep):
    """out[r] = relu(scale * grouped3x3(a)[pixel idx3[r]] + shift) for the kept pixels of a Bernoulli pixel mask; the input rows are the
    dilated list's (everything else NaN), lda > C and ldo > C, a device-side count below the capacity with NaN behind it."""
    Hi, Wi = Ho * stride, Wo * stride
    big = B * Ho * Wo > 10000
    assert _rows_grid_caps_bite(B * Ho * Wo, C, gw) == big
    seed = 1000 + 7 * gw + C + stride
    mask = seeded_bernoulli((B, Ho // 2 if big else Ho, Wo // 2 if big else Wo), keep, seed)
    mask[0, 0, 0] = 1.0                     # a corner, an edge and its neighbour: every border class of the neighbour table
    mask[0, 0, 1] = 1.0
    mask[0, -1, -1] = 1.0
    x = torch.relu(seeded_randn((B, C, Hi, Wi), seed + 1))
    w, wk = _grouped_weight(C, gw, seed + 2)
    sc, sh = _affine(C, seed + 3)
    ix = ops.mask_to_index(mask.to(DEV), Ho, Wo, stride)
    torch.cuda.synchronize()
    n3, n1 = int(ix.cnt[0]), int(ix.cnt[1])
    assert 0 < n3 < ix.cap3, "the device-side count must be below the capacity"
    lda, ldo = C + 8, C + 4
    x2d = x.permute(0, 2, 3, 1).reshape(B * Hi * Wi, C)
    a = torch.full((ix.cap1, lda), NAN)
    a[:n1, :C] = x2d[ix.idx1[:n1].cpu().long()]
    out = torch.full((ix.cap3, ldo), NAN, device=DEV)
    ops.grouped_conv3x3_rows(a.to(DEV), ix.nbr, wk.to(DEV), gw, sc.to(DEV), sh.to(DEV), out, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)
    torch.cuda.synchronize()
    want = F.conv2d(x.double(), w.double(), padding=1, stride=stride, groups=C // gw)
    want = torch.relu(want * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    want = want.permute(0, 2, 3, 1).reshape(B * Ho * Wo, C)[ix.idx3[:n3].cpu().long()]
    got = out.cpu()
    err = assert_close(got[:n3, :C], want, 1e-4, 1e-4, f"gw {gw} C {C}")
    assert bool(torch.isnan(got[:n3, C:]).all()), "columns >= C of the output rows were written"
    assert bool(torch.isnan(got[n3:]).all()), "rows >= *m_count were written"
    print(f"[regnet rows] gw {gw} C {C} rows {n3}: max |err| {err:.2e}")


# ------------------------------------------------------------------ grouped 3x3 on per-image channel subsets
def _subset_mask(B, C, gw, gran, seed):
    """[B, C / gran] granule mask: image 0 nothing, image 1 everything, image 2 with group 0 wholly inactive, image 3 with exactly one
    active GRANULE in the last group -- a single active channel in the granularity-1 rows of the table (one per group width), a pair at
    granularity 2, the whole group where the granule is the group; Bernoulli draws elsewhere."""
    gm = seeded_bernoulli((B, C // gran), 0.6, seed)
    per_group = gw // gran
    gm[0] = 0.0
    gm[1] = 1.0
    gm[2, :per_group] = 0.0
    gm[3, -per_group:] = 0.0
    gm[3, -1 if per_group == 1 else -2] = 1.0
    return gm


IMAGE_CASES = [
    # gw, C, gran, B, Hi, Wi, stride
    (8, 64, 1, 5, 7, 7, 1), (8, 64, 2, 4, 9, 5, 1), (8, 32, 8, 4, 14, 14, 2),
    (16, 64, 1, 4, 9, 7, 2), (16, 128, 2, 5, 7, 7, 1), (16, 64, 16, 4, 14, 10, 2),
    (24, 144, 1, 4, 7, 7, 1), (24, 72, 2, 5, 9, 7, 2), (24, 96, 24, 4, 5, 14, 1),
    (56, 112, 1, 4, 7, 5, 1), (56, 448, 2, 4, 7, 7, 2), (56, 224, 56, 5, 9, 9, 1),
]


@pytest.mark.parametrize("gw,C,gran,B,Hi,Wi,stride", IMAGE_CASES)
def test_grouped_conv3x3_image(ops, gw, C, gran, B, Hi, Wi, stride):
    """Channel mode (laud_regnet.py:160-189): the dense grouped conv of the input with masked channels as exact zeros, read at the
    image's active output channels; left-packed columns in, left-packed columns out, zeros behind the count."""
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    seed = 2000 + 5 * gw + C + gran + stride
    gm = _subset_mask(B, C, gw, gran, seed)
    chan = gm.repeat_interleave(gran, dim=1) > 0.5                  # [B, C]
    n = chan.sum(dim=1).tolist()
    per_group = chan.view(B, C // gw, gw).sum(dim=2)
    assert n[0] == 0 and n[1] == C
    assert per_group[2, 0] == 0 and n[2] > 0, "image 2: a whole group inactive"
    assert per_group[3, -1] == gran and n[3] > gran, "image 3: one active granule (gran channels) in its last group"
    if gran == 1:
        assert per_group[3, -1] == 1 and gw > 1, "granularity 1: a single active channel in a group"
    x = torch.relu(seeded_randn((B, C, Hi, Wi), seed + 1))
    w, wk = _grouped_weight(C, gw, seed + 2)
    sc, sh = _affine(C, seed + 3)
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, C // gran, gran, mask_in=gm.to(DEV))
    torch.cuda.synchronize()
    cidx = idx.cpu().long()
    assert cnt.cpu().tolist() == n
    a = torch.full((B, Hi, Wi, C), NAN)
    for b in range(B):
        assert torch.equal(cidx[b, :n[b]], torch.nonzero(chan[b]).reshape(-1))
        a[b, :, :, :n[b]] = x[b, cidx[b, :n[b]]].permute(1, 2, 0)
    out = torch.full((B, Ho, Wo, C), NAN, device=DEV)
    ops.grouped_conv3x3_image(a.to(DEV), wk.to(DEV), gw, idx, cnt, sc.to(DEV), sh.to(DEV), out, stride=stride, relu=1)
    torch.cuda.synchronize()
    xm = x.double() * chan.view(B, C, 1, 1)
    want = F.conv2d(xm, w.double(), padding=1, stride=stride, groups=C // gw)        # (g0 = group * gw: each group reads ITS channels)
    want = torch.relu(want * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    assert tuple(want.shape[2:]) == (Ho, Wo)
    got = out.cpu()
    err = 0.0
    for b in range(B):
        err = max(err, assert_close(got[b, :, :, :n[b]], want[b, cidx[b, :n[b]]].permute(1, 2, 0), 1e-4, 1e-4, f"image {b}"))
        assert bool((got[b, :, :, n[b]:] == 0).all()), f"image {b}: columns >= ch_cnt must be exactly zero"
    print(f"[regnet image] gw {gw} C {C} gran {gran}: max |err| {err:.2e}")


# ------------------------------------------------------------------ squeeze-excitation over packed rows
SE_CASES = [
    # C, S, rows per image:   k_rows_gap layouts C/4 >= 256 | 256 % (C/4) != 0 | C/4 divides 256;  k_se_head fc2 tails 16 / 8 / 1
    (64, 8, 3136), (320, 80, 196), (784, 196, 49), (1024, 14, 196), (1296, 20, 49), (1296, 196, 196), (64, 14, 49), (320, 20, 3136),
]


def _se_weights(C, S, seed):
    return (seeded_randn((S, C), seed) * (1.0 / C) ** 0.5, seeded_randn((S,), seed + 1) * 0.1,
            seeded_randn((C, S), seed + 2) * (1.0 / S) ** 0.5, seeded_randn((C,), seed + 3) * 0.1)


def _se_prefix(rows):
    counts = [rows, rows // 2 + 1, 0, rows, 3]                 # unequal, an empty image in the middle
    pre = [0]
    for c in counts:
        pre.append(pre[-1] + c)
    return counts, pre


@pytest.mark.parametrize("C,S,rows", SE_CASES)
@pytest.mark.parametrize("lists", [False, True], ids=["dense", "lists"])
def test_se_packed(ops, C, S, rows, lists):
    """torchvision SqueezeExcitation in place on every image's packed rows: mean over the image's rows -> fc1 -> ReLU -> fc2 -> sigmoid ->
    multiply.  The first row of every image is all ones, so that row of the result IS the gate.  With channel lists the columns are the
    image's active channels and the weights are gathered through the list."""
    counts, pre = _se_prefix(rows)
    B, total = len(counts), pre[-1]
    assert pre[2] == pre[3] and 0 < 2 < B - 1 and len(set(counts)) > 2
    seed = 3000 + C + S + rows
    w1, b1, w2, b2 = _se_weights(C, S, seed)
    lda = C + 4
    base = torch.full((total + 5, lda), 7.0)
    base[:total, :C] = torch.relu(seeded_randn((total, C), seed + 4))
    for b in range(B):
        if counts[b]:
            base[pre[b], :C] = 1.0
    idx = cnt = None
    chans = [torch.arange(C)] * B
    if lists:
        gm = seeded_bernoulli((B, C // 4), 0.6, seed + 5)
        gm[0] = 0.0                                              # an image without a channel: its rows stay all zero
        gm[1] = 1.0
        _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, C // 4, 4, mask_in=gm.to(DEV))
        torch.cuda.synchronize()
        n = cnt.cpu().tolist()
        assert n[0] == 0 and n[1] == C and all(0 < v < C for v in n[2:])
        chans = [idx.cpu()[b, :n[b]].long() for b in range(B)]
        for b in range(B):
            base[pre[b]:pre[b + 1], n[b]:C] = 0.0                # columns behind the count are zeros (what conv b leaves)
    prefix = torch.tensor(pre, dtype=torch.int32, device=DEV)
    runs = []
    for _ in range(2):
        a = base.clone().to(DEV)
        ops.se_packed(a, prefix, w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), rows, ch_idx=idx, ch_cnt=cnt)
        torch.cuda.synchronize()
        runs.append(a.cpu())
    got = runs[0]
    assert torch.equal(runs[0], runs[1]), "two launches on the same input differ: the additions are not in a fixed order"
    assert not bool(torch.isnan(got).any())
    assert bool((got[:, C:] == 7.0).all()) and bool((got[total:] == 7.0).all()), "columns >= C / rows past the last image were written"
    gate_err = row_err = 0.0
    for b in range(B):
        if counts[b] == 0:
            continue
        ch, k = chans[b], len(chans[b])
        rows_b = base[pre[b]:pre[b + 1], :k]
        gate, want = se_f64(rows_b, w1[:, ch], b1, w2[ch], b2[ch])
        got_b = got[pre[b]:pre[b + 1]]
        assert bool((got_b[:, k:C] == 0).all()), f"image {b}: columns behind its channel count must stay zero"
        if k == 0:
            continue
        gerr = (got_b[0, :k].double() - gate).abs().max().item()
        rerr = (got_b[:, :k].double() - want).abs().max().item()
        assert gerr < 1e-5, f"image {b} ({counts[b]} rows, {k} channels): gate off by {gerr:.3e}"
        assert rerr < 1e-4 * max(1.0, want.abs().max().item()), f"image {b}: scaled rows off by {rerr:.3e}"
        gate_err, row_err = max(gate_err, gerr), max(row_err, rerr)
    print(f"[regnet se] C {C} S {S} rows {rows} lists {lists}: max gate err {gate_err:.2e}, rows {row_err:.2e}")


# ------------------------------------------------------------------ the FLOPs bookkeeping of a forward
def _stats_reference(terms, static, st, cs_cnt=None):
    """include/ldn_hip.h:276-283 in float64.  st [n, 4] = (s3, s2, s1, cs) after the channel counts have replaced cs."""
    s3, s2, s1, cs = (st[:, i].double() for i in range(4))
    t = terms.double()
    sparse = t[:, 0] + t[:, 1] * cs * s1 + t[:, 2] * cs * cs * s2 + t[:, 3] * cs * s3 + t[:, 4]
    return sparse / t.sum(dim=1), sparse.sum() + static


def _rel(got, want):
    return ((got.double().cpu() - want).abs() / want.abs().clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("n", [1, 33, 512])
def test_forward_stats(ops, n):
    g = torch.Generator().manual_seed(40 + n)
    terms = (torch.rand(n, 5, generator=g, dtype=torch.float64) * 1e8 + 1e5)
    static = 2.3e8
    B = 37
    width = 64
    cnt = torch.randint(0, width + 1, (n, B), generator=g, dtype=torch.int32)
    denom = torch.full((n,), float(B * width))
    denom[2::3] = 0.0                                  # not a channel-mode block: cs stays what st_in says (or 1); block 0 always counts
    if n > 1:
        denom[1] = -1.0
    cs_cnt = cnt.sum(dim=1).double() / denom.double().clamp_min(1.0)
    # form 1: cnt + denom only
    st, perc, flops = ops.forward_stats(terms.to(DEV), static, cnt=cnt.to(DEV), denom=denom.to(DEV))
    torch.cuda.synchronize()
    want_st = torch.ones(n, 4, dtype=torch.float64)
    want_st[:, 3] = torch.where(denom > 0, cs_cnt, torch.ones(n, dtype=torch.float64))
    assert bool((denom > 0).any()) and (n == 1 or bool((denom <= 0).any()))
    assert bool((st.cpu()[denom <= 0, 3] == 1.0).all()), "denom <= 0: cs stays 1"
    want_perc, want_flops = _stats_reference(terms, static, want_st)
    assert _rel(st, want_st) < 1e-6 and _rel(perc, want_perc) < 1e-6 and _rel(flops, want_flops) < 1e-5
    # form 2: st_in with 3 and with 4 columns, alone and together with the counts
    for cols in (3, 4):
        st_in = torch.rand(n, cols, generator=g) * 0.9 + 0.05
        full = torch.cat((st_in, torch.ones(n, 1)), dim=1) if cols == 3 else st_in.clone()
        st, perc, flops = ops.forward_stats(terms.to(DEV), static, st_in=st_in.to(DEV))
        torch.cuda.synchronize()
        want_perc, want_flops = _stats_reference(terms, static, full)
        assert torch.equal(st.cpu(), full), "st_out must repeat st_in (cs = 1 with three columns)"
        assert _rel(perc, want_perc) < 1e-6 and _rel(flops, want_flops) < 1e-5
        st, perc, flops = ops.forward_stats(terms.to(DEV), static, cnt=cnt.to(DEV), denom=denom.to(DEV), st_in=st_in.to(DEV))
        torch.cuda.synchronize()
        both = full.double()
        both[:, 3] = torch.where(denom > 0, cs_cnt, both[:, 3])
        want_perc, want_flops = _stats_reference(terms, static, both)
        assert _rel(st, both) < 1e-6 and _rel(perc, want_perc) < 1e-6 and _rel(flops, want_flops) < 1e-5


def test_forward_stats_rejects_bad_arguments(ops):
    from laudnet_amd import LdnError
    terms = torch.ones(513, 5, dtype=torch.float64, device=DEV)
    with pytest.raises(LdnError):                      # more blocks than the kernel's table holds
        ops.forward_stats(terms, 0.0)
    t4 = terms[:4].contiguous()
    cnt = torch.ones(4, 8, dtype=torch.int32, device=DEV)
    with pytest.raises(LdnError):                      # counts without their denominators
        ops.forward_stats(t4, 0.0, cnt=cnt)
    with pytest.raises(LdnError):                      # ... and the other way round
        ops.forward_stats(t4, 0.0, denom=torch.ones(4, device=DEV))
    with pytest.raises(LdnError):                      # a denominator per block
        ops.forward_stats(t4, 0.0, cnt=cnt, denom=torch.ones(3, device=DEV))
    with pytest.raises(LdnError):
        ops.forward_stats(t4, 0.0, st_in=torch.ones(4, 5, device=DEV))


# ------------------------------------------------------------------ 2 x 2 cell means
@pytest.mark.parametrize("S", [1, 3, 7, 14])
@pytest.mark.parametrize("C", [4, 64, 2048])
def test_coarsen_cell_means(ops, S, C):
    B = 3
    fine = seeded_randn((B, 2 * S, 2 * S, C), 50 + S + C)
    got = ops.coarsen_cell_means(fine.to(DEV), S)
    torch.cuda.synchronize()
    want = fine.double().view(B, S, 2, S, 2, C).mean((2, 4))
    assert_close(got, want, 1e-4, 1e-4, f"S {S} C {C}")
    from laudnet_amd import LdnError
    with pytest.raises(LdnError):
        ops.coarsen_cell_means(fine[:, :, : 2 * S - 1].contiguous().to(DEV), S)
