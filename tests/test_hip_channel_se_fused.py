"""-m gpu: the SE block of a LAD-RegNet CHANNEL-mode bottleneck folded into its neighbours (laud_regnet.USE_CHANNEL_SE_FUSED), through the ops.

Reference semantics: laud_regnet.py:194-197 `x = self.b(x); x = self.se(x); x = self.c(x)` on the kept channels of every image.  Unfused the
library runs conv b, a channel-sum pass, the SE head, an in-place scaling pass and conv c; fused, conv b's epilogue leaves the channel sums in
packed-column order (ldn_grouped_chan_mfma_conv3x3_image_gap), the head makes a gate per image (ldn_se_gate_image) and conv c multiplies its
input by it in flight (ldn_conv_image_gated).

1. conv b with sums, on the shapes of tests/test_hip_grouped_chan_mfma.py (imported, with their cached problems): the three widths, whole-image
   and banded plans, both strides, ragged pixel tiles; granularity 1 and = width; images with no channel, with every channel, with a whole
   group inactive.
2. se_gate_image against float64 torchvision SE on the gathered channels.
3. conv_image_gated: bit-identical to conv_image on the pre-scaled input, one shape per row of LDN_CONV_GATED_KERNELS (the rows are asked of
   the library's own chooser on the CPU, tests/test_conv_gated_plan.py); against float64; unread columns; refusals.
4. the block and the regnet_tiny model with the switch on."""
import functools

import pytest
import torch
import torch.nn as nn

import test_conv_gated_plan as GP
import test_hip_grouped_chan_mfma as G
from fill import fill_state_dict, seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -7.0


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


# ------------------------------------------------------------------------------------------------ 1. conv b with sums
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gran", [1, "gw"])
@pytest.mark.parametrize("gw,C,B,Hi,Wi,stride", G.CASES + G.BANDED)
def test_conv_b_leaves_its_channel_sums_in_packed_order(ops, gw, C, B, Hi, Wi, stride, gran, relu):
    gran = gw if gran == "gw" else gran
    prob = G._problem(gw, C, B, Hi, Wi, stride, gran)
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = prob
    Ho, Wo = y64.shape[2], y64.shape[3]
    bands = ops.grouped_chan_mfma_bands(C, gw, Hi, Wi, Ho, stride)
    assert bands >= (2 if (gw, C, B, Hi, Wi, stride) in G.BANDED else 1) and ops.grouped_chan_mfma_gap_ok(C, gw, Hi, Wi, stride)
    if B >= 4:
        assert n[0] == 0 and n[1] == C          # an image without a channel, one with all; image 2 has a whole group inactive where C > gw
    want = G._run(ops, prob, gw, stride, relu)
    frag, sc, sh = G._pack(ops, wk, gw), scale.to(DEV), shift.to(DEV)
    runs = []
    for _ in range(2):
        out = torch.full((B, Ho, Wo, C + 4), SENTINEL, device=DEV)
        gap = torch.full((B, bands, C), NAN, device=DEV)
        got = ops.grouped_chan_mfma_conv3x3_image_gap(a, frag, gw, idx, cnt, sc, sh, out, stride=stride, relu=relu, gap=gap)
        torch.cuda.synchronize()
        assert got is gap
        runs.append((out, gap))
    out, gap = runs[0]
    assert torch.equal(out, want), "out differs from the plain op's"
    assert torch.isfinite(gap).all(), "an element of gap_partial was not written"
    assert torch.equal(runs[1][0], out) and torch.equal(runs[1][1], gap), "two launches differ"
    ref = out[..., :C].double().sum(dim=(1, 2)).cpu()                 # [B, C] float64 sums of the kernel's own output, packed-column order
    tot = gap.double().sum(dim=1).cpu()
    for b in range(B):
        assert bool((gap[b, :, n[b]:] == 0).all()), f"image {b}: sums behind the count must be exactly zero"
    err, bound = (tot - ref).abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item())
    print(f"chan gap gw {gw} C {C} {Hi}x{Wi} stride {stride} gran {gran} relu {relu} bands {bands}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound


def test_conv_b_gap_refusals(ops):
    from laudnet_amd._lib import LdnError
    gw, C, B, Hi, Wi, stride = G.CASES[1]
    a, wk, scale, shift, idx, cnt, n, cidx, y64 = G._problem(gw, C, B, Hi, Wi, stride, 1)
    frag, sc, sh = G._pack(ops, wk, gw), scale.to(DEV), shift.to(DEV)
    out = torch.full((B, Hi, Wi, C + 4), SENTINEL, device=DEV)
    gap = torch.full((B * C + 1,), SENTINEL, device=DEV)
    with pytest.raises(LdnError):                   # not 16-byte aligned
        ops.grouped_chan_mfma_conv3x3_image_gap(a, frag, gw, idx, cnt, sc, sh, out, gap=gap[1:].view(B, 1, C))
    with pytest.raises(LdnError):                   # another band count
        ops.grouped_chan_mfma_conv3x3_image_gap(a, frag, gw, idx, cnt, sc, sh, out, gap=torch.zeros(B, 2, C, device=DEV))
    with pytest.raises(LdnError):                   # width 56
        ops.grouped_chan_mfma_conv3x3_image_gap(a, frag, 56, idx, cnt, sc, sh, out)
    with pytest.raises(LdnError):                   # a channel list without its counts
        ops.grouped_chan_mfma_conv3x3_image_gap(a, frag, gw, idx, None, sc, sh, out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((gap == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 2. the gate
def _lists(B, C, counts, seed):
    """ascending random channel lists [B, C] int32 (entries past the count: 0) for the given counts"""
    idx = torch.zeros(B, C, dtype=torch.int32)
    g = torch.Generator().manual_seed(seed)
    for b, k in enumerate(counts):
        idx[b, :k] = torch.sort(torch.randperm(C, generator=g)[:k]).values.to(torch.int32)
    return idx, torch.tensor(counts, dtype=torch.int32)


@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("C,S", [(48, 8), (120, 12), (888, 222)])
def test_se_gate_image(ops, C, S, bands):
    """gate[b, j] = sigmoid(W2[ch] . relu(W1[:, list] . mean + b1) + b2[ch]) at the gathered channels ch = list[j]; zeros past the count"""
    B, rows = 4, 49
    counts = [0, C, C // 3, 1]
    idx, cnt = _lists(B, C, counts, 40 + C)
    gap = torch.rand(B, bands, C, generator=torch.Generator().manual_seed(41 + C)) * rows / bands
    for b in range(B):
        gap[b, :, counts[b]:] = NAN             # the sums behind the count are zeros in real use: they must not be read at all
    w1 = seeded_randn((S, C), 42) * (1.0 / C) ** 0.5
    b1 = seeded_randn((S,), 43) * 0.1
    w2 = seeded_randn((C, S), 44) * (1.0 / S) ** 0.5
    b2 = seeded_randn((C,), 45) * 0.1
    gate = ops.se_gate_image(gap.to(DEV), rows, w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), idx.to(DEV), cnt.to(DEV))
    torch.cuda.synchronize()
    assert gate.shape == (B, C)
    got = gate.cpu()
    err = 0.0
    for b, k in enumerate(counts):
        assert bool((got[b, k:] == 0).all()), f"image {b}: gates past the count must be exactly zero"
        if k:
            ch = idx[b, :k].long()
            mean = gap[b, :, :k].double().sum(dim=0) / rows
            hid = torch.relu(w1.double()[:, ch] @ mean + b1.double())
            ref = torch.sigmoid(w2.double()[ch] @ hid + b2.double()[ch])
            err = max(err, (got[b, :k].double() - ref).abs().max().item())
    print(f"se_gate_image C {C} S {S} bands {bands}: max |err| {err:.3e} (bound 1e-5)")
    assert err < 1e-5


# ------------------------------------------------------------------------------------------------ 3. conv c with the gate
# (H, W, cin, cout, residual, scale, kgran, out aliases residual) -> the row of LDN_CONV_GATED_KERNELS it runs; none of them is a shape that
# ldn_conv_image would hand to its streaming kernel (whose K order is another one: the bit-identity below is k_conv_bf3 against k_conv_bf3)
GATED = [((14, 14, 48, 64, True, True, 1, False), "k_conv_bf3<6,2,2,B_KN4>"),
         ((14, 14, 104, 128, False, True, 8, False), "k_conv_bf3<4,4,4,B_KN4>"),
         ((28, 28, 120, 128, True, False, 24, True), "k_conv_bf3<4,4,2,B_KN4>"),
         ((14, 14, 336, 336, True, True, 1, True), "k_conv_bf3<4,4,2,B_KN4>"),
         ((7, 7, 120, 160, True, True, 1, False), "k_conv_bf3<8,6,4,B_KN4>"),
         ((10, 10, 104, 320, False, False, 8, False), "k_conv_bf3<4,10,2,B_KN4>"),
         ((7, 7, 48, 320, True, True, 24, True), "k_conv_bf3<2,10,2,B_KN4>"),
         ((7, 7, 888, 888, True, True, 24, False), "k_conv_bf3<2,10,2,B_KN4>")]
GB = 5


def test_the_gated_cases_cover_the_gated_list():
    """(CPU arithmetic) every case runs the row it names, the cases reach every row of the list, and the sweep of the CPU test does too"""
    plans = GP.plan([(GB, H * W, cin, cout, res, scale) for (H, W, cin, cout, res, scale, _, _), _ in GATED])
    assert [(p["kernel"], p["ok"]) for p in plans] == [(k, 1) for _, k in GATED]
    assert {k for _, k in GATED} == set(GP.GATED_ROWS) == set(GP.reach())


@functools.lru_cache(maxsize=None)
def _gated_problem(H, W, cin, cout, kgran):
    seed = 900 + H + 3 * cin + cout + kgran
    g = torch.Generator().manual_seed(seed)
    counts = [0, kgran, cin] + [kgran * int(torch.randint(1, cin // kgran, (1,), generator=g)) for _ in range(GB - 3)]
    idx, cnt = _lists(GB, cin, counts, seed + 1)
    a = torch.relu(seeded_randn((GB, H, W, cin), seed + 2))
    gate = torch.sigmoid(seeded_randn((GB, cin), seed + 3))
    for b, k in enumerate(counts):
        a[b, :, :, k:] = 0.0
        gate[b, k:] = 0.0
    w = seeded_randn((1, cin, cout), seed + 4) * (2.0 / cin) ** 0.5          # k-major
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g) * 0.1
    base = torch.relu(seeded_randn((GB, H, W, cout), seed + 5))
    return counts, idx, cnt, a, gate, w, sc, sh, base


@pytest.mark.parametrize("case,kernel", GATED)
def test_conv_c_with_the_gate_on_its_input(ops, case, kernel):
    H, W, cin, cout, has_res, has_scale, kgran, alias = case
    assert ops.conv_image_gated_ok(GB, H * W, cin, cout, has_res, has_scale)
    counts, idx, cnt, a, gate, w, sc, sh, base = _gated_problem(H, W, cin, cout, kgran)
    assert counts[:3] == [0, kgran, cin] and (kgran > 1 or counts[1] == 1)
    d = lambda t: t.to(DEV)
    a_d, gate_d, w_d, idx_d, cnt_d = d(a), d(gate), d(w), d(idx), d(cnt)
    sc_d, sh_d = (d(sc) if has_scale else None), d(sh)

    def run(op, inp, *extra):
        resid = d(base) if has_res else None
        out = resid if alias else torch.full((GB, H, W, cout), SENTINEL, device=DEV)
        op(inp, w_d, sc_d, sh_d, out, *extra, k_idx=idx_d, k_cnt=cnt_d, kgran=kgran, relu=1, residual=resid)
        torch.cuda.synchronize()
        return out
    scaled = (a_d * gate_d.view(GB, 1, 1, cin)).contiguous()
    want = run(ops.conv_image, scaled)
    got = run(ops.conv_image_gated, a_d, gate_d)
    assert torch.equal(got, want), "not bit-identical to conv_image on the pre-scaled input"
    # float64
    ref = torch.empty(GB, H, W, cout, dtype=torch.float64)
    for b, k in enumerate(counts):
        ch = idx[b, :k].long()
        y = (a[b, :, :, :k].double() * gate[b, :k].double()) @ w[0].double()[ch]
        y = y * (sc.double() if has_scale else 1.0) + sh.double()
        ref[b] = torch.relu(y + (base[b].double() if has_res else 0.0))
    err, bound = (got.cpu().double() - ref).abs().max().item(), 1e-4 * max(1.0, ref.abs().max().item())
    print(f"conv_image_gated {kernel} {H}x{W} {cin}->{cout} res {has_res} scale {has_scale} kgran {kgran} alias {alias}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    # columns at or past the count, of the input and of the gate, are never used
    a_nan, gate_nan = a.clone(), gate.clone()
    for b, k in enumerate(counts):
        a_nan[b, :, :, k:] = NAN
        gate_nan[b, k:] = NAN
    got_nan = run(ops.conv_image_gated, d(a_nan), d(gate_nan))
    assert torch.isfinite(got_nan).all(), "a column at or past the count was used"
    assert torch.equal(got_nan, got)


def test_conv_c_gated_refusals(ops):
    from laudnet_amd._lib import LdnError
    H, W, cin, cout, kgran = 7, 7, 48, 64, 1
    counts, idx, cnt, a, gate, w, sc, sh, base = _gated_problem(H, W, cin, cout, kgran)
    d = lambda t: t.to(DEV)
    a_d, gate_d, w_d, idx_d, cnt_d, sc_d, sh_d = d(a), d(gate), d(w), d(idx), d(cnt), d(sc), d(sh)
    out = torch.full((GB, H, W, cout), SENTINEL, device=DEV)
    kw = dict(k_idx=idx_d, k_cnt=cnt_d, kgran=kgran, relu=1)
    nidx, ncnt = d(_lists(GB, cout, [cout] * GB, 5)[0]), torch.full((GB,), cout, dtype=torch.int32, device=DEV)
    odd = torch.zeros(GB * cin + 1, device=DEV)[1:].view(GB, cin)
    bad = [dict(math="fp32"), dict(n_idx=nidx, n_cnt=ncnt), dict(colsum=torch.zeros(GB, 2, cout, device=DEV)), dict(post_sub=sc_d),
           dict(k_idx=None, k_cnt=None)]
    for over in bad:
        with pytest.raises(LdnError):
            ops.conv_image_gated(a_d, w_d, sc_d, sh_d, out, gate_d, **dict(kw, **over))
    with pytest.raises(LdnError):                                   # ksize 3
        ops.conv_image_gated(a_d, d(seeded_randn((9, cin, cout), 1)), sc_d, sh_d, out, gate_d, ksize=3, **kw)
    with pytest.raises(LdnError):                                   # out_format 1
        ops.conv_image_gated(a_d, w_d, sc_d, sh_d, out, gate_d, out_split=True, **kw)
    with pytest.raises(LdnError):                                   # no gate
        ops.conv_image_gated(a_d, w_d, sc_d, sh_d, out, None, **kw)
    from laudnet_amd import _lib as L
    args = [L.ptr(a_d), cin, GB, H, W, 1, 1, H, W, L.ptr(w_d), cin, cout, L.ptr(idx_d), L.ptr(cnt_d), 1, None, None, L.ptr(sc_d), L.ptr(sh_d), 1, None,
            1, None, 0, L.ptr(out), cout, None, 0, None, 1, None]
    assert L.load().ldn_conv_image_gated(*args) == -1             # a null gate, at the C ABI
    with pytest.raises(LdnError):                                   # a gate that is not 16-byte aligned
        ops.conv_image_gated(a_d, w_d, sc_d, sh_d, out, odd, **kw)
    with pytest.raises(LdnError):                                   # 16 shift classes
        ops.conv_image_gated(a_d, w_d, sc_d, sh_d.repeat(16, 1).contiguous(), out, gate_d, **kw)
    with pytest.raises(LdnError):                                   # stride 2
        ops.conv_image_gated(a_d, w_d, sc_d, sh_d, torch.full((GB, 4, 4, cout), SENTINEL, device=DEV), gate_d, stride=2, **kw)
    with pytest.raises(LdnError):                                   # a plan beyond the LDS of a CU
        ops.conv_image_gated(torch.zeros(1, 7, 7, 8192, device=DEV), torch.zeros(1, 8192, 320, device=DEV), None, torch.zeros(320, device=DEV),
                             torch.zeros(1, 7, 7, 320, device=DEV), torch.ones(1, 8192, device=DEV), k_idx=torch.zeros(1, 8192, dtype=torch.int32, device=DEV),
                             k_cnt=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert not ops.conv_image_gated_ok(1, 49, 8192, 320, False, False)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 4. the block, the model
def _counted(ops, monkeypatch):
    calls = {n: 0 for n in ("se_packed", "conv_image_gated", "grouped_chan_mfma_conv3x3_image_gap", "se_gate_image", "grouped_chan_mfma_conv3x3_image")}
    for name in calls:
        real = getattr(ops, name)

        def counted(*a, _real=real, _n=name, **kw):
            calls[_n] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


def _block_run(ops, monkeypatch, gw, stride, Ho, inplace, fused):
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_CHANNEL", True)
    monkeypatch.setattr(laud_regnet, "USE_CHANNEL_SE_FUSED", fused)
    blk = laud_regnet.ResBottleneckBlock(96, 96, stride, lambda c: nn.BatchNorm2d(c, eps=1e-5, momentum=0.1), nn.ReLU, group_width=gw,
                                         bottleneck_multiplier=1.0, se_ratio=0.25, channel_dyn_granularity=1, output_size=Ho,
                                         mask_spatial_granularity=1, dyn_mode="channel", channel_masker="MLP", channel_masker_layers=1).eval()
    assert (blk.proj is not None) == (stride == 2) and blk.f.group_width == gw and blk.f.w_b == 96
    blk.load_state_dict(fill_state_dict(blk.state_dict(), 177 + gw))
    blk = blk.to(DEV)
    B = 5
    assert blk.f.masker_channel.channel_dyn_group == 96           # granularity 1
    cm = seeded_bernoulli((B, 96), 0.5, 1500 + gw + stride + Ho)
    cm[0] = 0.0                                                     # no channel, every channel, a whole group inactive
    cm[1] = 1.0
    cm[2, :gw] = 0.0
    blk.f.forced_channel_mask = cm.to(DEV)
    x = torch.relu(seeded_randn((B, 96, Ho * stride, Ho * stride), 1700 + gw)).to(DEV).contiguous(memory_format=torch.channels_last)
    calls = _counted(ops, monkeypatch)
    with torch.no_grad():
        out, _ = blk.run_dynamic(x, inplace=inplace)
    torch.cuda.synchronize()
    if inplace and stride == 1:
        assert out.data_ptr() == x.data_ptr(), "the in-place identity block writes its input's rows"
    return out.clone(), dict(calls)


@pytest.mark.parametrize("stride,inplace", [(1, False), (1, True), (2, False)])
@pytest.mark.parametrize("Ho", [7, 14])
@pytest.mark.parametrize("gw", [8, 16, 24])
def test_channel_block_with_folded_se_matches_the_five_launch_path(ops, monkeypatch, gw, Ho, stride, inplace):
    on, calls = _block_run(ops, monkeypatch, gw, stride, Ho, inplace, True)
    assert calls == dict(se_packed=0, conv_image_gated=1, grouped_chan_mfma_conv3x3_image_gap=1, se_gate_image=1, grouped_chan_mfma_conv3x3_image=0), calls
    monkeypatch.undo()
    off, calls = _block_run(ops, monkeypatch, gw, stride, Ho, inplace, False)
    assert calls == dict(se_packed=1, conv_image_gated=0, grouped_chan_mfma_conv3x3_image_gap=0, se_gate_image=0, grouped_chan_mfma_conv3x3_image=1), calls
    err, bound = (on - off).abs().max().item(), 1e-5 * max(1.0, off.abs().max().item())
    print(f"channel block gw {gw} {Ho}x{Ho} stride {stride} inplace {inplace}: folded vs five launches max |diff| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(on).all() and err < bound


@pytest.mark.parametrize("case", ["channel_g2", "both"])
def test_regnet_tiny_with_the_switch_on(ops, monkeypatch, case):
    """the whole model at the fixture's tolerance; the channel blocks take the fold, the 'both' blocks (conv c over packed rows) never do"""
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_CHANNEL", True)
    monkeypatch.setattr(laud_regnet, "USE_CHANNEL_SE_FUSED", True)
    calls = _counted(ops, monkeypatch)
    G._regnet_injected(case)
    if case == "channel_g2":
        assert calls["se_packed"] == 0 and calls["grouped_chan_mfma_conv3x3_image"] == 0, calls
        assert calls["conv_image_gated"] == calls["grouped_chan_mfma_conv3x3_image_gap"] == calls["se_gate_image"] == 5, calls
    else:
        assert calls["conv_image_gated"] == calls["grouped_chan_mfma_conv3x3_image_gap"] == calls["se_gate_image"] == 0, calls
        assert calls["grouped_chan_mfma_conv3x3_image"] > 0, calls


def test_switch_off_runs_none_of_the_new_ops(ops, monkeypatch):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_CHANNEL_SE_FUSED is False
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_CHANNEL", True)
    calls = _counted(ops, monkeypatch)
    G._regnet_injected("channel_g2")
    assert calls["conv_image_gated"] == calls["grouped_chan_mfma_conv3x3_image_gap"] == calls["se_gate_image"] == 0 and calls["se_packed"] == 5, calls
