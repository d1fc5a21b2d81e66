"""-m gpu: the SE block of a LAD-RegNet 'BOTH'-mode bottleneck folded into its neighbours (laud_regnet.USE_BOTH_SE_FUSED), through the ops.

Reference semantics: laud_regnet.py:194-200 `x = self.b(x); x = self.se(x); x = self.c(x)` on the kept channels of every image, conv c's
output masked per pixel.  Unfused the library runs conv b, a channel-sum pass and an in-place scaling pass over every pixel of h_b
(ldn_se_packed) and, per mask group, conv c over the packed rows of the active pixels; folded, conv b's epilogue leaves the channel sums
(the channel mode's _gap forms), ldn_se_gate_image makes a gate per image and conv c multiplies its packed rows by it in flight
(ldn_conv_packed_gated), the same gate for every mask group.

1. conv_packed_gated: bit-identical to conv_packed on the pre-scaled input, one shape per row of LDN_CONV_GATED_KERNELS that packed shapes
   reach (the rows are asked of the library's own chooser on the CPU, tests/test_conv_packed_gated_plan.py); against float64; unread rows
   and columns; rows outside out_map; out aliasing the residual; column slices; refusals.
2. the 'both' block, switch on vs off.
3. the regnet_tiny model and the two-mask-group model with the switches on."""
import functools

import pytest
import torch
import torch.nn as nn

import test_conv_packed_gated_plan as PP
import test_hip_grouped_chan_mfma as G
from fill import fill_state_dict, seeded_bernoulli, seeded_randn
from helpers import assert_tuple_close, load_golden

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


# ------------------------------------------------------------------------------------------------ 1. conv c over packed rows with the gate
# (H, W, cin, cout, residual, scale, kgran, variant) -> the row of LDN_CONV_GATED_KERNELS it runs.  variant: "" = out a buffer of its own,
# "alias" = out is the residual (the in-place identity block), "slice" = out / residual the second of two column slices (the mask-group loop),
# "rot" = the pixel counts rotated by one image, so that the image without a channel has active pixels.  None of the shapes is one that
# ldn_conv_packed would hand to its streaming kernel (cout is no multiple of 128): the bit-identity below is k_conv_bf3 against k_conv_bf3.
PACKED = [((7, 7, 8, 32, True, True, 1, ""), "k_conv_bf3<6,2,2,B_KN4>"),
          ((14, 14, 48, 160, False, True, 8, ""), "k_conv_bf3<4,4,4,B_KN4>"),
          ((14, 14, 104, 160, True, False, 1, "alias"), "k_conv_bf3<4,4,2,B_KN4>"),
          ((14, 14, 888, 320, True, True, 24, "slice"), "k_conv_bf3<4,4,2,B_KN4>"),
          ((7, 7, 104, 160, True, True, 1, "rot"), "k_conv_bf3<8,6,4,B_KN4>"),
          ((10, 10, 104, 320, False, False, 8, ""), "k_conv_bf3<4,10,2,B_KN4>"),
          ((10, 10, 48, 320, True, True, 1, "slice"), "k_conv_bf3<4,10,2,B_KN4>"),
          ((7, 7, 888, 320, True, True, 1, "alias"), "k_conv_bf3<2,10,2,B_KN4>")]
GB = 5


def test_the_packed_cases_cover_the_rows_that_packed_shapes_reach():
    """(CPU arithmetic) every case runs the row it names, and the cases reach every row that the CPU sweep's packed shapes reach"""
    plans = PP.plan([(GB, H * W, cin, cout, res, scale) for (H, W, cin, cout, res, scale, _, _), _ in PACKED])
    assert [(p["kernel"], p["ok"]) for p in plans] == [(k, 1) for _, k in PACKED]
    assert {k for _, k in PACKED} == set(PP.reach()) == set(PP.GATED_ROWS)
    assert {H * W for (H, W, *_), _ in PACKED} == {49, 100, 196} and {c[2] for c, _ in PACKED} == {8, 48, 104, 888}
    assert {c[3] for c, _ in PACKED} == {32, 160, 320}


def _lists(B, C, counts, seed):
    """ascending random channel lists [B, C] int32 (entries past the count: 0) for the given counts"""
    idx = torch.zeros(B, C, dtype=torch.int32)
    g = torch.Generator().manual_seed(seed)
    for b, k in enumerate(counts):
        idx[b, :k] = torch.sort(torch.randperm(C, generator=g)[:k]).values.to(torch.int32)
    return idx, torch.tensor(counts, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _packed_problem(H, W, cin, cout, kgran, rot):
    """a dense batch a [GB * H * W, cin] (h_b of a block), its channel lists, a gate per image, and the packed list of the active pixels"""
    HW = H * W
    seed = 2900 + H + 3 * cin + cout + kgran
    g = torch.Generator().manual_seed(seed)
    counts = [0, kgran, cin] + [kgran * int(torch.randint(1, cin // kgran, (1,), generator=g)) for _ in range(GB - 3)]
    pix = [0, 1, 33, HW, int(torch.randint(2, HW, (1,), generator=g))]        # no row, one, one past a subtile, all, some
    if rot:
        pix = pix[-1:] + pix[:-1]
    idx, cnt = _lists(GB, cin, counts, seed + 1)
    a = torch.relu(seeded_randn((GB * HW, cin), seed + 2))
    gate = torch.sigmoid(seeded_randn((GB, cin), seed + 3))
    for b, k in enumerate(counts):
        a[b * HW:(b + 1) * HW, k:] = 0.0
        gate[b, k:] = 0.0
    rows = [b * HW + torch.sort(torch.randperm(HW, generator=g)[:n]).values for b, n in enumerate(pix)]
    idx3 = torch.cat(rows).to(torch.int32)                                    # flat row of every active pixel, image-major and ascending
    pre = torch.tensor([0] + pix, dtype=torch.int32).cumsum(0).to(torch.int32)
    w = seeded_randn((1, cin, cout), seed + 4) * (2.0 / cin) ** 0.5          # k-major
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g) * 0.1
    base = torch.relu(seeded_randn((GB * HW, cout), seed + 5))
    return counts, pix, idx, cnt, a, gate, idx3, pre, w, sc, sh, base


@pytest.mark.parametrize("case,kernel", PACKED)
def test_conv_c_over_packed_rows_with_the_gate_on_its_input(ops, case, kernel):
    H, W, cin, cout, has_res, has_scale, kgran, variant = case
    HW = H * W
    assert ops.conv_packed_gated_ok(GB, HW, cin, cout, has_res, has_scale)
    counts, pix, idx, cnt, a, gate, idx3, pre, w, sc, sh, base = _packed_problem(H, W, cin, cout, kgran, variant == "rot")
    assert counts[:3] == [0, kgran, cin] and sorted(pix)[:2] == [0, 1] and 33 in pix and HW in pix
    assert (pix[0] > 0) == (variant == "rot")
    d = lambda t: t.to(DEV)
    a_d, gate_d, w_d, idx_d, cnt_d, idx3_d, pre_d = d(a), d(gate), d(w), d(idx), d(cnt), d(idx3), d(pre)
    sc_d, sh_d = (d(sc) if has_scale else None), d(sh)
    img_of_row = torch.arange(GB).repeat_interleave(HW)
    active = torch.zeros(GB * HW, dtype=torch.bool)
    active[idx3.long()] = True

    def run(op, inp, *extra):
        """-> (the whole buffer out lives in, out)"""
        if variant == "slice":
            resid_full = torch.cat((torch.full((GB * HW, cout), SENTINEL), base), dim=1).to(DEV) if has_res else None
            full = torch.full((GB * HW, 2 * cout), SENTINEL, device=DEV)
            resid, out = (resid_full[:, cout:] if has_res else None), full[:, cout:]
        else:
            resid = d(base) if has_res else None
            out = resid if variant == "alias" else torch.full((GB * HW, cout), SENTINEL, device=DEV)
            full = out
        assert variant != "alias" or has_res
        op(inp, w_d, sc_d, sh_d, out, *extra, B=GB, row_prefix=pre_d, m_cap=HW, a_map=idx3_d, out_map=idx3_d, k_idx=idx_d, k_cnt=cnt_d, kgran=kgran,
           relu=1, residual2d=resid)
        torch.cuda.synchronize()
        return full, out
    scaled = (a_d * gate_d[d(img_of_row)]).contiguous()                       # fp32(a * gate), materialised
    want_full, _ = run(ops.conv_packed, scaled)
    got_full, got = run(ops.conv_packed_gated, a_d, gate_d)
    assert torch.equal(got_full, want_full), "not bit-identical to conv_packed on the pre-scaled input"
    again_full, _ = run(ops.conv_packed_gated, a_d, gate_d)
    assert torch.equal(again_full, got_full), "two launches differ"
    # rows outside out_map keep what they held; the first column slice is never written
    keep = d(base) if variant == "alias" else torch.full((GB * HW, cout), SENTINEL, device=DEV)
    assert torch.equal(got[d(~active)], keep[d(~active)]), "a row outside out_map was written"
    if variant == "slice":
        assert bool((got_full[:, :cout] == SENTINEL).all()), "the first column slice was written"
    # float64
    ref = torch.zeros(GB * HW, cout, dtype=torch.float64)
    for b, k in enumerate(counts):
        ch = idx[b, :k].long()
        y = (a[b * HW:(b + 1) * HW, :k].double() * gate[b, :k].double()) @ w[0].double()[ch]
        y = y * (sc.double() if has_scale else 1.0) + sh.double()
        ref[b * HW:(b + 1) * HW] = torch.relu(y + (base[b * HW:(b + 1) * HW].double() if has_res else 0.0))
    err = (got.cpu().double() - ref)[active].abs().max().item()
    bound = 1e-4 * max(1.0, ref[active].abs().max().item())
    print(f"conv_packed_gated {kernel} {H}x{W} {cin}->{cout} res {has_res} scale {has_scale} kgran {kgran} {variant or 'plain'} pixels {pix} "
          f"channels {counts}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    # inactive rows of the input, and columns at or past the count of the input and of the gate, are never used
    a_nan, gate_nan = a.clone(), gate.clone()
    a_nan[~active] = NAN
    for b, k in enumerate(counts):
        a_nan[b * HW:(b + 1) * HW, k:] = NAN
        gate_nan[b, k:] = NAN
    nan_full, _ = run(ops.conv_packed_gated, d(a_nan), d(gate_nan))
    assert torch.isfinite(nan_full).all(), "an inactive row, or a column at or past the count, was used"
    assert torch.equal(nan_full, got_full)


def test_conv_c_packed_gated_refusals(ops):
    from laudnet_amd import _lib as L
    LdnError = L.LdnError
    H, W, cin, cout, kgran = 7, 7, 48, 32, 1
    HW = H * W
    counts, pix, idx, cnt, a, gate, idx3, pre, w, sc, sh, base = _packed_problem(H, W, cin, cout, kgran, False)
    d = lambda t: t.to(DEV)
    a_d, gate_d, w_d, idx_d, cnt_d, sc_d, sh_d, idx3_d, pre_d = d(a), d(gate), d(w), d(idx), d(cnt), d(sc), d(sh), d(idx3), d(pre)
    out = torch.full((GB * HW, cout), SENTINEL, device=DEV)
    kw = dict(B=GB, row_prefix=pre_d, m_cap=HW, a_map=idx3_d, out_map=idx3_d, k_idx=idx_d, k_cnt=cnt_d, kgran=kgran, relu=1)
    nidx, ncnt = d(_lists(GB, cout, [cout] * GB, 5)[0]), torch.full((GB,), cout, dtype=torch.int32, device=DEV)
    odd = torch.zeros(GB * cin + 1, device=DEV)[1:].view(GB, cin)
    rows_i32 = torch.zeros(idx3.numel(), dtype=torch.int32, device=DEV)
    bad = [dict(math="fp32"), dict(n_idx=nidx, n_cnt=ncnt), dict(post_sub=sc_d), dict(pix_map=rows_i32, geom=(H, W, H, W, 1)),
           dict(relu=2, relu_if_neg=rows_i32), dict(relu=2), dict(row_prefix=None)]
    for over in bad:
        with pytest.raises(LdnError):
            ops.conv_packed_gated(a_d, w_d, sc_d, sh_d, out, gate_d, **dict(kw, **over))
    with pytest.raises(LdnError):                                   # no input-channel list (the weights n-major, as that launch would have them)
        ops.conv_packed_gated(a_d, d(w.permute(2, 0, 1).contiguous()), sc_d, sh_d, out, gate_d, **dict(kw, k_idx=None, k_cnt=None))
    with pytest.raises(LdnError):                                   # nine taps
        ops.conv_packed_gated(a_d, d(seeded_randn((9, cin, cout), 1)), sc_d, sh_d, out, gate_d, taps=9,
                              **dict(kw, a_map=torch.full((idx3.numel(), 9), -1, dtype=torch.int32, device=DEV)))
    with pytest.raises(LdnError):                                   # no gate
        ops.conv_packed_gated(a_d, w_d, sc_d, sh_d, out, None, **kw)
    args = [L.ptr(a_d), cin, GB, L.ptr(pre_d), None, HW, L.ptr(idx3_d), 1, L.ptr(idx3_d), None, 0, 0, 0, 0, 1, L.ptr(w_d), cin, cout, L.ptr(idx_d),
            L.ptr(cnt_d), 1, None, None, L.ptr(sc_d), L.ptr(sh_d), 1, None, 1, None, None, 0, L.ptr(out), cout, None, 1, None]
    assert L.load().ldn_conv_packed_gated(*args) == -1            # a null gate, at the C ABI
    with pytest.raises(LdnError):                                   # a gate that is not 16-byte aligned
        ops.conv_packed_gated(a_d, w_d, sc_d, sh_d, out, odd, **kw)
    with pytest.raises(LdnError):                                   # 16 shift classes
        ops.conv_packed_gated(a_d, w_d, sc_d, sh_d.repeat(16, 1).contiguous(), out, gate_d, pix_map=rows_i32, geom=(H, W, H, W, 1), **kw)
    # a plan beyond the LDS of a CU: the smallest such shape of the CPU sweep's refused set
    over = [s for s, p in PP.refused() if p["shape_ok"] and p["built"] and p["lds"] > PP.LDS_LIMIT]
    _, rows, big, co, _, _ = min(over, key=lambda s: (s[2], s[1], s[3]))
    assert not ops.conv_packed_gated_ok(1, rows, big, co, False, False)
    small = torch.full((rows, co), SENTINEL, device=DEV)
    with pytest.raises(LdnError):
        ops.conv_packed_gated(torch.zeros(rows, big, device=DEV), torch.zeros(1, big, co, device=DEV), None, torch.zeros(co, device=DEV), small,
                              torch.ones(1, big, device=DEV), B=1, row_prefix=torch.tensor([0, rows], dtype=torch.int32, device=DEV), m_cap=rows,
                              k_idx=torch.zeros(1, big, dtype=torch.int32, device=DEV), k_cnt=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((small == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 2. the block
NEW = ("conv_packed_gated", "se_gate_image", "grouped_chan_mfma_conv3x3_image_gap", "grouped_wide_conv3x3_image_gap")
OLD = ("se_packed", "conv_packed", "grouped_chan_mfma_conv3x3_image", "grouped_wide_conv3x3_image")


def _counted(ops, monkeypatch):
    calls = {n: 0 for n in NEW + OLD}
    for name in calls:
        real = getattr(ops, name)

        def counted(*a, _real=real, _n=name, **kw):
            calls[_n] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


def _switches(monkeypatch, both, channel=True):
    from laudnet_amd import laud_regnet
    for name in ("USE_GROUPED_MFMA_CHANNEL", "USE_GROUPED_MFMA_WIDE"):
        monkeypatch.setattr(laud_regnet, name, True)
    for name in ("USE_CHANNEL_SE_FUSED", "USE_CHANNEL_SE_FUSED_WIDE"):
        monkeypatch.setattr(laud_regnet, name, channel)
    monkeypatch.setattr(laud_regnet, "USE_BOTH_SE_FUSED", both)


BLOCK_B = 5


def _block_run(ops, monkeypatch, gw, stride, Ho, inplace, groups, fused):
    from laudnet_amd import laud_regnet
    _switches(monkeypatch, fused)
    w_b = 112 if gw == 56 else 96
    blk = laud_regnet.ResBottleneckBlock(w_b, w_b, stride, lambda c: nn.BatchNorm2d(c, eps=1e-5, momentum=0.1), nn.ReLU, group_width=gw,
                                         bottleneck_multiplier=1.0, se_ratio=0.25, spatial_mask_channel_group=groups, channel_dyn_granularity=1,
                                         output_size=Ho, mask_spatial_granularity=1, dyn_mode="both", channel_masker="MLP",
                                         channel_masker_layers=1).eval()
    assert (blk.proj is not None) == (stride == 2) and blk.f.group_width == gw and blk.f.w_b == w_b and blk.f.dyn_mode == "both"
    blk.load_state_dict(fill_state_dict(blk.state_dict(), 277 + gw))
    blk = blk.to(DEV)
    B = BLOCK_B
    assert blk.f.masker_channel.channel_dyn_group == w_b and blk.f.masker_spatial.mask_size == Ho           # granularity 1, a mask per pixel
    cm = seeded_bernoulli((B, w_b), 0.5, 2500 + gw + stride + Ho)
    cm[0] = 0.0                                                     # no channel, every channel, a whole group inactive
    cm[1] = 1.0
    cm[2, :gw] = 0.0
    blk.f.forced_channel_mask = cm.to(DEV)
    pm = seeded_bernoulli((B, groups, Ho, Ho), 0.5, 2600 + gw + stride + Ho)
    pm[1] = 0.0                                                     # an image with no active pixel (it has every channel), one with all;
    pm[3] = 1.0                                                     # the image without a channel keeps its random pixels
    blk.f.forced_spatial_mask = pm.to(DEV)
    x = torch.relu(seeded_randn((B, w_b, Ho * stride, Ho * stride), 2700 + gw)).to(DEV).contiguous(memory_format=torch.channels_last)
    calls = _counted(ops, monkeypatch)
    with torch.no_grad():
        out, stats = blk.run_dynamic(x, inplace=inplace)
    torch.cuda.synchronize()
    if inplace and stride == 1:
        assert out.data_ptr() == x.data_ptr(), "the in-place identity block writes its input's rows"
    return out.clone(), stats.clone(), blk.f.last_spatial_mask.clone(), blk.f.last_channel_mask.clone(), dict(calls)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("stride,inplace", [(1, False), (1, True), (2, False)])
@pytest.mark.parametrize("Ho", [7, 14])
@pytest.mark.parametrize("gw", [8, 16, 24, 56])
def test_both_block_with_folded_se_matches_the_unfolded_path(ops, monkeypatch, gw, Ho, stride, inplace, groups):
    gap, plain = ("grouped_wide_conv3x3_image_gap", "grouped_wide_conv3x3_image") if gw == 56 else \
        ("grouped_chan_mfma_conv3x3_image_gap", "grouped_chan_mfma_conv3x3_image")
    zero = {n: 0 for n in NEW + OLD}
    on, st_on, sm_on, cm_on, calls = _block_run(ops, monkeypatch, gw, stride, Ho, inplace, groups, True)
    assert calls == dict(zero, **{gap: 1, "se_gate_image": 1, "conv_packed_gated": groups}), calls
    monkeypatch.undo()
    off, st_off, sm_off, cm_off, calls = _block_run(ops, monkeypatch, gw, stride, Ho, inplace, groups, False)
    assert calls == dict(zero, **{plain: 1, "se_packed": 1, "conv_packed": groups}), calls
    err, bound = (on - off).abs().max().item(), 1e-5 * max(1.0, off.abs().max().item())
    print(f"both block gw {gw} {Ho}x{Ho} stride {stride} inplace {inplace} mask groups {groups}: folded vs unfolded "
          f"max |diff| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(on).all() and err < bound
    assert torch.equal(st_on, st_off) and torch.equal(sm_on, sm_off) and torch.equal(cm_on, cm_off)


# ------------------------------------------------------------------------------------------------ 3. the models
def test_regnet_tiny_both_takes_the_fold(ops, monkeypatch):
    """the 'both' case of regnet_tiny.pt at the fixture's tolerance with every needed switch on: its blocks take the fold"""
    _switches(monkeypatch, True)
    calls = _counted(ops, monkeypatch)
    G._regnet_injected("both")
    assert calls["se_packed"] == 0 and calls["conv_packed"] == 0 and calls["grouped_chan_mfma_conv3x3_image"] == 0, calls
    assert calls["conv_packed_gated"] == calls["grouped_chan_mfma_conv3x3_image_gap"] == calls["se_gate_image"] > 0, calls


REGNET_X = load_golden("regnet_extra.pt")


def _regnet_groups_injected(name="both_grp2"):
    """tests/test_hip_blocks.py::test_regnet_two_spatial_mask_groups, its injected run at its bf16x3 tolerance"""
    import laudnet_amd
    fx = REGNET_X["cases"][name]
    model = laudnet_amd.LAD_RegNet(laudnet_amd.BlockParams(**G.REGNET["tiny_params"]), **fx["kw"]).eval()
    assert list(model.state_dict().keys()) == fx["keys"]
    model.load_state_dict(fill_state_dict(model.state_dict(), fx["seed"]))
    size = fx["kw"]["input_size"]
    model, x = model.to(DEV), seeded_randn((fx["batch"], 3, size, size), fx["x_seed"]).to(DEV)
    for i, blk in enumerate(model.blocks()):
        ms = blk.f.masker_spatial
        assert blk.f.dyn_mode == "both" and ms.mask_channel_group == 2
        blk.f.forced_spatial_mask = seeded_bernoulli((fx["batch"], ms.mask_channel_group, ms.mask_size, ms.mask_size), 0.5, fx["mask_seed"] + 2 * i)
        blk.f.forced_channel_mask = seeded_bernoulli((fx["batch"], blk.f.masker_channel.channel_dyn_group), 0.62, fx["mask_seed"] + 2 * i + 1).to(DEV)
    with torch.no_grad():
        got = model(x, 1.0)
    want = fx["injected_run"]
    assert_tuple_close(got[:1], want[:1], atol=G.TOL + G.LOGIT_SCALE_TOL * float(torch.as_tensor(want[0]).abs().max()), rtol=G.LOGIT_RTOL,
                       what=name + " injected logits")
    assert_tuple_close(got[1:6], want[1:6], atol=1e-6, what=name + " injected stats")
    assert_tuple_close(got[6:], want[6:], atol=0.0, rtol=1e-5, what=name + " injected flops")
    return len(list(model.blocks()))


def test_regnet_two_mask_groups_both_takes_the_fold(ops, monkeypatch):
    """the both_grp2 case of the regnet-groups golden: one gate per block, conv c once per mask group"""
    _switches(monkeypatch, True)
    calls = _counted(ops, monkeypatch)
    n = _regnet_groups_injected()
    assert calls["se_packed"] == 0 and calls["conv_packed"] == 0 and calls["grouped_chan_mfma_conv3x3_image"] == 0, calls
    assert calls["grouped_chan_mfma_conv3x3_image_gap"] == calls["se_gate_image"] == n and calls["conv_packed_gated"] == 2 * n, calls


@pytest.mark.parametrize("model", ["tiny", "groups"])
def test_both_switch_off_runs_none_of_the_new_ops(ops, monkeypatch, model):
    """USE_BOTH_SE_FUSED off and every other switch on: the 'both' blocks run today's calls"""
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_BOTH_SE_FUSED is False
    _switches(monkeypatch, False)
    calls = _counted(ops, monkeypatch)
    n = G._regnet_injected("both") if model == "tiny" else _regnet_groups_injected()
    assert all(calls[k] == 0 for k in NEW) and calls["se_packed"] > 0 and calls["conv_packed"] > 0, calls
    assert n is None or (calls["se_packed"] == n and calls["conv_packed"] == 2 * n), calls
