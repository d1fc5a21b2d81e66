"""lad_regnet_y_32gf (group width 232) on the matrix-core kernels of the `wide` family, end to end.

1. Training: one layer-skip block with w_b = 464 (two groups of 232), stride 1 and 2, through training.sparse_block_train with
   laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS and training.USE_WGRAD_GROUPED_WIDE on, in bf16x3 -- the forward's conv b and its adjoint on
   ops.grouped_wide_conv3x3_rows, conv b's weight gradient on ops.wgrad_grouped_wide_rows (exactly one call per backward, none of the
   gather + bmm fallback) -- against the float64 restatement of tests/train_ref.py on tie-free inputs, with the statement and the bound of
   tests/test_hip_training_grouped_wide_rows.py: the forward within 1e-3 of max |out64| with its sign pattern, every gradient within 1e-3 of
   max |want64| elementwise.  Cases (batch 3, image mask [1, 0, 1], 8 -> 464 with a projection shortcut): train_ref.make_tie_free's worst-case
   forward bound grows with the reduction length (K = 2088 in conv b, 464 in conv c), so the construction clears its factor 4 only on a 2 x 2
   output map at this width -- 8 kept rows -- at the first of the four seeds 31 / 1031 / 2031 / 3031 that succeeds (stride 1: 31, stride 2:
   2031; 3 x 3 and 4 x 4 fail at all four).  The clearance is asserted.
2. Full-width smoke: lad_regnet_y_32gf at 224 px with seeded weights and forced masks, in layer-skip and in channel mode, all three switches
   on against all off: the logits agree to 1e-3 max(1, |off|max), the project's model-level bound, and the new ops are called at all four
   stages (w_b 232 / 696 / 1392 / 3712).  Batch 2; the channel-mode switch-off leg runs the fp32 VALU kernel at width 232."""
import functools
from types import SimpleNamespace

import pytest
import torch

import train_ref as R
from fill import damp_residual_branches, fill_state_dict, seeded_bernoulli, seeded_randn
from helpers import assert_close
from test_hip_training_f64 import BOUND, _hip_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GW = 232
# name -> (width_in, width_out, stride, output map, seed)
CASES = {"gw232_s1_proj": (8, 464, 1, 2, 31), "gw232_s2_proj": (8, 464, 2, 2, 2031)}
STAGE_WIDTHS = [232, 696, 1392, 3712]


@functools.lru_cache(maxsize=None)
def _case(name):
    """the tie-free case and its float64 reference, built once per process and never modified"""
    win, wout, stride, omap, seed = CASES[name]
    size = omap * stride
    fx = dict(kind="regnet", mode="layer", stride=stride, gw=GW, widths=(win, wout), output_size=omap, seed=seed, x_seed=seed + 1,
              x_shape=[R.BATCH, win, size, size], masks={"spatial": torch.tensor(R.LAYER_MASK).view(R.BATCH, 1, 1, 1)},
              has_downsample=win != wout or stride != 1)
    x, params0 = R.case_input(fx), R.case_params(fx)
    params, got, moved = R.make_tie_free(params0, x, fx["masks"])
    case = SimpleNamespace(name=name, variant=None, fx=fx, params0=params0, params=params, x=x, masks=fx["masks"], clearance=got, moved=moved)
    gout = R.case_gout(case)
    out64, want, _ = R.gradients(params, x, fx["masks"], gout, torch.float64)
    return case, gout, out64, want


@pytest.mark.parametrize("name", list(CASES))
def test_block_trains_on_the_new_kernels_vs_float64(name, monkeypatch):
    from laudnet_amd import laud_regnet, ops, training
    from laudnet_amd.training import sparse_block_train
    case, gout, out64, want = _case(name)
    W = case.fx["widths"][1]
    assert case.clearance >= R.CLEARANCE, case.clearance
    assert R.BATCH == 3 and list(R.LAYER_MASK) == [1, 0, 1]
    assert training.USE_WGRAD_GROUPED_WIDE is False and laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS is False
    calls, valu, wgrad, fallback = [], [], [], []
    real, real_valu, real_wgrad, real_fallback = (ops.grouped_wide_conv3x3_rows, ops.grouped_conv3x3_rows, ops.wgrad_grouped_wide_rows,
                                                  training._weight_grad_grouped_3x3)

    def counted(a2d, nbr, w_frag, group_width, *args, **kwargs):
        calls.append((group_width, ops.get_math_mode(), tuple(a2d.shape)))
        return real(a2d, nbr, w_frag, group_width, *args, **kwargs)

    def counted_valu(a2d, nbr, w, group_width, *args, **kwargs):
        valu.append(group_width)
        return real_valu(a2d, nbr, w, group_width, *args, **kwargs)

    def counted_wgrad(dy2d, a2d, nbr, group_width, **kwargs):
        wgrad.append((group_width, dy2d.shape[1], ops.get_math_mode()))
        return real_wgrad(dy2d, a2d, nbr, group_width, **kwargs)

    def counted_fallback(*args, **kwargs):
        fallback.append(1)
        return real_fallback(*args, **kwargs)
    monkeypatch.setattr(ops, "grouped_wide_conv3x3_rows", counted)
    monkeypatch.setattr(ops, "grouped_conv3x3_rows", counted_valu)
    monkeypatch.setattr(ops, "wgrad_grouped_wide_rows", counted_wgrad)
    monkeypatch.setattr(training, "_weight_grad_grouped_3x3", counted_fallback)
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE_ROWS", True)
    monkeypatch.setattr(training, "USE_WGRAD_GROUPED_WIDE", True)
    ops.set_math_mode("bf16x3")
    try:
        blk = _hip_block(case)
        for p_ in blk.parameters():
            p_.requires_grad_(True)
        x = case.x.to(DEV).requires_grad_(True)
        mask = case.masks["spatial"].float().to(DEV).requires_grad_(True)
        out = sparse_block_train(blk, x, mask)
        forward_calls = len(calls)
        out.backward(gout.to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.set_math_mode("fp32")
    grads = {"x": x.grad, "mask.spatial": mask.grad, **{k: p_.grad for k, p_ in blk.named_parameters() if "masker" not in k}}
    for k, w in want.items():          # every figure before any assertion
        g = grads.get(k)
        scale = w.abs().max().item()
        fig = "missing" if g is None else (format(R.worst_ratio(g, w), ".3e") if scale > 0 else f"max |got| {g.abs().max().item():.3e}")
        print(f"training regnet_y32 {name}: d {k} ratio {fig} (scale {scale:.3e})")
    print(f"training regnet_y32 {name}: clearance {case.clearance:.2f}; forward ratio {R.worst_ratio(out.detach(), out64):.3e}; calls {calls}; wgrad {wgrad}")
    assert_close(out.detach(), out64, BOUND * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out.detach().cpu() > 0, out64 > 0), "the sign pattern of the output differs from float64's"
    assert len(want) == 1 + 1 + 3 + 6 + 4 + 3, sorted(want)
    for k, w in want.items():
        scale = w.abs().max().item()
        assert scale > 0, f"d {k}: the reference gradient vanishes"
        assert grads.get(k) is not None, f"d {k}: no gradient"
        assert_close(grads[k], w, BOUND * scale, 0, f"d {k}")
    assert forward_calls >= 1 and len(calls) - forward_calls >= 1, calls
    assert all(c[0] == GW and c[1] == "bf16x3" and c[2][1] == W for c in calls), calls
    assert valu == [] and fallback == [], (valu, fallback)
    assert wgrad == [(GW, W, "bf16x3")], f"exactly one call of ops.wgrad_grouped_wide_rows per backward: {wgrad}"


# ------------------------------------------------------------------ the whole model
def _logits(mode, on, monkeypatch):
    """-> (logits of one forward of the seeded model under its forced masks, the channel counts the two new forward ops were called with)"""
    import laudnet_amd
    from laudnet_amd import laud_regnet, ops, training
    B = 2
    for name in ("USE_GROUPED_MFMA_WIDE", "USE_GROUPED_MFMA_WIDE_ROWS"):
        monkeypatch.setattr(laud_regnet, name, on)
    monkeypatch.setattr(training, "USE_WGRAD_GROUPED_WIDE", on)
    if mode == "layer":
        net = laudnet_amd.lad_regnet_y_32gf(dyn_mode=["spatial"] * 4, mask_spatial_granularity=[56, 28, 14, 7], num_classes=1000, input_size=224)
    else:
        net = laudnet_amd.lad_regnet_y_32gf(dyn_mode=["channel"] * 4, channel_dyn_granularity=[8] * 4, channel_masker=["MLP"] * 4,
                                            channel_masker_layers=[2] * 4, num_classes=1000, input_size=224)
    net = net.eval()
    net.load_state_dict(damp_residual_branches(fill_state_dict(net.state_dict(), 1)))
    net = net.to(DEV)
    blocks = net.blocks()
    assert [b.f.w_b for b in blocks] == [232] * 2 + [696] * 5 + [1392] * 12 + [3712] and all(b.f.group_width == GW for b in blocks)
    for i, blk in enumerate(blocks):
        if mode == "layer":        # one decision per image; image 0 kept and image 1 skipped in turn, so every block has a kept image
            blk.f.forced_spatial_mask = torch.tensor([1.0, float(i % 2)]).view(B, 1, 1, 1).to(DEV)
        else:
            blk.f.forced_channel_mask = seeded_bernoulli((B, blk.f.masker_channel.channel_dyn_group), 0.5, 100 + i).to(DEV)
    x = seeded_randn((B, 3, 224, 224), 1000).to(DEV).contiguous(memory_format=torch.channels_last)
    seen = {"rows": [], "image": []}
    real_rows, real_image = ops.grouped_wide_conv3x3_rows, ops.grouped_wide_conv3x3_image

    def rows(a2d, nbr, w_frag, group_width, *args, **kwargs):
        seen["rows"].append(w_frag.shape[0] * group_width)
        return real_rows(a2d, nbr, w_frag, group_width, *args, **kwargs)

    def image(a, w_frag, group_width, *args, **kwargs):
        seen["image"].append(w_frag.shape[0] * group_width)
        return real_image(a, w_frag, group_width, *args, **kwargs)
    monkeypatch.setattr(ops, "grouped_wide_conv3x3_rows", rows)
    monkeypatch.setattr(ops, "grouped_wide_conv3x3_image", image)
    with torch.no_grad():
        y = net(x, 1.0)[0]
    torch.cuda.synchronize()
    out = y.clone()
    del net
    return out, seen


@pytest.mark.parametrize("mode", ["layer", "channel"])
def test_full_width_model_switches_on_against_off(mode, monkeypatch):
    from laudnet_amd import ops
    ops.set_math_mode("bf16x3")
    try:
        on, seen = _logits(mode, True, monkeypatch)
        monkeypatch.undo()
        off, seen_off = _logits(mode, False, monkeypatch)
    finally:
        ops.set_math_mode("fp32")
    assert tuple(on.shape) == (2, 1000) and torch.isfinite(on).all() and torch.isfinite(off).all()
    new = seen["rows"] if mode == "layer" else seen["image"]
    assert sorted(set(new)) == STAGE_WIDTHS, f"the new op must run at all four stages: {new}"
    assert len(new) == 20, new
    assert seen_off == {"rows": [], "image": []}, seen_off
    err, bound = (on - off).abs().max().item(), 1e-3 * max(1.0, off.abs().max().item())
    print(f"lad_regnet_y_32gf {mode}: switches on vs off max |logit diff| {err:.3e} (bound {bound:.3e}, |off|max {off.abs().max().item():.3e})")
    assert err < bound
