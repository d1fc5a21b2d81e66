"""Training gradients of ONE block against float64 on inputs where no ReLU can flip: every element of every tensor within 1e-3 of the tensor's own
maximum, both arithmetic modes -- no share of elements left out, no Frobenius substitute, no floor of 1 on the scale.

tests/test_hip_training.py::_close grants bf16x3 arithmetic 8 % of a tensor's elements and 5 % Frobenius error, because on the reference-generated
fixtures a pre-activation within the forward error of zero may land on the other side of its ReLU; that allowance cannot tell such a flip from a
kernel that drops a border tap or a ragged last tile.  Here the inputs are built so that no flip can happen (tests/train_ref.py: make_tie_free --
every pre-activation of every ReLU stands clear of zero by 4 x the worst-case bf16x3 forward error; tests/test_train_ref.py proves that for every
case on the CPU), so the backward is the same linear map on both sides and the reference is tests/train_ref.py's float64 restatement (tied to the
oracle's autograd there), computed once per case and shared by both modes.

Cases (train_ref.CASES; batch 3): ResNet bottlenecks narrow (planes 16: the channel algebra on conv_packed), mid (planes 32: in k_dense's
epilogue) and wide (inplanes 256 / planes 64), stride 1 + identity and stride 2 + projection, modes spatial (2 x 2-pixel patches), layer (image mask
[1, 0, 1]), channel (granularity 2) and both; LAD-RegNet layer-skip blocks at group widths 8 / 16 / 24.  The narrow cases run on the intended maps
(300 rows; 432 -> 108: a second, ragged 256-row tile, every kept list shorter than its capacity).  The worst-case bound grows with the reduction
lengths, so the wider cases can only be made tie-free on smaller maps (train_ref._MAPS states each and why); the factor 4 is never reduced.
Consequences, stated plainly: the 64-wide cases run on 12 - 192 rows, so the 64-wide k_dense / weight-gradient path sees no second row tile here
(the 32-wide mid cases carry that seam); and wide_s1_spatial / wide_s2_spatial have ONE patch per image -- a seeded per-image mask, layer skip
under another name, not 2 x 2-pixel patches.  "4 x the forward error" means 4 x train_ref's REFINED bound (the previous layer's bound counted at
the ON units only; its docstring gives the induction and what the unrefined formula would leave of this table).  Pixel-mask modes never call
ops.conv_packed at any width (training.py runs their chain on ops.conv_rows): "narrow -> conv_packed" holds for channel / both only.

Asserted per case and mode: the forward within 1e-3 of max |out64| with the sign pattern of out64; every gradient -- x, each mask, the three
convolutions, every BatchNorm weight and bias, the projection, SE's four tensors -- within 1e-3 max |want64| elementwise (helpers.assert_close names
the worst element); max |want64| > 0 for every tensor; and the intended kernels ran, counted by wrappers around the public ops: ops.wgrad_rows three
times per ResNet backward (taps 1, 1, 9; twice + ops.wgrad_grouped_rows once for LAD-RegNet) through the wrapper of tests/test_hip_training_wgrad.py
that poisons the rows past a device-side count with NaN, the convolutions on ops.conv_rows, and ops.conv_packed exactly where the channel algebra
cannot run in k_dense's epilogue (narrow channel / both; fp32 arithmetic of mid / wide channel / both) -- and every one of those calls, the
backward's included (autograd runs it on a thread of its own), under the arithmetic mode the test selected.

`measure` returns the figures without asserting (tools/train_parity_f64.py records them in profiles/train_parity_f64.json)."""
import pytest
import torch
import torch.nn as nn

import train_ref as R
from fill import fill_state_dict
from helpers import apply_math_mode, assert_close, make_block  # noqa: F401  (apply_math_mode: autouse)
from test_hip_training_wgrad import poisoning_wgrad_rows

DEV = "cuda:0"
BOUND = 1e-3        # of the tensor's own maximum: the project's parity bar (include/ldn_hip.h), here without floor or allowance


def _poisoning_wgrad_grouped(real, calls, poisoned):
    """poisoning_wgrad_rows for ops.wgrad_grouped_rows: NaN in the rows of dY past the device-side count, out-of-range indices in the table's"""
    def counted(dy2d, a2d, nbr, group_width, *, m_count=None, m_cap=None, a_valid=None, out=None, math=None):
        if m_count is not None:
            dead = torch.arange(dy2d.shape[0], device=dy2d.device) >= m_count.long()
            dy2d = dy2d.clone().masked_fill_(dead.unsqueeze(1), float("nan"))
            t = nbr.view(-1, 9)
            dead_t = torch.arange(t.shape[0], device=t.device) >= m_count.long()
            nbr = torch.where(dead_t.unsqueeze(1), torch.full_like(t, 1 << 30), t).reshape(nbr.shape).contiguous()
            poisoned.append(dy2d)
        calls.append((group_width, tuple(dy2d.shape), m_count is not None))
        return real(dy2d, a2d, nbr, group_width, m_count=m_count, m_cap=m_cap, a_valid=a_valid, out=out, math=math)
    return counted


def _hip_block(case):
    """the HIP-backed block of a case with the tie-free parameters"""
    from laudnet_amd.laud_regnet import ResBottleneckBlock
    from laudnet_amd.laud_resnet import Bottleneck
    fx = case.fx
    if fx["kind"] == "resnet":
        blk = make_block(Bottleneck, fx)
    else:
        S = fx["output_size"]
        blk = ResBottleneckBlock(*fx["widths"], fx["stride"], nn.BatchNorm2d, nn.ReLU, fx["gw"], 1.0, 0.25, spatial_mask_channel_group=1,
                                 channel_dyn_granularity=1, output_size=S, mask_spatial_granularity=S, dyn_mode="spatial").eval()
        blk.load_state_dict(fill_state_dict(blk.state_dict(), fx["seed"]))
    sd = blk.state_dict()
    if case.variant is not None:        # the variant's edit of the block's own seeded fill: what case.params0 must hold
        R.edit_bn_weights(sd, case.variant)
    for k, v in case.params["sd"].items():
        assert k in sd and sd[k].shape == v.shape, k
        moved = not torch.equal(v, case.params0["sd"][k])
        assert moved or torch.equal(sd[k].double(), v), f"{k}: the block's seeded fill differs from the reference's"
        sd[k] = v.float()
    blk.load_state_dict(sd)
    return blk.to(DEV)


def run_hip(name, variant=None):
    """sparse_block_train + backward of a case under the current arithmetic mode -> (out, grads named as train_ref.gradients names them, calls)"""
    from laudnet_amd import ops
    from laudnet_amd.training import sparse_block_train
    case = R.tie_free_case(name, variant)
    blk = _hip_block(case)
    for p_ in blk.parameters():
        p_.requires_grad_(True)
    x = case.x.to(DEV).requires_grad_(True)
    masks = {k: v.float().to(DEV).requires_grad_(True) for k, v in case.masks.items()}
    mask = (masks["spatial"], masks["channel"]) if case.fx["mode"] == "both" else next(iter(masks.values()))
    gout = R.case_gout(case).to(DEV)
    calls = {"wgrad_rows": [], "wgrad_grouped_rows": [], "conv_rows": [], "conv_packed": []}
    poisoned, modes = [], []
    real = {k: getattr(ops, k) for k in calls}

    def in_mode(fn):
        """notes the arithmetic mode the calling thread has selected (autograd runs the backward on a thread of its own)"""
        def noted(*args, **kwargs):
            modes.append(ops.get_math_mode())
            return fn(*args, **kwargs)
        return noted

    def counting(key):
        def counted(*args, **kwargs):
            calls[key].append(kwargs.get("taps", 1))
            return real[key](*args, **kwargs)
        return counted

    try:
        ops.wgrad_rows = in_mode(poisoning_wgrad_rows(real["wgrad_rows"], calls["wgrad_rows"], poisoned))
        ops.wgrad_grouped_rows = in_mode(_poisoning_wgrad_grouped(real["wgrad_grouped_rows"], calls["wgrad_grouped_rows"], poisoned))
        ops.conv_rows, ops.conv_packed = in_mode(counting("conv_rows")), in_mode(counting("conv_packed"))
        out = sparse_block_train(blk, x, mask)
        forward = {k: len(v) for k, v in calls.items()}          # what follows in each list is the backward's
        out.backward(gout)
        torch.cuda.synchronize()
    finally:
        for k, fn in real.items():
            setattr(ops, k, fn)
        for t in poisoned:          # before they go back to the caching allocator
            t.zero_()
    grads = {"x": x.grad, **{f"mask.{k}": v.grad for k, v in masks.items()}}
    grads.update({k: p_.grad for k, p_ in blk.named_parameters() if "masker" not in k})
    calls["modes"] = modes
    calls["backward"] = {k: calls[k][n:] for k, n in forward.items()}
    return out.detach(), grads, calls


def measure(name, variant=None):
    """-> {"forward" / tensor name: max |err| / max |want64|} of the HIP path under the current arithmetic mode, nothing asserted.  Where want64
    is identically zero (a BatchNorm scale variant) the figure is max |err| itself: 0.0 is the only passing value."""
    out64, want, _ = R.reference(name, variant=variant)
    out, grads, _ = run_hip(name, variant)
    res = {"forward": R.worst_ratio(out, out64)}
    for k, w in want.items():
        g = grads.get(k)
        res[k] = None if g is None else (R.worst_ratio(g, w) if w.abs().max().item() > 0 else float(g.double().abs().max()))
    return res


def _check_routes(case, calls, math_mode):
    from laudnet_amd import ops
    fx = case.fx
    # forward AND backward in the selected arithmetic: the weight-gradient calls come last and only from the backward
    assert set(calls["modes"]) == {math_mode}, f"kernels ran under {sorted(set(calls['modes']))}, the test selected {math_mode}"
    if fx["kind"] == "regnet":
        C, gw = fx["widths"][1], fx["gw"]
        assert ops.wgrad_grouped_rows_ok(C, gw) and ops.wgrad_rows_ok(fx["widths"][0], C, 1) and ops.wgrad_rows_ok(C, C, 1)
        assert len(calls["wgrad_grouped_rows"]) == 1 and calls["wgrad_grouped_rows"][0][0] == gw and calls["wgrad_grouped_rows"][0][2], calls
        assert sorted(c[0] for c in calls["wgrad_rows"]) == [1, 1] and all(c[3] for c in calls["wgrad_rows"]), calls
        assert calls["conv_rows"] and not calls["conv_packed"], calls
        assert calls["backward"]["conv_rows"].count(1) >= 2, calls["backward"]      # c^T and a^T (b^T is the grouped kernel over the transposed table)
        return
    Cin, W, mode = fx["kw"]["inplanes"], fx["kw"]["planes"], fx["mode"]
    assert ops.wgrad_rows_ok(Cin, W, 1) and ops.wgrad_rows_ok(W, W, 9) and ops.wgrad_rows_ok(W, 4 * W, 1)
    assert sorted(c[0] for c in calls["wgrad_rows"]) == [1, 1, 9], f"ops.wgrad_rows must run three times per backward: {calls['wgrad_rows']}"
    assert all(c[3] for c in calls["wgrad_rows"]) == (mode != "channel")      # pixel masks pass their device-side counts, the channel path none
    fwd_rows = calls["conv_rows"][:len(calls["conv_rows"]) - len(calls["backward"]["conv_rows"])]
    assert len(fwd_rows) + len(calls["conv_packed"]) - len(calls["backward"]["conv_packed"]) >= 3, calls      # the forward's three convolutions
    bwd = calls["backward"]["conv_rows"]                                        # the backward's transposed convolutions: conv3^T, conv2^T (nine
    assert bwd.count(1) >= 2 and bwd.count(9) >= 1, bwd                         # taps, through the transposed table), conv1^T -- on conv_rows
    assert len(calls["backward"]["wgrad_rows"]) == len(calls["wgrad_rows"])      # weight gradients: the backward's alone
    # this expectation MIRRORS training._conv_const / _shared.dense_channel_convs (ops.dense_kernel_ok(): bf16x3; every width a multiple of 32) --
    # a tripwire for a silent change of route, not an independent statement of where the channel algebra should run
    packed = mode in ("channel", "both") and (W % 32 != 0 or math_mode != "bf16x3")
    assert bool(calls["conv_packed"]) == packed, f"conv_packed ran {len(calls['conv_packed'])} times, expected {'some' if packed else 'none'}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.CASES)
def test_block_gradients_vs_float64_on_tie_free_inputs(name, math_mode):
    case = R.tie_free_case(name)
    assert case.clearance >= R.CLEARANCE
    out64, want, _ = R.reference(name)
    out, grads, calls = run_hip(name)
    for k, w in want.items():          # every figure before any assertion
        g = grads.get(k)
        print(f"training f64 {name}[{math_mode}]: d {k} ratio {'missing' if g is None else format(R.worst_ratio(g, w), '.3e')} (scale {w.abs().max().item():.3e})")
    print(f"training f64 {name}[{math_mode}]: forward ratio {R.worst_ratio(out, out64):.3e}")
    assert_close(out, out64, BOUND * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out.cpu() > 0, out64 > 0), "the sign pattern of the output differs from float64's"
    # x, the mask(s), three convolutions, three BatchNorms (weight + bias) [, SE's four tensors] [, the projection and its BatchNorm]
    n = 1 + len(case.masks) + 3 + 6 + (4 if case.fx["kind"] == "regnet" else 0) + (3 if case.fx["has_downsample"] else 0)
    assert len(want) == n, (sorted(want), n)
    for k, w in want.items():
        scale = w.abs().max().item()
        assert scale > 0, f"d {k}: the reference gradient vanishes"
        assert grads.get(k) is not None, f"d {k}: no gradient"
        assert_close(grads[k], w, BOUND * scale, 0, f"d {k}")
    _check_routes(case, calls, math_mode)
