"""Training's weight gradients on the library's own kernel (laudnet_amd/training.py: USE_WGRAD_KERNEL -> ops.wgrad_rows) at FULL-WIDTH blocks,
where ops.wgrad_rows_ok holds: inplanes 256 / width 64 / 256 output channels, the block's INPUT a 28 x 28 map, batch 2 -- spatial, layer and
channel modes, stride 1 (identity shortcut, 28 x 28 out) and stride 2 with a projection (14 x 14 out).

For every block the gradients of conv1 / conv2 / conv3 (and of everything else: input, BatchNorm affine terms, the mask's straight-through
term) come from `sparse_block_train` with the kernel ON, with it OFF (the gather + PyTorch GEMM path) and from the oracle's autograd
(oracle.torch_ref.BottleneckRef, BatchNorm in eval mode = frozen statistics).  Bounds, those of tests/test_hip_training.py::_close (imported):
    fp32 arithmetic:   every element within 1e-3 of max(1, max |want|);
    bf16x3 arithmetic: a pre-activation within the 1e-5-class forward error of zero takes the other side of its ReLU and ONE flipped unit moves
                       a 3x3 neighbourhood of d x and one filter of the weight gradients by O(1): at most 8 % of the elements outside that
                       tolerance (tensors of >= 2000 elements) and a relative Frobenius error below 5 %.
The kernel must have run exactly three times per backward with the switch on and not at all with it off (a wrapper around ops.wgrad_rows
counts: otherwise the fallback alone could pass).  The same wrapper is the test hook that POISONS what the kernel may not read: where a
device-side count is passed, the rows of dY past it are overwritten with NaN and the rows of a_rows past it with out-of-range indices before
the call -- so no saved row buffer's tail needed zero-initialising for the gradient to come out right.

The 28 x 28 input is the size the restated bf16x3 bar (one or two flipped ReLU units per tensor) was written for."""
import pytest
import torch

from fill import seeded_bernoulli, seeded_randn
from helpers import apply_math_mode, block_input, make_block  # noqa: F401  (apply_math_mode: autouse)
from test_hip_training import _close, _err, _start

DEV = "cuda:0"
CASES = [("spatial", 1), ("layer", 1), ("channel", 1), ("spatial", 2), ("layer", 2), ("channel", 2)]


def _fixture(mode, stride):
    planes, batch, inplanes = 64, 2, 256
    out_size = 28 // stride                                        # the block's input map is 28 x 28
    kw = dict(inplanes=inplanes, planes=planes, stride=stride, spatial_mask_channel_group=1, channel_dyn_granularity=2 if mode == "channel" else 1,
              output_size=out_size, mask_spatial_granularity=(4 // stride) if mode == "spatial" else 1, dyn_mode=mode, channel_masker="MLP",
              channel_masker_layers=2, reduction=16)
    seed = 900 + 10 * stride + len(mode)
    fx = dict(kw=kw, seed=seed, x_seed=seed + 1, x_shape=[batch, inplanes, out_size * stride, out_size * stride], has_downsample=stride != 1)
    if mode == "spatial":
        fx["mask"] = seeded_bernoulli((batch, 1, 7, 7), 0.5, seed + 2)
    elif mode == "layer":
        fx["mask"] = torch.tensor([1.0, 0.0]).view(batch, 1, 1, 1)
    else:
        fx["mask"] = seeded_bernoulli((batch, planes // 2), 0.6, seed + 3)
    return fx


def poisoning_wgrad_rows(real, calls, poisoned):
    """A stand-in for ops.wgrad_rows that counts the call (calls += (taps, dY shape, A shape, counted?)) and POISONS every row the kernel may not
    read: where a device-side count is passed, the rows of dY past it become NaN and the rows of a_rows past it out-of-range indices.  The
    poisoned copies are appended to `poisoned`: the caller zeroes them once the backward is over (a recycled NaN block would otherwise surface
    in the next torch.empty of some (uninitialised * 0) product).  Shared with tests/test_hip_training_f64.py."""
    def counted(dy2d, a2d, *, a_rows=None, taps=1, m_count=None, m_cap=None, a_valid=None, out=None, math=None):
        if m_count is not None:
            cap = m_cap if m_cap is not None else dy2d.shape[0]
            dead = torch.arange(dy2d.shape[0], device=dy2d.device) >= m_count.long()
            dy2d = dy2d.clone().masked_fill_(dead.unsqueeze(1), float("nan"))        # (in place on the copy: no temporary NaN block)
            if a_rows is not None:
                t = a_rows.view(-1, taps)
                dead_t = torch.arange(t.shape[0], device=t.device) >= m_count.long()
                a_rows = torch.where(dead_t.unsqueeze(1), torch.full_like(t, 1 << 30), t).reshape(a_rows.shape).contiguous()
            assert cap <= dy2d.shape[0]
            poisoned.append(dy2d)
        calls.append((taps, tuple(dy2d.shape), tuple(a2d.shape), m_count is not None))
        return real(dy2d, a2d, a_rows=a_rows, taps=taps, m_count=m_count, m_cap=m_cap, a_valid=a_valid, out=out, math=math)
    return counted


@pytest.mark.gpu
@pytest.mark.parametrize("mode,stride", CASES, ids=[f"{m}_s{s}" for m, s in CASES])
def test_full_width_block_weight_gradients(mode, stride, math_mode, monkeypatch):
    from laudnet_amd import ops, training
    from laudnet_amd.laud_resnet import Bottleneck
    from oracle import torch_ref as TR
    fx = _fixture(mode, stride)
    W, Cin, cout = 64, 256, 256
    assert ops.wgrad_rows_ok(Cin, W, 1) and ops.wgrad_rows_ok(W, W, 9) and ops.wgrad_rows_ok(W, cout, 1)
    ref = make_block(TR.BottleneckRef, fx).to(DEV)
    x0 = block_input(fx).to(DEV)
    mask0 = fx["mask"].float().to(DEV)
    assert (mask0 < 0.5).any() and (mask0 > 0.5).any(), "the fixture must keep and drop units"

    xr, mr = x0.clone().requires_grad_(True), mask0.clone().requires_grad_(True)
    if mode == "channel":
        ref.forced_channel_mask = mr
    else:
        ref.forced_spatial_mask = mr
    for p_ in ref.parameters():
        p_.requires_grad_(True)
    out_r = ref(_start(xr), 1.0)[0]
    gout = seeded_randn(tuple(out_r.shape), 77).to(DEV)
    out_r.backward(gout)
    want = {n: p_.grad for n, p_ in ref.named_parameters()}

    calls, poisoned = [], []
    counted = poisoning_wgrad_rows(ops.wgrad_rows, calls, poisoned)
    monkeypatch.setattr(ops, "wgrad_rows", counted)
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(training, "USE_WGRAD_KERNEL", on)
        calls.clear()
        hip = make_block(Bottleneck, fx).to(DEV)
        for p_ in hip.parameters():
            p_.requires_grad_(True)
        xh, mh = x0.clone().requires_grad_(True), mask0.clone().requires_grad_(True)
        out_h = training.sparse_block_train(hip, xh, mh)
        out_h.backward(gout)
        torch.cuda.synchronize()
        for t in poisoned:
            t.zero_()
        poisoned.clear()
        if on:
            assert len(calls) == 3, f"the kernel ran {len(calls)} times in one backward, expected 3: {calls}"
            assert sorted(c[0] for c in calls) == [1, 1, 9]
            assert all(c[3] for c in calls) == (mode != "channel")          # pixel masks pass their device-side counts, the channel path none
        else:
            assert not calls, f"USE_WGRAD_KERNEL = False still called the kernel: {calls}"
        tag = "kernel" if on else "gemm path"
        assert _err(out_h.detach(), out_r.detach()) < 1e-3, "forward"
        for name in ("conv1.weight", "conv2.weight", "conv3.weight"):
            g = dict(hip.named_parameters())[name].grad
            assert g is not None and bool(torch.isfinite(g).all()), f"{tag}: d {name} missing or not finite"
            print(f"training wgrad {mode}_s{stride}[{math_mode}] {tag}: d {name} err {_err(g, want[name]):.3e}")
            _close(g, want[name], math_mode, f"{tag}: d {name}")
            grads[(on, name)] = g.clone()
        checked = 0
        for name, p_ in hip.named_parameters():                              # nothing else moved: BatchNorm terms, the projection
            if "masker" in name:
                continue
            _close(p_.grad, want[name], math_mode, f"{tag}: d {name}")
            checked += 1
        assert checked >= 9 + (2 if fx["has_downsample"] else 0)
        _close(xh.grad, xr.grad, math_mode, f"{tag}: d x")
        _close(mh.grad, mr.grad, math_mode, f"{tag}: d mask")
    for name in ("conv1.weight", "conv2.weight", "conv3.weight"):            # the two paths sum the same products (same forward, same ReLU
        _close(grads[(True, name)], grads[(False, name)], "fp32", f"kernel vs gemm path: d {name}")      # decisions): the strict bound in both modes
