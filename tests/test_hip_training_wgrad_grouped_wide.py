"""Training with conv b's weight gradient on ldn_wgrad_grouped_wide_rows (training.USE_WGRAD_GROUPED_WIDE on; group widths 56 and 112): one
layer-skip LAD-RegNet block per case through training.sparse_block_train against the float64 restatement of tests/train_ref.py, on the cases
and with the statement of tests/test_hip_training_grouped_wide_rows.py -- the forward within 1e-3 of max |out64| with its sign pattern, every
gradient within 1e-3 of its own maximum elementwise, the gradients float64 has identically zero exactly zero.

Runs: all four cases in bf16x3 with the forward's switch (laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS) on too; gw56_s1_proj once more with the
forward on the VALU kernel -- the two switches are independent -- in bf16x3 and in fp32.  In every run ops.wgrad_grouped_wide_rows is called
exactly once per backward, with the case's group width and a device-side count, through the poisoning wrapper of tests/test_hip_training_f64.py
(NaN in dY's rows past the count, out-of-range table entries there), and training._weight_grad_grouped_3x3 is not called.

Two guards that nothing changed: with the new switch off (the default), and with it on under USE_WGRAD_KERNEL off, the fallback is called
once and the new op never."""
import pytest
import torch

import train_ref as R
from helpers import assert_close
from test_hip_training_f64 import BOUND, _hip_block, _poisoning_wgrad_grouped
from test_hip_training_grouped_wide_rows import CASES, ZERO_IN_FLOAT64, _case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(name, monkeypatch, mode, *, wide_wgrad, wide_forward, wgrad_kernel=True):
    """one forward + backward of the case -> (out, grads, calls of the new op, calls of the fallback)"""
    from laudnet_amd import laud_regnet, ops, training
    case, gout, out64, want = _case(name)
    assert case.clearance >= R.CLEARANCE, case.clearance
    calls, poisoned, fallback = [], [], []
    real_fallback = training._weight_grad_grouped_3x3

    def counted_fallback(*args, **kwargs):
        fallback.append(args[4])
        return real_fallback(*args, **kwargs)
    monkeypatch.setattr(ops, "wgrad_grouped_wide_rows", _poisoning_wgrad_grouped(ops.wgrad_grouped_wide_rows, calls, poisoned))
    monkeypatch.setattr(training, "_weight_grad_grouped_3x3", counted_fallback)
    monkeypatch.setattr(training, "USE_WGRAD_GROUPED_WIDE", wide_wgrad)
    monkeypatch.setattr(training, "USE_WGRAD_KERNEL", wgrad_kernel)
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE_ROWS", wide_forward)
    ops.set_math_mode(mode)
    try:
        blk = _hip_block(case)
        for p_ in blk.parameters():
            p_.requires_grad_(True)
        x = case.x.to(DEV).requires_grad_(True)
        mask = case.masks["spatial"].float().to(DEV).requires_grad_(True)
        out = training.sparse_block_train(blk, x, mask)
        assert calls == [] and fallback == [], "the forward computes no weight gradient"
        out.backward(gout.to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.set_math_mode("fp32")
        for t in poisoned:          # before they go back to the caching allocator
            t.zero_()
    grads = {"x": x.grad, "mask.spatial": mask.grad, **{k: p_.grad for k, p_ in blk.named_parameters() if "masker" not in k}}
    return out.detach(), grads, calls, fallback


def _assert_statement(name, tag, out, grads):
    case, gout, out64, want = _case(name)
    for k, w in want.items():          # every figure before any assertion
        g = grads.get(k)
        scale = w.abs().max().item()
        fig = "missing" if g is None else (format(R.worst_ratio(g, w), ".3e") if scale > 0 else f"max |got| {g.abs().max().item():.3e}")
        print(f"training wgrad_grouped_wide {name}[{tag}]: d {k} ratio {fig} (scale {scale:.3e})")
    print(f"training wgrad_grouped_wide {name}[{tag}]: clearance {case.clearance:.2f}; forward ratio {R.worst_ratio(out, out64):.3e}")
    assert_close(out, out64, BOUND * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out.cpu() > 0, out64 > 0), "the sign pattern of the output differs from float64's"
    n = 1 + 1 + 3 + 6 + 4 + (3 if case.fx["has_downsample"] else 0)
    assert len(want) == n, (sorted(want), n)
    for k, w in want.items():
        scale = w.abs().max().item()
        assert (scale == 0) == (k in ZERO_IN_FLOAT64.get(name, ())), f"d {k}: the reference gradient has scale {scale:.3e}"
        assert grads.get(k) is not None, f"d {k}: no gradient"
        if scale == 0:
            assert bool((grads[k] == 0).all()), f"d {k}: identically zero in float64, max |got| {grads[k].abs().max().item():.3e}"
        else:
            assert_close(grads[k], w, BOUND * scale, 0, f"d {k}")


def _assert_one_kernel_call(name, calls, fallback):
    case = _case(name)[0]
    gw, W = case.fx["gw"], case.fx["widths"][1]
    assert len(calls) == 1 and fallback == [], (calls, fallback)
    group_width, dy_shape, device_count = calls[0]
    assert group_width == gw and dy_shape[1] == W and device_count, calls


@pytest.mark.parametrize("name", list(CASES))
def test_block_gradients_vs_float64_with_the_wide_weight_gradient(name, monkeypatch):
    out, grads, calls, fallback = _run(name, monkeypatch, "bf16x3", wide_wgrad=True, wide_forward=True)
    _assert_statement(name, "bf16x3, forward on the matrix cores", out, grads)
    _assert_one_kernel_call(name, calls, fallback)


@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
def test_the_weight_gradient_switch_is_independent_of_the_forward_switch(mode, monkeypatch):
    name = "gw56_s1_proj"
    out, grads, calls, fallback = _run(name, monkeypatch, mode, wide_wgrad=True, wide_forward=False)
    _assert_statement(name, f"{mode}, forward on the VALU kernel", out, grads)
    _assert_one_kernel_call(name, calls, fallback)


def test_switch_off_is_the_default_and_runs_the_fallback(monkeypatch):
    from laudnet_amd import training
    assert training.USE_WGRAD_GROUPED_WIDE is False
    assert not training._wgrad_grouped_wide_kernel(112, 56) and not training._wgrad_grouped_kernel(112, 56)
    name = "gw56_s1_proj"
    out, grads, calls, fallback = _run(name, monkeypatch, "bf16x3", wide_wgrad=False, wide_forward=True)
    assert calls == [] and fallback == [56], (calls, fallback)
    _assert_statement(name, "bf16x3, switch off", out, grads)


def test_wgrad_kernel_switch_off_forces_the_fallback(monkeypatch):
    from laudnet_amd import training
    name = "gw56_s1_proj"
    out, grads, calls, fallback = _run(name, monkeypatch, "bf16x3", wide_wgrad=True, wide_forward=True, wgrad_kernel=False)
    assert not training._wgrad_grouped_wide_kernel(112, 56)
    assert calls == [] and fallback == [56], (calls, fallback)
    _assert_statement(name, "bf16x3, LDN_WGRAD off", out, grads)
