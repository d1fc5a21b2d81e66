"""Zero, tiny (+-2^-24) and negative BatchNorm scales, against float64: the training path and, with the same parameters, the inference kernels.

Every parameter a test loads comes from tests/golden/fill.py, whose BatchNorm weights lie in [0.5, 1.5).  Real checkpoints hold zero, very small
and negative ones, and `LAD_MMDet_ResNet` is constructed with zero_init_residual: every bn3.weight exactly 0.  tests/train_ref.py's VARIANT_CASES
put such weights into eleven of the tie-free cases of tests/test_hip_training_f64.py (`mixed`: by channel index 0 / negated / +2^-24 / -2^-24 in
every BatchNorm of the block, the projection's included; `zero_last`: the last BatchNorm's weight all zero) BEFORE the tie-free construction,
which works at any scale (its bound carries |s|); tests/test_train_ref.py proves each of the 22 on the CPU, that `mixed` is not vacuous and which
gradients `zero_last` zeroes.

Training (both arithmetic modes, test_hip_training_f64's run_hip and _check_routes -- the same kernels run): the forward within 1e-3 of
max |out64| with its sign pattern; every gradient within 1e-3 max |want64| elementwise; exactly zero where want64 is identically zero; no NaN or
Inf anywhere.  What this caught: training.py used to recover d scale as sum dz (h - t) / s with the divisor 1 at s == 0 -- there h - t == 0, so
every zero-weight channel got d weight == 0 (a freshly constructed detection backbone could never leave bn3.weight == 0), and at |s| = 2^-24 the
difference h - t is rounding noise (profiles/train_parity_bn_scales.json: the parent's figures beside the fixed tree's).  One `mixed` case
runs the gather + GEMM weight gradients (training.USE_WGRAD_KERNEL off) to the same bounds.

Inference: the `mixed` parameters of the nine ResNet cases through the eval-mode `Bottleneck` (k_head / k_tail, conv_packed, the fused epilogues)
with the case's masks forced, both arithmetic modes: within 1e-3 of max |out64| with its sign pattern.  The tie-free construction bounds the
forward error of either arithmetic, so there is no allowance."""
import pytest
import torch

import train_ref as R
from helpers import apply_math_mode, assert_close, start_state  # noqa: F401  (apply_math_mode: autouse)
from test_hip_training_f64 import BOUND, DEV, _check_routes, _hip_block, run_hip

IDS = [f"{n}-{v}" for n, v in R.VARIANT_CASES]
RESNET_BASES = [n for n in R.VARIANT_BASES if not n.startswith("regnet")]


def _assert_against_float64(name, variant, math_mode, out, grads):
    case = R.tie_free_case(name, variant)
    out64, want, _ = R.reference(name, variant=variant)
    tag = f"training bn scales {name}/{variant}[{math_mode}]"
    for k, w in want.items():          # every figure before any assertion
        g, scale = grads.get(k), w.abs().max().item()
        fig = "missing" if g is None else (format(R.worst_ratio(g, w), ".3e") if scale > 0 else f"max |got| {g.abs().max().item():.3e}")
        print(f"{tag}: d {k} ratio {fig} (scale {scale:.3e})")
    print(f"{tag}: forward ratio {R.worst_ratio(out, out64):.3e}")
    assert_close(out, out64, BOUND * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out.cpu() > 0, out64 > 0), "the sign pattern of the output differs from float64's"
    n = 1 + len(case.masks) + 3 + 6 + (4 if case.fx["kind"] == "regnet" else 0) + (3 if case.fx["has_downsample"] else 0)
    assert len(want) == n, (sorted(want), n)
    for k, w in want.items():
        g, scale = grads.get(k), w.abs().max().item()
        assert g is not None, f"d {k}: no gradient"
        assert bool(torch.isfinite(g).all()), f"d {k} holds NaN or Inf"
        if scale == 0:
            assert bool((g == 0).all()), f"d {k}: identically zero in float64, max |got| {g.abs().max().item():.3e}"
        else:
            assert_close(g, w, BOUND * scale, 0, f"d {k}")
    return case, want


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", R.VARIANT_CASES, ids=IDS)
def test_block_gradients_vs_float64_with_edited_bn_scales(name, variant, math_mode):
    out, grads, calls = run_hip(name, variant)
    case, want = _assert_against_float64(name, variant, math_mode, out, grads)
    if variant == "mixed":             # stated directly: the zero-weight channels of the last BatchNorm get their gradient
        key = R.last_bn(case.params["sd"]) + ".weight"
        zero = R.mixed_classes(want[key].numel())["zero"]
        assert grads[key].cpu()[zero].abs().max().item() >= 0.1 * want[key].abs().max().item() - BOUND * want[key].abs().max().item()
    _check_routes(case, calls, math_mode)


@pytest.mark.gpu
def test_gather_gemm_weight_gradients_with_edited_bn_scales(monkeypatch):
    """the path without ldn_wgrad_rows (training.USE_WGRAD_KERNEL off) makes d W and d scale of the same dz^T A: the same bounds, fp32
    arithmetic, no route check (the weight-gradient kernel must NOT run)"""
    from laudnet_amd import ops, training
    monkeypatch.setattr(training, "USE_WGRAD_KERNEL", False)
    ops.set_math_mode("fp32")
    out, grads, calls = run_hip("narrow_s2_both", "mixed")
    assert not calls["wgrad_rows"], calls["wgrad_rows"]
    _assert_against_float64("narrow_s2_both", "mixed", "fp32", out, grads)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RESNET_BASES)
def test_eval_forward_vs_float64_with_mixed_bn_scales(name, math_mode):
    """the inference kernels on the same parameters: the eval-mode Bottleneck with the case's masks forced"""
    case = R.tie_free_case(name, "mixed")
    out64, _, _ = R.reference(name, variant="mixed")
    blk = _hip_block(case).eval()
    blk.forced_spatial_mask = case.masks["spatial"].float() if "spatial" in case.masks else None
    blk.forced_channel_mask = case.masks["channel"].float().to(DEV) if "channel" in case.masks else None
    with torch.no_grad():
        out = blk(start_state(case.x.to(DEV)), 1.0)[0]
    torch.cuda.synchronize()
    print(f"eval bn scales {name}/mixed[{math_mode}]: forward ratio {R.worst_ratio(out, out64):.3e}")
    assert bool(torch.isfinite(out).all())
    assert_close(out, out64, BOUND * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out.cpu() > 0, out64 > 0), "the sign pattern of the output differs from float64's"
