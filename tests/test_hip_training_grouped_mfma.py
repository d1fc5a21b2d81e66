"""Training through the matrix-core grouped 3x3 for group widths 8 and 24 (laud_regnet.USE_GROUPED_MFMA_WIDTHS on, bf16x3): one layer-skip
LAD-RegNet block per case through training.sparse_block_train -- the forward's conv b AND its adjoint (the same kernel over the transposed
neighbour table with per-group transposed weights) on ops.grouped_mfma_conv3x3_rows -- against the float64 restatement of tests/train_ref.py on
tie-free inputs, with the statement and the bound of tests/test_hip_training_f64.py: the forward within 1e-3 of max |out64| with its sign
pattern, every gradient (x, the mask, the three convolutions, every BatchNorm weight and bias, SE's four tensors, the projection) within 1e-3 of
max |want64| elementwise.

Cases (batch 3, image mask [1, 0, 1], 8 x 8 output maps): width 8 with w_b = 24 (24 -> 24, identity shortcut); width 24 with w_b = 48, stride 1
and stride 2 (16 x 16 -> 8 x 8), both 8 -> 48 with a projection shortcut.  The input width 8 is what lets train_ref.make_tie_free clear every
ReLU by 4 x the bf16x3 forward bound on an 8 x 8 map at w_b = 48: the bound grows with conv a's reduction length, and 48 -> 48 only clears on
3 x 3 maps (train_ref._MAPS: regnet_gw24_s1).  Seeds: the first of train_ref.find_map's ladder (31 + 1000 k) at which the construction succeeds."""
import functools
from types import SimpleNamespace

import pytest
import torch

import train_ref as R
from helpers import assert_close
from test_hip_training_f64 import BOUND, _hip_block

DEV = "cuda:0"
# name -> (width_in, width_out, group width, stride, seed)
CASES = {"gw8_s1": (24, 24, 8, 1, 2031), "gw24_s1_proj": (8, 48, 24, 1, 31), "gw24_s2_proj": (8, 48, 24, 2, 31)}
OUT_MAP = 8


@functools.lru_cache(maxsize=None)
def _case(name):
    """the tie-free case and its float64 reference, built once per process and never modified (train_ref.build_fixture's LAD-RegNet form)"""
    win, wout, gw, stride, seed = CASES[name]
    size = OUT_MAP * stride
    fx = dict(kind="regnet", mode="layer", stride=stride, gw=gw, widths=(win, wout), output_size=OUT_MAP, seed=seed, x_seed=seed + 1,
              x_shape=[R.BATCH, win, size, size], masks={"spatial": torch.tensor(R.LAYER_MASK).view(R.BATCH, 1, 1, 1)},
              has_downsample=win != wout or stride != 1)
    x, params0 = R.case_input(fx), R.case_params(fx)
    params, got, moved = R.make_tie_free(params0, x, fx["masks"])
    case = SimpleNamespace(name=name, variant=None, fx=fx, params0=params0, params=params, x=x, masks=fx["masks"], clearance=got, moved=moved)
    gout = R.case_gout(case)
    out64, want, _ = R.gradients(params, x, fx["masks"], gout, torch.float64)
    return case, gout, out64, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_block_gradients_vs_float64_on_the_new_kernel(name, monkeypatch):
    from laudnet_amd import laud_regnet, ops
    from laudnet_amd.training import sparse_block_train
    case, gout, out64, want = _case(name)
    gw, W = case.fx["gw"], case.fx["widths"][1]
    assert case.clearance >= R.CLEARANCE and case.fx["output_size"] == OUT_MAP
    calls, real = [], ops.grouped_mfma_conv3x3_rows

    def counted(a2d, nbr, w_frag, group_width, *args, **kwargs):
        calls.append((group_width, ops.get_math_mode(), tuple(a2d.shape)))
        return real(a2d, nbr, w_frag, group_width, *args, **kwargs)
    monkeypatch.setattr(ops, "grouped_mfma_conv3x3_rows", counted)
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS", True)
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
        print(f"training grouped_mfma {name}: d {k} ratio {'missing' if g is None else format(R.worst_ratio(g, w), '.3e')} (scale {w.abs().max().item():.3e})")
    print(f"training grouped_mfma {name}: forward ratio {R.worst_ratio(out.detach(), out64):.3e}; calls {calls}")
    assert_close(out.detach(), out64, BOUND * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out.detach().cpu() > 0, out64 > 0), "the sign pattern of the output differs from float64's"
    n = 1 + 1 + 3 + 6 + 4 + (3 if case.fx["has_downsample"] else 0)
    assert len(want) == n, (sorted(want), n)
    for k, w in want.items():
        scale = w.abs().max().item()
        assert scale > 0, f"d {k}: the reference gradient vanishes"
        assert grads.get(k) is not None, f"d {k}: no gradient"
        assert_close(grads[k], w, BOUND * scale, 0, f"d {k}")
    # the forward's conv b and its adjoint, both in bf16x3 (autograd runs the backward on a thread of its own)
    assert forward_calls >= 1 and len(calls) - forward_calls >= 1, calls
    assert all(c[0] == gw and c[1] == "bf16x3" and c[2][1] == W for c in calls), calls
