"""Training through the matrix-core packed-row grouped 3x3 at group widths 56 and 112 (laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS on, bf16x3): one
layer-skip LAD-RegNet block per case through training.sparse_block_train -- the forward's conv b AND its adjoint (the same kernel over the
transposed neighbour table with per-group transposed weights, packed by the same ops.pack_grouped_wide_weights) on
ops.grouped_wide_conv3x3_rows -- against the float64 restatement of tests/train_ref.py on tie-free inputs, with the statement and the bound of
tests/test_hip_training_f64.py: the forward within 1e-3 of max |out64| with its sign pattern, every gradient (x, the mask, the three
convolutions, every BatchNorm weight and bias, SE's four tensors, the projection) within 1e-3 of max |want64| elementwise.  The weight gradient
of conv b stays on the gather + PyTorch path at these widths (ops.wgrad_grouped_rows_ok is False: asserted).

Cases (batch 3, image mask [1, 0, 1]; every one 8 -> w_b with a projection shortcut, for the reason the width-24 test's docstring gives: the
bf16x3 forward bound that train_ref.make_tie_free has to clear 4 x grows with conv a's reduction length and with the map):
    gw56_s1_proj    8 -> 112, stride 1, 5 x 5 map, seed 31     50 kept rows: a full row tile and a ragged one
    gw56_s2_proj    8 -> 112, stride 2, 5 x 5 map, seed 31     50
    gw112_s1_proj   8 -> 224, stride 1, 4 x 4 map, seed 31     32: exactly one tile, two groups
    gw112_s2_proj   8 -> 112, stride 2, 3 x 3 map, seed 2031   18: a partial tile
Width 112 clears only on 3 x 3 and 4 x 4 maps.  The construction's clearance is asserted, so a drift in it fails loudly.

The two width-112 cases: SE squeezes to 0.25 x 8 = 2 channels, and in float64 fc1's output is negative in both of them for both kept images,
so fc1's ReLU passes nothing: d fc1.weight, d fc1.bias and d fc2.weight are IDENTICALLY ZERO in the reference (d fc2.bias and every other
gradient is not).  Those three are pinned by name in ZERO_IN_FLOAT64 and must come out exactly zero (the statement of
tests/test_hip_training_bn_scales.py for a gradient that float64 has identically zero); any other vanishing reference gradient fails the
test, as in tests/test_hip_training_f64.py.  The two width-56 cases exercise all four SE gradients; SE's backward does not depend on the
group width."""
import functools
from types import SimpleNamespace

import pytest
import torch

import train_ref as R
from helpers import assert_close
from test_hip_training_f64 import BOUND, _hip_block

DEV = "cuda:0"
# name -> (width_in, width_out, group width, stride, output map, seed)
CASES = {"gw56_s1_proj": (8, 112, 56, 1, 5, 31), "gw56_s2_proj": (8, 112, 56, 2, 5, 31),
         "gw112_s1_proj": (8, 224, 112, 1, 4, 31), "gw112_s2_proj": (8, 112, 112, 2, 3, 2031)}
_DEAD_FC1 = {"f.se.fc1.weight", "f.se.fc1.bias", "f.se.fc2.weight"}                               # (a dead fc1 ReLU: the docstring)
ZERO_IN_FLOAT64 = {"gw112_s1_proj": _DEAD_FC1, "gw112_s2_proj": _DEAD_FC1}


@functools.lru_cache(maxsize=None)
def _case(name):
    """the tie-free case and its float64 reference, built once per process and never modified (train_ref.build_fixture's LAD-RegNet form)"""
    win, wout, gw, stride, omap, seed = CASES[name]
    size = omap * stride
    fx = dict(kind="regnet", mode="layer", stride=stride, gw=gw, widths=(win, wout), output_size=omap, seed=seed, x_seed=seed + 1,
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
    gw, W, omap = case.fx["gw"], case.fx["widths"][1], case.fx["output_size"]
    assert case.clearance >= R.CLEARANCE, case.clearance
    assert R.BATCH == 3 and list(R.LAYER_MASK) == [1, 0, 1]
    assert not ops.wgrad_grouped_rows_ok(W, gw), "the weight gradient of conv b runs on the gather + PyTorch path at these widths"
    calls, real = [], ops.grouped_wide_conv3x3_rows
    valu, real_valu = [], ops.grouped_conv3x3_rows

    def counted(a2d, nbr, w_frag, group_width, *args, **kwargs):
        calls.append((group_width, ops.get_math_mode(), tuple(a2d.shape), kwargs.get("m_cap")))
        return real(a2d, nbr, w_frag, group_width, *args, **kwargs)

    def counted_valu(a2d, nbr, w, group_width, *args, **kwargs):
        valu.append(group_width)
        return real_valu(a2d, nbr, w, group_width, *args, **kwargs)
    monkeypatch.setattr(ops, "grouped_wide_conv3x3_rows", counted)
    monkeypatch.setattr(ops, "grouped_conv3x3_rows", counted_valu)
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE_ROWS", True)
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
        print(f"training grouped_wide_rows {name}: d {k} ratio {fig} (scale {scale:.3e})")
    print(f"training grouped_wide_rows {name}: clearance {case.clearance:.2f}; forward ratio {R.worst_ratio(out.detach(), out64):.3e}; calls {calls}")
    assert_close(out.detach(), out64, BOUND * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out.detach().cpu() > 0, out64 > 0), "the sign pattern of the output differs from float64's"
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
    # the forward's conv b and its adjoint, both in bf16x3 (autograd runs the backward on a thread of its own), none on the VALU kernel
    assert forward_calls >= 1 and len(calls) - forward_calls >= 1, calls
    assert all(c[0] == gw and c[1] == "bf16x3" and c[2][1] == W for c in calls), calls
    assert valu == [], valu
