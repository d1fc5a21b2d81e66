"""The closed forms of LAD-RegNet channel-mode training (tests/regnet_channel_ref.py: the equations behind training._RegNetChannelBranchFn,
ldn_rows_postmask_bwd and ldn_rows_img_dot) against autograd of oracle/regnet_ref.ResBlockRef, both in float64 on the CPU, on the block cases
of the GPU tests.  Bound: 1e-11 of max(1, the tensor's own maximum) -- two float64 evaluations of sums of at most a few thousand O(1) terms
differ by reordering alone, ~1e-13.  Imports nothing of laudnet_amd."""
import pytest
import torch

import regnet_channel_ref as R
from fill import seeded_randn


def _err(got, want):
    return (got - want).abs().max().item() / max(1.0, want.abs().max().item())


def test_closed_forms_vs_oracle_autograd_f64_mixed_bn_scales():
    """zero, negated and +-2^-24 BatchNorm weights (train_ref's `mixed` edit) in the state dict of gw16_s2_proj_g2: the closed forms divide by no
    scale, and the zero-weight channels of every BatchNorm of the branch carry a weight gradient"""
    from train_ref import mixed_classes
    got = _closed_forms_vs_oracle("gw16_s2_proj_g2", "mixed")
    for k in ("f.a.1.weight", "f.b.1.weight", "f.c.1.weight", "proj.1.weight"):
        assert got[3][k][mixed_classes(got[3][k].numel())["zero"]].abs().max().item() > 0, k


@pytest.mark.parametrize("name", list(R.CASES))
def test_closed_forms_vs_oracle_autograd_f64(name):
    _closed_forms_vs_oracle(name)


def _closed_forms_vs_oracle(name, variant=None):
    ref, sd = R.make_ref_block(name, variant=variant)
    ref = ref.double()
    x, m = R.case_inputs(name)
    xr, mr = x.double().requires_grad_(True), m.double().requires_grad_(True)
    ref.f.forced_channel_mask = mr
    out = ref(R.start_state(xr), 1.0)[0]
    gout = seeded_randn(tuple(out.shape), 77)
    out.backward(gout.double())
    got = R.closed_form_f64(name, sd, x, m, gout)
    assert _err(got[0], out.detach()) < 1e-11, "forward"
    assert _err(got[1], xr.grad) < 1e-11, "d x"
    assert _err(got[2], mr.grad) < 1e-11, "d mask"
    assert mr.grad.abs().max().item() > 0, "the straight-through term must not vanish"
    checked = 0
    for pname, p_ in ref.named_parameters():
        if "masker" in pname:
            assert p_.grad is None, pname                     # (the mask is an input: the masker is not part of the graph)
            continue
        assert _err(got[3][pname], p_.grad) < 1e-11, f"d {pname}"
        checked += 1
    assert checked == 13 + (3 if ref.proj is not None else 0) == len(got[3])
    if name == "gw8_s1_all_off":
        # every unit masked: no gradient reaches the branch's weights -- c's BatchNorm shift t_c = bias - mean * s_c excepted, which both of its
        # affine parameters feed -- while the mask's own gradient lives
        for pname, gr in got[3].items():
            if not pname.startswith("f.c.1.") and not pname.startswith("proj"):
                assert gr.abs().max().item() == 0, pname
        assert got[2].abs().max().item() > 0
    return got
