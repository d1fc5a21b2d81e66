"""The float64 restatement of LAD-RegNet channel-mode training on BATCH statistics (tests/regnet_bn_ref.py: the equations behind
training._RegNetBatchStatsBranchFn, ldn_rows_bn_postmask_fwd and ldn_rows_bn_postmask_bwd) against autograd of oracle/regnet_ref.ResBlockRef in
.train(), both in float64 on the CPU, on the block cases of the GPU tests, plain and with train_ref's `mixed` BatchNorm-weight edit.  Checked:
the forward, d x, d mask, all 13 (+3 with proj) parameter gradients, the batch statistics (through the running statistics the oracle's
BatchNorms keep after the forward -- they are affine in the batch mean and the unbiased batch variance).  Bound: 1e-11 of max(1, the tensor's own
maximum), the bound of tests/test_regnet_channel_ref.py -- two float64 evaluations of sums of at most a few thousand O(1) terms differ by
reordering alone, ~1e-13.  Imports nothing of laudnet_amd."""
import pytest
import torch

import regnet_bn_ref as R
from fill import seeded_randn

BOUND = 1e-11


def _err(got, want):
    return (got - want).abs().max().item() / max(1.0, want.abs().max().item())


def _step_vs_oracle(name, variant=None):
    ref, sd = R.make_ref_block(name, variant=variant)
    ref = ref.double()
    bns = {k: m_ for k, m_ in ref.named_modules() if isinstance(m_, torch.nn.BatchNorm2d) and "masker" not in k}
    assert all(bn.training and bn.momentum == R.MOMENTUM and bn.eps == R.EPS for bn in bns.values())
    x, m = R.case_inputs(name)
    xr, mr = x.double().requires_grad_(True), m.double().requires_grad_(True)
    ref.f.forced_channel_mask = mr
    out = ref(R.start_state(xr), 1.0)[0]
    gout = seeded_randn(tuple(out.shape), 77)
    out.backward(gout.double())
    got = R.block_step_f64(name, sd, x, m, gout)
    assert _err(got[0], out.detach()) < BOUND, "forward"
    assert _err(got[1], xr.grad) < BOUND, "d x"
    assert _err(got[2], mr.grad) < BOUND, "d mask"
    assert mr.grad.abs().max().item() > 0, "the straight-through term must not vanish"
    checked = 0
    for pname, p_ in ref.named_parameters():
        if "masker" in pname:
            assert p_.grad is None, pname                     # (the mask is an input: the masker is not part of the graph)
            continue
        assert _err(got[3][pname], p_.grad) < BOUND, f"d {pname}"
        checked += 1
    assert checked == 13 + (3 if ref.proj is not None else 0) == len(got[3])
    # the batch statistics, as the oracle's BatchNorms recorded them: running = 0.9 old + 0.1 batch (unbiased variance), once
    assert sorted(got[4]) == sorted(bns) and len(bns) == 3 + (1 if ref.proj is not None else 0)
    for pre, (mean, var, run_mean, run_var) in got[4].items():
        assert _err(run_mean, bns[pre].running_mean) < BOUND, f"{pre}.running_mean"
        assert _err(run_var, bns[pre].running_var) < BOUND, f"{pre}.running_var"
        assert (run_mean - sd[pre + ".running_mean"].double()).abs().max().item() > 1e-3, f"{pre}: the statistics must have moved"
        assert int(bns[pre].num_batches_tracked) == int(sd[pre + ".num_batches_tracked"]) + 1
        assert bool((var >= 0).all()) and mean.shape == var.shape
    return got


@pytest.mark.parametrize("variant", [None, "mixed"], ids=["plain", "mixed"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_block_step_vs_oracle_autograd_f64(name, variant):
    got = _step_vs_oracle(name, variant)
    if name == "gw8_s1_all_off" and variant is None:
        # every unit masked: conv c sees zeros, so its BatchNorm's output is the constant bias -- only f.c.1.bias and the mask keep a gradient
        # on the branch (the statistics' terms of bn_c cancel d weight exactly at var == 0: xhat == 0)
        for pname, gr in got[3].items():
            if pname != "f.c.1.bias" and not pname.startswith("proj"):
                assert gr.abs().max().item() == 0, pname
        assert got[3]["f.c.1.bias"].abs().max().item() > 0 and got[2].abs().max().item() > 0


def test_mixed_bn_scales_keep_their_weight_gradients():
    """zero, negated and +-2^-24 BatchNorm weights: nothing divides by a weight, and the zero-weight channels of bn_a / bn_b / bn_c carry a
    weight gradient while du of their layer is zero"""
    from train_ref import mixed_classes
    got = _step_vs_oracle("gw16_s2_proj_g2", "mixed")
    for k in ("f.a.1.weight", "f.b.1.weight", "f.c.1.weight", "proj.1.weight"):
        assert got[3][k][mixed_classes(got[3][k].numel())["zero"]].abs().max().item() > 0, k


def test_row_ops_restatement_properties():
    """the two ops on rows, by themselves: the gate is read from the stored h, g_mask lives on a channel dropped in every image, gamma == 0
    leaves du == 0 with d_gamma != 0"""
    g = torch.Generator().manual_seed(5)
    n, C, B = 50, 8, 2
    u, dz = torch.randn(n, C, generator=g).double(), torch.randn(n, C, generator=g).double()
    img = (torch.arange(n) >= 20).long()
    cm = torch.ones(B, C).double()
    cm[:, 1] = 0.0
    gamma, beta = torch.randn(C, generator=g).double(), torch.randn(C, generator=g).double()
    gamma[4] = 0.0
    beta[4] = 0.5
    mean, var, inv = R.bn_stats(u)
    h = R.bn_postmask_fwd(u, mean, inv, gamma, beta, cm, img)
    assert bool((h[:, 1] == 0).all())
    du, dg, db, gm = R.bn_postmask_bwd(dz, u, h, mean, inv, gamma, beta, cm, img, B=B)
    assert gm[:, 1].abs().max().item() > 0 and dg[1] == 0 and db[1] == 0
    assert bool((du[:, 4] == 0).all()) and dg[4].abs().item() > 0
    assert (du.sum(0).abs().max().item() < 1e-12), "d u sums to zero over the rows: the mean's own gradient"
