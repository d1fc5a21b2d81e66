"""Training of LAD-RegNet layer-skip blocks under frozen BatchNorm statistics (laudnet_amd/training.py: _RegNetSkipBranchFn) against the ORACLE's
autograd (oracle/regnet_ref.py: the reference's dense emulation, every BatchNorm in eval mode, the same hard mask as a leaf that requires grad).

Blocks (random weights, se_ratio 0.25, BatchNorm running statistics away from (0, 1): tests/golden/fill.py): the forward value and ALL gradients --
x, the mask's straight-through term, the a / b / c weights and their BatchNorm affine parameters, se.fc1 / se.fc2 weight and bias, proj and its
BatchNorm -- at group widths 8 / 16 / 24, stride 1 and stride 2 + proj, with kept and dropped images, all kept and all dropped; one case with the
weight-gradient kernels off (training.USE_WGRAD_KERNEL, the LDN_WGRAD=0 path) against the kernel path.  Whole model: the layer-skip configuration
of regnet_tiny.pt through train_forward against RegNetRef in training mode with identical Gumbel noise, fp32 arithmetic: the 7-tuple and the
gradient of every parameter of a loss over the logits and the FLOPs.  Tolerances: those of tests/test_hip_training.py (restated below)."""
import pytest
import torch
import torch.nn as nn

from fill import fill_state_dict, seeded_randn
from helpers import load_golden
from test_hip_training import GumbelTape, _relative_param_grads, oracle_cpu_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REGNET = load_golden("regnet_tiny.pt")


def _err(got, want):
    """max |got - want|, in units of max(1, max |want|): plain absolute error for O(1) tensors"""
    return (got - want).abs().max().item() / max(1.0, want.abs().max().item())


def _close(got, want, math_mode, what):
    """tests/test_hip_training.py::_close: fp32 arithmetic -- every element within 1e-3 (of max(1, scale)); bf16x3 arithmetic -- a pre-activation
    within the forward error of zero takes the other side of its ReLU: at most 8 % of the elements outside the tolerance, relative Frobenius
    error below 5 %.  That allowance is for inputs with near-ties and cannot tell a flipped unit from a wrong kernel; the strict statement --
    every element within 1e-3 of the tensor's own maximum, both modes, against float64, on inputs where no ReLU can flip -- lives in
    tests/test_hip_training_f64.py."""
    if math_mode != "bf16x3":
        assert _err(got, want) < 1e-3, f"{what}: {_err(got, want):.2e} (scale {want.abs().max().item():.2e})"
        return
    d = (got - want).abs()
    tol = 1e-3 * max(1.0, want.abs().max().item())
    frac = (d > tol).float().mean().item()
    fro = (d.norm() / want.norm().clamp(min=1e-12)).item()
    few = got.numel() < 2000
    assert (few or frac <= 0.08) and fro < 0.05, f"{what}: {100 * frac:.2f} % of the elements outside 1e-3, relative Frobenius error {fro:.2e}"


def _start(x):
    return (x, None, None, None, None, None, torch.tensor(0.0, device=x.device))


# name -> (width_in, width_out, group width, stride, output size, mask)
BLOCKS = {
    "gw8_s1": (32, 32, 8, 1, 14, [1, 0, 1, 1]),
    "gw16_s2_proj": (32, 64, 16, 2, 8, [0, 1, 1, 0]),
    "gw24_s1": (48, 48, 24, 1, 7, [1, 1, 0]),
    "gw8_s1_all_kept": (32, 32, 8, 1, 14, [1, 1, 1, 1]),
    "gw8_s1_all_dropped": (32, 32, 8, 1, 14, [0, 0, 0, 0]),
}


def _dyn(S, dyn_mode="spatial", gran=None):
    return dict(spatial_mask_channel_group=1, channel_dyn_granularity=1, output_size=S, mask_spatial_granularity=S if gran is None else gran,
                dyn_mode=dyn_mode)


def _make(name, seed=31):
    from laudnet_amd.laud_regnet import ResBottleneckBlock
    from oracle import regnet_ref as RR
    win, wout, gw, stride, S, mask = BLOCKS[name]
    hip = ResBottleneckBlock(win, wout, stride, nn.BatchNorm2d, nn.ReLU, gw, 1.0, 0.25, **_dyn(S)).eval()
    ref = RR.ResBlockRef(win, wout, stride, gw, 1.0, 0.25, **_dyn(S)).eval()          # eval mode: BatchNorm on its running statistics (frozen)
    sd = fill_state_dict(hip.state_dict(), seed)
    hip.load_state_dict(sd)
    ref.load_state_dict(sd)                                                             # the same state dict
    x = torch.relu(seeded_randn((len(mask), win, S * stride, S * stride), seed + 1))
    m = torch.tensor(mask, dtype=torch.float32).view(-1, 1, 1, 1)
    return hip.to(DEV), ref.to(DEV), x.to(DEV), m.to(DEV)


def _run_ref(ref, x0, mask0):
    xr, mr = x0.clone().requires_grad_(True), mask0.clone().requires_grad_(True)
    ref.f.forced_spatial_mask = mr
    for p_ in ref.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    out = ref(_start(xr), 1.0)[0]
    gout = seeded_randn(tuple(out.shape), 77).to(DEV)           # upstream gradient
    out.backward(gout)
    return out.detach(), xr.grad, mr.grad, {k: v.grad for k, v in ref.named_parameters()}, gout


def _run_hip(hip, x0, mask0, gout):
    from laudnet_amd.training import sparse_block_train
    xh, mh = x0.clone().requires_grad_(True), mask0.clone().requires_grad_(True)
    for p_ in hip.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    out = sparse_block_train(hip, xh, mh)
    out.backward(gout)
    torch.cuda.synchronize()
    return out.detach(), xh.grad, mh.grad, {k: v.grad for k, v in hip.named_parameters()}


def _compare(got, want, math_mode, has_proj):
    out_h, gx_h, gm_h, gp_h = got
    out_r, gx_r, gm_r, gp_r = want
    assert _err(out_h, out_r) < 1e-3, f"forward: {_err(out_h, out_r):.2e}"
    _close(gx_h, gx_r, math_mode, "d x")
    _close(gm_h, gm_r, math_mode, "straight-through term d mask")
    checked = []
    for pname, gh in gp_h.items():
        if "masker" in pname:
            continue                                             # (the mask is an input here: the masker is not part of the graph)
        assert gh is not None and gp_r[pname] is not None, pname
        _close(gh, gp_r[pname], math_mode, f"d {pname}")
        checked.append(pname)
    # three convs, three BatchNorms (weight + bias), the SE's two layers (weight + bias) [+ proj and its BatchNorm]
    assert len(checked) == 13 + (3 if has_proj else 0), checked
    for k in ("f.a.0.weight", "f.b.0.weight", "f.c.0.weight", "f.a.1.bias", "f.b.1.weight", "f.c.1.weight", "f.se.fc1.weight", "f.se.fc1.bias",
              "f.se.fc2.weight", "f.se.fc2.bias"):
        assert k in checked, k


@pytest.mark.parametrize("name", list(BLOCKS))
def test_regnet_block_gradients_vs_oracle_autograd(name, math_mode):
    from laudnet_amd import ops
    ops.set_math_mode(math_mode)
    try:
        hip, ref, x0, mask0 = _make(name)
        want = _run_ref(ref, x0, mask0)
        got = _run_hip(hip, x0, mask0, want[4])
        _compare(got, want[:4], math_mode, hip.proj is not None)
        assert want[2].abs().max().item() > 0, "the straight-through term must not vanish"
        if name.endswith("all_dropped"):
            for pname, gh in got[3].items():
                if pname.startswith("f.") and "masker" not in pname:
                    assert gh.abs().max().item() == 0, f"{pname}: a dropped image must leave no gradient on the branch"
            assert got[2].abs().max().item() > 0
    finally:
        ops.set_math_mode("fp32")


def test_regnet_block_wgrad_switch_off_agrees_with_the_kernel_path(monkeypatch):
    """training.USE_WGRAD_KERNEL = False (env LDN_WGRAD=0): the gather + bmm / GEMM weight gradients against the kernels' and the oracle's"""
    from laudnet_amd import ops, training
    ops.set_math_mode("fp32")
    hip, ref, x0, mask0 = _make("gw16_s2_proj")
    want = _run_ref(ref, x0, mask0)
    assert training.USE_WGRAD_KERNEL and training._wgrad_grouped_kernel(64, 16)
    on = _run_hip(hip, x0, mask0, want[4])
    monkeypatch.setattr(training, "USE_WGRAD_KERNEL", False)
    assert not training._wgrad_grouped_kernel(64, 16)
    off = _run_hip(hip, x0, mask0, want[4])
    _compare(off, want[:4], "fp32", True)
    _close(off[0], on[0], "fp32", "forward: switch off vs kernel")
    _close(off[1], on[1], "fp32", "d x: switch off vs kernel")
    for pname, g_on in on[3].items():
        if "masker" not in pname:
            _close(off[3][pname], g_on, "fp32", f"d {pname}: switch off vs kernel")


def test_regnet_training_scope_is_enforced():
    from laudnet_amd import LdnError
    from laudnet_amd.laud_regnet import ResBottleneckBlock
    from laudnet_amd.training import sparse_block_train
    x = torch.relu(seeded_randn((2, 32, 8, 8), 5)).to(DEV)
    bit = torch.ones(2, 1, 1, 1, device=DEV)
    mk = lambda **dyn: ResBottleneckBlock(32, 32, 1, nn.BatchNorm2d, nn.ReLU, 8, 1.0, 0.25, **dyn).eval().to(DEV)
    with pytest.raises(LdnError, match="not built"):                 # a channel block
        sparse_block_train(mk(**_dyn(8, "channel")), x, torch.ones(2, 32, device=DEV))
    with pytest.raises(LdnError, match="not built"):                 # a both block
        sparse_block_train(mk(**_dyn(8, "both")), x, (bit, torch.ones(2, 32, device=DEV)))
    with pytest.raises(LdnError, match="not built"):                 # patch masks: mask_size 2
        sparse_block_train(mk(**_dyn(8, "spatial", gran=4)), x, torch.ones(2, 1, 2, 2, device=DEV))
    with pytest.raises(LdnError, match="not built"):                 # two mask groups
        sparse_block_train(mk(**dict(_dyn(8), spatial_mask_channel_group=2)), x, torch.ones(2, 2, 1, 1, device=DEV))
    blk = mk(**_dyn(8))
    with pytest.raises(LdnError):                                    # a patch mask for a layer-skip block
        sparse_block_train(blk, x, torch.ones(2, 1, 2, 2, device=DEV))
    blk.f.b[1].train()
    with pytest.raises(LdnError):                                    # BatchNorm in batch-statistics mode
        sparse_block_train(blk, x, bit)


def _freeze_bn_train(model):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    return model


def test_regnet_train_step_vs_oracle():
    """The layer-skip configuration of regnet_tiny.pt: one training forward + backward of the whole model under frozen BatchNorm statistics, the
    keep / skip bits sampled from its own maskers with the oracle's Gumbel noise: the 7-tuple, and the gradient of EVERY parameter (stem,
    convolutions, BatchNorm affine terms, SE, proj, maskers, classifier) of a loss over the logits and the FLOPs."""
    import laudnet_amd
    from laudnet_amd import ops
    from laudnet_amd.training import prepare_for_training, train_forward
    from oracle import regnet_ref as RR
    ops.set_math_mode("fp32")     # (true-fp32 arithmetic: the Gumbel samples and every ReLU decision must coincide with the oracle's)
    fx = REGNET["cases"]["layerskip"]
    ref = RR.RegNetRef(REGNET["tiny_params"] | {}, se_ratio=REGNET["tiny_params"]["se_ratio"], **fx["kw"])
    hip = laudnet_amd.LAD_RegNet(laudnet_amd.BlockParams(**REGNET["tiny_params"]), **fx["kw"])
    sd = fill_state_dict(ref.state_dict(), fx["seed"])
    ref.load_state_dict(sd)
    hip.load_state_dict(sd)
    ref, hip = _freeze_bn_train(ref.to(DEV)), prepare_for_training(hip.to(DEV))
    size = fx["kw"]["input_size"]
    B = fx["batch"]
    x = seeded_randn((B, 3, size, size), fx["x_seed"]).to(DEV)
    g = seeded_randn((B, fx["kw"]["num_classes"]), 9).to(DEV)

    def loss_of(out):
        return (out[0] * g.to(out[0].device)).sum() / 10.0 + 10.0 * (out[5].mean() - 0.5) ** 2 + 1e-14 * out[6] ** 2

    tape = GumbelTape()
    torch.manual_seed(77)
    with tape.record():
        out_r = ref(x, 1.0)
    loss_of(out_r).backward()
    torch.manual_seed(77)
    out_h = train_forward(hip, x, 1.0)
    loss_of(out_h).backward()
    torch.cuda.synchronize()
    assert _err(out_h[0].detach(), out_r[0].detach()) < 1e-3, "logits"
    for i in (1, 2, 3, 4):
        assert len(out_h[i]) == len(out_r[i]) == 4
        for a, b in zip(out_h[i], out_r[i]):
            assert a.shape == b.shape and torch.allclose(a.detach().float(), b.detach().float(), atol=1e-6), i     # identical Gumbel samples
    assert torch.allclose(out_h[5].detach(), out_r[5].detach(), atol=1e-5)
    assert abs(float(out_h[6]) - float(out_r[6])) <= 1e-5 * float(out_r[6])
    kept = torch.cat([v.detach() for v in out_r[1]])
    assert 0 < float(kept.sum()) < kept.numel(), "the sampled bits must keep some blocks and drop some images"
    want = dict(ref.named_parameters())
    n = 0
    for name, p_ in hip.named_parameters():
        w = want[name].grad
        assert (w is None) == (p_.grad is None), f"{name}: gradient present on one side only"
        if w is not None:
            _close(p_.grad, w, "fp32", f"d {name}")
            n += 1
    assert n == len(want), (n, len(want))
    # the scale-relative statement for the tensors on which the oracle's CPU and GPU steps agree (tests/test_hip_training.py)
    cpu_grads = oracle_cpu_grads(ref, tape, lambda m, dev: loss_of(m(x.to(dev), 1.0)).backward())
    _relative_param_grads(hip, ref, cpu_grads, "regnet_tiny.pt::layerskip")
