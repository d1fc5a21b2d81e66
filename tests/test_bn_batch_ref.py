"""tests/bn_batch_ref.py (the float64 restatement the batch-statistics kernels are tested against) tied to torch: the three ops against
torch.nn.functional.batch_norm(training=True) autograd in float64 -- plain and with the channel mask / the pixel-mask row factor -- and one
training step of a block of each dyn_mode against autograd of oracle.torch_ref.BottleneckRef with its BatchNorms in .train().  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import bn_batch_ref as R
from helpers import block_input, load_golden, make_block

BLOCKS = dict(load_golden("blocks_s1.pt"))
BLOCKS.update(load_golden("blocks_s2.pt"))
EPS = 1e-5


@pytest.mark.parametrize("masked,relu,scaled", [(False, True, False), (True, True, False), (False, False, True), (True, False, True)])
def test_ops_vs_functional_batch_norm_autograd(masked, relu, scaled):
    g = torch.Generator().manual_seed(5)
    B, P, C = 3, 7, 8
    n = B * P
    u = torch.randn(n, C, dtype=torch.float64, generator=g) * 2 + 1
    img = torch.arange(B).repeat_interleave(P)
    cm = (torch.rand(B, C, generator=g) < 0.6).double() if masked else None
    rs = (torch.rand(n, generator=g) < 0.5).double() if scaled else None
    gamma = torch.randn(C, dtype=torch.float64, generator=g)
    gamma[0] = 0.0
    beta = torch.randn(C, dtype=torch.float64, generator=g)
    beta[0] = 0.5                                            # (gamma == 0: z = beta, the ReLU stays open)
    dh = torch.randn(n, C, dtype=torch.float64, generator=g)

    ua, ga, ba = u.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    cma = None if cm is None else cm.clone().requires_grad_(True)
    x = ua if cma is None else ua * cma[img]
    z = F.batch_norm(x, None, None, ga, ba, training=True, eps=EPS)
    h = torch.relu(z) if relu else z
    h = h if rs is None else h * rs.unsqueeze(1)
    h.backward(dh)

    mean, var, inv = R.bn_stats(u, EPS, cm, img)
    xd = R._x(u, cm, img)
    assert torch.allclose(mean, xd.mean(0), atol=1e-12) and torch.allclose(var, xd.var(0, unbiased=False), atol=1e-12)
    got_h = R.bn_fwd(u, mean, inv, gamma, beta, cm, img, rs, relu)
    assert torch.allclose(got_h, h.detach(), atol=1e-12)
    du, dg, db, gm = R.bn_bwd(dh, u, got_h if relu else None, mean, inv, gamma, cm, img, rs, B=B if masked else None)
    assert torch.allclose(du, ua.grad, atol=1e-12), (du - ua.grad).abs().max()
    assert torch.allclose(dg, ga.grad, atol=1e-12) and torch.allclose(db, ba.grad, atol=1e-12)
    assert dg[0].abs() > 0, "d gamma at gamma == 0 must not vanish"
    if masked:
        assert torch.allclose(gm, cma.grad, atol=1e-12), (gm - cma.grad).abs().max()


def test_no_rows():
    mean, var, inv = R.bn_stats(torch.zeros(0, 4), EPS)
    assert mean.abs().max() == 0 and var.abs().max() == 0 and torch.allclose(inv, torch.full((4,), EPS, dtype=torch.float64) ** -0.5)


@pytest.mark.parametrize("name", ["spatial_g1_s1", "layer_s2", "channel_g2_s2", "both_s1"])
def test_block_step_vs_oracle_autograd(name):
    """one block of each dyn_mode: BottleneckRef.double() with every BatchNorm in .train() and the injected masks as differentiable inputs"""
    from oracle import torch_ref as TR
    fx = BLOCKS[name]
    mode = fx["kw"]["dyn_mode"]
    ref = make_block(TR.BottleneckRef, fx).double().train()
    hand = make_block(TR.BottleneckRef, fx).double().train()
    x0 = block_input(fx).double()
    xr = x0.clone().requires_grad_(True)
    sm = cmk = None
    if mode != "channel":
        sm = fx["spatial_mask"].double().clone().requires_grad_(True)
        ref.forced_spatial_mask = sm
    if mode in ("channel", "both"):
        cmk = fx["channel_mask"].double().clone().requires_grad_(True)
        ref.forced_channel_mask = cmk
    out_r = ref((xr, None, None, None, None, None, torch.tensor(0.0)), 1.0)[0]
    gout = torch.randn(out_r.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(77))
    out_r.backward(gout)

    W = ref.conv1.out_channels
    m3 = None if sm is None else F.interpolate(sm.detach(), size=out_r.shape[2:], mode="nearest")
    assert m3 is None or m3.shape[1] == 1
    chm = None if cmk is None else TR.broadcast_channel_mask(cmk.detach(), W).reshape(x0.shape[0], W)
    out_h, grads, stats = R.block_step(hand, x0, gout, m3, chm)
    assert torch.allclose(out_h, out_r.detach(), atol=1e-10)
    assert torch.allclose(grads["x"], xr.grad, atol=1e-9), (grads["x"] - xr.grad).abs().max()
    want = {n: p_.grad for n, p_ in ref.named_parameters()}
    for k in ("conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias", "bn3.weight", "bn3.bias"):
        scale = max(1.0, want[k].abs().max().item())
        assert torch.allclose(grads[k], want[k], atol=1e-9 * scale), (k, (grads[k] - want[k]).abs().max())
    if sm is not None:       # the gradient of the mask at ITS size: nearest upsampling's adjoint sums the cells
        S = sm.shape[2]
        gm = grads["m3"].view(*grads["m3"].shape[:2], S, m3.shape[2] // S, S, m3.shape[3] // S).sum((3, 5))
        assert torch.allclose(gm, sm.grad, atol=1e-9 * max(1.0, sm.grad.abs().max().item()))
    if cmk is not None:
        G = cmk.shape[1]
        gc = grads["chm"].view(x0.shape[0], G, W // G).sum(2)
        assert torch.allclose(gc, cmk.grad, atol=1e-9 * max(1.0, cmk.grad.abs().max().item()))
    for bn, (mean, var, n) in zip((ref.bn1, ref.bn2, ref.bn3), stats):     # the oracle's running statistics moved once from their loaded values
        bn0 = getattr(hand, {ref.bn1: "bn1", ref.bn2: "bn2", ref.bn3: "bn3"}[bn])
        assert torch.allclose(bn.running_mean, 0.9 * bn0.running_mean + 0.1 * mean, atol=1e-12)
        assert torch.allclose(bn.running_var, 0.9 * bn0.running_var + 0.1 * var * n / (n - 1), atol=1e-12)
