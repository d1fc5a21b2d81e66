"""Shared test helpers (CPU and GPU tests)."""
from __future__ import annotations

import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn  # tests/golden/fill.py

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return torch.load(os.path.join(GOLDEN, name), weights_only=False)


def block_input(fx):
    return F.relu(seeded_randn(fx["x_shape"], fx["x_seed"]))


def start_state(x):
    return (x, None, None, None, None, None, torch.tensor(0.0, device=x.device))


def make_block(block_cls, fx, conv_cls=nn.Conv2d):
    """Instantiate `block_cls` (oracle BottleneckRef or the HIP-backed Bottleneck) from a block fixture."""
    kw = dict(fx["kw"])
    down = None
    if fx["has_downsample"]:
        down = nn.Sequential(nn.Conv2d(kw["inplanes"], kw["planes"] * 4, 1, stride=kw["stride"], bias=False),
                             nn.BatchNorm2d(kw["planes"] * 4))
    blk = block_cls(downsample=down, **kw).eval()
    blk.load_state_dict(fill_state_dict(blk.state_dict(), fx["seed"]))
    return blk


def full_model_blocks(model):
    return [(f"layer{s}.{j}", b) for s in (1, 2, 3, 4) for j, b in enumerate(getattr(model, f"layer{s}"))]


def injected_masks_for(blocks, batch, seed, p_spatial=0.5, p_channel=0.62):
    """Same recipe as tests/golden/make_golden.py:injected_masks_for (kept in step by
    test_oracle_golden.py::test_full_models_injected)."""
    masks = {}
    for i, (name, blk) in enumerate(blocks):
        entry = {}
        if blk.masker_spatial is not None:
            entry["spatial"] = seeded_bernoulli((batch, blk.masker_spatial.groups, blk.masker_spatial.mask_size,
                                                 blk.masker_spatial.mask_size), p_spatial, seed + 2 * i)
        if blk.masker_channel is not None:
            entry["channel"] = seeded_bernoulli((batch, blk.masker_channel.groups), p_channel, seed + 2 * i + 1)
        masks[name] = entry
    return masks


def assert_tuple_close(got, want, atol, rtol=0.0, what=""):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, (list, tuple)):
            assert_tuple_close(g, w, atol, rtol, f"{what}[{i}]")
        else:
            g = torch.as_tensor(g).detach().float().cpu()
            w = torch.as_tensor(w).detach().float().cpu()
            assert g.shape == w.shape, f"{what}[{i}] shape {tuple(g.shape)} vs {tuple(w.shape)}"
            err = (g - w).abs()
            bound = atol + rtol * w.abs()
            assert bool((err <= bound).all()), f"{what}[{i}] max err {err.max().item():.3e} (atol {atol}, rtol {rtol})"


# ---- float64 references of the op-level parity tests (test_hip_packed.py, test_hip_regnet_ops.py) ----------------------------
def upsample_mask(mask, Ho, Wo):
    """[..., Sy, Sx] patch mask -> [..., Ho, Wo] (nearest; even grids, where F.interpolate(mode="nearest") is this repeat)."""
    Sy, Sx = mask.shape[-2:]
    assert Ho % Sy == 0 and Wo % Sx == 0
    return mask.repeat_interleave(Ho // Sy, dim=-2).repeat_interleave(Wo // Sx, dim=-1)


def bn_shift_f64(bn):
    """eval BatchNorm as y = scale * x + shift: the shift, in float64."""
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return bn.bias.double() - bn.running_mean.double() * scale


def bottleneck_stages_f64(blk, x, group_mask, m3):
    """Every intermediate tensor of a `both`-mode bottleneck by the dense-emulation algebra of oracle.torch_ref.BottleneckRef.forward
    (laud_resnet.py:115-144: channel mask before bn1 / bn2, spatial mask on bn3's output), in float64.
    blk: a BottleneckRef in .double(); x [B,cin,H,W]; group_mask [B,G] {0,1}; m3 [B,g,Ho,Wo] {0,1} at the OUTPUT resolution.
    Returns (h1, h2, y3, identity, out), NCHW float64."""
    from oracle import torch_ref as TR
    with torch.no_grad():
        x = x.double()
        cm = TR.broadcast_channel_mask(group_mask.double(), blk.conv1.out_channels)
        h1 = F.relu(blk.bn1(blk.conv1(x) * cm))
        h2 = F.relu(blk.bn2(blk.conv2(h1) * cm))
        y3 = blk.bn3(blk.conv3(h2))
        identity = x if blk.downsample is None else blk.downsample(x)
        out = F.relu(y3 * TR.broadcast_spatial_mask(m3.double(), y3.shape[1]) + identity)
    return h1, h2, y3, identity, out


def se_f64(rows, w1, b1, w2, b2):
    """torchvision SqueezeExcitation on one image's packed rows [n, C] in float64: (gate [C], scaled rows [n, C])."""
    rows = rows.double()
    mean = rows.mean(dim=0)
    gate = torch.sigmoid(w2.double() @ torch.relu(w1.double() @ mean + b1.double()) + b2.double())
    return gate, rows * gate


def assert_close(got, want, atol, rtol, what=""):
    """|got - want| <= atol + rtol |want| elementwise, want in float64; prints the worst element."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if got.numel() == 0:
        return 0.0
    excess = (got - want).abs() - (atol + rtol * want.abs())
    assert not bool(torch.isnan(got).any()), f"{what}: NaN in the result"
    worst = int(excess.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(worst), got.shape))
    err = (got - want).abs().max().item()
    assert excess.flatten()[worst].item() <= 0, (f"{what}: |err| {abs(got[idx] - want[idx]).item():.3e} at {idx} (want {want[idx].item():.6g}) exceeds "
                                                 f"atol {atol} + rtol {rtol}; max |err| {err:.3e}")
    return err


@pytest.fixture(autouse=True)
def apply_math_mode(request):
    """Import into a test module: every test there that takes the conftest's `math_mode` parameter runs with that arithmetic mode as
    the thread's default and leaves "fp32" behind."""
    if "math_mode" not in request.fixturenames:
        yield
        return
    from laudnet_amd import ops
    ops.set_math_mode(request.getfixturevalue("math_mode"))
    yield
    ops.set_math_mode("fp32")
