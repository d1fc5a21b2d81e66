"""Training of token-skipping blocks with MORE than 256 kept tokens per image (adavit.USE_LONG_BWD: the attention backward on
ldn_packed_mha_bwd_long) against float64 autograd of oracle/adavit_ref.py -- the oracle step, the fill and the checks of
tests/test_hip_adavit_training.py: every element of every gradient within 1e-3 of that tensor's own maximum (BOUND), forward values within
1e-4 * max(1, max |want|).  Without the switch these shapes are refused (test_scope_refusals).  `measure` returns the figures without
asserting (tools/train_adavit_grad_err.py records them)."""
import subprocess
import sys

import pytest
import torch

import test_hip_adavit_training as short
from attn_bwd_ref import BOUND, grad_err, keep_pattern
from fill import seeded_bernoulli, seeded_randn
from oracle import adavit_ref as AR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (B, L, dim, heads, depth, head + layer skipping, keep probability)
CASES = {
    "block_300": (3, 300, 128, 2, 1, True, 0.93),            # kept [276, 1, 300]
    "trunk2_320": (3, 320, 64, 1, 2, False, 0.93),           # kept [301, 1, 320] and [296, 1, 320]
    "block_384px": (2, 577, 384, 6, 1, False, 0.7),          # kept [417, 394]: the 384 px DeiT-S shape
}
KEPT = {"block_300": [[276, 1, 300]], "trunk2_320": [[301, 1, 320], [296, 1, 320]], "block_384px": [[417, 394]]}
_BUILT = {}


def build(name):
    """(oracle trunk, x, upstream gradient, masks, float64 forward value, float64 gradients): computed once per case and left unchanged"""
    if name not in _BUILT:
        B, L, dim, heads, depth, skip, p = CASES[name]
        ref = AR.TokenSkipViTRef(depth, dim, heads)
        short._fill(ref, 100 + L)
        x = seeded_randn((B, L, dim), 21 + L)
        g = seeded_randn((B, L, dim), 22 + L)
        keeps = [keep_pattern(B, L, p, 23 + L + i) for i in range(depth)]
        if name == "block_384px":     # keep_pattern leaves image 1 its CLS token only: give it a Bernoulli row of its own
            keeps[0][1] = seeded_bernoulli((L,), p, 99)
            keeps[0][1, 0] = 1.0
        hks = aks = mks = None
        if skip:      # block_head_layer_skip's: image 0 drops head 0; image 2's attention is skipped but its MLP trains, image 0 the other way round
            hk = torch.ones(B, heads)
            hk[0, 0] = 0.0
            hks, aks, mks = [hk], [torch.tensor([1.0, 1.0, 0.0])], [torch.tensor([0.0, 1.0, 1.0])]
        masks = (keeps, hks, aks, mks)
        want_out, want = short._oracle_step(ref, x, g, masks, torch.float64, "cpu")
        _BUILT[name] = (ref, x, g, masks, want_out, want)
    return _BUILT[name]


def hip_step(name):
    """one forward + backward through train_forward with USE_LONG_BWD on -> (forward value, {name: gradient}) with the oracle's parameter names"""
    from laudnet_amd import adavit, ops
    ref, x, g, masks, _, _ = build(name)
    B, L, dim, heads, depth, _, _ = CASES[name]
    trunk = adavit.TokenSkipViT(depth, dim, heads)
    trunk.load_state_dict(ref.state_dict())
    trunk = trunk.to(DEV).train()
    xv = x.to(DEV).requires_grad_(True)
    dev = lambda seq: None if seq is None else [t.to(DEV) for t in seq]
    was = adavit.USE_LONG_BWD
    adavit.USE_LONG_BWD = True
    ops.set_math_mode("bf16x3")
    try:
        out = adavit.train_forward(trunk, xv, *[dev(m) for m in masks])
        (out * g.to(DEV)).sum().backward()
    finally:
        ops.set_math_mode("fp32")
        adavit.USE_LONG_BWD = was
    grads = {"x": xv.grad}
    grads.update({n: p.grad for n, p in trunk.named_parameters()})
    return out.detach(), grads


def measure(name):
    ref, x, g, masks, want_out, want = build(name)
    _, got = hip_step(name)
    _, ref32 = short._oracle_step(ref, x, g, masks, torch.float32, DEV)
    return {k: grad_err(got[k], w) for k, w in want.items()}, {k: grad_err(ref32[k], w) for k, w in want.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_train_beyond_256_kept_tokens_vs_float64_oracle(name, monkeypatch):
    from laudnet_amd import adavit
    monkeypatch.setattr(adavit, "USE_LONG_BWD", True)
    ref, x, g, masks, want_out, want = build(name)
    depth = CASES[name][4]
    kept = [k.sum(1).int().tolist() for k in masks[0]]
    assert kept == KEPT[name] and all(max(k) > 256 for k in kept), kept       # every block has an image beyond the one-launch kernel
    out, got = hip_step(name)
    assert (out.cpu().double() - want_out).abs().max().item() < 1e-4 * max(1.0, want_out.abs().max().item())
    assert len(want) == 1 + 12 * depth                                        # d x and all twelve parameter gradients of every block
    errs = {}
    for k, w in want.items():
        assert got[k] is not None and w is not None, k
        errs[k] = grad_err(got[k], w)
    print(f"{name}: worst {max(errs.values()):.3e}  {errs}")
    bad = {k: e for k, e in errs.items() if not e < BOUND}
    assert not bad, bad
    dropped = torch.stack([k < 0.5 for k in masks[0]]).all(0)                 # dropped by every block: the gradient passes through untouched
    assert dropped.any() and torch.equal(got["x"].cpu()[dropped], g[dropped])


def test_switch_is_off_by_default_and_read_from_the_environment():
    code = ("import os, importlib; os.environ.pop('LDN_MHA_BWD_LONG', None); from laudnet_amd import adavit; print(adavit.USE_LONG_BWD is False, "
            "adavit.BWD_MAX_TOKENS); os.environ['LDN_MHA_BWD_LONG'] = '1'; print(importlib.reload(adavit).USE_LONG_BWD is True)")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.split() == ["True", "256", "True"], res.stdout


def test_switch_does_not_change_the_floats_up_to_256_tokens(monkeypatch):
    from laudnet_amd import adavit
    monkeypatch.setattr(adavit, "USE_LONG_BWD", False)
    _, _, off = short.hip_step("block")
    monkeypatch.setattr(adavit, "USE_LONG_BWD", True)
    _, _, on = short.hip_step("block")                                        # L 40: the dispatch is by L, the one-launch kernel runs
    assert set(on) == set(off) and len(on) == 13
    for k in off:
        assert torch.equal(on[k], off[k]), k


def test_long_shapes_stay_refused_with_the_switch_off(monkeypatch):
    from laudnet_amd import LdnError, adavit, ops
    monkeypatch.setattr(adavit, "USE_LONG_BWD", False)
    blk = adavit.TokenSkipBlock(64, 1).to(DEV).train()
    ops.set_math_mode("bf16x3")
    try:
        with pytest.raises(LdnError, match="not built.*USE_LONG_BWD"):
            adavit.block_train(blk, torch.zeros(2, 300, 64, device=DEV), torch.ones(2, 300, device=DEV))
    finally:
        ops.set_math_mode("fp32")
