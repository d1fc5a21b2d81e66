"""Training of the token-skipping blocks (laudnet_amd.adavit.block_train / train_forward) against float64 autograd of oracle/adavit_ref.py, the dense
masked restatement (its masked_fill keys and gated residual updates are differentiable in x and the parameters).  Bound: every element of every
gradient within 1e-3 of that tensor's own maximum (tests/attn_bwd_ref.py: BOUND; no allowance); forward values within 1e-4 * max(1, max |want|),
the bound of test_token_skip_block_vs_oracle.  `measure` returns the figures without asserting (tools/train_adavit_grad_err.py records them in
profiles/train_adavit_grad_err.json beside fp32 autograd of the oracle on the GPU)."""
import copy

import pytest
import torch

from attn_bwd_ref import BOUND, grad_err, keep_pattern
from fill import seeded_randn
from oracle import adavit_ref as AR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (B, L, dim, heads, depth, head + layer skipping)
CASES = {
    "block": (3, 40, 128, 2, 1, False),
    "block_head_layer_skip": (3, 40, 128, 2, 1, True),
    "trunk3": (3, 33, 64, 1, 3, False),
    "block_deit_s": (2, 197, 384, 6, 1, False),
}
_BUILT = {}


def _fill(model, seed):
    """linear weights N(0, 0.05), biases N(0, 0.1), LayerNorm weight N(1, 0.1) from a local generator"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() > 1:
                p.copy_(0.05 * torch.randn(p.shape, generator=gen))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))


def _oracle_step(ref, x, g, masks, dtype, dev):
    m = copy.deepcopy(ref).to(dev, dtype)
    xv = x.to(dev, dtype).requires_grad_(True)
    cast = lambda seq: None if seq is None else [t.to(dev, dtype) for t in seq]
    keeps, hks, aks, mks = masks
    out = m(xv, cast(keeps), cast(hks), cast(aks), cast(mks))
    (out * g.to(dev, dtype)).sum().backward()
    grads = {"x": xv.grad}
    grads.update({n: p.grad for n, p in m.named_parameters()})
    return out.detach(), grads


def build(name):
    """(oracle trunk, x, upstream gradient, masks, float64 forward value, float64 gradients): computed once per case and left unchanged"""
    if name not in _BUILT:
        B, L, dim, heads, depth, skip = CASES[name]
        ref = AR.TokenSkipViTRef(depth, dim, heads)
        _fill(ref, 100 + L)
        x = seeded_randn((B, L, dim), 21 + L)
        g = seeded_randn((B, L, dim), 22 + L)
        keeps = [keep_pattern(B, L, 0.5, 23 + L + i) for i in range(depth)]
        hks = aks = mks = None
        if skip:      # image 0 drops head 0; image 2's attention is skipped but its MLP trains, image 0 the other way round
            hk = torch.ones(B, heads)
            hk[0, 0] = 0.0
            hks, aks, mks = [hk], [torch.tensor([1.0, 1.0, 0.0])], [torch.tensor([0.0, 1.0, 1.0])]
        masks = (keeps, hks, aks, mks)
        want_out, want = _oracle_step(ref, x, g, masks, torch.float64, "cpu")
        _BUILT[name] = (ref, x, g, masks, want_out, want)
    return _BUILT[name]


def hip_step(name, trunk=None):
    """one forward + backward through train_forward -> (trunk, forward value, {name: gradient}) with the oracle's parameter names"""
    from laudnet_amd import ops
    from laudnet_amd.adavit import TokenSkipViT, train_forward
    ref, x, g, masks, _, _ = build(name)
    B, L, dim, heads, depth, _ = CASES[name]
    if trunk is None:
        trunk = TokenSkipViT(depth, dim, heads)
        trunk.load_state_dict(ref.state_dict())
        trunk = trunk.to(DEV).train()
    for p in trunk.parameters():
        p.grad = None
    xv = x.to(DEV).requires_grad_(True)
    dev = lambda seq: None if seq is None else [t.to(DEV) for t in seq]
    ops.set_math_mode("bf16x3")
    try:
        out = train_forward(trunk, xv, *[dev(m) for m in masks])
        (out * g.to(DEV)).sum().backward()
    finally:
        ops.set_math_mode("fp32")
    grads = {"x": xv.grad}
    grads.update({n: p.grad for n, p in trunk.named_parameters()})
    return trunk, out.detach(), grads


def measure(name):
    ref, x, g, masks, want_out, want = build(name)
    _, _, got = hip_step(name)
    _, ref32 = _oracle_step(ref, x, g, masks, torch.float32, DEV)
    return {k: grad_err(got[k], w) for k, w in want.items()}, {k: grad_err(ref32[k], w) for k, w in want.items()}


def _check(name):
    ref, x, g, masks, want_out, want = build(name)
    _, out, got = hip_step(name)
    depth = CASES[name][4]
    assert (out.cpu().double() - want_out).abs().max().item() < 1e-4 * max(1.0, want_out.abs().max().item())
    assert len(want) == 1 + 12 * depth
    compared = 0
    errs = {}
    for k, w in want.items():
        assert got[k] is not None and w is not None, k
        errs[k] = grad_err(got[k], w)
        compared += 1
    print(f"{name}: worst {max(errs.values()):.3e}  {errs}")
    assert compared == 1 + 12 * depth                                    # d x and all twelve parameter gradients of every block
    bad = {k: e for k, e in errs.items() if not e < BOUND}
    assert not bad, bad
    return got


def test_block_train_vs_float64_oracle():
    got = _check("block")
    _, x, g, masks, _, _ = build("block")
    dropped = masks[0][0] < 0.5
    assert dropped.any() and torch.equal(got["x"].cpu()[dropped], g[dropped])        # a dropped token's gradient passes through untouched


def test_block_train_head_and_layer_skipping():
    got = _check("block_head_layer_skip")
    _, x, g, masks, _, want = build("block_head_layer_skip")
    # image 2 (attention skipped) still trains its MLP, image 0 (MLP skipped) its attention: d x differs from the upstream gradient on both
    gx = got["x"].cpu()
    kept0, kept2 = masks[0][0][0] > 0.5, masks[0][0][2] > 0.5
    assert not torch.equal(gx[0][kept0], g[0][kept0]) and not torch.equal(gx[2][kept2], g[2][kept2])
    assert want["blocks.0.fc1.weight"].abs().max() > 0 and want["blocks.0.qkv.weight"].abs().max() > 0


def test_train_forward_depth3_trunk():
    _check("trunk3")


def test_block_train_deit_s_width():
    _check("block_deit_s")


def test_block_train_without_wgrad_kernel(monkeypatch):
    from laudnet_amd import ops, training
    calls = []
    real = ops.wgrad_rows
    monkeypatch.setattr(ops, "wgrad_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    _, _, on = hip_step("block")
    assert len(calls) == 4                                               # qkv, proj, fc1, fc2
    monkeypatch.setattr(training, "USE_WGRAD_KERNEL", False)
    _, _, off = hip_step("block")
    assert len(calls) == 4                                               # the gather + GEMM path
    _, _, _, _, _, want = build("block")
    for k, w in want.items():
        assert grad_err(off[k], w) < BOUND, k
        assert grad_err(off[k], on[k]) < BOUND, k


def test_scope_refusals():
    from laudnet_amd import LdnError, ops
    from laudnet_amd.adavit import TokenSkipBlock, block_train
    blk = TokenSkipBlock(64, 1).to(DEV).train()
    x = torch.zeros(2, 40, 64, device=DEV, requires_grad=True)
    keep = torch.ones(2, 40, device=DEV)
    ops.set_math_mode("bf16x3")
    try:
        with pytest.raises(LdnError, match="not built"):
            block_train(blk, x, keep.clone().requires_grad_(True))
        with pytest.raises(LdnError, match="not built"):
            block_train(blk, x, keep, head_keep=torch.ones(2, 1, device=DEV, requires_grad=True))
        with pytest.raises(LdnError, match="not built"):
            block_train(blk, x, keep, attn_keep=torch.ones(2, device=DEV, requires_grad=True))
        with pytest.raises(LdnError, match="not built"):
            block_train(blk, x, keep, mlp_keep=torch.ones(2, device=DEV, requires_grad=True))
        with pytest.raises(LdnError, match="not built"):                 # L = 300 with everything kept
            block_train(blk, torch.zeros(2, 300, 64, device=DEV), torch.ones(2, 300, device=DEV))
        try:
            TokenSkipBlock.qkv_kept_only = False
            with pytest.raises(LdnError, match="not built"):
                block_train(blk, x, keep)
        finally:
            TokenSkipBlock.qkv_kept_only = True
        with pytest.raises(LdnError):                                    # the module surface stays eval-only
            blk(x, keep)
    finally:
        ops.set_math_mode("fp32")
    with pytest.raises(LdnError, match="bf16x3"):
        block_train(blk, x, keep)


def test_eval_forward_unchanged_by_a_training_step():
    from laudnet_amd import ops
    ref, x, g, masks, want_out, _ = build("block")
    trunk, _, _ = hip_step("block")

    def eval_forward():
        ops.set_math_mode("bf16x3")
        try:
            with torch.no_grad():
                return trunk.eval()(x.to(DEV), [k.to(DEV) for k in masks[0]])
        finally:
            ops.set_math_mode("fp32")
            trunk.train()

    before = eval_forward()
    hip_step("block", trunk)
    after = eval_forward()
    assert torch.equal(before, after)
    assert (before.cpu().double() - want_out).abs().max().item() < 1e-4 * max(1.0, want_out.abs().max().item())
