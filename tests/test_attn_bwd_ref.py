"""CPU: the closed forms of tests/attn_bwd_ref.py (what ldn_packed_mha_bwd and ldn_rows_ln_bwd implement) against float64 autograd, on the
shapes of the GPU tests -- the one-token image and a dropped head included."""
import pytest
import torch
import torch.nn.functional as F

from attn_bwd_ref import grad_err, keep_pattern, ln_bwd_closed_form, mha_bwd_autograd, mha_bwd_closed_form, mha_dense
from fill import seeded_randn


@pytest.mark.parametrize("B,L,heads,p", [(3, 40, 2, 0.5), (2, 33, 1, 1.0), (2, 256, 1, 0.7), (4, 197, 6, 0.5)])
def test_mha_closed_form_matches_autograd(B, L, heads, p):
    dim = 64 * heads
    qkv = seeded_randn((B, L, 3 * dim), 3 + L).double()
    keep = keep_pattern(B, L, p, 5 + L)
    d_out = seeded_randn((B, L, dim), 7 + L).double() * keep[:, :, None].double()
    want = mha_bwd_autograd(qkv, keep, heads, d_out)
    got = mha_bwd_closed_form(qkv, keep, heads, d_out)
    assert grad_err(got, want) < 1e-12
    assert torch.equal(want[keep < 0.5], torch.zeros_like(want[keep < 0.5]))        # dropped tokens: neither queries nor keys
    if B > 1:       # the one-token image: P = 1, so dQ = dK = 0 and dV = dO
        g = got[1, 0].reshape(3, dim)
        assert torch.equal(g[0], torch.zeros_like(g[0])) and torch.equal(g[1], torch.zeros_like(g[1])) and torch.equal(g[2], d_out[1, 0])


def test_mha_closed_form_dropped_head():
    B, L, heads = 3, 40, 2
    qkv = seeded_randn((B, L, 3 * 128), 43).double()
    keep = keep_pattern(B, L, 0.5, 45)
    d_out = seeded_randn((B, L, 128), 47).double() * keep[:, :, None].double()
    hk = torch.tensor([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0]])
    want = mha_bwd_autograd(qkv, keep, heads, d_out, hk)
    got = mha_bwd_closed_form(qkv, keep, heads, d_out, hk)
    assert grad_err(got, want) < 1e-12
    g = got[0].reshape(L, 3, heads, 64)
    assert torch.equal(g[:, :, 0], torch.zeros_like(g[:, :, 0])) and g[:, :, 1].abs().max() > 0
    out = mha_dense(qkv, keep, heads, hk)
    assert torch.equal(out[0, :, :64], torch.zeros_like(out[0, :, :64]))


@pytest.mark.parametrize("C", [64, 192, 384, 1280])
def test_ln_closed_form_matches_autograd(C):
    rows = 37
    x = seeded_randn((rows, C), 11 + C).double()
    x[::3] += 30.0                                               # mean / std = 30 on every third row
    gamma = (1.0 + 0.1 * seeded_randn((C,), 12 + C)).double().requires_grad_(True)
    beta = (0.1 * seeded_randn((C,), 13 + C)).double().requires_grad_(True)
    dy = seeded_randn((rows, C), 14 + C).double()
    xv = x.clone().requires_grad_(True)
    (F.layer_norm(xv, (C,), gamma, beta, 1e-5) * dy).sum().backward()
    dx, dg, db = ln_bwd_closed_form(x, gamma.detach(), dy, 1e-5)
    assert grad_err(dx, xv.grad) < 1e-10 and grad_err(dg, gamma.grad) < 1e-12 and grad_err(db, beta.grad) < 1e-12
