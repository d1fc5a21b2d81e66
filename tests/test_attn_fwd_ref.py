"""CPU: the float64 restatement of ldn_packed_mha in tests/attn_fwd_ref.py against torch's scaled_dot_product_attention (boolean mask,
explicit scale), against attn_bwd_ref.mha_dense (default scale, a dropped head) and against the max_tokens rule on an example small enough
to write down."""
import math

import pytest
import torch
import torch.nn.functional as F

from attn_bwd_ref import keep_pattern, mha_dense
from attn_fwd_ref import attending, mha_packed_f64
from fill import seeded_randn


def _packed_rows(keep):
    """flat dense rows of the kept tokens, image-major and ascending: tok_rows of ops.token_lists"""
    return torch.nonzero(keep.reshape(-1) > 0.5).reshape(-1)


@pytest.mark.parametrize("B,L,heads,p,scale", [(3, 40, 2, 0.5, 0.2), (2, 33, 1, 1.0, 1.0), (4, 70, 3, 0.3, 0.03)])
def test_reference_matches_torch_sdpa_float64(B, L, heads, p, scale):
    dim = 64 * heads
    qkv = seeded_randn((B, L, 3 * dim), 3 + L).double()
    keep = keep_pattern(B, L, p, 5 + L)                     # every image keeps its CLS token: no query row without a key
    q, k, v = qkv.reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    mask = (keep > 0.5)[:, None, None, :].expand(B, heads, L, L)
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale).transpose(1, 2).reshape(B * L, dim)
    got, written = mha_packed_f64(qkv, keep, heads, scale=scale)
    rows = _packed_rows(keep)
    assert got.dtype == torch.float64 and got.shape == (rows.numel(), dim)
    assert torch.equal(written, torch.arange(rows.numel()))                  # no max_tokens: every kept token's row is written
    assert (got - want[rows]).abs().max().item() < 1e-13


def test_reference_matches_mha_dense_at_the_default_scale():
    B, L, heads = 4, 50, 3
    qkv = seeded_randn((B, L, 3 * 64 * heads), 43).double()
    keep = keep_pattern(B, L, 0.5, 45)
    hk = torch.tensor([[0.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    rows = _packed_rows(keep)
    for head_keep in (None, hk):
        want = mha_dense(qkv, keep, heads, head_keep).reshape(B * L, -1)[rows]
        got, written = mha_packed_f64(qkv, keep, heads, head_keep=head_keep)
        assert torch.equal(written, torch.arange(rows.numel()))
        assert (got - want).abs().max().item() < 1e-13
    img = rows // L
    assert torch.equal(got[img == 0][:, :64], torch.zeros(int((img == 0).sum()), 64, dtype=torch.float64))   # a dropped head: exact zeros
    # max_tokens at or above every count changes nothing
    again, w2 = mha_packed_f64(qkv, keep, heads, max_tokens=L, head_keep=hk)
    assert torch.equal(again, got) and torch.equal(w2, written)


def test_reference_with_an_image_that_keeps_nothing():
    B, L, heads = 3, 12, 1
    qkv = seeded_randn((B, L, 192), 61).double()
    keep = torch.zeros(B, L)
    keep[0, [0, 3, 7]] = 1.0
    keep[2, [1, 2]] = 1.0
    got, written = mha_packed_f64(qkv, keep, heads)
    assert got.shape == (5, 64) and written.tolist() == [0, 1, 2, 3, 4] and torch.isfinite(got).all()


def test_truncation_rule_on_a_hand_written_example():
    """L = 5, heads = 1, max_tokens = 2.  Image 0 keeps tokens 0, 2, 3, 4 -> attends with 0 and 2 only; image 1 keeps tokens 1 and 4
    (at the bound).  Packed rows: image 0 owns 0..3 (its last two are NOT written), image 1 owns 4..5."""
    L, hd = 5, 64
    keep = torch.tensor([[1.0, 0.0, 1.0, 1.0, 1.0], [0.0, 1.0, 0.0, 0.0, 1.0]])
    assert attending(keep, 2).tolist() == [[True, False, True, False, False], [False, True, False, False, True]]
    assert attending(keep, 1).tolist() == [[True, False, False, False, False], [False, True, False, False, False]]
    assert torch.equal(attending(keep, 4), keep > 0.5) and torch.equal(attending(keep), keep > 0.5)
    qkv = seeded_randn((2, L, 3 * hd), 77).double()
    scale = 0.25
    got, written = mha_packed_f64(qkv, keep, 1, scale=scale, max_tokens=2)
    assert got.shape == (6, hd) and written.tolist() == [0, 1, 4, 5]
    assert torch.equal(got[2:4], torch.zeros(2, hd, dtype=torch.float64))
    # two attending tokens i, j: the softmax over two logits is a logistic function of their difference, written out with math.exp
    for b, (i, j), (ni, nj) in ((0, (0, 2), (0, 1)), (1, (1, 4), (4, 5))):
        q, k, v = qkv[b].reshape(L, 3, hd).unbind(1)
        for tok, n in ((i, ni), (j, nj)):
            si, sj = scale * float(q[tok] @ k[i]), scale * float(q[tok] @ k[j])
            wi = 1.0 / (1.0 + math.exp(sj - si))
            want = wi * v[i] + (1.0 - wi) * v[j]
            assert (got[n] - want).abs().max().item() < 1e-14, (b, tok)
    # the same thing said another way: the cut mask, without max_tokens, scattered to the uncut numbering
    cut, w_cut = mha_packed_f64(qkv, attending(keep, 2).float(), 1, scale=scale)
    assert w_cut.tolist() == [0, 1, 2, 3] and torch.equal(cut, got[written])
    # max_tokens = 1: every attending token sees itself alone -> its own v
    one, w1 = mha_packed_f64(qkv, keep, 1, max_tokens=1)
    assert w1.tolist() == [0, 4]
    assert (one[0] - qkv[0, 0, 2 * hd:]).abs().max().item() < 1e-15 and (one[4] - qkv[1, 1, 2 * hd:]).abs().max().item() < 1e-15


def test_reference_is_differentiable_and_cut_tokens_get_no_gradient():
    B, L, heads = 2, 9, 1
    qkv = seeded_randn((B, L, 192), 81).double().requires_grad_(True)
    keep = torch.ones(B, L)
    keep[1, 4:] = 0.0
    out, written = mha_packed_f64(qkv, keep, heads, max_tokens=5)
    assert written.tolist() == [0, 1, 2, 3, 4, 9, 10, 11, 12]
    out.sum().backward()
    assert torch.equal(qkv.grad[0, 5:], torch.zeros_like(qkv.grad[0, 5:])) and qkv.grad[0, :5].abs().max() > 0
    assert torch.equal(qkv.grad[1, 4:], torch.zeros_like(qkv.grad[1, 4:]))
