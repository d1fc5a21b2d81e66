"""CPU: the float64 restatement of the two-launch attention backward (tests/attn_bwd_tiled_ref.py: tiles of 256, chunks of 32, statistics handed
over through an array, dK / dV accumulated over query tiles) against float64 autograd, at the seam counts of tests/test_hip_attn_bwd_long.py."""
import pytest
import torch

from attn_bwd_ref import grad_err, mha_bwd_autograd
from attn_bwd_tiled_ref import mha_bwd_tiled
from fill import seeded_randn

SEAMS = [(320, [257, 1, 256, 288], 1), (600, [512, 513, 33, 600], 1), (577, [300, 40, 577], 2)]


def keep_counts(L, counts, seed):
    """[len(counts), L] keep masks with exactly counts[b] kept tokens in image b, the CLS token among them (counts[b] = 0: none)."""
    keep = torch.zeros(len(counts), L)
    for b, n in enumerate(counts):
        if n > 0:
            perm = torch.randperm(L - 1, generator=torch.Generator().manual_seed(seed + b))[: n - 1] + 1
            keep[b, 0] = 1.0
            keep[b, perm] = 1.0
    assert keep.sum(1).tolist() == [float(n) for n in counts]
    return keep


@pytest.mark.parametrize("L,counts,heads", SEAMS)
def test_tiled_scheme_matches_autograd(L, counts, heads):
    B, dim = len(counts), 64 * heads
    qkv = seeded_randn((B, L, 3 * dim), 3 + L).double()
    keep = keep_counts(L, counts, 5 + L)
    d_out = seeded_randn((B, L, dim), 7 + L).double() * keep[:, :, None].double()
    want = mha_bwd_autograd(qkv, keep, heads, d_out)
    got = mha_bwd_tiled(qkv, keep, heads, d_out)
    assert torch.isfinite(got).all()                                 # the workspace starts as NaN: every entry read was written
    assert grad_err(got, want) < 1e-12
    assert torch.equal(got[keep < 0.5], torch.zeros_like(got[keep < 0.5]))


def test_tiled_scheme_dropped_head_and_empty_image():
    L, heads = 300, 3
    keep = keep_counts(L, [300, 280, 0], 11)
    qkv = seeded_randn((3, L, 3 * 64 * heads), 13).double()
    d_out = seeded_randn((3, L, 64 * heads), 17).double() * keep[:, :, None].double()
    hk = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0]])
    got = mha_bwd_tiled(qkv, keep, heads, d_out, hk)
    want = mha_bwd_autograd(qkv[:2], keep[:2], heads, d_out[:2], hk[:2])     # an image without a kept token makes the dense reference NaN
    assert grad_err(got[:2], want) < 1e-12
    assert torch.equal(got[2], torch.zeros_like(got[2]))
    g = got[0].reshape(L, 3, heads, 64)
    assert torch.equal(g[:, :, 1], torch.zeros_like(g[:, :, 1])) and g[:, :, 0].abs().max() > 0
