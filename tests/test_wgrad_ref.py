"""CPU: the float64 reference the GPU weight-gradient tests lean on (tests/wgrad_ref.py) against torch.autograd.grad of F.conv2d -- 3x3 pad 1,
stride 1 and 2, on a dense tiny case whose neighbour table comes from oracle/index_ref.py; and its handling of the rows past the count."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fill import seeded_bernoulli, seeded_randn
from wgrad_ref import wgrad_error, wgrad_ref_f64


def _dense_case(stride, mask=None):
    from oracle import index_ref as IR
    B, cin, cout = 2, 3, 4
    Ho, Wo = (6, 5) if stride == 1 else (4, 3)
    Hi, Wi = Ho * stride, Wo * stride
    m3 = np.ones((B, Ho, Wo), dtype=bool) if mask is None else mask
    m1 = IR.dilate_mask(m3, stride, 1)
    idx3, _ = IR.nonzero_rows(m3)
    idx1, _ = IR.nonzero_rows(m1)
    nbr = torch.from_numpy(IR.neighbour_table(m3, m1, stride).astype(np.int32)).reshape(-1, 9)
    x = seeded_randn((B, cin, Hi, Wi), 3).double().requires_grad_(False)
    w = seeded_randn((cout, cin, 3, 3), 4).double().requires_grad_(True)
    g = seeded_randn((B, cout, Ho, Wo), 5).double()
    g = g * torch.from_numpy(m3).unsqueeze(1)                      # upstream gradient at the kept output pixels only
    want = torch.autograd.grad(F.conv2d(x, w, stride=stride, padding=1), w, g)[0]           # [cout, cin, 3, 3]
    x2d = x.permute(0, 2, 3, 1).reshape(B * Hi * Wi, cin)
    a = x2d[torch.from_numpy(idx1).long()]                         # the packed rows of the dilated list
    dy = g.permute(0, 2, 3, 1).reshape(B * Ho * Wo, cout)[torch.from_numpy(idx3).long()]
    return dy, a, nbr, want


@pytest.mark.parametrize("stride", [1, 2])
def test_reference_matches_conv2d_autograd(stride):
    dy, a, nbr, want = _dense_case(stride)
    got, bound = wgrad_ref_f64(dy, a, nbr, taps=9)
    got = got.permute(0, 2, 1).reshape(want.shape)                 # [n, t, k] -> [n, k, 3, 3]
    assert (nbr < 0).any() and (got - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item())
    assert bool((bound.permute(0, 2, 1).reshape(want.shape) >= want.abs() - 1e-12).all())


@pytest.mark.parametrize("stride", [1, 2])
def test_reference_on_a_masked_map(stride):
    """kept pixels only: the packed lists of a seeded patch mask, the upstream gradient zero at the dropped pixels"""
    from oracle import index_ref as IR
    Ho, Wo = (6, 5) if stride == 1 else (4, 3)
    m3 = IR.upsample_patch_mask(seeded_bernoulli((2, 2, 1), 0.6, 11).numpy(), Ho, Wo).astype(bool)
    assert m3.any() and not m3.all()
    dy, a, nbr, want = _dense_case(stride, m3)
    got, _ = wgrad_ref_f64(dy, a, nbr, taps=9)
    assert (got.permute(0, 2, 1).reshape(want.shape) - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item())


def test_reference_ignores_rows_past_the_count_and_zero_rows():
    dy, a, nbr, _ = _dense_case(1)
    n = dy.shape[0] - 7
    want, bound = wgrad_ref_f64(dy[:n], a, nbr[:n], taps=9)
    dy2, nbr2 = dy.clone(), nbr.clone()
    dy2[n:] = float("nan")
    nbr2[n:] = 1 << 30
    got, _ = wgrad_ref_f64(dy2, a, nbr2, taps=9, count=n)
    assert torch.equal(got, want) and wgrad_error(got, want, bound) == 0.0
    # an index >= a_valid is a zero row, like -1
    cut = a.shape[0] - 5
    hi = torch.where(nbr >= cut, torch.full_like(nbr, -1), nbr)
    assert torch.equal(wgrad_ref_f64(dy, a, nbr, taps=9, a_valid=cut)[0], wgrad_ref_f64(dy, a, hi, taps=9)[0])
    # taps == 1 without a list: plain dY^T A
    g1, _ = wgrad_ref_f64(dy, a[:dy.shape[0]], None, taps=1)
    assert torch.allclose(g1[:, 0], dy.t() @ a[:dy.shape[0]], atol=1e-12)
    z, zb = wgrad_ref_f64(dy, a, nbr, taps=9, count=0)
    assert z.abs().max().item() == 0 and wgrad_error(z, z, zb) == 0.0
