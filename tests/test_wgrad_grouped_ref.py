"""CPU: the float64 references of tests/wgrad_grouped_ref.py against torch.autograd.grad of F.conv2d(groups=C / gw) on the kept pixels of a
pixel mask, over the neighbour table of oracle/index_ref.py -- stride 1 and 2, group widths 8 / 16 / 24:
  * the weight gradient formula of ldn_wgrad_grouped_rows;
  * the adjoint identity training.py relies on: the grouped conv over the TRANSPOSED neighbour table with per-group transposed weights
    (training.transposed_neighbour_table, training.grouped_weight_T) equals the autograd input gradient on the rows of the dilated list."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fill import seeded_bernoulli, seeded_randn
from wgrad_grouped_ref import grouped_conv_rows_f64, wgrad_grouped_ref_f64


def _case(gw, stride, seed):
    from oracle import index_ref as IR
    B, Ho, Wo, C = 2, 5, 4, 2 * gw
    Hi, Wi = Ho * stride, Wo * stride
    m3 = seeded_bernoulli((B, Ho, Wo), 0.5, seed).numpy().astype(bool)
    m3[0, 0, 0] = m3[0, 0, 1] = m3[0, -1, -1] = True                 # a corner, an edge and its neighbour
    m1 = IR.dilate_mask(m3, stride, 1)
    idx3, _ = IR.nonzero_rows(m3)
    idx1, _ = IR.nonzero_rows(m1)
    nbr = torch.from_numpy(IR.neighbour_table(m3, m1, stride))
    x = seeded_randn((B, C, Hi, Wi), seed + 1).double().requires_grad_(True)
    w = seeded_randn((C, gw, 3, 3), seed + 2).double().requires_grad_(True)
    y = F.conv2d(x, w, stride=stride, padding=1, groups=C // gw)
    gy = seeded_randn(tuple(y.shape), seed + 3).double() * torch.from_numpy(m3).unsqueeze(1)      # upstream gradient on the kept pixels only
    gx, gw_auto = torch.autograd.grad(y, (x, w), gy)
    rows = lambda t, idx: t.detach().permute(0, 2, 3, 1).reshape(-1, C)[torch.from_numpy(idx).long()]
    ix = SimpleNamespace(idx1=torch.from_numpy(idx1.astype(np.int32)), pos3=torch.from_numpy(IR.position_map(m3).reshape(-1).astype(np.int32)),
                         cap1=len(idx1), cnt=torch.tensor([len(idx3), len(idx1)], dtype=torch.int32))
    wk = w.detach().permute(0, 2, 3, 1).reshape(C, 9, gw)
    return SimpleNamespace(B=B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, C=C, nbr=nbr, ix=ix, wk=wk, a=rows(x, idx1), dy=rows(gy, idx3), gx=gx, gx_rows=rows(gx, idx1),
                           gw_auto=gw_auto.permute(0, 2, 3, 1).reshape(C, 9, gw), m1=torch.from_numpy(m1))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("gw", [8, 16, 24])
def test_wgrad_grouped_ref_is_the_autograd_weight_gradient(gw, stride):
    c = _case(gw, stride, 100 + gw + stride)
    got, bound = wgrad_grouped_ref_f64(c.dy, c.a, c.nbr, gw)
    assert tuple(got.shape) == (c.C, 9, gw)
    assert (got - c.gw_auto).abs().max().item() < 1e-12 * max(1.0, c.gw_auto.abs().max().item())
    assert bool((bound >= got.abs() - 1e-12).all())
    # rows past the count and table entries >= a_valid are not looked at
    dy_nan = torch.cat((c.dy, torch.full((3, c.C), float("nan"), dtype=torch.float64)))
    nbr_junk = torch.cat((c.nbr, torch.full((3, 9), 1 << 28, dtype=c.nbr.dtype)))
    again, _ = wgrad_grouped_ref_f64(dy_nan, c.a, nbr_junk, gw, count=c.dy.shape[0])
    assert torch.equal(again, got)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("gw", [8, 16, 24])
def test_transposed_table_with_transposed_group_weights_is_the_autograd_input_gradient(gw, stride):
    from laudnet_amd.training import grouped_weight_T, transposed_neighbour_table
    c = _case(gw, stride, 200 + gw + stride)
    n1 = c.a.shape[0]
    # the forward statement first: the packed-row conv equals F.conv2d on the kept pixels (it is what the adjoint is the adjoint of)
    nbrT = transposed_neighbour_table(c.ix, c.B, c.Hi, c.Wi, stride, c.Ho, c.Wo)
    wT = grouped_weight_T(c.wk.contiguous(), gw)
    got = grouped_conv_rows_f64(c.dy, nbrT, wT, gw, n1)
    assert (got - c.gx_rows).abs().max().item() < 1e-12 * max(1.0, c.gx_rows.abs().max().item())
    outside = c.gx.detach() * (~c.m1).unsqueeze(1)
    assert outside.abs().max().item() == 0, "the input gradient lives on the dilated list's pixels only"
    assert c.gx_rows.abs().max().item() > 0
