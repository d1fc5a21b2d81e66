"""ops.rows_ln_bwd (ldn_rows_ln_bwd) against float64 autograd of F.layer_norm on the listed rows.  Bound: every element of dx / d_gamma / d_beta
within 1e-3 of the tensor's own maximum (tests/attn_bwd_ref.py: BOUND).  `measure` returns the figures without asserting
(tools/train_adavit_grad_err.py records them, beside fp32 autograd on the GPU)."""
import pytest
import torch
import torch.nn.functional as F

from attn_bwd_ref import BOUND, grad_err
from fill import seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = [64, 192, 384, 1280]
ROWS, EPS = 150, 1e-5          # 150 rows: more than one split of the row plan (32 rows each), a ragged last one
_CASES = {}


def case(C):
    """x [ROWS, C] with mean / std = 30 on every third row, gamma, a keep mask over the rows, dy dense (zero off the list), and the float64
    autograd reference (dx dense, d_gamma, d_beta): computed once per width and left unchanged"""
    if C not in _CASES:
        x = seeded_randn((ROWS, C), 11 + C)
        x[::3] += 30.0
        gamma = 1.0 + 0.1 * seeded_randn((C,), 12 + C)
        keep = seeded_bernoulli((ROWS,), 0.6, 13 + C)
        keep[0], keep[ROWS - 1] = 1.0, 0.0
        dy = seeded_randn((ROWS, C), 14 + C) * keep[:, None]
        _CASES[C] = (x, gamma, keep, dy, reference(x, gamma, dy, torch.float64, "cpu"))
    return _CASES[C]


def reference(x, gamma, dy, dtype, dev):
    xv = x.to(dev, dtype).requires_grad_(True)
    g = gamma.to(dev, dtype).requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    (F.layer_norm(xv, (x.shape[1],), g, b, EPS) * dy.to(dev, dtype)).sum().backward()
    return xv.grad, g.grad, b.grad


def run(C, base=None):
    """-> (dx buffer after the call, d_gamma, d_beta, xhat, the listed rows, the buffer before the call)"""
    from laudnet_amd import ops
    x, gamma, keep, dy, _ = case(C)
    xd = x.to(DEV)
    rows, _, count = ops.token_lists(keep.view(1, ROWS).to(DEV))       # a list shorter than its capacity, its count on the device
    n = int(count.item())
    assert 0 < n < rows.numel()
    st = ops.row_stats(xd, EPS, rows=rows, count=count)
    packed = torch.full((ROWS, C), float("nan"), device=DEV)           # rows past the count are not read
    packed[:n] = dy.to(DEV)[rows[:n].long()]
    before = (seeded_randn((ROWS, C), 15 + C) if base is None else base).to(DEV)
    dx = before.clone()
    dg, db, xh = ops.rows_ln_bwd(xd, st, gamma.to(DEV), packed, dx, rows=rows, count=count, want_xhat=True)
    return dx, dg, db, xh, rows[:n].long(), before


def measure(C):
    x, gamma, keep, dy, (wx, wg, wb) = case(C)
    dx, dg, db, _, _, before = run(C)
    r32 = reference(x, gamma, dy, torch.float32, DEV)
    return ({"dx": grad_err(dx - before, wx), "d_gamma": grad_err(dg, wg), "d_beta": grad_err(db, wb)},
            {"dx": grad_err(r32[0], wx), "d_gamma": grad_err(r32[1], wg), "d_beta": grad_err(r32[2], wb)})


@pytest.mark.parametrize("C", WIDTHS)
def test_rows_ln_bwd_vs_float64(C):
    x, gamma, keep, dy, (wx, wg, wb) = case(C)
    dx, dg, db, xh, rows, before = run(C, base=torch.zeros(ROWS, C))
    errs = {"dx": grad_err(dx, wx), "d_gamma": grad_err(dg, wg), "d_beta": grad_err(db, wb)}
    print(f"rows_ln_bwd C {C}: {errs}")
    assert all(e < BOUND for e in errs.values()), errs
    hot = torch.arange(0, ROWS, 3)[keep[::3] > 0.5]                  # the listed rows with mean / std = 30: the cancellation case
    assert hot.numel() > 5 and grad_err(dx[hot], wx[hot]) < BOUND
    xd = x.double()
    want_xh = (xd - xd.mean(1, keepdim=True)) * (xd.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()
    assert grad_err(xh[:rows.numel()], want_xh[rows.cpu()]) < BOUND


@pytest.mark.parametrize("C", [64, 384])
def test_rows_ln_bwd_adds_into_the_buffer_and_is_deterministic(C):
    x, gamma, keep, dy, (wx, _, _) = case(C)
    dx, dg, db, xh, rows, before = run(C)
    unlisted = (keep < 0.5).to(DEV)
    assert torch.equal(dx[unlisted], before[unlisted])                # unlisted rows stay bit-identical
    top = wx.abs().max().item()
    assert ((dx - before)[rows].double().cpu() - wx[rows.cpu()]).abs().max().item() < BOUND * top + 2.0 ** -22 * before.abs().max().item()   # dx is ADDED (one fp32 rounding of the sum)
    dx2, dg2, db2, xh2, _, _ = run(C)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2) and torch.equal(xh[:rows.numel()], xh2[:rows.numel()])


def test_rows_ln_bwd_empty_list_and_errors():
    from laudnet_amd import LdnError, ops
    C = 192
    x, gamma, _, _, _ = case(C)
    xd, g = x.to(DEV), gamma.to(DEV)
    rows, _, count = ops.token_lists(torch.zeros(1, ROWS, device=DEV))
    assert int(count.item()) == 0
    st = ops.row_stats(xd, EPS)
    dy = torch.full((ROWS, C), float("nan"), device=DEV)
    dx = torch.full((ROWS, C), 3.5, device=DEV)
    dg, db, _ = ops.rows_ln_bwd(xd, st, g, dy, dx, rows=rows, count=count)
    assert torch.equal(dg, torch.zeros_like(dg)) and torch.equal(db, torch.zeros_like(db))         # zero sums
    assert torch.equal(dx, torch.full_like(dx, 3.5))                                                 # and no write
    dy = torch.zeros(ROWS, C, device=DEV)
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd.double(), st, g, dy, dx)
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd[:, :190], st, g[:190], dy[:, :190], dx[:, :190])        # C % 4
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd, st[:10], g, dy, dx)
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd, st, g[:64], dy, dx)
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd, st, g, dy[:, :64], dx)
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd, st, g, dy, dx[:10])
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd, st, g, dy, dx, rows=rows.long(), count=count)
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd, st, g, dy, dx, count=count)
    with pytest.raises(LdnError):
        ops.rows_ln_bwd(xd, st, g, dy, dx, m_cap=ROWS + 1)
