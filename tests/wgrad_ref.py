"""float64 reference of the packed-row weight gradient (include/ldn_hip.h: ldn_wgrad_rows), shared by tests/test_wgrad_ref.py (which pins
it against torch.autograd.grad of F.conv2d on the CPU) and the GPU parity tests (tests/test_hip_wgrad.py, tests/test_hip_training_wgrad.py).

    dW[n, t, k] = sum_{r < count} dY[r, n] * A[src(r, t), k],   src(r, t) = a_rows[r, t] (an index < 0 or >= a_valid: a zero row) or r
"""
from __future__ import annotations

import torch


def gather_taps_f64(a, a_rows, taps, count, a_valid=None):
    """[count, taps, cin] float64: the explicit gather A[src(r, t), :] for the first `count` rows (zero rows for missing neighbours)."""
    a = a.detach().double().cpu()
    a_valid = a.shape[0] if a_valid is None else a_valid
    if a_rows is None:
        return a[:count].unsqueeze(1).expand(count, taps, a.shape[1])
    idx = a_rows.detach().cpu().long().reshape(-1, taps)[:count]
    ok = (idx >= 0) & (idx < a_valid)
    g = a[idx.clamp(0, max(a.shape[0] - 1, 0)).reshape(-1)].view(count, taps, a.shape[1])
    return torch.where(ok.unsqueeze(2), g, torch.zeros((), dtype=torch.float64))      # (a select, not a product: a zero row's source may hold NaN)


def wgrad_ref_f64(dy, a, a_rows=None, taps=1, count=None, a_valid=None):
    """-> (dW [cout, taps, cin] float64, bound [cout, taps, cin] float64 = sum_r |dY| |A|: the componentwise error scale).  Only the first
    `count` rows of dy / a_rows are looked at (whatever lies behind them -- NaN, garbage indices -- is sliced away before any arithmetic)."""
    count = dy.shape[0] if count is None else int(count)
    d = dy.detach().double().cpu()[:count]
    g = gather_taps_f64(a, a_rows, taps, count, a_valid)
    return torch.einsum("rn,rtk->ntk", d, g), torch.einsum("rn,rtk->ntk", d.abs(), g.abs())


def wgrad_error(got, ref, bound):
    """e = max |got - ref| / max(bound)   (0 when the bound matrix is zero and the result exact)"""
    err = (got.detach().double().cpu() - ref).abs().max().item()
    scale = bound.max().item()
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
