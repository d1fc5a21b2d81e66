"""float64 references of the grouped 3x3 on packed rows, shared by tests/test_wgrad_grouped_ref.py (which pins them against torch.autograd.grad
of F.conv2d(groups=C / gw) on the CPU) and the GPU parity test tests/test_hip_wgrad_grouped.py.

    weight gradient (include/ldn_hip.h: ldn_wgrad_grouped_rows)
        dW[c, t, j] = sum_{r < count} dY[r, c] * A[nbr[r, t], (c // gw) * gw + j]           (an index < 0 or >= a_valid: a zero row)
    the convolution itself on packed rows (ldn_grouped_conv3x3_rows without its epilogue)
        out[r, c]   = sum_t sum_{i < gw} A[nbr[r, t], (c // gw) * gw + i] * w[c, t, i]
    whose adjoint is the same sum over the transposed neighbour table with per-group transposed weights (training.grouped_weight_T).
"""
from __future__ import annotations

import torch

from wgrad_ref import gather_taps_f64


def wgrad_grouped_ref_f64(dy, a, nbr, gw, count=None, a_valid=None):
    """-> (dW [C, 9, gw] float64, bound [C, 9, gw] float64 = sum_r |dY| |A|: the componentwise error scale).  Only the first `count` rows of
    dy / nbr are looked at (whatever lies behind them -- NaN, garbage indices -- is sliced away before any arithmetic)."""
    count = dy.shape[0] if count is None else int(count)
    C = dy.shape[1]
    G = C // gw
    d = dy.detach().double().cpu()[:count].reshape(count, G, gw)
    g = gather_taps_f64(a, nbr, 9, count, a_valid).reshape(count, 9, G, gw)
    dw = torch.einsum("rgi,rtgj->gitj", d, g).reshape(C, 9, gw)
    bound = torch.einsum("rgi,rtgj->gitj", d.abs(), g.abs()).reshape(C, 9, gw)
    return dw, bound


def grouped_conv_rows_f64(a, nbr, w, gw, count, a_valid=None):
    """out [count, C] float64 = the grouped 3x3 over a neighbour table; w [C, 9, gw] (out channel, tap, in channel of the group)"""
    C = w.shape[0]
    G = C // gw
    g = gather_taps_f64(a, nbr, 9, count, a_valid).reshape(count, 9, G, gw)
    return torch.einsum("rtgi,goti->rgo", g, w.detach().double().cpu().reshape(G, gw, 9, gw)).reshape(count, C)
