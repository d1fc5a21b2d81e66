#!/usr/bin/env python3
"""ops.rows_bn_stats + ops.rows_bn_postmask_fwd + ops.rows_bn_postmask_bwd (one BatchNorm layer of a LAD-RegNet channel block on batch
statistics, forward and backward: BatchNorm, ReLU, the channel mask BEHIND it, the squeeze-excitation prologue, d gamma / d beta, the gradient
through the statistics and the mask's straight-through sum -- 6 launches) beside the chain of the kernels that existed before them, which is what
training would otherwise run per layer -- 10 launches:
    forward   rows_bn_stats (2), rows_bn_fwd with ReLU (1), a clone of the unmasked output (1), rows_chanmask on the copy (1)
    backward  rows_postmask_bwd with a scale of ones (SE prologue, mask, ReLU gate, g_mask: 2), rows_bn_bwd without a gate (3)
Shapes: the four stages of RegNetY-800MF at 224 x 224 (bottleneck widths 64 / 144 / 320 / 784 on 56^2 / 28^2 / 14^2 / 7^2 pixels), all pixels
of `--batch` images.

The two legs ALTERNATE round by round in one process; a round is `--iters` back-to-back calls between two device events behind a synchronise; the
figure is the median over `--rounds` (>= 9) rounds, and the spread of a leg is its max - min over the rounds.  `bytes_min` is what the fused
kernels' contract must move (statistics: read u; forward: read u, write h; backward: read dz, u, h twice -- once per pass -- and write du: 10
matrices; the chain moves about 15).  Outputs are compared once per shape (per output, max |fused - chain| relative to the chain's maximum).
One JSON line per shape.
usage: tools/bench_rows_bn_postmask.py [--batch 32] [--rounds 11] [--iters 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from laudnet_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
assert args.rounds >= 9, "the median of at least 9 rounds"
dev = torch.device("cuda", 0)
EPS = 1e-5
STAGES = [(64, 56), (144, 28), (320, 14), (784, 7)]          # (w_b, output size) of RegNetY-800MF's four stages


def chain(u, dz, m, gate, dsq, gamma, beta, pre, one, zero):
    """the kernels of before: -> (h, du, d_gamma, d_beta, g_mask)"""
    mean, _, inv = ops.rows_bn_stats(u, EPS)
    r = ops.rows_bn_fwd(u, mean, inv, gamma, beta)
    h = ops.rows_chanmask(r.clone(), pre, m)
    a, _, _, g_mask = ops.rows_postmask_bwd(dz, r, one, zero, chan_mask=m, row_prefix=pre, gate=gate, dsq=dsq, want_mask=True)
    du, d_gamma, d_beta, _ = ops.rows_bn_bwd(a, u, None, mean, inv, gamma, out=a)
    return h, du, d_gamma, d_beta, g_mask


def fused(u, dz, m, gate, dsq, gamma, beta, pre):
    mean, _, inv = ops.rows_bn_stats(u, EPS)
    h = ops.rows_bn_postmask_fwd(u, mean, inv, gamma, beta, chan_mask=m, row_prefix=pre)
    du, d_gamma, d_beta, g_mask = ops.rows_bn_postmask_bwd(dz, u, h, mean, inv, gamma, beta, chan_mask=m, row_prefix=pre, gate=gate, dsq=dsq,
                                                           want_mask=True)
    return h, du, d_gamma, d_beta, g_mask


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters          # microseconds per call


for W, S in STAGES:
    B, P = args.batch, S * S
    gen = torch.Generator(device=dev).manual_seed(W)
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=gen)
    u, dz = rnd(B * P, W) + 0.5, rnd(B * P, W)
    m = (torch.rand(B, W, device=dev, generator=gen) < 0.6).float()
    gate, dsq = torch.rand(B, W, device=dev, generator=gen), rnd(B, W) / P
    gamma, beta = 0.5 + torch.rand(W, device=dev, generator=gen), 0.1 * rnd(W)
    pre = (torch.arange(B + 1, device=dev, dtype=torch.int32) * P).contiguous()
    one, zero = torch.ones(W, device=dev), torch.zeros(W, device=dev)
    legs = {"fused": lambda: fused(u, dz, m, gate, dsq, gamma, beta, pre), "chain": lambda: chain(u, dz, m, gate, dsq, gamma, beta, pre, one, zero)}
    got, want = legs["fused"](), legs["chain"]()
    errs = {n: ((g - w).abs().max() / w.abs().max().clamp(min=1e-30)).item() for n, g, w in zip(("h", "du", "d_gamma", "d_beta", "g_mask"), got, want)}
    for fn in legs.values():                        # warm-up of both legs
        timed(fn, 3)
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    nbytes = 10 * B * P * W * 4
    print(json.dumps({"what": "one BatchNorm layer of a LAD-RegNet channel block on batch statistics, forward + backward: rows_bn_stats + "
                              "rows_bn_postmask_fwd + rows_bn_postmask_bwd (mask, SE prologue, g_mask) vs the chain of the earlier kernels",
                      "launches": {"fused": 2 + 1 + 3, "chain": 2 + 1 + 1 + 1 + 2 + 3},
                      "batch": B, "width": W, "rows": B * P, "rounds": args.rounds, "iters_per_round": args.iters,
                      "fused_us_median": round(med["fused"], 2), "chain_us_median": round(med["chain"], 2),
                      "fused_us_min_max": [round(min(us["fused"]), 2), round(max(us["fused"]), 2)],
                      "chain_us_min_max": [round(min(us["chain"]), 2), round(max(us["chain"]), 2)],
                      "spread_us": {k: round(v, 2) for k, v in spread.items()},
                      "chain_over_fused": round(med["chain"] / med["fused"], 2),
                      "fused_faster_beyond_spread": bool(med["chain"] - med["fused"] > max(spread.values())),
                      "fused_slower_beyond_spread": bool(med["fused"] - med["chain"] > max(spread.values())),
                      "bytes_min": nbytes, "fused_GBps": round(nbytes / med["fused"] / 1e3, 1),
                      "max_rel_diff": {k: float(f"{v:.3g}") for k, v in errs.items()}}), flush=True)
