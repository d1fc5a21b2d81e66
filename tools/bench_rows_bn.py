#!/usr/bin/env python3
"""ops.rows_bn_stats + ops.rows_bn_fwd + ops.rows_bn_bwd (one BatchNorm layer of a LAUD-ResNet block on batch statistics, forward and backward: the
channel mask in front, ReLU, d gamma / d beta, the gradient through the statistics and the mask's straight-through sum) beside the equivalent
chain of PyTorch tensor ops on the same GPU -- what training._BatchStatsBranchFn would otherwise run per layer.  Shapes: the four stages of
LAUD-ResNet50 at 224 x 224 (bottleneck widths 64 / 128 / 256 / 512 on 56^2 / 28^2 / 14^2 / 7^2 pixels), all pixels of `--batch` images.

The two legs ALTERNATE round by round in one process; a round is `--iters` back-to-back calls between two device events behind a synchronise; the
figure is the median over `--rounds` (>= 9) rounds.  `bytes_min` is what the kernels' contract must move (statistics: read u; forward: read u, write
h; backward: read dh, u, h twice -- once per pass -- and write du: 10 matrices), `kernels_GBps` that over the kernels' median.  Outputs are compared
once per shape (per output, max |kernels - chain| relative to the chain's maximum; `relu_gates_that_differ` counts the elements whose pre-activation
rounds to the other side of zero on one leg -- each moves du there by O(1)).  One JSON line per shape.
usage: tools/bench_rows_bn.py [--batch 32] [--rounds 11] [--iters 20]"""
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
STAGES = [(64, 56), (128, 28), (256, 14), (512, 7)]          # (bottleneck width, output size) of LAUD-ResNet50's four stages


def chain(u, dh, m, gamma, beta, B, P, W):
    """the tensor-op form: -> (h, du, d_gamma, d_beta, g_mask)"""
    uv, mv = u.view(B, P, W), m.unsqueeze(1)
    x = uv * mv
    var, mean = torch.var_mean(x, dim=(0, 1), unbiased=False)
    inv = torch.rsqrt(var + EPS)
    xhat = (x - mean) * inv
    h = torch.relu(gamma * xhat + beta)
    dz = dh.view(B, P, W) * (h > 0)
    d_beta, d_gamma = dz.sum((0, 1)), (dz * xhat).sum((0, 1))
    g = (gamma * inv) * (dz - d_beta / (B * P) - xhat * (d_gamma / (B * P)))
    return h.view(B * P, W), (g * mv).view(B * P, W), d_gamma, d_beta, (g * uv).sum(1)


def kernels(u, dh, m, gamma, beta, pre):
    mean, _, inv = ops.rows_bn_stats(u, EPS, chan_mask=m, row_prefix=pre)
    h = ops.rows_bn_fwd(u, mean, inv, gamma, beta, chan_mask=m, row_prefix=pre)
    du, d_gamma, d_beta, g_mask = ops.rows_bn_bwd(dh, u, h, mean, inv, gamma, chan_mask=m, row_prefix=pre, want_mask=True)
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
    u, dh = rnd(B * P, W) + 0.5, rnd(B * P, W)
    m = (torch.rand(B, W, device=dev, generator=gen) < 0.6).float()
    gamma, beta = 0.5 + torch.rand(W, device=dev, generator=gen), 0.1 * rnd(W)
    pre = (torch.arange(B + 1, device=dev, dtype=torch.int32) * P).contiguous()
    legs = {"kernels": lambda: kernels(u, dh, m, gamma, beta, pre), "tensor_ops": lambda: chain(u, dh, m, gamma, beta, B, P, W)}
    got, want = legs["kernels"](), legs["tensor_ops"]()
    errs = {n: ((g - w).abs().max() / w.abs().max().clamp(min=1e-30)).item() for n, g, w in zip(("h", "du", "d_gamma", "d_beta", "g_mask"), got, want)}
    # a pre-activation within rounding of zero may open the ReLU on one leg only; such an element moves du (and the sums) by O(1): counted, not hidden
    flips = int(((got[0] > 0) != (want[0] > 0)).sum())
    for fn in legs.values():                        # warm-up of both legs
        timed(fn, 3)
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    nbytes = 10 * B * P * W * 4
    print(json.dumps({"what": "one BatchNorm layer on batch statistics, forward + backward: rows_bn_stats + rows_bn_fwd + rows_bn_bwd (channel mask, g_mask) "
                              "vs the tensor-op chain", "launches": 2 + 1 + 4,
                      "batch": B, "width": W, "rows": B * P, "rounds": args.rounds, "iters_per_round": args.iters,
                      "kernels_us_median": round(med["kernels"], 2), "tensor_ops_us_median": round(med["tensor_ops"], 2),
                      "kernels_us_min_max": [round(min(us["kernels"]), 2), round(max(us["kernels"]), 2)],
                      "tensor_ops_us_min_max": [round(min(us["tensor_ops"]), 2), round(max(us["tensor_ops"]), 2)],
                      "speedup": round(med["tensor_ops"] / med["kernels"], 2), "bytes_min": nbytes,
                      "kernels_GBps": round(nbytes / med["kernels"] / 1e3, 1), "max_rel_diff": {k: float(f"{v:.3g}") for k, v in errs.items()}, "relu_gates_that_differ": flips}), flush=True)
