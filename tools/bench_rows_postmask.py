#!/usr/bin/env python3
"""ops.rows_img_dot + ops.rows_postmask_bwd (layer b of a LAD-RegNet channel block's backward: SE prologue, channel mask, ReLU gate, scale, and the
reductions d shift / d scale / d gate / d mask) beside the equivalent chain of PyTorch tensor ops on the same GPU -- the lines of
training._RegNetSkipBranchFn.backward they stand for, with the per-image channel mask and the mask's straight-through sum added.  Shapes: the four
stages of RegNetY-800MF at 224 x 224 (bottleneck widths 64 / 144 / 320 / 784 on 56^2 / 28^2 / 14^2 / 7^2 pixels), all pixels of `--batch` images.

The two legs ALTERNATE round by round in one process; a round is `--iters` back-to-back calls between two device events behind a synchronise; the
figure is the median over `--rounds` (>= 9) rounds.  `bytes_min` is what the kernels' contract must move (read dz and r twice -- once per kernel --,
write du: 5 matrices), `kernels_GBps` that over the kernels' median.  Outputs are compared once per shape (max |kernels - chain| relative to the
chain's maximum).  One JSON line per shape.
usage: tools/bench_rows_postmask.py [--batch 32] [--rounds 11] [--iters 20]"""
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
STAGES = [(64, 56), (144, 28), (320, 14), (784, 7)]          # (bottleneck width, output size) of RegNetY-800MF's four stages


def chain(dz, r, m, gate, dsq, s, t, B, P, W):
    """the tensor-op form: -> (du, g_shift, g_scale_num, g_mask, d gate)"""
    dzv, rv = dz.view(B, P, W), r.view(B, P, W)
    dgate = (dzv * rv).sum(1) * m
    dh = dzv * gate.unsqueeze(1) + dsq.unsqueeze(1)
    a = dh * (rv > 0) * m.unsqueeze(1)
    du = (a * s).view(B * P, W)
    a2 = a.view(B * P, W)
    return du, a2.sum(0), (a2 * (r - t)).sum(0), (dh * rv).sum(1), dgate


def kernels(dz, r, m, gate, dsq, s, t, pre):
    dgate = ops.rows_img_dot(dz, r, pre) * m
    du, g_shift, g_scale, g_mask = ops.rows_postmask_bwd(dz, r, s, t, chan_mask=m, row_prefix=pre, gate=gate, dsq=dsq, want_mask=True)
    return du, g_shift, g_scale, g_mask, dgate


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
    dz, r = rnd(B * P, W), torch.relu(rnd(B * P, W))
    m = (torch.rand(B, W, device=dev, generator=gen) < 0.5).float()
    gate, dsq = torch.sigmoid(rnd(B, W)), (rnd(B, W) / P).contiguous()
    s, t = 0.5 + torch.rand(W, device=dev, generator=gen), 0.1 * rnd(W)
    pre = (torch.arange(B + 1, device=dev, dtype=torch.int32) * P).contiguous()
    legs = {"kernels": lambda: kernels(dz, r, m, gate, dsq, s, t, pre), "tensor_ops": lambda: chain(dz, r, m, gate, dsq, s, t, B, P, W)}
    got, want = legs["kernels"](), legs["tensor_ops"]()
    err = max(((g - w).abs().max() / w.abs().max().clamp(min=1e-30)).item() for g, w in zip(got, want))
    for fn in legs.values():                        # warm-up of both legs
        timed(fn, 3)
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    nbytes = 5 * B * P * W * 4
    print(json.dumps({"what": "layer b of the channel block's backward: rows_img_dot + rows_postmask_bwd (prologue, mask, g_mask) vs the tensor-op chain",
                      "batch": B, "width": W, "rows": B * P, "rounds": args.rounds, "iters_per_round": args.iters,
                      "kernels_us_median": round(med["kernels"], 2), "tensor_ops_us_median": round(med["tensor_ops"], 2),
                      "kernels_us_min_max": [round(min(us["kernels"]), 2), round(max(us["kernels"]), 2)],
                      "tensor_ops_us_min_max": [round(min(us["tensor_ops"]), 2), round(max(us["tensor_ops"]), 2)],
                      "speedup": round(med["tensor_ops"] / med["kernels"], 2), "bytes_min": nbytes,
                      "kernels_GBps": round(nbytes / med["kernels"] / 1e3, 1), "max_rel_diff": err}), flush=True)
