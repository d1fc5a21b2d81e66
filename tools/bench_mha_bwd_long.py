#!/usr/bin/env python3
"""Tuning only: the attention backward beyond 256 kept tokens per image (ldn_packed_mha_bwd_long: k_packed_mha_bwd_q + k_packed_mha_bwd_kv) --
one JSON line per shape, appended to profiles/mha_bwd_long.jsonl (or --out), B = 64 and 6 heads by default:
  (a) L = 197, keep 1.0 and 0.5: the one-launch kernel (ops.packed_mha_bwd) against the pair on the same lists -- identical work and
      bit-identical rows (checked here too): what the second launch and the round trip of the statistics through the workspace cost;
  (b) the DeiT-S 384 px shape, L = 577, keep 1.0 and 0.5: the pair alone (nothing else runs this shape).
The variants of a shape alternate inside every round (device events around `--iters` calls, the output buffer and the workspace allocated
once outside the timed region); median and minimum over the rounds, in microseconds per call."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from laudnet_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mha_bwd_long.jsonl"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--heads", type=int, default=6)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")
B, heads = args.batch, args.heads
dim = 64 * heads


def time_variants(fns):
    """{name: fn} -> {name: (median us, min us)}; the variants alternate inside every round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {n: [] for n in fns}
    for _ in range(args.rounds):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[n].append(1000.0 * e0.elapsed_time(e1) / args.iters)
    return {n: (statistics.median(v), min(v)) for n, v in us.items()}


def shape(name, L, p, short):
    g = torch.Generator().manual_seed(7 + L)
    keep = (torch.rand(B, L, generator=g) < p).float()
    keep[:, 0] = 1.0
    keep = keep.to(dev)
    gd = torch.Generator(device=dev).manual_seed(3)
    qkv = torch.randn(B * L, 3 * dim, device=dev, generator=gd)
    d_out = torch.randn(B * L, dim, device=dev, generator=gd)          # packed rows; those past the count are not read
    tok_rows, prefix, count = ops.token_lists(keep)
    out = torch.zeros(B * L, 3 * dim, device=dev)
    ws = torch.empty(3 * heads * B * L, device=dev)
    fns = {"long": lambda: ops.packed_mha_bwd_long(qkv, tok_rows, prefix, B, heads, L, d_out, out=out, ws=ws)}
    rec = {"shape": name, "B": B, "heads": heads, "L": L, "keep": p, "kept_per_image": int(count.item()) / B, "gpu": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "iters": args.iters}
    if short:
        out_s = torch.zeros(B * L, 3 * dim, device=dev)
        fns["short"] = lambda: ops.packed_mha_bwd(qkv, tok_rows, prefix, B, heads, L, d_out, out=out_s)
        fns["long"](), fns["short"]()
        rec["long_bit_identical_to_short"] = bool(torch.equal(out, out_s))
    t = time_variants(fns)
    for nme, (med, mn) in t.items():
        rec[f"us_{nme}_median"], rec[f"us_{nme}_min"] = round(med, 2), round(mn, 2)
    if short:
        rec["long_over_short_median"] = round(t["long"][0] / t["short"][0], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


shape("a_L197_keep1.0", 197, 1.0, True)
shape("a_L197_keep0.5", 197, 0.5, True)
shape("b_deit_s_384px_keep1.0", 577, 1.0, False)
shape("b_deit_s_384px_keep0.5", 577, 0.5, False)
