#!/usr/bin/env python3
"""Tuning only: ldn_packed_mha beyond 256 kept tokens per image (k_packed_mha_long) -- one JSON line per shape, appended to
profiles/mha_long.jsonl (or --out):
  (a) B = 64, 6 heads, 256 kept of L = 320 tokens: max_tokens = 256 (k_packed_mha) against max_tokens = 320 (k_packed_mha_long,
      identical work, bit-identical rows -- checked here too);
  (b) the DeiT-S 384 px shape, L = 577, keep 0.7 and keep 1.0: k_packed_mha_long alone.
Each beside torch's dense masked attention (scaled_dot_product_attention, fp32, all L tokens as queries, the keep mask on the keys) on
the same GPU.  The variants of a shape alternate inside every round (device events around `--iters` launches); median and minimum over
the rounds, in microseconds per launch."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from laudnet_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mha_long.jsonl"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--heads", type=int, default=6)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")
B, heads = args.batch, args.heads
dim = 64 * heads


def keep_mask(L, kept, p, seed):
    """[B, L]: exactly `kept` tokens per image (CLS among them), or Bernoulli(p) with CLS kept."""
    g = torch.Generator().manual_seed(seed)
    if kept is not None:
        k = torch.zeros(B, L)
        for b in range(B):
            k[b, torch.randperm(L - 1, generator=g)[: kept - 1] + 1] = 1.0
    else:
        k = (torch.rand(B, L, generator=g) < p).float()
    k[:, 0] = 1.0
    return k


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


def shape(name, L, kept=None, p=None, short=False):
    keep = keep_mask(L, kept, p, 7 + L).to(dev)
    qkv = torch.randn(B * L, 3 * dim, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    tok_rows, prefix, count = ops.token_lists(keep)
    q, k, v = (t.contiguous() for t in qkv.view(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4))
    mask = (keep > 0.5).view(B, 1, 1, L)
    fns = {"long": lambda: ops.packed_mha(qkv, tok_rows, prefix, B, heads, L)}
    if short:
        fns["short"] = lambda: ops.packed_mha(qkv, tok_rows, prefix, B, heads, 256)
    fns["torch_sdpa"] = lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    n = int(count.item())
    got = fns["long"]()[:n]
    want = fns["torch_sdpa"]().transpose(1, 2).reshape(B * L, dim)[tok_rows[:n].long()]
    rec = {"shape": name, "B": B, "heads": heads, "L": L, "kept_per_image": n / B, "gpu": torch.cuda.get_device_name(0),
           "max_abs_diff_vs_torch_fp32": (got - want).abs().max().item()}
    if short:
        rec["long_bit_identical_to_short"] = bool(torch.equal(got, fns["short"]()[:n]))
    t = time_variants(fns)
    for nme, (med, mn) in t.items():
        rec[f"us_{nme}_median"], rec[f"us_{nme}_min"] = round(med, 2), round(mn, 2)
    if short:
        rec["long_over_short_median"] = round(t["long"][0] / t["short"][0], 4)
    rec["torch_over_long_median"] = round(t["torch_sdpa"][0] / t["long"][0], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


shape("a_256_kept_of_320", 320, kept=256, short=True)
shape("b_deit_s_384px_keep0.7", 577, p=0.7)
shape("b_deit_s_384px_keep1.0", 577, p=1.0)
