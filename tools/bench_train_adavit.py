#!/usr/bin/env python3
"""One forward + backward of a DeiT-S-shaped token-skipping trunk (12 x 384 / 6 heads, L 197; --tokens 577 = the 384 px input) on the packed kernels
(laudnet_amd.adavit.train_forward) beside oracle/adavit_ref.TokenSkipViTRef under PyTorch autograd in fp32 on the same GPU, at keep 0.5 and
keep 1.0.  Same process, the two legs ALTERNATE step by step behind warm-up steps of each; the figure is the median of each leg's own
device-event intervals.  One JSON line per keep ratio (profiles/train_step_adavit.jsonl).
Beyond 256 tokens the attention backward is ldn_packed_mha_bwd_long: the tool turns adavit.USE_LONG_BWD on for such a run.
usage: tools/bench_train_adavit.py [--batch 64] [--steps 10] [--warmup 3] [--keeps 0.5,1.0] [--depth 12] [--tokens 197]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

from fill import seeded_bernoulli, seeded_randn  # noqa: E402
from laudnet_amd import adavit, ops, training  # noqa: E402
from laudnet_amd.adavit import TokenSkipViT, train_forward  # noqa: E402
from oracle import adavit_ref as AR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--keeps", default="0.5,1.0")
ap.add_argument("--depth", type=int, default=12)
ap.add_argument("--tokens", type=int, default=197, help="sequence length L (197: 224 px, 577: 384 px)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
L, dim, heads = args.tokens, 384, 6
if L > adavit.BWD_MAX_TOKENS:
    adavit.USE_LONG_BWD = True
ops.set_math_mode("bf16x3")
ref = AR.TokenSkipViTRef(args.depth, dim, heads)
gen = torch.Generator().manual_seed(1)
with torch.no_grad():
    for p in ref.parameters():
        if p.dim() > 1:
            p.copy_(0.03 * torch.randn(p.shape, generator=gen))
hip = TokenSkipViT(args.depth, dim, heads)
hip.load_state_dict(ref.state_dict())
ref, hip = ref.to(dev).train(), hip.to(dev).train()
x = seeded_randn((args.batch, L, dim), 31).to(dev)
g = seeded_randn((args.batch, L, dim), 32).to(dev)
for keep_p in (float(k) for k in args.keeps.split(",")):
    keeps = []
    for i in range(args.depth):
        k = seeded_bernoulli((args.batch, L), keep_p, 40 + i)
        k[:, 0] = 1.0
        keeps.append(k.to(dev))

    def step(model, fwd):
        for p in model.parameters():
            p.grad = None
        xv = x.clone().requires_grad_(True)
        (fwd(xv) * g).sum().backward()

    legs = {"hip_packed_kernels": (hip, lambda xv: train_forward(hip, xv, keeps)), "oracle_pytorch_fp32": (ref, lambda xv: ref(xv, keeps))}
    times = {k: [] for k in legs}
    for it in range(args.warmup + args.steps):
        for name, (model, fwd) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(model, fwd)
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append(a.elapsed_time(b))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"workload": f"token-skip trunk {args.depth} x {dim} / {heads} heads, L {L}", "batch": args.batch, "keep": keep_p,
                      "kept_tokens_mean": round(float(torch.stack(keeps).mean()), 4), "steps": args.steps, "warmup": args.warmup,
                      "wgrad_kernel": training.USE_WGRAD_KERNEL, "long_bwd": L > adavit.BWD_MAX_TOKENS, "what": "one forward + backward (d x and every parameter), median of device-event intervals, legs alternating",
                      "ms_per_step_median": {k: round(v, 3) for k, v in med.items()},
                      "ms_per_step_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
                      "speedup_vs_oracle": round(med["oracle_pytorch_fp32"] / med["hip_packed_kernels"], 3)}), flush=True)
