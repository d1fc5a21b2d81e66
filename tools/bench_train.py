#!/usr/bin/env python3
"""One training step (forward + backward, frozen BatchNorm statistics, Gumbel-hard masks, sparsity criterion) of a full-width LAUD-ResNet on the row
kernels (laudnet_amd.training.train_forward) beside the oracle's dense emulation run through PyTorch on the same GPU.  One JSON line per workload;
it names the weight-gradient path (`wgrad_kernel`: laudnet_amd.training.USE_WGRAD_KERNEL, env LDN_WGRAD=0 | 1) and the peak memory of ONE step on
the row kernels (`peak_MiB_one_step`: torch.cuda.max_memory_allocated of a step of its own after the timed ones).
`both` is the reference's constructor default (pixel x channel masks: spatial S=4-4-2-1 and channel-2222 together), same model, batch and loss
convention as the other three.  `regnet` is the full-width LAD-RegNetY-800MF in its layer-skip form (bench.py's workload, keep 0.5) beside
oracle/regnet_ref.py's dense emulation; `regnet_channel` is the same model in dyn_mode 'channel' (the one LAD-RegNet recipe the reference trains:
MLP maskers, two layers, reduction 16, granularity 1; training.USE_REGNET_CHANNEL is turned on for it) -- dense in the channels on the row kernels,
so about the dense emulation's time is what to expect.  `--ab-wgrad` adds `wgrad_ab`: further steps of the row-kernel leg with the weight-gradient kernels
(training.USE_WGRAD_KERNEL) off and on ALTERNATING step by step in this one process, the median of each setting's device-event intervals.
`ms_per_step` is the mean of the timed steps (wall clock over the loop), `ms_per_step_median` the median of the
steps' own device-event intervals.
`--batch-stats` is the reference's own ImageNet recipe: every BatchNorm on the statistics of the batch (plain model.train() on both legs;
training.USE_BATCH_STATS is turned on), on the full-width LAUD-ResNet50 that train_scripts.sh trains for the LAUD-ResNet workloads, and on
LAD-RegNetY-800MF for `regnet_channel` (train_scripts.sh's third command); LAD-RegNet layer skip is not built in this mode.  Dense by
construction on both legs (the masks save no FLOPs), so about the dense emulation's time is what to expect.
usage: [LDN_WGRAD=0] tools/bench_train.py [--batch 32] [--steps 5] [--warmup 2] [--workloads layer,spatial,channel,both,regnet,regnet_channel] [--no-reference] [--ab-wgrad] [--batch-stats]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

import bench  # noqa: E402
import laudnet_amd  # noqa: E402
from fill import damp_residual_branches, fill_state_dict, seeded_randn  # noqa: E402
from laudnet_amd import ops, training  # noqa: E402
from laudnet_amd.training import prepare_for_training, train_forward  # noqa: E402
from oracle import regnet_ref as RR  # noqa: E402
from oracle import torch_ref as TR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--workloads", default="layer,spatial,channel")
ap.add_argument("--math", default="bf16x3")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-reference", action="store_true", help="time the row kernels only (no dense emulation through PyTorch, no speedup)")
ap.add_argument("--ab-wgrad", action="store_true", help="also time the row-kernel leg with the weight-gradient kernels off / on, alternating per step")
ap.add_argument("--batch-stats", action="store_true", help="BatchNorm on batch statistics (plain model.train()) on a LAUD-ResNet50 / LAD-RegNetY-800MF channel, both legs")
args = ap.parse_args()
dev = torch.device("cuda", 0)
ops.set_math_mode(args.math)
WORKLOADS = dict(bench.WORKLOADS)
WORKLOADS["both"] = dict(name="LAUD-ResNet101 both (spatial S=4-4-2-1 x channel-2222) @224",
                         kw=dict(dyn_mode=["both"] * 4, mask_spatial_granularity=[4, 4, 2, 1], channel_dyn_granularity=[2, 2, 2, 2],
                                 channel_masker=["MLP"] * 4, channel_masker_layers=[2, 2, 2, 2], reduction_ratio=[16] * 4),
                         p_channel=0.62, p_spatial=0.5)
WORKLOADS["regnet_channel"] = dict(name="LAUD-RegNetY-800MF channel target-0.5 @224", arch="lad_regnet_y_800mf",
                                   kw=dict(dyn_mode=["channel"] * 4, channel_dyn_granularity=[1, 1, 1, 1], channel_masker=["MLP"] * 4,
                                           channel_masker_layers=[2, 2, 2, 2], reduction_ratio=[16] * 4), p_channel=0.5, p_spatial=None)


def calibrate_regnet_channel(model, x, p_channel):
    """bench.calibrate_maskers for LAD-RegNet channel maskers (its channel branch reads an attribute LAUD-ResNet blocks alone carry): one sequential
    pass that shifts each masker's keep-logit bias so that the requested fraction of channel groups is kept on this batch"""
    with torch.no_grad():
        state = (model.stem(x.contiguous(memory_format=torch.channels_last)), None, None, None, None, None, torch.tensor(0.0, device=x.device))
        for blk in model.blocks():
            mk = blk.f.masker_channel
            G = mk.channel_dyn_group
            _, _, _, logits = mk.lists(state[0], blk.f.w_b // G, want_logits=True)
            diff = (logits[:, :G] - logits[:, G:]).flatten().float()
            last = mk.conv[-1] if mk.layers == 2 else mk.conv
            last.bias.data[:G] -= torch.quantile(diff.cpu(), 1.0 - p_channel).item()
            mk._drop_cache()
            state = blk(state, 1.0)


for w in args.workloads.split(","):
    wl = WORKLOADS[w]
    if w == "regnet_channel":
        training.USE_REGNET_CHANNEL = True
    kw = dict(wl["kw"], num_classes=1000, input_size=224)
    arch = wl.get("arch", "uni_resnet101")
    if args.batch_stats:
        assert w == "regnet_channel" or not arch.startswith("lad_regnet"), \
            "--batch-stats: LAUD-ResNet workloads and regnet_channel only (LAD-RegNet layer skip on batch statistics is not built)"
        training.USE_BATCH_STATS = True
        if w != "regnet_channel":
            arch, wl = "uni_resnet50", dict(wl, name=wl["name"].replace("ResNet101", "ResNet50"))
    hip = getattr(laudnet_amd, arch)(**kw)
    hip.load_state_dict(damp_residual_branches(fill_state_dict(hip.state_dict(), 1)))      # (the last BatchNorm of every residual branch x 0.3)
    hip = hip.to(dev).eval()
    x = seeded_randn((args.batch, 3, 224, 224), 1000).to(dev).contiguous(memory_format=torch.channels_last)
    if w == "regnet_channel":
        calibrate_regnet_channel(hip, x, wl["p_channel"])
    else:
        bench.calibrate_maskers(hip, x, wl["p_channel"], wl["p_spatial"])
    sd = {k: v.detach().clone() for k, v in hip.state_dict().items()}
    ref = RR.regnet_y_ref(arch, **kw) if arch.startswith("lad_regnet") else (TR.resnet50_ref if arch == "uni_resnet50" else TR.resnet101_ref)(**kw)
    ref.load_state_dict(sd)
    ref = ref.to(dev).train()
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and not args.batch_stats:
            m.eval()
    prepare_for_training(hip, batch_stats=args.batch_stats)
    g = seeded_randn((args.batch, 1000), 5).to(dev)

    def step(fwd, model):
        for p in model.parameters():
            p.grad = None
        out = fwd()
        loss = (out[0] * g).sum() / 10.0 + 10.0 * (out[5].mean() - 0.5) ** 2
        loss.backward()
        return out

    res = {}
    legs = [("hip_row_kernels", lambda: train_forward(hip, x, 1.0), hip)]
    if not args.no_reference:
        legs.append(("dense_emulation_pytorch", lambda: ref(x, 1.0), ref))
    for name, fwd, model in legs:
        torch.manual_seed(3)
        for _ in range(args.warmup):
            out = step(fwd, model)
        torch.cuda.synchronize()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(args.steps):
            out = step(fwd, model)
            marks[i + 1].record()
        torch.cuda.synchronize()
        per_step = sorted(a.elapsed_time(b) for a, b in zip(marks, marks[1:]))
        res[name] = {"ms_per_step": 1e3 * (time.perf_counter() - t0) / args.steps, "ms_per_step_median": per_step[len(per_step) // 2],
                     "mean_block_flops_ratio": round(float(out[5].detach().mean()), 4)}
        if name == "hip_row_kernels":      # one more step, alone between a reset and a read of the allocator's high-water mark
            out = None
            for p in model.parameters():
                p.grad = None
            torch.cuda.reset_peak_memory_stats()
            step(fwd, model)
            torch.cuda.synchronize()
            res[name]["peak_MiB_one_step"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    if args.ab_wgrad:
        # the A/B of the weight-gradient kernels on this workload: off and on alternate step by step behind a warm-up step of each, same process
        shipped = training.USE_WGRAD_KERNEL
        fwd, times = legs[0][1], {False: [], True: []}
        torch.manual_seed(3)
        for k in range(2 * (args.steps + 1)):
            training.USE_WGRAD_KERNEL = on = bool(k % 2)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(fwd, hip)
            b.record()
            torch.cuda.synchronize()
            if k >= 2:
                times[on].append(a.elapsed_time(b))
        training.USE_WGRAD_KERNEL = shipped
        med = lambda v: sorted(v)[len(v) // 2]
        res["wgrad_ab"] = {"steps_each": args.steps, "ms_per_step_median_wgrad_off": med(times[False]), "ms_per_step_median_wgrad_on": med(times[True])}
    if not args.no_reference:
        res["speedup"] = res["dense_emulation_pytorch"]["ms_per_step"] / res["hip_row_kernels"]["ms_per_step"]
    print(json.dumps({"workload": wl["name"], "batch": args.batch, "steps": args.steps, "math": args.math, "wgrad_kernel": training.USE_WGRAD_KERNEL,
                      "batch_stats": args.batch_stats,
                      "what": "one training step = forward + backward of every parameter, " + ("BatchNorm on batch statistics" if args.batch_stats else
                                                                                              "frozen BatchNorm statistics") + ", Gumbel-hard masks", **res}), flush=True)
    del hip, ref
    torch.cuda.empty_cache()
