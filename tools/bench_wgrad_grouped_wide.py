#!/usr/bin/env python3
"""ops.wgrad_grouped_wide_rows (the weight gradient of LAD-RegNet's conv b over packed rows at group widths 56, 112 and 232 on the matrix
cores, bf16x3) beside the two ways to compute it without that kernel, then a whole training step of `--step-model` (lad_regnet_y_8gf) with
training.USE_WGRAD_GROUPED_WIDE on and off.  The yardstick is always the switch-off path in the same run.

Legs per shape:
    (a) kernel       ops.wgrad_grouped_wide_rows: one launch over all groups (+ the reduce launch when the rows are split)
    (b) gather_bmm   training._weight_grad_grouped_3x3: the [rows, 9, C] gather, the per-group permute and one torch.bmm -- what training runs
                     at these widths while the switch is off
    (c) slice_loop   a host loop of ops.wgrad_rows over the G column slices of dY and h_a into row slices of one output (2 G launches); left
                     out, and said so in the record, where ops.wgrad_rows refuses the slice's width

Shapes: conv b of the four stages of RegNetY-8GF (group width 56, w_b 224 / 448 / 896 / 2016) and RegNetY-16GF (group width 112, w_b 224 /
448 / 1232 / 3024) and RegNetY-32GF (group width 232, w_b 232 / 696 / 1392 / 3712; `--models` picks) on 56^2 / 28^2 / 14^2 / 7^2 output maps at stride 1, and each stage's stride-2 first-block shape (input map twice the
output map); `--batch` images of which a seeded half are kept (layer skip: the packed rows are the kept images' pixels, the lists built by
ops.mask_to_index).  dY is a seeded normal matrix with zero rows past the count (what the backward hands over), h_a a seeded ReLU output.

The legs ALTERNATE round by round in one process.  A round is a window of back-to-back calls between two device events behind a
synchronise, as many calls as fill `--window` seconds (>= 0.5; sized from a warm-up window per leg); the figure is the median over `--rounds`
(>= 9) rounds, and a difference counts only where the two legs' ranges (min to max over the rounds) do not overlap.  Before the timing legs
(a) and (c) are compared with (b) at the timed size and must agree to 1e-4 max(1, |ref|max) (asserted).  `frac_bf16_roof_executed` = 3 x the
algorithmic FLOP rate (2 rows C 9 gw per call; bf16x3 executes three products per one) over the 2500 TFLOP/s dense bf16 matrix peak, as
bench.py --full computes `frac_executed`.  One JSON line per shape and one for the model step; `--out` also appends them to a file
(profiles/wgrad_grouped_wide.jsonl).
usage: tools/bench_wgrad_grouped_wide.py [--batch 32] [--rounds 9] [--window 0.5] [--out FILE] [--no-kernels] [--no-models]
                                         [--models regnet_y_8gf,regnet_y_16gf,regnet_y_32gf] [--step-model regnet_y_8gf]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

import laudnet_amd  # noqa: E402
from fill import damp_residual_branches, fill_state_dict, seeded_bernoulli, seeded_randn  # noqa: E402
from laudnet_amd import laud_regnet, ops, training  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--out", default=None)
ap.add_argument("--no-kernels", action="store_true")
ap.add_argument("--no-models", action="store_true")
ap.add_argument("--models", default=None)
ap.add_argument("--step-model", default="regnet_y_8gf")
args = ap.parse_args()
assert args.rounds >= 9, "the median of at least 9 rounds"
assert args.window >= 0.5, "windows of at least half a second"
dev = torch.device("cuda", 0)
laudnet_amd.load_library()
ops.set_math_mode("bf16x3")
MODELS = {"regnet_y_8gf": (56, [224, 448, 896, 2016]), "regnet_y_16gf": (112, [224, 448, 1232, 3024]), "regnet_y_32gf": (232, [232, 696, 1392, 3712])}
MAPS = [56, 28, 14, 7]
BF16_MFMA_PEAK_TFLOPS = 2500.0      # bench.py


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def window(fn, calls):
    """milliseconds per call over `calls` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(legs, warm=10):
    """-> {leg: (median, min, max, calls per window)} in milliseconds per call; the legs alternate round by round"""
    calls = {}
    for k, fn in legs.items():                      # warm-up, and the size of a window
        window(fn, 2)
        calls[k] = max(3, int(args.window * 1e3 / window(fn, warm)) + 1)
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(window(fn, calls[k]))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v), calls[k]) for k, v in ms.items()}


def verdict(res, new, old):
    """a difference is real only where the two ranges (min to max of the rounds) do not overlap"""
    return {"old_over_new": round(res[old][0] / res[new][0], 3),
            "new_faster_ranges_apart": bool(res[new][2] < res[old][1]), "new_slower_ranges_apart": bool(res[new][1] > res[old][2])}


def us(r):
    return [round(1e3 * r[0], 2), round(1e3 * r[1], 2), round(1e3 * r[2], 2)]


if not args.no_kernels:
    for model in (args.models.split(",") if args.models else MODELS):
        gw, widths = MODELS[model]
        for stride in (1, 2):
            for stage, (C, S) in enumerate(zip(widths, MAPS)):
                B, G = args.batch, C // gw
                keep = seeded_bernoulli((B, 1, 1), 0.5, 7 + stage)
                ix = ops.mask_to_index(keep.to(dev), S, S, stride)
                n3 = int(ix.cnt[0].item())
                h_a = torch.relu(seeded_randn((ix.cap1, C), 11 + C)).to(dev)
                dy = seeded_randn((ix.cap3, C), 12 + C).to(dev)
                dy[n3:] = 0.0
                out_a, out_c = torch.zeros(C, 9, gw, device=dev), torch.zeros(C, 9, gw, device=dev)
                held = {}

                def kernel():
                    ops.wgrad_grouped_wide_rows(dy, h_a, ix.nbr, gw, m_count=ix.cnt[0:1], m_cap=ix.cap3, a_valid=ix.cap1, out=out_a)

                def gather_bmm():
                    held["b"] = training._weight_grad_grouped_3x3(dy, h_a, ix.nbr, ix.cap1, gw, ix.cnt[0])

                def slice_loop():
                    for g in range(G):
                        ops.wgrad_rows(dy[:, g * gw:(g + 1) * gw], h_a[:, g * gw:(g + 1) * gw], a_rows=ix.nbr, taps=9, m_count=ix.cnt[0:1],
                                       m_cap=ix.cap3, a_valid=ix.cap1, out=out_c[g * gw:(g + 1) * gw])
                legs = {"kernel": kernel, "gather_bmm": gather_bmm, "slice_loop": slice_loop}
                try:
                    slice_loop()
                except laudnet_amd.LdnError as e:            # ops.wgrad_rows does not take this width: two legs
                    del legs["slice_loop"]
                    refused = str(e)
                for fn in legs.values():
                    fn()
                torch.cuda.synchronize()
                ref = held["b"].reshape(C, gw, 9).permute(0, 2, 1)
                ref_max = ref.abs().max().item()
                diffs = {"kernel": (out_a - ref).abs().max().item()}
                if "slice_loop" in legs:
                    diffs["slice_loop"] = (out_c - ref).abs().max().item()
                for k, d in diffs.items():
                    assert d <= 1e-4 * max(1.0, ref_max), f"{model} stage {stage + 1} stride {stride} {k}: differs from the gather + bmm path by {d:.3e} (|ref|max {ref_max:.3e})"
                held.clear()
                res = alternate(legs, warm=3)
                held.clear()
                tflops = 2.0 * n3 * C * 9 * gw / (res["kernel"][0] * 1e-3) / 1e12
                vb = verdict(res, "kernel", "gather_bmm")
                if "slice_loop" in legs:
                    vc = verdict(res, "kernel", "slice_loop")
                    third = {"slice_loop_us_median_min_max": us(res["slice_loop"]), "slice_loop_over_kernel": vc["old_over_new"],
                             "kernel_faster_than_slice_loop_ranges_apart": vc["new_faster_ranges_apart"],
                             "kernel_slower_than_slice_loop_ranges_apart": vc["new_slower_ranges_apart"]}
                else:
                    third = {"slice_loop": "not timed: " + refused}
                emit({"what": "d W of LAD-RegNet conv b (grouped 3x3) over the packed rows of the kept images: (a) ops.wgrad_grouped_wide_rows (bf16x3, matrix "
                              "cores) vs (b) training._weight_grad_grouped_3x3 (gather + torch.bmm, the switch-off path) vs (c) a host loop of ops.wgrad_rows "
                              "over the G column slices",
                      "model": model, "stage": stage + 1, "stride": stride, "group_width": gw, "C": C, "groups": G, "map": S, "batch": B, "rows": n3,
                      "m_cap": ix.cap3, "rounds": args.rounds,
                      "kernel_us_median_min_max": us(res["kernel"]), "gather_bmm_us_median_min_max": us(res["gather_bmm"]),
                      **third, "calls_per_window": {k: v[3] for k, v in res.items()},
                      "gather_bmm_over_kernel": vb["old_over_new"], "kernel_faster_than_gather_bmm_ranges_apart": vb["new_faster_ranges_apart"],
                      "kernel_slower_than_gather_bmm_ranges_apart": vb["new_slower_ranges_apart"],
                      "algorithmic_tflops_kernel": round(tflops, 2), "frac_bf16_roof_executed": round(3 * tflops / BF16_MFMA_PEAK_TFLOPS, 4),
                      "max_abs_diff_vs_gather_bmm": {k: float(f"{d:.3g}") for k, d in diffs.items()}, "ref_max": float(f"{ref_max:.3g}")})
                del h_a, dy, out_a, out_c, ref, ix
                torch.cuda.empty_cache()

if not args.no_models:
    from laudnet_amd.training import prepare_for_training, train_forward
    model, gw = args.step_model, MODELS[args.step_model][0]
    net = getattr(laudnet_amd, "lad_" + model)(dyn_mode=["spatial"] * 4, mask_spatial_granularity=MAPS, num_classes=1000, input_size=224).eval()
    net.load_state_dict(damp_residual_branches(fill_state_dict(net.state_dict(), 1)))
    net = net.to(dev)
    for i, blk in enumerate(net.blocks()):      # layer skip: one decision per image, a seeded half kept in every block
        blk.f.forced_spatial_mask = seeded_bernoulli((args.batch, 1, 1, 1), 0.5, 100 + i).to(dev)
    x = seeded_randn((args.batch, 3, 224, 224), 1000).to(dev).contiguous(memory_format=torch.channels_last)
    prepare_for_training(net)
    gout = seeded_randn((args.batch, 1000), 1001).to(dev)
    before = (laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS, training.USE_WGRAD_GROUPED_WIDE)
    laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS = True

    def train_step(on):
        training.USE_WGRAD_GROUPED_WIDE = on
        for p_ in net.parameters():
            p_.grad = None
        out = train_forward(net, x, 1.0)
        ((out[0] * gout).sum() / 10.0).backward()
        return out[0]

    def grads(on):
        train_step(on)
        return {k: p_.grad.detach().clone() for k, p_ in net.named_parameters() if p_.grad is not None}
    try:
        g_on, g_off = grads(True), grads(False)
        worst = max(((g_on[k] - g_off[k]).abs().max().item() / max(g_off[k].abs().max().item(), 1e-30), k) for k in g_off)
        assert worst[0] <= 1e-3, f"a gradient differs between the switch on and off by {worst[0]:.3e} of its maximum: {worst[1]}"
        del g_on, g_off
        res = alternate({"on": lambda: train_step(True), "off": lambda: train_step(False)}, warm=2)
    finally:
        laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS, training.USE_WGRAD_GROUPED_WIDE = before
    emit({"what": "training step = forward + backward of every parameter (layer skip, a seeded half of the images kept in every block, frozen BatchNorm "
                  "statistics, bf16x3, laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS on) with training.USE_WGRAD_GROUPED_WIDE on vs off",
          "model": model, "group_width": gw, "batch": args.batch, "rounds": args.rounds,
          "on_ms_median": round(res["on"][0], 3), "off_ms_median": round(res["off"][0], 3),
          "on_ms_min_max": [round(res["on"][1], 3), round(res["on"][2], 3)], "off_ms_min_max": [round(res["off"][1], 3), round(res["off"][2], 3)],
          "calls_per_window": {k: v[3] for k, v in res.items()}, **verdict(res, "on", "off"),
          "worst_gradient_diff_over_its_max": float(f"{worst[0]:.3g}"), "worst_gradient": worst[1]})
