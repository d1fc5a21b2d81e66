#!/usr/bin/env python3
"""ops.grouped_mfma_conv3x3_rows (LAD-RegNet conv b at group widths 8 and 24 on the matrix cores, bf16x3) beside ops.grouped_conv3x3_rows (the fp32
VALU kernel those widths run on while laud_regnet.USE_GROUPED_MFMA_WIDTHS is off), then a whole layer-skip eval step of each model with the
switch on and off.  This comparison -- the switch being the only difference -- is what decides a later flip of the default.

Shapes: conv b (stride 1, folded BatchNorm, ReLU) of the four stages of RegNetY-400MF (group width 8, w_b 48 / 104 / 208 / 440) and RegNetY-1.6GF
(group width 24, w_b 48 / 120 / 336 / 888) on 56^2 / 28^2 / 14^2 / 7^2 output maps, `--batch` images of which a seeded half are kept (layer
skip: the packed rows are the kept images' pixels, the list built by ops.mask_to_index).

The two legs ALTERNATE round by round in one process.  A round is a window of back-to-back calls between two device events behind a
synchronise, as many calls as fill `--window` seconds (>= 0.5; sized from a warm-up window per leg); the figure is the median over `--rounds`
(>= 9) rounds and the spread of a leg is its max - min over the rounds.  Before the timing the two outputs are compared at the timed size and
must agree to 1e-4 max(1, |ref|max) (asserted).  One JSON line per shape and one per model; `--out` also appends them to a file
(profiles/grouped_mfma_widths.jsonl).
usage: tools/bench_grouped_mfma.py [--batch 64] [--rounds 9] [--window 0.5] [--out FILE] [--no-models]"""
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
from laudnet_amd import laud_regnet, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--out", default=None)
ap.add_argument("--no-models", action="store_true")
args = ap.parse_args()
assert args.rounds >= 9, "the median of at least 9 rounds"
assert args.window >= 0.5, "windows of at least half a second"
dev = torch.device("cuda", 0)
laudnet_amd.load_library()
ops.set_math_mode("bf16x3")
MODELS = {"regnet_y_400mf": ("lad_regnet_y_400mf", 8, [48, 104, 208, 440]), "regnet_y_1_6gf": ("lad_regnet_y_1_6gf", 24, [48, 120, 336, 888])}
MAPS = [56, 28, 14, 7]


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


def alternate(legs):
    """-> {leg: (median, min, max, calls per window)} in milliseconds per call; the legs alternate round by round"""
    calls = {}
    for k, fn in legs.items():                      # warm-up, and the size of a window
        window(fn, 3)
        calls[k] = max(3, int(args.window * 1e3 / window(fn, 10)) + 1)
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(window(fn, calls[k]))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v), calls[k]) for k, v in ms.items()}


def verdict(res, new, old):
    spread = max(res[new][2] - res[new][1], res[old][2] - res[old][1])
    return {"old_over_new": round(res[old][0] / res[new][0], 3),
            "new_faster_beyond_spread": bool(res[old][0] - res[new][0] > spread), "new_slower_beyond_spread": bool(res[new][0] - res[old][0] > spread)}


for model, (arch, gw, widths) in MODELS.items():
    for stage, (C, S) in enumerate(zip(widths, MAPS)):
        B = args.batch
        keep = seeded_bernoulli((B, 1, 1), 0.5, 7 + stage)
        ix = ops.mask_to_index(keep.to(dev), S, S, 1)
        n3 = int(ix.cnt[0].item())
        h_a = torch.relu(seeded_randn((ix.cap1, C), 11 + C)).to(dev)
        w = (seeded_randn((C, 9, gw), 12 + C) * (2.0 / (9 * gw)) ** 0.5).to(dev)
        g = torch.Generator().manual_seed(13 + C)
        scale, shift = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
        frag = ops.pack_grouped_mfma_weights(w, gw)
        out_new, out_old = torch.zeros(ix.cap3, C, device=dev), torch.zeros(ix.cap3, C, device=dev)
        legs = {"mfma": lambda: ops.grouped_mfma_conv3x3_rows(h_a, ix.nbr, frag, gw, scale, shift, out_new, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1),
                "valu": lambda: ops.grouped_conv3x3_rows(h_a, ix.nbr, w, gw, scale, shift, out_old, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        diff, ref_max = (out_new[:n3] - out_old[:n3]).abs().max().item(), out_old[:n3].abs().max().item()
        assert diff <= 1e-4 * max(1.0, ref_max), f"{model} stage {stage + 1}: the two kernels differ by {diff:.3e} (|ref|max {ref_max:.3e})"
        res = alternate(legs)
        nbytes = 2 * n3 * C * 4                     # the kept rows once in, once out
        emit({"what": "LAD-RegNet conv b (grouped 3x3 + BN + ReLU) over the packed rows of the kept images: ops.grouped_mfma_conv3x3_rows (bf16x3, matrix "
                      "cores) vs ops.grouped_conv3x3_rows (fp32 VALU)",
              "model": model, "stage": stage + 1, "group_width": gw, "C": C, "map": S, "batch": B, "rows": n3, "rounds": args.rounds,
              "mfma_us_median": round(1e3 * res["mfma"][0], 2), "valu_us_median": round(1e3 * res["valu"][0], 2),
              "mfma_us_min_max": [round(1e3 * res["mfma"][1], 2), round(1e3 * res["mfma"][2], 2)],
              "valu_us_min_max": [round(1e3 * res["valu"][1], 2), round(1e3 * res["valu"][2], 2)],
              "calls_per_window": {k: v[3] for k, v in res.items()}, **verdict(res, "mfma", "valu"),
              "rows_in_out_GBps_mfma": round(nbytes / (res["mfma"][0] * 1e-3) / 1e9, 1), "max_abs_diff": float(f"{diff:.3g}"), "ref_max": float(f"{ref_max:.3g}")})

if not args.no_models:
    for model, (arch, gw, widths) in MODELS.items():
        net = getattr(laudnet_amd, arch)(dyn_mode=["spatial"] * 4, mask_spatial_granularity=MAPS, num_classes=1000, input_size=224).eval()
        net.load_state_dict(damp_residual_branches(fill_state_dict(net.state_dict(), 1)))
        net = net.to(dev)
        for i, blk in enumerate(net.blocks()):      # layer skip: one decision per image, a seeded half kept in every block
            blk.f.forced_spatial_mask = seeded_bernoulli((args.batch, 1, 1, 1), 0.5, 100 + i)
        x = seeded_randn((args.batch, 3, 224, 224), 1000).to(dev).contiguous(memory_format=torch.channels_last)

        def step(on):
            laud_regnet.USE_GROUPED_MFMA_WIDTHS = on
            with torch.no_grad():
                return net(x, 1.0)[0]
        before = laud_regnet.USE_GROUPED_MFMA_WIDTHS
        try:
            y_on, y_off = step(True), step(False)
            diff, ref_max = (y_on - y_off).abs().max().item(), y_off.abs().max().item()
            res = alternate({"on": lambda: step(True), "off": lambda: step(False)})
        finally:
            laud_regnet.USE_GROUPED_MFMA_WIDTHS = before
        emit({"what": "layer-skip eval step (a seeded half of the images kept in every block, bf16x3) with laud_regnet.USE_GROUPED_MFMA_WIDTHS on vs off",
              "model": model, "group_width": gw, "batch": args.batch, "rounds": args.rounds,
              "on_ms_median": round(res["on"][0], 3), "off_ms_median": round(res["off"][0], 3),
              "on_ms_min_max": [round(res["on"][1], 3), round(res["on"][2], 3)], "off_ms_min_max": [round(res["off"][1], 3), round(res["off"][2], 3)],
              "calls_per_window": {k: v[3] for k, v in res.items()}, **verdict(res, "on", "off"),
              "logits_max_abs_diff": float(f"{diff:.3g}"), "logits_ref_max": float(f"{ref_max:.3g}")})
