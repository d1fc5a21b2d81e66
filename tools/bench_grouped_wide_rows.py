#!/usr/bin/env python3
"""ops.grouped_wide_conv3x3_rows (LAD-RegNet conv b over packed rows at group widths 56, 112 and 232 on the matrix cores, bf16x3) beside
ops.grouped_conv3x3_rows (the fp32 VALU kernel those widths run on while laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS is off), then a whole
layer-skip eval step and a whole training step of `--step-model` (lad_regnet_y_8gf) with the switch on and off.  The baseline is always the switch-off path
in the same run -- the switch being the only difference -- which is what decides a later flip of the default.

Shapes: conv b (folded BatchNorm, ReLU) of the four stages of RegNetY-8GF (group width 56, w_b 224 / 448 / 896 / 2016) and RegNetY-16GF
(group width 112, w_b 224 / 448 / 1232 / 3024) and RegNetY-32GF (group width 232, w_b 232 / 696 / 1392 / 3712; `--models` picks) on 56^2 / 28^2 / 14^2 / 7^2 output maps at stride 1, and each stage's stride-2 first-block
shape (input map twice the output map); `--batch` images of which a seeded half are kept (layer skip: the packed rows are the kept images'
pixels, the lists built by ops.mask_to_index).

The legs ALTERNATE round by round in one process.  A round is a window of back-to-back calls between two device events behind a
synchronise, as many calls as fill `--window` seconds (>= 0.5; sized from a warm-up window per leg); the figure is the median over `--rounds`
(>= 9) rounds (a leg whose one window takes more than 5 s -- the VALU kernel at width 232 -- runs 3 rounds: `rounds_per_leg`), and a difference counts only where the two legs' ranges (min to max over the rounds) do not overlap.  Before the timing the
two outputs are compared at the timed size and must agree to 1e-4 max(1, |ref|max) (asserted).  `frac_bf16_roof_executed` = 3 x the
algorithmic FLOP rate (2 rows C 9 gw per call; bf16x3 executes three products per one) over the 2500 TFLOP/s dense bf16 matrix peak, as
bench.py --full computes `frac_executed`.  `--forms` adds the other compiled wave roles (LDN_GROUPED_WIDE_ROWS_FORM = a / b1 / b4:
csrc/ldn_grouped_wide_rows.hip; width 232: a / b1, the forms compiled there) as further alternating legs on the stride-1 shapes.  One JSON line per shape and one per
model step; `--out` also appends them to a file (profiles/grouped_wide_rows.jsonl).
usage: tools/bench_grouped_wide_rows.py [--batch 64] [--train-batch 32] [--rounds 9] [--window 0.5] [--out FILE] [--forms] [--no-kernels]
                                        [--no-models] [--models regnet_y_8gf,regnet_y_16gf,regnet_y_32gf] [--step-model regnet_y_8gf]"""
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
ap.add_argument("--train-batch", type=int, default=32)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--out", default=None)
ap.add_argument("--forms", action="store_true")
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
SLOW_WINDOW_S, SLOW_ROUNDS = 5.0, 3
MAPS = [56, 28, 14, 7]
BF16_MFMA_PEAK_TFLOPS = 2500.0      # bench.py
FORM_ENV = "LDN_GROUPED_WIDE_ROWS_FORM"


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
    for i in range(args.rounds):
        for k, fn in legs.items():
            if i < SLOW_ROUNDS or 1e-3 * ms[k][0] * calls[k] <= SLOW_WINDOW_S:      # a leg whose window takes more than 5 s: 3 rounds
                ms[k].append(window(fn, calls[k]))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v), calls[k], len(v)) for k, v in ms.items()}


def verdict(res, new, old):
    """a difference is real only where the two ranges (min to max of the rounds) do not overlap"""
    return {"old_over_new": round(res[old][0] / res[new][0], 3),
            "new_faster_ranges_apart": bool(res[new][2] < res[old][1]), "new_slower_ranges_apart": bool(res[new][1] > res[old][2])}


def with_form(form, fn):
    def run():
        if form is None:
            os.environ.pop(FORM_ENV, None)
        else:
            os.environ[FORM_ENV] = form
        fn()
    return run


if not args.no_kernels:
    for model in (args.models.split(",") if args.models else MODELS):
        gw, widths = MODELS[model]
        for stride in (1, 2):
            for stage, (C, S) in enumerate(zip(widths, MAPS)):
                B = args.batch
                keep = seeded_bernoulli((B, 1, 1), 0.5, 7 + stage)
                ix = ops.mask_to_index(keep.to(dev), S, S, stride)
                n3 = int(ix.cnt[0].item())
                h_a = torch.relu(seeded_randn((ix.cap1, C), 11 + C)).to(dev)
                w = (seeded_randn((C, 9, gw), 12 + C) * (2.0 / (9 * gw)) ** 0.5).to(dev)
                g = torch.Generator().manual_seed(13 + C)
                scale, shift = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
                frag = ops.pack_grouped_wide_weights(w, gw)
                out_new, out_old = torch.zeros(ix.cap3, C, device=dev), torch.zeros(ix.cap3, C, device=dev)
                new = lambda: ops.grouped_wide_conv3x3_rows(h_a, ix.nbr, frag, gw, scale, shift, out_new, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)
                legs = {"mfma": with_form(None, new),
                        "valu": lambda: ops.grouped_conv3x3_rows(h_a, ix.nbr, w, gw, scale, shift, out_old, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)}
                forms = (("a", "b1") if gw == 232 else ("a", "b1", "b4")) if args.forms and stride == 1 else ()
                for form in forms:
                    legs["form_" + form] = with_form(form, new)
                legs["valu"]()
                ref_max = out_old[:n3].abs().max().item()
                diffs = {}
                for k, fn in legs.items():
                    if k != "valu":
                        out_new.zero_()
                        fn()
                        torch.cuda.synchronize()
                        diffs[k] = (out_new[:n3] - out_old[:n3]).abs().max().item()
                        assert diffs[k] <= 1e-4 * max(1.0, ref_max), f"{model} stage {stage + 1} {k}: differs from the VALU kernel by {diffs[k]:.3e} (|ref|max {ref_max:.3e})"
                res = alternate(legs, warm=3)
                os.environ.pop(FORM_ENV, None)
                tflops = 2.0 * n3 * C * 9 * gw / (res["mfma"][0] * 1e-3) / 1e12
                rec = {"what": "LAD-RegNet conv b (grouped 3x3 + BN + ReLU) over the packed rows of the kept images: ops.grouped_wide_conv3x3_rows (bf16x3, "
                               "matrix cores) vs ops.grouped_conv3x3_rows (fp32 VALU, the switch-off path)",
                       "model": model, "stage": stage + 1, "stride": stride, "group_width": gw, "C": C, "map": S, "batch": B, "rows": n3, "rounds": args.rounds,
                       "mfma_us_median": round(1e3 * res["mfma"][0], 2), "valu_us_median": round(1e3 * res["valu"][0], 2),
                       "mfma_us_min_max": [round(1e3 * res["mfma"][1], 2), round(1e3 * res["mfma"][2], 2)],
                       "valu_us_min_max": [round(1e3 * res["valu"][1], 2), round(1e3 * res["valu"][2], 2)],
                       "calls_per_window": {k: v[3] for k, v in res.items()}, "rounds_per_leg": {k: v[4] for k, v in res.items()},
                       **verdict(res, "mfma", "valu"), "algorithmic_tflops_mfma": round(tflops, 2), "frac_bf16_roof_executed": round(3 * tflops / BF16_MFMA_PEAK_TFLOPS, 4),
                       "max_abs_diff": float(f"{diffs['mfma']:.3g}"), "ref_max": float(f"{ref_max:.3g}")}
                for form in forms:
                    r = res["form_" + form]
                    rec["form_" + form + "_us_median_min_max"] = [round(1e3 * r[0], 2), round(1e3 * r[1], 2), round(1e3 * r[2], 2)]
                emit(rec)

if not args.no_models:
    from laudnet_amd.training import prepare_for_training, train_forward
    model, gw = args.step_model, MODELS[args.step_model][0]

    def build(batch):
        net = getattr(laudnet_amd, "lad_" + model)(dyn_mode=["spatial"] * 4, mask_spatial_granularity=MAPS, num_classes=1000, input_size=224).eval()
        net.load_state_dict(damp_residual_branches(fill_state_dict(net.state_dict(), 1)))
        net = net.to(dev)
        for i, blk in enumerate(net.blocks()):      # layer skip: one decision per image, a seeded half kept in every block
            blk.f.forced_spatial_mask = seeded_bernoulli((batch, 1, 1, 1), 0.5, 100 + i).to(dev)
        return net, seeded_randn((batch, 3, 224, 224), 1000).to(dev).contiguous(memory_format=torch.channels_last)

    def ab(step, what, batch, key):
        before = laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS
        try:
            y_on, y_off = step(True).detach().clone(), step(False).detach().clone()
            diff, ref_max = (y_on - y_off).abs().max().item(), y_off.abs().max().item()
            res = alternate({"on": lambda: step(True), "off": lambda: step(False)}, warm=2)
        finally:
            laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS = before
        emit({"what": what, "model": model, "group_width": gw, "batch": batch, "rounds": args.rounds,
              "on_ms_median": round(res["on"][0], 3), "off_ms_median": round(res["off"][0], 3),
              "on_ms_min_max": [round(res["on"][1], 3), round(res["on"][2], 3)], "off_ms_min_max": [round(res["off"][1], 3), round(res["off"][2], 3)],
              "calls_per_window": {k: v[3] for k, v in res.items()}, "rounds_per_leg": {k: v[4] for k, v in res.items()}, **verdict(res, "on", "off"),
              key + "_max_abs_diff": float(f"{diff:.3g}"), key + "_ref_max": float(f"{ref_max:.3g}")})

    net, x = build(args.batch)

    def eval_step(on):
        laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS = on
        with torch.no_grad():
            return net(x, 1.0)[0]
    ab(eval_step, "layer-skip eval step (a seeded half of the images kept in every block, bf16x3) with laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS on vs off",
       args.batch, "logits")
    del net, x
    torch.cuda.empty_cache()

    net, x = build(args.train_batch)
    prepare_for_training(net)
    gout = seeded_randn((args.train_batch, 1000), 1001).to(dev)

    def train_step(on):
        laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS = on
        for p_ in net.parameters():
            p_.grad = None
        out = train_forward(net, x, 1.0)
        ((out[0] * gout).sum() / 10.0).backward()
        return out[0]
    ab(train_step, "training step = forward + backward of every parameter (layer skip, a seeded half of the images kept in every block, frozen BatchNorm "
                   "statistics, bf16x3; conv b's weight gradient on the gather + PyTorch path either way) with laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS on vs off",
       args.train_batch, "logits")
