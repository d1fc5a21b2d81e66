#!/usr/bin/env python3
"""ops.grouped_wide_conv3x3_image (LAD-RegNet conv b of channel / both mode on the matrix cores at group widths 56, 112 and 232, bf16x3,
k_grouped_wide<56 | 112 | 232>) beside ops.grouped_conv3x3_image (k_grouped3x3_chan, the fp32 VALU kernel that runs while
laud_regnet.USE_GROUPED_MFMA_WIDE is off), then a whole channel-mode eval step of lad_regnet_y_8gf (`--only step`) or lad_regnet_y_32gf (`--only step32`) with the switch on and off under the same
forced masks.  This comparison -- the switch being the only difference -- is what decides a later flip of the default.

Shapes: conv b (folded BatchNorm, ReLU) of the four stages of RegNetY-8GF (group width 56, w_b 224 / 448 / 896 / 2016) and RegNetY-16GF (112,
224 / 448 / 1232 / 3024; `--only regnet_y_32gf`: 232, w_b 232 / 696 / 1392 / 3712, which the driver leaves out) on 56^2 / 28^2 / 14^2 / 7^2 output maps at stride 1, and each stage's stride-2 first-block shape (input map twice
the output map), `--batch` images.  Every image keeps each channel GRANULE with probability 0.5 (seeded), at granularity 1 and at
granularity = group width -- the second is where whole groups drop, which is the only way a mask saves the matrix-core form any work.

The protocol is that of tools/bench_grouped_chan_mfma.py: the two legs ALTERNATE round by round in one process; a round is a window of
back-to-back calls between two device events behind a synchronise, as many calls as fill `--window` seconds (>= 0.5); the figure is the median
over `--rounds` (>= 9) rounds and the spread of a leg is its max - min over the rounds.  Before the timing the two outputs are compared at the
timed size and must agree to 1e-4 max(1, |ref|max) (asserted).  The VALU leg can be slow at these widths, so the size of a window comes from
a warm-up that starts with ONE call and grows only while a call is short.  Every record carries the FLOPs the matrix cores execute (3 x 2 x
pixels x padded out channels x padded K per active (image, group) pair) and their fraction of the 2.5 PFLOP/s bf16 matrix roof.

Without `--only` this is a driver: every step is a child process under its own time limit, and the driver stops at the first step that
fails or runs into its limit.  The first child (`--only probe`) times one warm-up window of each leg at every shape; the limit of a model's
child is derived from that: twice (rounds x both windows + the warm-ups + a second per shape to build its inputs), plus a minute.
usage: tools/bench_grouped_wide.py [--batch 64] [--rounds 9] [--window 0.5] [--out FILE]
                                   [--only probe|regnet_y_8gf|regnet_y_16gf|regnet_y_32gf|step|step32]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"regnet_y_8gf": (56, [224, 448, 896, 2016]), "regnet_y_16gf": (112, [224, 448, 1232, 3024]), "regnet_y_32gf": (232, [232, 696, 1392, 3712])}
DRIVEN = ("regnet_y_8gf", "regnet_y_16gf")     # the models of the driver and its probe; the 32GF shapes run by name (--only regnet_y_32gf, step32)
SLOW_WINDOW_S, SLOW_ROUNDS = 5.0, 3            # a leg whose one window takes longer (the VALU kernel at width 232) runs 3 rounds
MAPS = [56, 28, 14, 7]
PAD = {56: (64, 512), 112: (128, 1008), 232: (256, 2096)}        # padded out channels, padded K of a group
ROOF = 2.5e15                                  # bf16 matrix FLOP/s of one MI355X
PROBE_LIMIT, STEP_CHILD_LIMIT = 420, 420       # seconds: the probe child, the eval-step child

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--out", default=None)
ap.add_argument("--only", default=None, choices=["probe", "step", "step32"] + sorted(MODELS))
args = ap.parse_args()
assert args.rounds >= 9, "the median of at least 9 rounds"
assert args.window >= 0.5, "windows of at least half a second"

if args.only is None:
    def child(step, limit, capture=False):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", step, "--batch", str(args.batch), "--rounds", str(args.rounds),
               "--window", str(args.window)] + (["--out", args.out] if args.out and not capture else [])
        try:
            p = subprocess.run(cmd, timeout=limit, stdout=subprocess.PIPE if capture else None, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"{step}: ran into its time limit of {limit} s -- nothing more is started")
        if p.returncode != 0:
            sys.exit(f"{step}: exit status {p.returncode} -- nothing more is started")
        return p.stdout

    probe = [json.loads(l[6:]) for l in child("probe", PROBE_LIMIT, capture=True).splitlines() if l.startswith("PROBE ")]
    for model in DRIVEN:
        need = 0.0
        for r in (r for r in probe if r["model"] == model):
            need += 1.0 + sum(r["warmup_s"].values()) + args.rounds * sum(max(args.window, 1e-3 * ms) for ms in r["ms_per_call"].values())
        limit = int(60 + 2 * need)
        print(f"[driver] {model}: {need:.0f} s expected from the probe's warm-up windows, limit {limit} s", flush=True)
        child(model, limit)
    child("step", STEP_CHILD_LIMIT)
    sys.exit(0)

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import time  # noqa: E402

import torch  # noqa: E402

import laudnet_amd  # noqa: E402
from fill import damp_residual_branches, fill_state_dict, seeded_bernoulli, seeded_randn  # noqa: E402
from laudnet_amd import laud_regnet, ops  # noqa: E402

dev = torch.device("cuda", 0)
laudnet_amd.load_library()
ops.set_math_mode("bf16x3")


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


def warm_up(fn):
    """-> (milliseconds per call, calls that fill a window, seconds the warm-up took): one call first, then a window of at most ten calls and
    at most a fifth of a second, so a slow leg is not run ten times just to be sized"""
    t0 = time.time()
    one = window(fn, 1)
    ms = window(fn, max(1, min(10, int(200.0 / max(one, 1e-3)))))
    return ms, max(1, int(args.window * 1e3 / ms) + 1), time.time() - t0


def alternate(legs):
    """-> {leg: (median, min, max, calls per window)} in milliseconds per call; the legs alternate round by round"""
    calls = {k: warm_up(fn)[1] for k, fn in legs.items()}
    ms = {k: [] for k in legs}
    for i in range(args.rounds):
        for k, fn in legs.items():
            if i < SLOW_ROUNDS or 1e-3 * ms[k][0] * calls[k] <= SLOW_WINDOW_S:
                ms[k].append(window(fn, calls[k]))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v), calls[k], len(v)) for k, v in ms.items()}


def verdict(res, new, old):
    spread = max(res[new][2] - res[new][1], res[old][2] - res[old][1])
    return {"old_over_new": round(res[old][0] / res[new][0], 3),
            "new_faster_beyond_spread": bool(res[old][0] - res[new][0] > spread), "new_slower_beyond_spread": bool(res[new][0] - res[old][0] > spread)}


def problems(model):
    """every (stage, stride, granularity) of the model -> its operands and the two legs"""
    gw, widths = MODELS[model]
    B = args.batch
    lib = laudnet_amd._lib.load()
    for stage, (C, S) in enumerate(zip(widths, MAPS)):
        for stride in (1, 2):
            Hi = S * stride
            h_a = torch.relu(seeded_randn((B, Hi, Hi, C), 11 + C + stride)).to(dev)
            w = (seeded_randn((C, 9, gw), 12 + C) * (2.0 / (9 * gw)) ** 0.5).to(dev)
            g = torch.Generator().manual_seed(13 + C)
            scale, shift = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
            frag = ops.pack_grouped_wide_weights(w, gw)
            plan = {"bands": lib.ldn_grouped_wide_bands(C, gw, Hi, Hi, S, stride), "strips": lib.ldn_grouped_wide_strips(C, gw, Hi, Hi, stride),
                    "images": lib.ldn_grouped_wide_images(C, gw, Hi, Hi, stride)}
            assert ops.grouped_wide_ok(C, gw, Hi, Hi, stride) and plan["bands"] >= 1
            for gran in (1, gw):
                gm = seeded_bernoulli((B, C // gran), 0.5, 17 + C + gran + stage)
                _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, C // gran, gran, mask_in=gm.to(dev))
                chan = gm.repeat_interleave(gran, dim=1) > 0.5
                pairs = int((chan.view(B, C // gw, gw).sum(dim=2) > 0).sum())              # active (image, group) pairs
                out_new, out_old = torch.zeros(B, S, S, C, device=dev), torch.zeros(B, S, S, C, device=dev)
                legs = {"mfma": lambda: ops.grouped_wide_conv3x3_image(h_a, frag, gw, idx, cnt, scale, shift, out_new, stride=stride, relu=1),
                        "valu": lambda: ops.grouped_conv3x3_image(h_a, w, gw, idx, cnt, scale, shift, out_old, stride=stride, relu=1)}
                head = {"model": model, "stage": stage + 1, "group_width": gw, "C": C, "map_out": S, "stride": stride, "batch": B, "granularity": gran,
                        "keep_probability": 0.5, "kept_channels": round(float(chan.float().mean()), 4),
                        "active_groups": round(pairs / (B * (C // gw)), 4), **plan}
                yield head, legs, (out_new, out_old), 6.0 * S * S * PAD[gw][0] * PAD[gw][1] * pairs
            del h_a


def probe():
    for model in DRIVEN:
        for head, legs, _, _ in problems(model):
            wu = {k: warm_up(fn) for k, fn in legs.items()}
            print("PROBE " + json.dumps({"model": model, "stage": head["stage"], "stride": head["stride"], "granularity": head["granularity"],
                                         "ms_per_call": {k: v[0] for k, v in wu.items()}, "warmup_s": {k: v[2] for k, v in wu.items()}}), flush=True)


def shapes(model):
    for head, legs, (out_new, out_old), flops in problems(model):
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        diff, ref_max = (out_new - out_old).abs().max().item(), out_old.abs().max().item()
        assert diff <= 1e-4 * max(1.0, ref_max), f"{model} stage {head['stage']}: the two kernels differ by {diff:.3e} (|ref|max {ref_max:.3e})"
        res = alternate(legs)
        emit({"what": "LAD-RegNet conv b (grouped 3x3 + BN + ReLU) on per-image channel subsets: ops.grouped_wide_conv3x3_image (bf16x3, matrix "
                      "cores) vs ops.grouped_conv3x3_image (fp32 VALU)", **head, "rounds": args.rounds,
              "mfma_us_median": round(1e3 * res["mfma"][0], 2), "valu_us_median": round(1e3 * res["valu"][0], 2),
              "mfma_us_min_max": [round(1e3 * res["mfma"][1], 2), round(1e3 * res["mfma"][2], 2)],
              "valu_us_min_max": [round(1e3 * res["valu"][1], 2), round(1e3 * res["valu"][2], 2)],
              "calls_per_window": {k: v[3] for k, v in res.items()}, "rounds_per_leg": {k: v[4] for k, v in res.items()}, **verdict(res, "mfma", "valu"),
              "executed_gflop": round(flops / 1e9, 3), "executed_tflops": round(flops / (res["mfma"][0] * 1e-3) / 1e12, 1),
              "fraction_of_bf16_matrix_roof": round(flops / (res["mfma"][0] * 1e-3) / ROOF, 4),
              "max_abs_diff": float(f"{diff:.3g}"), "ref_max": float(f"{ref_max:.3g}")})


def steps(model="regnet_y_8gf"):
    gw = MODELS[model][0]
    for gran in (1, gw):
        net = getattr(laudnet_amd, "lad_" + model)(dyn_mode=["channel"] * 4, channel_dyn_granularity=[gran] * 4, channel_masker=["MLP"] * 4,
                                           channel_masker_layers=[2] * 4, num_classes=1000, input_size=224).eval()
        net.load_state_dict(damp_residual_branches(fill_state_dict(net.state_dict(), 1)))
        net = net.to(dev)
        for i, blk in enumerate(net.blocks()):      # the same forced masks in both legs: every channel granule kept with probability 0.5
            blk.f.forced_channel_mask = seeded_bernoulli((args.batch, blk.f.masker_channel.channel_dyn_group), 0.5, 100 + i).to(dev)
        x = seeded_randn((args.batch, 3, 224, 224), 1000).to(dev).contiguous(memory_format=torch.channels_last)
        calls = []
        real = ops.grouped_wide_conv3x3_image

        def counted(*a, **k):
            calls.append(1)
            return real(*a, **k)

        def step(on):
            laud_regnet.USE_GROUPED_MFMA_WIDE = on
            with torch.no_grad():
                return net(x, 1.0)[0]
        before = laud_regnet.USE_GROUPED_MFMA_WIDE
        try:
            ops.grouped_wide_conv3x3_image = counted
            y_on = step(True)
            n_on = len(calls)
            y_off = step(False)
            assert n_on == len(net.blocks()) and len(calls) == n_on, "the switch must move every block's conv b, and only with it on"
            ops.grouped_wide_conv3x3_image = real
            diff, ref_max = (y_on - y_off).abs().max().item(), y_off.abs().max().item()
            res = alternate({"on": lambda: step(True), "off": lambda: step(False)})
        finally:
            ops.grouped_wide_conv3x3_image = real
            laud_regnet.USE_GROUPED_MFMA_WIDE = before
        emit({"what": f"channel-mode eval step of lad_{model} (forced masks, every granule kept with probability 0.5, bf16x3) with "
                      "laud_regnet.USE_GROUPED_MFMA_WIDE on vs off",
              "model": model, "group_width": gw, "batch": args.batch, "granularity": gran, "rounds": args.rounds,
              "on_ms_median": round(res["on"][0], 3), "off_ms_median": round(res["off"][0], 3),
              "on_ms_min_max": [round(res["on"][1], 3), round(res["on"][2], 3)], "off_ms_min_max": [round(res["off"][1], 3), round(res["off"][2], 3)],
              "calls_per_window": {k: v[3] for k, v in res.items()}, "rounds_per_leg": {k: v[4] for k, v in res.items()}, **verdict(res, "on", "off"),
              "logits_max_abs_diff": float(f"{diff:.3g}"), "logits_ref_max": float(f"{ref_max:.3g}")})
        del net


if args.only == "probe":
    probe()
elif args.only == "step":
    steps()
elif args.only == "step32":
    steps("regnet_y_32gf")
else:
    shapes(args.only)
