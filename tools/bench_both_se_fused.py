#!/usr/bin/env python3
"""The SE block of a LAD-RegNet 'both'-mode bottleneck folded into conv b and the packed conv c (laud_regnet.USE_BOTH_SE_FUSED) beside today's
path, then whole 'both'-mode eval steps of lad_regnet_y_800mf and lad_regnet_y_8gf with the switch on and off under the same forced masks.
The matrix-core conv b and the channel-mode fold's switches are on in both legs: the fold exists only where they route conv b.

Shapes: b -> SE -> c of the four stages of RegNetY-800MF (group width 16, w_b 64 / 144 / 320 / 784), RegNetY-1.6GF (24, 48 / 120 / 336 / 888) and
RegNetY-8GF (56, 224 / 448 / 896 / 2016) on 56^2 / 28^2 / 14^2 / 7^2 output maps: the stride-1 block and the stage's stride-2 first block (input map
twice the output map), `--batch` images; conv c is w_b -> w_b over the packed rows of the active pixels (one mask group) with a scale vector, a
residual (the identity / the projection's output, a buffer of its own here) and ReLU, scattered through the pixel list; the SE squeeze is w_b / 4
wide.  Every image keeps each channel and each pixel with probability 0.5 (forced masks, seeded), granularity 1.
    today   conv b (ops.grouped_chan_mfma_conv3x3_image / ops.grouped_wide_conv3x3_image), ops.se_packed (row sums, head, row scaling over
            every pixel), ops.conv_packed
    folded  conv b's _gap form, ops.se_gate_image, ops.conv_packed_gated

The protocol of tools/bench_channel_se_fused.py: the two legs ALTERNATE round by round in one process; a round is a window of back-to-back
calls between two device events behind a synchronise, as many calls as fill `--window` seconds (>= 0.5; sized from a warm-up window per leg);
the figure is the median over `--rounds` (>= 9) rounds and the spread of a leg is its max - min over the rounds.  Before the timing the two
outputs are compared at the timed size and must agree to 1e-5 max(1, |ref|max) (asserted).  One JSON line per shape and one per model step;
`--out` also appends them to a file (profiles/both_se_fused.jsonl).

Without `--only` this is a driver: every step (one model's shapes, or one eval step) is a child process of its own under its own time
limit, and the driver stops at the first step that fails or runs into its limit.
usage: tools/bench_both_se_fused.py [--batch 64] [--rounds 9] [--window 0.5] [--out FILE]
                                    [--only regnet_y_800mf|regnet_y_1_6gf|regnet_y_8gf|step_800mf|step_8gf]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"regnet_y_800mf": (16, [64, 144, 320, 784]), "regnet_y_1_6gf": (24, [48, 120, 336, 888]), "regnet_y_8gf": (56, [224, 448, 896, 2016])}
MAPS = [56, 28, 14, 7]
STEP_MODELS = {"step_800mf": ("regnet_y_800mf", "lad_regnet_y_800mf", 16), "step_8gf": ("regnet_y_8gf", "lad_regnet_y_8gf", 56)}
STEP_LIMIT = {"regnet_y_800mf": 240, "regnet_y_1_6gf": 240, "regnet_y_8gf": 300, "step_800mf": 180, "step_8gf": 240}     # seconds per child
SWITCHES = ("USE_GROUPED_MFMA_CHANNEL", "USE_GROUPED_MFMA_WIDE", "USE_CHANNEL_SE_FUSED", "USE_CHANNEL_SE_FUSED_WIDE", "USE_BOTH_SE_FUSED")

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--out", default=None)
ap.add_argument("--only", default=None, choices=sorted(STEP_LIMIT))
args = ap.parse_args()
assert args.rounds >= 9, "the median of at least 9 rounds"
assert args.window >= 0.5, "windows of at least half a second"

if args.only is None:
    for step, limit in STEP_LIMIT.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--only", step, "--batch", str(args.batch), "--rounds", str(args.rounds),
               "--window", str(args.window)] + (["--out", args.out] if args.out else [])
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{step}: ran into its time limit of {limit} s -- nothing more is started")
        if rc != 0:
            sys.exit(f"{step}: exit status {rc} -- nothing more is started")
    sys.exit(0)

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
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


def shapes(model):
    gw, widths = MODELS[model]
    wide = gw == 56
    B = args.batch
    conv_b = ops.grouped_wide_conv3x3_image if wide else ops.grouped_chan_mfma_conv3x3_image
    conv_b_gap = ops.grouped_wide_conv3x3_image_gap if wide else ops.grouped_chan_mfma_conv3x3_image_gap
    for stage, (C, S) in enumerate(zip(widths, MAPS)):
        for stride in (1, 2):
            Hi = S * stride
            g = torch.Generator().manual_seed(13 + C)
            affine = lambda n: ((torch.rand(n, generator=g) + 0.5).to(dev), (torch.randn(n, generator=g) * 0.1).to(dev))
            h_a = torch.relu(seeded_randn((B, Hi, Hi, C), 11 + C + stride)).to(dev)
            w = (seeded_randn((C, 9, gw), 12 + C) * (2.0 / (9 * gw)) ** 0.5).to(dev)
            sb, tb = affine(C)
            frag = ops.pack_grouped_wide_weights(w, gw) if wide else ops.pack_grouped16_weights(w) if gw == 16 else ops.pack_grouped_mfma_weights(w, gw)
            Sq = C // 4
            se = [(seeded_randn((Sq, C), 21) * (1.0 / C) ** 0.5).to(dev), (seeded_randn((Sq,), 22) * 0.1).to(dev),
                  (seeded_randn((C, Sq), 23) * (1.0 / Sq) ** 0.5).to(dev), (seeded_randn((C,), 24) * 0.1).to(dev)]
            wc = (seeded_randn((1, C, C), 25 + C) * (2.0 / C) ** 0.5).to(dev)                        # k-major
            sc, tc = affine(C)
            resid = torch.relu(seeded_randn((B * S * S, C), 26 + C)).to(dev)
            prefix = (torch.arange(B + 1, device=dev, dtype=torch.int32) * (S * S)).contiguous()
            if wide:
                splits = ops.grouped_wide_splits(C, gw, Hi, Hi, S, stride)
                assert ops.grouped_wide_gap_ok(C, gw, Hi, Hi, stride)
            else:
                splits = ops.grouped_chan_mfma_bands(C, gw, Hi, Hi, S, stride)
                assert ops.grouped_chan_mfma_gap_ok(C, gw, Hi, Hi, stride)
            assert ops.conv_packed_gated_ok(B, S * S, C, C, True, True)
            gm = seeded_bernoulli((B, C), 0.5, 17 + C + stage)
            _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, C, 1, mask_in=gm.to(dev))
            pm = seeded_bernoulli((B, S, S), 0.5, 19 + C + stage)
            ix = ops.mask_to_index(pm.to(dev).contiguous(), S, S, stride)
            h_new, h_old = torch.zeros(B, S, S, C, device=dev), torch.zeros(B, S, S, C, device=dev)
            out_new, out_old = torch.zeros(B * S * S, C, device=dev), torch.zeros(B * S * S, C, device=dev)
            gap = torch.empty(B, splits, C, device=dev)
            rows = dict(B=B, row_prefix=ix.pre3, m_cap=S * S, a_map=ix.idx3, out_map=ix.idx3, k_idx=idx, k_cnt=cnt, kgran=1, relu=1, residual2d=resid)

            def today():
                conv_b(h_a, frag, gw, idx, cnt, sb, tb, h_old, stride=stride, relu=1)
                ops.se_packed(h_old.view(B * S * S, C), prefix, *se, S * S, ch_idx=idx, ch_cnt=cnt)
                ops.conv_packed(h_old.view(B * S * S, C), wc, sc, tc, out_old, taps=1, **rows)

            def folded():
                conv_b_gap(h_a, frag, gw, idx, cnt, sb, tb, h_new, stride=stride, relu=1, gap=gap)
                gate = ops.se_gate_image(gap, S * S, *se, idx, cnt)
                ops.conv_packed_gated(h_new.view(B * S * S, C), wc, sc, tc, out_new, gate, **rows)
            legs = {"folded": folded, "today": today}
            for fn in legs.values():
                fn()
            torch.cuda.synchronize()
            diff, ref_max = (out_new - out_old).abs().max().item(), out_old.abs().max().item()
            assert diff <= 1e-5 * max(1.0, ref_max), f"{model} stage {stage + 1}: the two paths differ by {diff:.3e} (|ref|max {ref_max:.3e})"
            res = alternate(legs)
            emit({"what": "LAD-RegNet 'both' mode, conv b -> SE -> packed conv c (one mask group): the SE block folded into its neighbours (three "
                          "launches, no pass over h_b) vs today's path (ops.se_packed over every pixel, ops.conv_packed); conv b on the matrix cores in "
                          "both legs",
                  "model": model, "stage": stage + 1, "group_width": gw, "C": C, "map_out": S, "stride": stride, "batch": B, "granularity": 1,
                  "keep_probability": 0.5, "kept_channels": round(float(gm.mean()), 4), "kept_pixels": round(float(pm.mean()), 4), "splits": splits,
                  "rounds": args.rounds,
                  "folded_us_median": round(1e3 * res["folded"][0], 2), "today_us_median": round(1e3 * res["today"][0], 2),
                  "folded_us_min_max": [round(1e3 * res["folded"][1], 2), round(1e3 * res["folded"][2], 2)],
                  "today_us_min_max": [round(1e3 * res["today"][1], 2), round(1e3 * res["today"][2], 2)],
                  "calls_per_window": {k: v[3] for k, v in res.items()}, **verdict(res, "folded", "today"),
                  "max_abs_diff": float(f"{diff:.3g}"), "ref_max": float(f"{ref_max:.3g}")})
            del h_a, resid, h_new, h_old, out_new, out_old


def step_of(which):
    name, factory, gw = STEP_MODELS[which]
    before = [getattr(laud_regnet, n) for n in SWITCHES]
    net = getattr(laudnet_amd, factory)(dyn_mode=["both"] * 4, mask_spatial_granularity=[1] * 4, channel_dyn_granularity=[1] * 4,
                                        channel_masker=["MLP"] * 4, channel_masker_layers=[2] * 4, num_classes=1000, input_size=224).eval()
    net.load_state_dict(damp_residual_branches(fill_state_dict(net.state_dict(), 1)))
    net = net.to(dev)
    for i, blk in enumerate(net.blocks()):      # the same forced masks in both legs: every channel and every pixel kept with probability 0.5
        ms = blk.f.masker_spatial
        assert ms.mask_channel_group == 1
        blk.f.forced_channel_mask = seeded_bernoulli((args.batch, blk.f.masker_channel.channel_dyn_group), 0.5, 100 + i).to(dev)
        blk.f.forced_spatial_mask = seeded_bernoulli((args.batch, 1, ms.mask_size, ms.mask_size), 0.5, 300 + i).to(dev)
    x = seeded_randn((args.batch, 3, 224, 224), 1000).to(dev).contiguous(memory_format=torch.channels_last)
    calls = []
    real = ops.conv_packed_gated

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    def step(on):
        laud_regnet.USE_BOTH_SE_FUSED = on
        with torch.no_grad():
            return net(x, 1.0)[0]
    try:
        for n in SWITCHES[:-1]:
            setattr(laud_regnet, n, True)
        ops.conv_packed_gated = counted
        y_on = step(True)
        n_on = len(calls)
        y_off = step(False)
        assert n_on == len(net.blocks()) and len(calls) == n_on, "the switch must move every block, and only when on"
        ops.conv_packed_gated = real
        diff, ref_max = (y_on - y_off).abs().max().item(), y_off.abs().max().item()
        res = alternate({"on": lambda: step(True), "off": lambda: step(False)})
    finally:
        ops.conv_packed_gated = real
        for n, v in zip(SWITCHES, before):
            setattr(laud_regnet, n, v)
    emit({"what": f"'both'-mode eval step of lad_{name} (forced masks, every channel and every pixel kept with probability 0.5, granularity 1, one "
                  "mask group, bf16x3, the matrix-core conv b and the channel-mode fold's switches on) with laud_regnet.USE_BOTH_SE_FUSED on vs off",
          "model": name, "group_width": gw, "batch": args.batch, "granularity": 1, "blocks": len(net.blocks()), "rounds": args.rounds,
          "on_ms_median": round(res["on"][0], 3), "off_ms_median": round(res["off"][0], 3),
          "on_ms_min_max": [round(res["on"][1], 3), round(res["on"][2], 3)], "off_ms_min_max": [round(res["off"][1], 3), round(res["off"][2], 3)],
          "calls_per_window": {k: v[3] for k, v in res.items()}, **verdict(res, "on", "off"),
          "logits_max_abs_diff": float(f"{diff:.3g}"), "logits_ref_max": float(f"{ref_max:.3g}")})


if args.only in STEP_MODELS:
    step_of(args.only)
else:
    shapes(args.only)
