#!/usr/bin/env python3
"""ops.grouped_mfma_conv3x3_images (LAD-RegNet conv b at group widths 8 and 24 over whole kept images staged in LDS; bf16x3) beside the two forms
those widths run on today -- ops.grouped_mfma_conv3x3_rows (matrix cores, neighbour table; LDN_GROUPED_MFMA_WIDTHS=1) and ops.grouped_conv3x3_rows
(fp32 VALU; the default) -- then b -> SE -> c of a layer-skip block fused into three launches against today's six-launch path, then a whole
layer-skip eval step of each model with both switches off, LDN_GROUPED_MFMA_WIDTHS only, and both on.  The input to a later flip of either default.

Shapes: conv b (folded BatchNorm, ReLU) of every stage of RegNetY-400MF (group width 8, w_b 48 / 104 / 208 / 440) and RegNetY-1.6GF (group width 24,
w_b 48 / 120 / 336 / 888): the stride-1 blocks on 56^2 / 28^2 / 14^2 / 7^2 maps and each stage's stride-2 first block from 112^2 / 56^2 / 28^2 / 14^2;
`--batch` images of which a seeded half are kept.

The legs ALTERNATE round by round in one process.  A round is a window of back-to-back calls between two device events behind a synchronise, as many
calls as fill `--window` seconds (>= 0.5; sized from a warm-up window per leg); the figure is the median over `--rounds` (>= 9) rounds with [min,
max].  Before the timing the legs' outputs are compared at the timed size: the image form must equal the row form bit for bit and agree with the
VALU kernel to 1e-4 max(1, |ref|max); the fused block must agree with the unfused one to 1e-5 max(1, |ref|max) (asserted).  One JSON line per
shape, per block and per model; `--out` also appends them to a file (profiles/grouped_mfma_images.jsonl).
usage: tools/bench_grouped_mfma_images.py [--batch 64] [--rounds 9] [--window 0.5] [--out FILE] [--no-kernels] [--no-blocks] [--no-models]"""
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
ap.add_argument("--no-kernels", action="store_true")
ap.add_argument("--no-blocks", action="store_true")
ap.add_argument("--no-models", action="store_true")
args = ap.parse_args()
assert args.rounds >= 9, "the median of at least 9 rounds"
assert args.window >= 0.5, "windows of at least half a second"
dev = torch.device("cuda", 0)
laudnet_amd.load_library()
ops.set_math_mode("bf16x3")
MODELS = {"regnet_y_400mf": ("lad_regnet_y_400mf", 8, [48, 104, 208, 440]), "regnet_y_1_6gf": ("lad_regnet_y_1_6gf", 24, [48, 120, 336, 888])}
MAPS = [56, 28, 14, 7]
STEM = 32


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


def figures(res, unit):
    """median and [min, max] per leg (unit 'us' or 'ms'), and for every other leg its median over the FIRST leg's with the beyond-spread verdicts"""
    mul, nd = (1e3, 2) if unit == "us" else (1.0, 3)
    rec = {"calls_per_window": {k: v[3] for k, v in res.items()}}
    for k, v in res.items():
        rec[f"{k}_{unit}_median"] = round(mul * v[0], nd)
        rec[f"{k}_{unit}_min_max"] = [round(mul * v[1], nd), round(mul * v[2], nd)]
    new = next(iter(res))
    for k, v in res.items():
        if k != new:
            spread = max(res[new][2] - res[new][1], v[2] - v[1])
            rec[f"{k}_over_{new}"] = round(v[0] / res[new][0], 3)
            rec[f"{new}_slower_than_{k}_beyond_spread"] = bool(res[new][0] - v[0] > spread)
            rec[f"{new}_faster_than_{k}_beyond_spread"] = bool(v[0] - res[new][0] > spread)
    return rec


def shapes():
    """(model, gw, stage, C, Ho, stride): the stride-2 first block of a stage, then its stride-1 blocks"""
    for model, (arch, gw, widths) in MODELS.items():
        for stage, (C, S) in enumerate(zip(widths, MAPS)):
            for stride in (2, 1):
                yield model, gw, stage, C, S, stride


if not args.no_kernels:
    for model, gw, stage, C, S, stride in shapes():
        B, Hi = args.batch, S * stride
        keep = seeded_bernoulli((B, 1, 1), 0.5, 7 + stage)
        ix = ops.mask_to_index(keep.to(dev), S, S, stride)
        n3, n1 = int(ix.cnt[0].item()), int(ix.cnt[1].item())
        h_a = torch.relu(seeded_randn((ix.cap1, C), 11 + C)).to(dev)
        w = (seeded_randn((C, 9, gw), 12 + C) * (2.0 / (9 * gw)) ** 0.5).to(dev)
        g = torch.Generator().manual_seed(13 + C)
        scale, shift = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
        frag = ops.pack_grouped_mfma_weights(w, gw)
        images = (B, Hi, Hi, S, S, stride)
        assert ops.grouped_mfma_images_fit(Hi, Hi, C, gw) > 0
        out = {k: torch.zeros(ix.cap3, C, device=dev) for k in ("images", "rows", "valu")}
        legs = {"images": lambda: ops.grouped_mfma_conv3x3_images(h_a, frag, gw, scale, shift, out["images"], m_count=ix.cnt[0:1], images=images, relu=1),
                "rows": lambda: ops.grouped_mfma_conv3x3_rows(h_a, ix.nbr, frag, gw, scale, shift, out["rows"], m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1),
                "valu": lambda: ops.grouped_conv3x3_rows(h_a, ix.nbr, w, gw, scale, shift, out["valu"], m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        assert torch.equal(out["images"], out["rows"]), f"{model} stage {stage + 1} stride {stride}: the image form and the row form differ"
        diff, ref_max = (out["images"][:n3] - out["valu"][:n3]).abs().max().item(), out["valu"][:n3].abs().max().item()
        assert diff <= 1e-4 * max(1.0, ref_max), f"{model} stage {stage + 1} stride {stride}: differs from the VALU kernel by {diff:.3e} (|ref|max {ref_max:.3e})"
        res = alternate(legs)
        nbytes = (n1 + n3) * C * 4                  # the kept images' input rows once in, their output rows once out
        emit({"what": "LAD-RegNet conv b (grouped 3x3 + BN + ReLU) over whole kept images: ops.grouped_mfma_conv3x3_images (LDS-staged, matrix cores) vs "
                      "ops.grouped_mfma_conv3x3_rows (neighbour table, matrix cores) vs ops.grouped_conv3x3_rows (fp32 VALU)", "level": "kernel",
              "model": model, "stage": stage + 1, "group_width": gw, "C": C, "map_out": S, "stride": stride, "batch": B, "rows": n3, "rounds": args.rounds,
              "bands": ops.grouped_mfma_images_bands(Hi, Hi, S, stride, C, gw), "groups_per_workgroup": ops.grouped_mfma_images_fit(Hi, Hi, C, gw),
              **figures(res, "us"), "rows_in_out_GBps_images": round(nbytes / (res["images"][0] * 1e-3) / 1e9, 1),
              "images_equals_rows_bitwise": True, "max_abs_diff_vs_valu": float(f"{diff:.3g}"), "ref_max": float(f"{ref_max:.3g}")})

if not args.no_blocks:
    # b -> SE -> c of a layer-skip block on the kept images: conv b with the SE squeeze as a by-product, the SE head, conv c with the gate on its input
    # rows (3 launches) against the row form, se_packed (channel sums, head, in-place rescale) and the plain conv c
    for model, gw, stage, C, S, stride in shapes():
        B, Hi = args.batch, S * stride
        keep = seeded_bernoulli((B, 1, 1), 0.5, 7 + stage)
        ix = ops.mask_to_index(keep.to(dev), S, S, stride)
        n3 = int(ix.cnt[0].item())
        h_a = torch.relu(seeded_randn((ix.cap1, C), 11 + C)).to(dev)
        w = (seeded_randn((C, 9, gw), 12 + C) * (2.0 / (9 * gw)) ** 0.5).to(dev)
        g = torch.Generator().manual_seed(13 + C)
        scale, shift = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
        sc_c, sh_c = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
        frag = ops.pack_grouped_mfma_weights(w, gw)
        Sq = max(8, ((STEM if stage == 0 else MODELS[model][2][stage - 1]) if stride == 2 else C) // 4)      # se_ratio 0.25 of the block's input width
        w1, b1 = (seeded_randn((Sq, C), 21 + C) * (1.0 / C) ** 0.5).to(dev), (seeded_randn((Sq,), 22) * 0.1).to(dev)
        w2, b2 = (seeded_randn((C, Sq), 23 + C) * (1.0 / Sq) ** 0.5).to(dev), (seeded_randn((C,), 24) * 0.1).to(dev)
        wc = (seeded_randn((C, 1, C), 25 + C) * (2.0 / C) ** 0.5).to(dev)
        images = (B, Hi, Hi, S, S, stride)
        if not ops.conv_rows_gated_fits(C, S * S):
            emit({"level": "block", "model": model, "stage": stage + 1, "stride": stride, "skipped": "conv_rows_gated_fits refuses the shape"})
            continue
        h_b = {k: torch.zeros(ix.cap3, C, device=dev) for k in ("fused", "unfused")}
        y = {k: torch.zeros(ix.cap3, C, device=dev) for k in ("fused", "unfused")}

        def fused():
            gap = ops.grouped_mfma_conv3x3_images_gap(h_a, frag, gw, scale, shift, h_b["fused"], m_count=ix.cnt[0:1], images=images, relu=1)
            gate = ops.se_gate_slots(gap, ix.cnt[0:1], S * S, w1, b1, w2, b2)
            ops.conv_rows_gated(h_b["fused"], wc, sc_c, sh_c, y["fused"], gate, S * S, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)

        def unfused():
            ops.grouped_mfma_conv3x3_rows(h_a, ix.nbr, frag, gw, scale, shift, h_b["unfused"], m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)
            ops.se_packed(h_b["unfused"], ix.pre3, w1, b1, w2, b2, S * S)
            ops.conv_rows(h_b["unfused"], wc, sc_c, sh_c, y["unfused"], taps=1, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)
        legs = {"fused": fused, "unfused": unfused}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        diff, ref_max = (y["fused"][:n3] - y["unfused"][:n3]).abs().max().item(), y["unfused"][:n3].abs().max().item()
        assert diff <= 1e-5 * max(1.0, ref_max), f"{model} stage {stage + 1} stride {stride}: fused and unfused differ by {diff:.3e} (|ref|max {ref_max:.3e})"
        res = alternate(legs)
        emit({"what": "b -> SE -> c of a layer-skip block over the kept images: grouped_mfma_conv3x3_images_gap + se_gate_slots + conv_rows_gated (3 launches) vs "
                      "grouped_mfma_conv3x3_rows + se_packed + conv_rows", "level": "block",
              "model": model, "stage": stage + 1, "group_width": gw, "C": C, "map_out": S, "stride": stride, "batch": B, "rows": n3, "rounds": args.rounds,
              **figures(res, "us"), "max_abs_diff": float(f"{diff:.3g}"), "ref_max": float(f"{ref_max:.3g}")})

if not args.no_models:
    SETTINGS = {"both_on": (True, True), "widths_only": (True, False), "both_off": (False, False)}
    for model, (arch, gw, widths) in MODELS.items():
        net = getattr(laudnet_amd, arch)(dyn_mode=["spatial"] * 4, mask_spatial_granularity=MAPS, num_classes=1000, input_size=224).eval()
        net.load_state_dict(damp_residual_branches(fill_state_dict(net.state_dict(), 1)))
        net = net.to(dev)
        for i, blk in enumerate(net.blocks()):      # layer skip: one decision per image, a seeded half kept in every block
            blk.f.forced_spatial_mask = seeded_bernoulli((args.batch, 1, 1, 1), 0.5, 100 + i)
        x = seeded_randn((args.batch, 3, 224, 224), 1000).to(dev).contiguous(memory_format=torch.channels_last)

        def step(setting):
            laud_regnet.USE_GROUPED_MFMA_WIDTHS, laud_regnet.USE_GROUPED_MFMA_WIDTHS_IMAGES = SETTINGS[setting]
            with torch.no_grad():
                return net(x, 1.0)[0]
        before = laud_regnet.USE_GROUPED_MFMA_WIDTHS, laud_regnet.USE_GROUPED_MFMA_WIDTHS_IMAGES
        try:
            ys = {k: step(k).clone() for k in SETTINGS}
            ref_max = ys["both_off"].abs().max().item()
            diffs = {k: (ys[k] - ys["both_off"]).abs().max().item() for k in ("both_on", "widths_only")}
            res = alternate({k: (lambda k=k: step(k)) for k in SETTINGS})
        finally:
            laud_regnet.USE_GROUPED_MFMA_WIDTHS, laud_regnet.USE_GROUPED_MFMA_WIDTHS_IMAGES = before
        emit({"what": "layer-skip eval step (a seeded half of the images kept in every block, bf16x3): LDN_GROUPED_MFMA_WIDTHS and LDN_GROUPED_MFMA_WIDTHS_IMAGES "
                      "both on / the first only / both off", "level": "model", "model": model, "group_width": gw, "batch": args.batch, "rounds": args.rounds,
              **figures(res, "ms"), "logits_max_abs_diff_vs_both_off": {k: float(f"{v:.3g}") for k, v in diffs.items()}, "logits_ref_max": float(f"{ref_max:.3g}")})
