#!/usr/bin/env python3
"""Records what tests/test_hip_training_f64.py and the whole-model relative check of tests/test_hip_training*.py MEASURE (they only assert):
profiles/train_parity_f64.json (one line per case / model: the tensor names once, then one column per quantity) =
  "blocks": per case of tests/train_ref.py -- its input map, rows, the achieved tie-free clearance |z| / E(bf16x3) under train_ref's refined bound and,
            beside it, under the unrefined formula ("clearance_unrefined": not asserted, below 4 for most cases), the largest bias move -- and per
            tensor max |err| / max |want64| of the HIP path in both arithmetic modes ("fp32", "bf16x3") and of the SAME restatement in float32 on the
            CPU ("float32_cpu": the reference alone);
  "worst":  the worst ratio per arithmetic mode over all cases and tensors (and the float32 restatement's);
  "models": per whole-model case each parameter gradient's scale, its eligibility for the scale-relative check (the oracle's CPU step against its
            GPU step, <= 2.5e-4 of the scale; a string of 0 / 1), and the HIP path's relative error -- columns in the sorted order of the names of the model's
            parameters that have a non-zero oracle gradient; the tensors that are not eligible are named.
The whole-model figures are what the tests themselves computed: this tool calls those test functions and reads test_hip_training.RELATIVE_RECORDS,
which they fill as they run (deliberately coupled to the tests: the record is of exactly what they assert on).
--bn-scales LABEL measures the BatchNorm scale variants instead (train_ref.VARIANT_CASES, tests/test_hip_training_bn_scales.py: zero, +-2^-24 and
negated weights) and merges the figures under LABEL into profiles/train_parity_bn_scales.json: per case, variant and arithmetic mode every tensor's
max |err| / max |want64| (max |got| itself where want64 is identically zero: only 0 passes), NaN / Inf reported as the string "nan".  The file
holds two labels: "parent" = the tree before d scale stopped being a division by the scale (training.py of the commit before; the tests were
run against it once to record what they catch) and "fixed".
Needs one MI355X.  usage: tools/train_parity_f64.py [--out profiles/train_parity_f64.json] [--no-models] | --bn-scales LABEL [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import test_hip_training as T  # noqa: E402
import test_hip_training_both as TB  # noqa: E402
import test_hip_training_f64 as T64  # noqa: E402
import test_hip_training_regnet as TRG  # noqa: E402
import train_ref as R  # noqa: E402
from laudnet_amd import ops  # noqa: E402


def _r(v):
    return None if v is None else float(f"{v:.2g}")


def write_compact(path, blocks, worst, models):
    """one line per case / model, one column of figures (two significant digits) per quantity: a block's tensor names once, a model's tensors in
    the order of its named_parameters() with only the non-eligible ones named"""
    dump = lambda v: json.dumps(v, separators=(",", ":"))
    lines = ['{', f'"bound": 0.001,', f'"worst": {dump({k: [_r(v[0]), v[1]] for k, v in worst.items()})},', '"blocks": {']
    rows = []
    for name, rec in blocks.items():
        names = list(rec["fp32"])
        col = {m: [_r(rec[m].get(k)) for k in names] for m in ("fp32", "bf16x3", "float32_cpu")}
        rows.append(f'"{name}": ' + dump({"input_map": rec["input_map"], "rows": rec["rows"], "clearance": rec["clearance"], "clearance_unrefined": rec["clearance_unrefined"],
                                          "largest_bias_move": rec["largest_bias_move"], "tensors": names, **col}))
    lines += [",\n".join(rows), '},', '"models": {']
    rows = []
    for name, rec in models.items():      # columns in the SORTED order of the names of the model's parameters with a non-zero oracle gradient
        names = sorted(rec)
        rows.append(f'"{name}": ' + dump({"tensors": len(names), "scale": [_r(rec[k]["scale"]) for k in names],
                                          "rel_err": [_r(rec[k]["rel_err"]) for k in names],
                                          "eligible": "".join(str(int(rec[k]["eligible"])) for k in names),
                                          "not_eligible": {k: {"oracle_cpu_vs_gpu": _r(rec[k]["oracle_cpu_vs_gpu"]), "scale": _r(rec[k]["scale"])}
                                                           for k in names if not rec[k]["eligible"]}}))
    lines += [",\n".join(rows), '}', '}']
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def bn_scales(label, path):
    """the 22 variant cases under both arithmetic modes -> `path`, merged under `label`: one line per case / variant / mode"""
    import math
    doc = {"bound": 0.001, "what": "max |err| / max |want64| per tensor; max |got| where want64 is identically zero", "labels": {}}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    fig = lambda v: None if v is None else ("nan" if not math.isfinite(v) else _r(v))
    rows, worst, failing = {}, [0.0, ""], 0
    for name, variant in R.VARIANT_CASES:
        for mode in ("fp32", "bf16x3"):
            ops.set_math_mode(mode)
            try:
                res = T64.measure(name, variant)
            finally:
                ops.set_math_mode("fp32")
            _, want, _ = R.reference(name, variant=variant)
            bad = sorted(k for k, v in res.items() if v is None or not math.isfinite(v) or (v > 1e-3 if k == "forward" or want[k].abs().max().item() > 0 else v != 0))
            rows[f"{name}/{variant}/{mode}"] = {"tensors": list(res), "ratio": [fig(v) for v in res.values()], "over_bound": bad}
            failing += bool(bad)
            for k, v in res.items():
                if v is not None and (not math.isfinite(v) or v > worst[0]):
                    worst = [v if math.isfinite(v) else float("inf"), f"{name}/{variant}/{mode}: {k}"]
            print(name, variant, mode, "over the bound:", bad, flush=True)
    doc["labels"][label] = {"worst": [fig(worst[0]) if math.isfinite(worst[0]) else "nan", worst[1]], "cases_over_bound": failing, "cases": rows}
    dump = lambda v: json.dumps(v, separators=(",", ":"))
    lines = ["{", f'"bound": {dump(doc["bound"])},', f'"what": {dump(doc["what"])},', '"labels": {']
    blocks = []
    for lab, rec in doc["labels"].items():
        body = ",\n".join(f'"{k}": {dump(v)}' for k, v in rec["cases"].items())
        blocks.append(f'"{lab}": {{"worst": {dump(rec["worst"])}, "cases_over_bound": {rec["cases_over_bound"]}, "cases": {{\n{body}\n}}}}')
    lines += [",\n".join(blocks), "}", "}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(label, "worst", worst, "cases over the bound:", failing, "of", len(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-models", action="store_true")
    ap.add_argument("--bn-scales", metavar="LABEL", default=None)
    a = ap.parse_args()
    if a.bn_scales is not None:
        return bn_scales(a.bn_scales, a.out or os.path.join(ROOT, "profiles", "train_parity_bn_scales.json"))
    a.out = a.out or os.path.join(ROOT, "profiles", "train_parity_f64.json")
    blocks, worst = {}, {"fp32": [0.0, ""], "bf16x3": [0.0, ""], "float32_cpu": [0.0, ""]}
    for name in R.CASES:
        case = R.tie_free_case(name)
        _, want, _ = R.reference(name)
        _, got32, _ = R.reference(name, torch.float32)
        rec = {"input_map": R._MAPS[name][0], "rows": R.BATCH * R._MAPS[name][0] ** 2, "clearance": round(case.clearance, 2),
               "clearance_unrefined": round(R.clearance(case.params, case.x, case.masks, gated=False), 2),
               "largest_bias_move": round(case.moved, 4), "float32_cpu": {k: R.worst_ratio(got32[k], w) for k, w in want.items()}}
        for mode in ("fp32", "bf16x3"):
            ops.set_math_mode(mode)
            try:
                rec[mode] = T64.measure(name)
            finally:
                ops.set_math_mode("fp32")
        for mode in worst:
            for k, v in rec[mode].items():
                if v is not None and v > worst[mode][0]:
                    worst[mode] = [v, f"{name}: {k}"]
        blocks[name] = rec
        print(name, {m: f"{max(v for v in rec[m].values() if v is not None):.2e}" for m in worst}, flush=True)
    if not a.no_models:
        for case in ("channel_r50", "layer_r50"):
            T.test_detection_backbone_train_step_vs_oracle(case)
        for case in ("r101_channel2222", "r101_layer", "r101_spatial4421"):
            T.test_classifier_train_step_vs_oracle(case)
        for case in ("r50_both", "r50_mixed"):
            TB.test_both_classifier_train_step_vs_oracle(case)
        TRG.test_regnet_train_step_vs_oracle()
    write_compact(a.out, blocks, worst, T.RELATIVE_RECORDS)
    print("worst", worst)


if __name__ == "__main__":
    main()
