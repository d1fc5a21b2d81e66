#!/usr/bin/env python3
"""Records what tests/test_hip_attn_bwd.py, tests/test_hip_attn_bwd_long.py, tests/test_hip_ln_bwd.py, tests/test_hip_adavit_training.py and
tests/test_hip_adavit_training_long.py MEASURE (they only assert):
profiles/train_adavit_grad_err.json = per case and tensor max |err| / max |want64| of the HIP path ("hip") and, beside it, of fp32 PyTorch
autograd of the same float64 reference on the same GPU ("fp32_autograd": the reference alone).  The bound the tests assert is 1e-3.
Needs one MI355X.  usage: tools/train_adavit_grad_err.py [--out profiles/train_adavit_grad_err.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import test_hip_adavit_training as TT  # noqa: E402
import test_hip_adavit_training_long as TTL  # noqa: E402
import test_hip_attn_bwd as TA  # noqa: E402
import test_hip_attn_bwd_long as TAL  # noqa: E402
import test_hip_ln_bwd as TL  # noqa: E402
from attn_bwd_ref import BOUND  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_adavit_grad_err.json"))
    a = ap.parse_args()
    r = lambda d: {k: float(f"{v:.2g}") for k, v in d.items()}
    cases = {}
    for shape in TA.SHAPES:
        cases["packed_mha_bwd B%d L%d heads%d keep%.1f" % shape] = TA.measure(*shape)
    for Lt, counts, heads in TAL.SEAMS:
        cases[f"packed_mha_bwd_long L{Lt} kept{list(counts)} heads{heads}"] = TAL.measure(Lt, counts, heads)
    for C in TL.WIDTHS:
        cases[f"rows_ln_bwd C{C}"] = TL.measure(C)
    for name in TT.CASES:
        cases["train " + name + " B%d L%d dim%d heads%d depth%d" % TT.CASES[name][:5]] = TT.measure(name)
    for name in TTL.CASES:
        cases["train long " + name + " B%d L%d dim%d heads%d depth%d" % TTL.CASES[name][:5]] = TTL.measure(name)
    worst = {"hip": [0.0, ""], "fp32_autograd": [0.0, ""]}
    lines = []
    for name, (hip, ref) in cases.items():
        for leg, d in (("hip", hip), ("fp32_autograd", ref)):
            k = max(d, key=d.get)
            if d[k] > worst[leg][0]:
                worst[leg] = [float(f"{d[k]:.2g}"), f"{name}: {k}"]
        lines.append(f'"{name}": ' + json.dumps({"hip": r(hip), "fp32_autograd": r(ref)}, separators=(",", ":")))
        print(name, f"hip {max(hip.values()):.2e}  fp32 autograd {max(ref.values()):.2e}", flush=True)
    with open(a.out, "w") as f:
        f.write('{\n"bound": %g,\n"worst": %s,\n"cases": {\n%s\n}\n}\n' % (BOUND, json.dumps(worst), ",\n".join(lines)))
    print("worst", worst)


if __name__ == "__main__":
    main()
