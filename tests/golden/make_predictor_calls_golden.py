#!/usr/bin/env python3
"""Records what the reference's block formulas return to the predictor harness (tools/predict_speedup.py: reproduce_v100) on the
V100 preset: the predictor's constructor arguments and, in call order, every block-latency call (function name, keyword arguments,
latency).  tests/test_predictor.py replays these records in place of the reference, so that the harness is pinned to
tests/golden/predictor_v100.json without the reference being present.  Numbers only.

  python tests/golden/make_predictor_calls_golden.py <reference checkout>/DyNetSimulator
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import predict_speedup as PS  # noqa: E402

PS.REF = os.path.abspath(sys.argv[1])
E, P = PS.load_reference()
FUNCS = ("get_static_block_latency", "get_dynamic_block_latency_spatial", "get_skipping_block_latency", "get_dynamic_block_latency_channel")


class RecordingE:
    def __init__(self, calls):
        for name in FUNCS:
            def rec(predictor, name=name, **kw):
                lat = float(getattr(E, name)(predictor, **kw))
                calls.append({"fn": name, "kw": kw, "latency": lat})
                return lat
            setattr(self, name, rec)


def recording_p(ctor):
    def make(*a, **kw):
        ctor.append({"args": list(a), "kwargs": kw})
        return P(*a, **kw)
    return make


gold = json.load(open(os.path.join(HERE, "predictor_v100.json")))["models"]
out = {"source": "reference DyNetSimulator block formulas called by tools/predict_speedup.py reproduce_v100 (V100 preset)", "models": {}}
for model in ("resnet50", "resnet101", "regnety008"):
    calls, ctor = [], []
    PS.load_reference = lambda: (RecordingE(calls), recording_p(ctor))
    got = PS.reproduce_v100(model)
    for k, v in gold[model].items():
        assert abs(got[k] - v) <= 1e-12 + 1e-9 * v, (model, k, got[k], v)
    out["models"][model] = {"predictor": ctor, "calls": calls}
    print(model, len(calls), "calls")
json.dump(out, open(os.path.join(HERE, "predictor_v100_calls.json"), "w"), indent=0)
