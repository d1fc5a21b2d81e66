"""The plan of ldn_conv_image_gated (conv_plan_gated / LDN_CONV_GATED_KERNELS of laudnet_amd/csrc/ldn_conv_plan.h) on the CPU, through
tests/conv_gated_plan_cli.cpp compiled with the host compiler.  No GPU.

The sweep is also the record of which admitted shape reaches which row of the gated list: reach() is what tests/test_hip_channel_se_fused.py
takes its one-shape-per-row cases from."""
import atexit
import functools
import itertools
import os
import shutil
import subprocess
import tempfile

import conv_plan as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = (1, 49, 100, 196, 784, 3136)
CIN = (8, 48, 104, 120, 336, 888)
COUT = (32, 64, 128, 160, 320, 888)          # (888 is a multiple of 4 already)
GATED_ROWS = ["k_conv_bf3<6,2,2,B_KN4>", "k_conv_bf3<4,4,4,B_KN4>", "k_conv_bf3<4,4,2,B_KN4>", "k_conv_bf3<8,6,4,B_KN4>", "k_conv_bf3<4,10,2,B_KN4>",
              "k_conv_bf3<2,10,2,B_KN4>"]


@functools.lru_cache(maxsize=None)
def cli():
    tmp = tempfile.mkdtemp(prefix="conv_gated_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "conv_gated_plan_cli")
    subprocess.run([P.host_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(HERE, "conv_gated_plan_cli.cpp"), "-o", exe], check=True)
    return exe


def plan(shapes):
    """[(B, rows, cin, cout, residual, scale)] -> [dict(ok, kernel, built, bn, ntn, bm, mtn, grid, lds, lds_ungated)]"""
    text = "".join(" ".join(str(int(v)) for v in s) + "\n" for s in shapes)
    out = subprocess.run([cli()], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(shapes)
    res = []
    for s, ln in zip(shapes, out):
        f = ln.split()
        assert tuple(map(int, f[:6])) == tuple(int(v) for v in s)
        res.append(dict(ok=int(f[6]), kernel=f[7], built=int(f[8]), bn=int(f[9]), ntn=int(f[10]), bm=int(f[11]), mtn=int(f[12]), grid=int(f[13]),
                        lds=int(f[14]), lds_ungated=int(f[15])))
    return res


def sweep_shapes(B=64):
    return [(B, rows, cin, cout, res, 1) for rows, cin, cout, res in itertools.product(ROWS, CIN, COUT, (0, 1))]


def reach(B=64):
    """{row of the gated list: [admitted shapes of the sweep that run it]}"""
    shapes = sweep_shapes(B)
    out = {}
    for s, p in zip(shapes, plan(shapes)):
        if p["ok"]:
            out.setdefault(p["kernel"], []).append(s)
    return out


def test_the_lists():
    lines = subprocess.run([cli(), "lists"], capture_output=True, text=True, check=True).stdout.splitlines()
    n_all, n_gated = map(int, lines[0].split())
    assert n_all == 16 + 22 + 2, "LDN_CONV_KERNELS is the 40 rows it was"
    assert lines[1:] == GATED_ROWS and n_gated == len(GATED_ROWS) == len(set(GATED_ROWS))


def test_every_admitted_shape_runs_a_gated_row_and_every_row_is_reached():
    shapes = sweep_shapes() + sweep_shapes(B=1)
    plans = plan(shapes)
    seen = set()
    for s, p in zip(shapes, plans):
        B, rows, cin, cout, res, scale = s
        assert p["ok"] == 1 and p["built"] == 1 and p["kernel"] in GATED_ROWS, (s, p)      # every shape of the sweep is admitted
        seen.add(p["kernel"])
        ms, ns = (int(v) for v in p["kernel"].split("<")[1].split(",")[:2])
        assert p["bn"] % 32 == 0 and p["bn"] <= ns * 32 and p["bm"] % 32 == 0 and p["bm"] <= ms * 32, (s, p)
        assert p["ntn"] * p["bn"] >= cout and p["mtn"] * p["bm"] >= rows, (s, p)
        assert p["grid"] == (B * p["mtn"] + 7) // 8 * 8 * p["ntn"] < 1 << 31, (s, p)
        assert p["lds"] == p["lds_ungated"] + (cin + 31) // 32 * 32 * 4 <= 160 * 1024, (s, p)                # the gate vector is counted
    assert seen == set(GATED_ROWS), f"never reached: {set(GATED_ROWS) - seen}"


def test_the_rules_row_by_row():
    """the chooser's tile rules on the gated shapes (an input list, no output list: B_KN4 whatever the granularity; never the streaming kernel)"""
    table = [((64, 3136, 48, 48, 1, 1), "k_conv_bf3<6,2,2,B_KN4>"), ((64, 784, 120, 120, 1, 1), "k_conv_bf3<4,4,2,B_KN4>"),
             ((64, 784, 120, 120, 0, 1), "k_conv_bf3<4,4,4,B_KN4>"), ((64, 196, 336, 336, 1, 1), "k_conv_bf3<4,4,2,B_KN4>"),
             ((64, 196, 320, 384, 1, 0), "k_conv_bf3<4,4,2,B_KN4>"),        # conv_plan() streams this one (cout % 128 == 0, no scale): the gated plan does not
             ((64, 49, 160, 160, 1, 1), "k_conv_bf3<8,6,4,B_KN4>"), ((64, 100, 320, 320, 1, 1), "k_conv_bf3<4,10,2,B_KN4>"),
             ((64, 49, 888, 888, 1, 1), "k_conv_bf3<2,10,2,B_KN4>"), ((64, 64, 8, 224, 1, 1), "k_conv_bf3<2,10,2,B_KN4>"),
             ((64, 65, 8, 224, 1, 1), "k_conv_bf3<4,10,2,B_KN4>")]
    got = plan([s for s, _ in table])
    assert [(p["kernel"], p["ok"]) for p in got] == [(k, 1) for _, k in table]


def test_refused_shapes():
    got = plan([(64, 49, 100, 320, 1, 1), (64, 49, 8192, 320, 1, 1), (64, 49, 104, 322, 1, 1), (0, 49, 104, 320, 1, 1)])
    assert [p["ok"] for p in got] == [0, 0, 0, 0]
    assert got[1]["lds"] > 160 * 1024 >= got[1]["lds_ungated"]          # the gate vector is what pushes this one over
