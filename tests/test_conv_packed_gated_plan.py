"""The plan of ldn_conv_packed_gated (conv_plan_packed_gated / LDN_CONV_GATED_KERNELS of laudnet_amd/csrc/ldn_conv_plan.h) on the CPU, through
tests/conv_packed_gated_plan_cli.cpp compiled with the host compiler.  No GPU.

The sweep is also the record of which admitted packed shape reaches which row of the gated list: reach() is what
tests/test_hip_both_se_fused.py takes its one-shape-per-row cases from, and refused() where it takes its plan beyond the LDS from."""
import atexit
import functools
import itertools
import os
import shutil
import subprocess
import tempfile

import conv_plan as P
import test_conv_gated_plan as GP

HERE = os.path.dirname(os.path.abspath(__file__))
M_CAP = (1, 49, 100, 196, 784, 3136)
CIN = (8, 48, 104, 120, 336, 888, 2016, 3712)
COUT = (32, 64, 128, 160, 320, 444, 888)
# Beside the sweep: input widths at which the plan outgrows the 160 KiB of a CU.  The largest plan is 14 subtiles of staging (114 688 B) + the
# column tables + (2 ms + ns + 2 ms) * 32 * 4 B of row tables + 8 B a channel (list + gate): it passes 163 840 B between cin 5248 and 5280 for
# the 8 x 6 tile, so cin 3712 of the sweep still fits everywhere and these two do not.
CIN_BEYOND = (5280, 8192)
GATED_ROWS = GP.GATED_ROWS
LDS_LIMIT = 160 * 1024


@functools.lru_cache(maxsize=None)
def cli():
    tmp = tempfile.mkdtemp(prefix="conv_packed_gated_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "conv_packed_gated_plan_cli")
    subprocess.run([P.host_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(HERE, "conv_packed_gated_plan_cli.cpp"), "-o", exe], check=True)
    return exe


def plan(shapes):
    """[(B, m_cap, cin, cout, residual, scale)] -> [dict(ok, shape_ok, kernel, built, bn, ntn, bm, mtn, grid, lds, lds_ungated, weight)]"""
    text = "".join(" ".join(str(int(v)) for v in s) + "\n" for s in shapes)
    out = subprocess.run([cli()], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(shapes)
    res = []
    for s, ln in zip(shapes, out):
        f = ln.split()
        assert tuple(map(int, f[:6])) == tuple(int(v) for v in s)
        res.append(dict(ok=int(f[6]), shape_ok=int(f[7]), kernel=f[8], built=int(f[9]), bn=int(f[10]), ntn=int(f[11]), bm=int(f[12]), mtn=int(f[13]),
                        grid=int(f[14]), lds=int(f[15]), lds_ungated=int(f[16]), weight=int(f[17])))
    return res


def entry_refuses(p):
    """what ldn_conv_packed_gated checks by shape before it launches (launch_conv_packed_gated, launch_conv_kernel)"""
    return not p["shape_ok"] or p["weight"] >= 1 << 31 or not p["built"] or p["lds"] > LDS_LIMIT


def sweep_shapes(B=64, cins=CIN):
    return [(B, rows, cin, cout, res, 1) for rows, cin, cout, res in itertools.product(M_CAP, cins, COUT, (0, 1))]


@functools.lru_cache(maxsize=None)
def _swept():
    shapes = sweep_shapes() + sweep_shapes(B=1) + sweep_shapes(cins=CIN_BEYOND)
    return list(zip(shapes, plan(shapes)))


def reach(B=64):
    """{row of the gated list: [admitted packed shapes of the sweep, at this B, that run it]}"""
    out = {}
    for s, p in _swept():
        if p["ok"] and s[0] == B and s[2] in CIN:
            out.setdefault(p["kernel"], []).append(s)
    return out


def refused():
    """the refused shapes of the sweep and of CIN_BEYOND, with their plans"""
    return [(s, p) for s, p in _swept() if not p["ok"]]


def test_the_lists_are_what_they_were():
    lines = subprocess.run([cli(), "lists"], capture_output=True, text=True, check=True).stdout.splitlines()
    n_all, n_gated = map(int, lines[0].split())
    assert n_all == 16 + 22 + 2 and n_gated == 6 and lines[1:] == GATED_ROWS


def test_every_admitted_shape_runs_a_gated_row_and_every_refused_one_is_refused_by_the_entry():
    seen = {}
    n_ok = n_refused = 0
    image = GP.plan([s for s, _ in _swept()])                 # the image form's plan of the same numbers
    for (s, p), img in zip(_swept(), image):
        B, rows, cin, cout, res, scale = s
        assert p["ok"] == (0 if entry_refuses(p) else 1), (s, p)                              # the query and the entry point agree
        if not p["ok"]:
            n_refused += 1
            continue
        n_ok += 1
        assert p["built"] == 1 and p["kernel"] in GATED_ROWS, (s, p)
        seen.setdefault(p["kernel"], s)
        ms, ns = (int(v) for v in p["kernel"].split("<")[1].split(",")[:2])
        assert p["bn"] % 32 == 0 and 0 < p["bn"] <= ns * 32 and p["bm"] % 32 == 0 and 0 < p["bm"] <= ms * 32, (s, p)
        assert p["ntn"] * p["bn"] >= cout and p["mtn"] * p["bm"] >= rows, (s, p)
        assert p["grid"] == (B * p["mtn"] + 7) // 8 * 8 * p["ntn"] < 1 << 31, (s, p)
        assert p["lds"] == p["lds_ungated"] + (cin + 31) // 32 * 32 * 4 <= LDS_LIMIT, (s, p)     # the gate vector is counted
        # the packed tables (the rows' out row and one A row per row) are in the ungated plan: the gate lies behind them
        assert p["lds_ungated"] == img["lds_ungated"] + ms * 32 * 2 * 4, (s, p)
    print(f"packed gated sweep: {n_ok} admitted, {n_refused} refused; rows reached: {sorted(seen.items())}")
    assert set(seen) == set(GATED_ROWS), f"never reached by a packed shape: {set(GATED_ROWS) - set(seen)}"
    # every shape of the sweep proper is admitted (the LDS bound is first passed beyond its largest cin) ...
    assert all(p["ok"] for s, p in _swept() if s[2] in CIN)
    # ... and CIN_BEYOND holds plans that only the LDS refuses, the gate vector being what pushes some of them over
    over = [(s, p) for s, p in refused() if p["shape_ok"] and p["built"] and p["lds"] > LDS_LIMIT]
    assert over and any(p["lds_ungated"] <= LDS_LIMIT for _, p in over)


def test_reach_is_the_same_at_both_batch_sizes():
    assert set(reach(64)) == set(reach(1)) == set(GATED_ROWS)


def test_refused_by_shape():
    got = plan([(64, 49, 100, 320, 1, 1), (64, 49, 104, 322, 1, 1), (0, 49, 104, 320, 1, 1), (64, 0, 104, 320, 1, 1), (64, 49, 8192, 320, 1, 1)])
    assert [p["ok"] for p in got] == [0] * 5 and all(entry_refuses(p) for p in got)
    assert [p["shape_ok"] for p in got] == [0, 0, 0, 0, 1]
