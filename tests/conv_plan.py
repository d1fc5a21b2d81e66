"""What a launch of ldn_conv_packed or ldn_conv_image runs, asked of the library's own chooser: conv_plan() of
laudnet_amd/csrc/ldn_conv_plan.h through tests/conv_plan_cli.cpp, compiled once per session with the host compiler.  tests/test_hip_packed.py
and tests/test_hip_conv_image.py prove from it, on the CPU, that their case tables run every instantiation a launch can reach.  No GPU."""
from __future__ import annotations

import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("B", "rows_per_image", "taps", "cin", "cout", "has_k", "has_n", "kgran", "shift_classes", "residual", "scale", "out_split", "stream_rows")
DEFAULTS = dict(B=1, out_split=False, stream_rows=512)      # (the kernel does not depend on B; LDN_STREAM_ROWS at its default)


def host_compiler():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cxx in (shutil.which("c++"), shutil.which("g++"), os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang++"),
                "/opt/rocm/llvm/bin/clang++"):
        if cxx and os.path.exists(cxx):
            return cxx
    raise AssertionError("no host C++ compiler: neither c++ nor the clang++ that hipcc ships")


@functools.lru_cache(maxsize=None)
def cli():
    """The path of conv_plan_cli, compiled on first use."""
    tmp = tempfile.mkdtemp(prefix="conv_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "conv_plan_cli")
    subprocess.run([host_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(HERE, "conv_plan_cli.cpp"), "-o", exe], check=True)
    return exe


def shape_line(packed, math, **kw):
    """A launch as the CLI reads it; a value may be a list (for a line of the "grid" form)."""
    kw = dict(DEFAULTS, **kw)
    text = lambda v: ",".join(str(int(x)) for x in v) if isinstance(v, (list, tuple)) else str(int(v))
    return " ".join(["packed" if packed else "image", math] + [text(kw[f]) for f in FIELDS])


def run(lines):
    """The CLI's answer to each line."""
    out = subprocess.run([cli()], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return out


_KERNEL = re.compile(r"(k_conv_image|k_conv_bf3|k_conv1x1_stream)<(?:(\d+),(\d+),(?:(\d+),)?)?(B_\w+)>$")


def parse_kernel(name):
    """"k_conv_bf3<4,4,2,B_KN4>" -> ("k_conv_bf3", 4, 4, "B_KN4", 2): (kernel, MS, NS, BMODE, WM); MS / NS / WM are None where the kernel has none."""
    m = _KERNEL.match(name)
    assert m, name
    num = lambda g: int(g) if g is not None else None
    return (m.group(1), num(m.group(2)), num(m.group(3)), m.group(5), num(m.group(4)))


_plans = {}


def plans(launches):
    """[(kernel, MS, NS, BMODE, WM)] for launches given as keyword dicts (those of expected_variant), through ONE run of the CLI."""
    keys = [shape_line(**kw) for kw in launches]
    todo = sorted(set(keys) - set(_plans))
    if todo:
        for line, got in zip(todo, run(todo)):
            rest = got[len(line):].split()
            assert got.startswith(line) and "UNBUILT" not in rest, got
            _plans[line] = parse_kernel(rest[0])
    return [_plans[k] for k in keys]


def expected_variant(**kw):
    """(kernel, MS, NS, BMODE) a conv launch runs.  rows_per_image: m_cap of a packed launch, Ho * Wo of an image launch; taps: 1 or 9;
    has_k / has_n: input / output channel list; math: "fp32" | "bf16x3"; out_split: out_format 1 of ldn_conv_image."""
    return plans([kw])[0][:4]


def expected_wave_rows(**kw):
    """WM of k_conv_bf3, the rows of its consumer wave grid (None for the other kernels)."""
    return plans([kw])[0][4]


def reachable(grid_lines):
    """{(kernel, MS, NS, BMODE, WM)} over lines of the "grid" form (shape_line with lists), refused shapes left out."""
    found = set()
    for got in run(["grid " + ln for ln in grid_lines]):
        assert "UNBUILT" not in got, got
        found |= {parse_kernel(name) for name in got.split()}
    return found
