"""LDN_DEBUG build of k_grouped_chan (csrc/ldn_grouped_chan.hip): the list checks k_grouped3x3_chan has (401-403) under codes of the new
kernel's own -- 411 a channel entry outside [0, C), 412 a list that is not ascending, 413 a count outside [0, C].  A clean call reports no
violation and computes what the release build computes, bit for bit; a corrupted list is counted, never trapped, and stays inside the
tensors (entries outside the workgroup's groups are dropped, the count is clamped).  Runs in a subprocess because the library path is fixed
at import time (as tests/test_hip_debug.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import ctypes, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests/golden")
import torch
from laudnet_amd import _lib, ops
from fill import seeded_bernoulli, seeded_randn
lib = _lib.load()
ops.set_math_mode("bf16x3")
def violations(reset=1):
    c, code = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.ldn_debug_violations(ctypes.byref(c), ctypes.byref(code), reset) == 0
    return c.value, code.value
res = {"initial": violations(), "sums": {}}
B, H = 3, 7
for gw, C in ((8, 40), (16, 64), (24, 72)):
    gm = seeded_bernoulli((B, C // 2), 0.6, 40 + gw)
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, C // 2, 2, mask_in=gm.cuda())
    a = torch.relu(seeded_randn((B, H, H, C), 41 + gw)).cuda()
    w = (seeded_randn((C, 9, gw), 42 + gw) * 0.1).cuda()
    frag = ops.pack_grouped16_weights(w) if gw == 16 else ops.pack_grouped_mfma_weights(w, gw)
    sc, sh = torch.ones(C).cuda(), torch.zeros(C).cuda()
    def run(idx, cnt):
        out = torch.zeros(B, H, H, C).cuda()
        ops.grouped_chan_mfma_conv3x3_image(a, frag, gw, idx, cnt, sc, sh, out)
        torch.cuda.synchronize()
        return out
    res["sums"][str(gw)] = run(idx, cnt).double().abs().sum().item()
    res["clean_%%d" %% gw] = violations()
    n0 = int(cnt[0])
    assert n0 >= 4
    bad = idx.clone(); bad[0, 1], bad[0, 2] = idx[0, 2].item(), idx[0, 1].item()        # not ascending
    run(bad, cnt); res["swapped_%%d" %% gw] = violations()
    bad = idx.clone(); bad[0, n0 - 1] = C + 5                                            # an entry past the channels
    run(bad, cnt); res["range_%%d" %% gw] = violations()
    bad = cnt.clone(); bad[1] = C + 3                                                    # a count past the channels
    run(idx, bad); res["count_%%d" %% gw] = violations()
print("RESULT " + json.dumps(res))
"""


def _run(lib):
    env = dict(os.environ, LDN_LIB_PATH=os.path.join(ROOT, "laudnet_amd", lib))
    p = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_debug_build_audits_the_channel_lists_of_the_matrix_core_kernel():
    assert os.path.exists(os.path.join(ROOT, "laudnet_amd", "libldn_hip_debug.so")), "build it: python -m laudnet_amd.build --debug"
    dbg = _run("libldn_hip_debug.so")
    rel = _run("libldn_hip.so")
    assert rel["clean_8"][0] == -1, "the release build must say that its checks are compiled away"
    assert dbg["sums"] == rel["sums"], "debug and release builds must compute identical results"
    assert dbg["initial"][0] == 0
    for gw in (8, 16, 24):
        assert dbg[f"clean_{gw}"] == [0, 0], f"violations in a clean run at width {gw}: {dbg[f'clean_{gw}']}"
        assert dbg[f"swapped_{gw}"][0] > 0 and dbg[f"swapped_{gw}"][1] == 412, dbg[f"swapped_{gw}"]
        assert dbg[f"range_{gw}"][0] > 0 and dbg[f"range_{gw}"][1] == 411, dbg[f"range_{gw}"]
        assert dbg[f"count_{gw}"][0] > 0 and dbg[f"count_{gw}"][1] in (411, 412, 413), dbg[f"count_{gw}"]
