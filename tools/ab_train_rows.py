#!/usr/bin/env python3
"""Bit-identity of the training row kernels under two builds of the library (a refactor of csrc/ldn_train_rows.hip / ldn_train_bn.hip /
ldn_rows_plan.h must move no bit: no formula and no order of a sum changes).

    python tools/ab_train_rows.py LIB_A LIB_B

Runs the GPU tests of the four op-level suites (their inputs are seeded on the CPU) once per library, each in a fresh child process with
LDN_LIB_PATH = that library, and records every output of every ops.rows_* call they make: du, the g_* vectors and slot sums, mean / var / invstd,
h, and d_gamma / d_beta / xhat / the accumulated dx of the LayerNorm backward.  Then compares call by call, tensor by tensor, on the BITS
(torch.equal of the int32 views: a NaN or a -0 cannot hide a difference).  Prints one JSON line; exit status 0 only if both suites passed and
every tensor is equal."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITES = ["tests/test_hip_train_rows.py", "tests/test_hip_rows_postmask.py", "tests/test_hip_rows_bn.py", "tests/test_hip_ln_bwd.py"]
OPS = ["rows_chanmask", "rows_act_bwd", "rows_postmask_bwd", "rows_img_dot", "rows_bn_stats", "rows_bn_fwd", "rows_bn_bwd", "rows_ln_bwd"]
CHILD_TIMEOUT_S = 420


def record(path):
    """child: the suites under pytest, every ops.rows_* wrapped"""
    sys.path.insert(0, ROOT)
    import pytest
    import torch
    from laudnet_amd import ops
    calls = []

    def wrap(name, fn):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            outs = list(out) if isinstance(out, tuple) else [out]
            if name == "rows_ln_bwd":
                # xhat is written below the count only (the rest is whatever the allocator held); dx, the accumulated argument, is an output too
                n = kw.get("count")
                n = int(n.item()) if n is not None else None
                outs = outs[:2] + [outs[2][:n] if outs[2] is not None else None, a[4]]
            torch.cuda.synchronize()
            test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
            calls.append((f"{test} {name}", [None if t is None else t.detach().contiguous().cpu().clone() for t in outs]))
            return out
        return wrapped

    for name in OPS:
        setattr(ops, name, wrap(name, getattr(ops, name)))
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider"] + [os.path.join(ROOT, s) for s in SUITES])
    torch.save(calls, path)
    return int(rc)


def main(lib_a, lib_b):
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, lib in (("a", lib_a), ("b", lib_b)):
            path = os.path.join(tmp, tag + ".pt")
            env = dict(os.environ, LDN_LIB_PATH=os.path.abspath(lib))
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--record", path], env=env, cwd=ROOT, timeout=CHILD_TIMEOUT_S).returncode
            if rc != 0:          # a failed or faulted child: nothing more is started on the GPU
                print(json.dumps({"tool": "ab_train_rows", "equal": False, "error": f"the suites ended with status {rc} under {lib}"}))
                return 1
            import torch
            runs.append(torch.load(path))
    import torch
    a, b = runs
    differ, tensors = [], 0
    if [k for k, _ in a] != [k for k, _ in b]:
        differ.append("the two runs made different calls")
    else:
        for (key, ta), (_, tb) in zip(a, b):
            for i, (x, y) in enumerate(zip(ta, tb)):
                if x is None and y is None:
                    continue
                tensors += 1
                if x is None or y is None or x.shape != y.shape or x.dtype != y.dtype or not torch.equal(x.view(torch.int32), y.view(torch.int32)):
                    differ.append(f"{key} output {i}")
    per_op = {name: sum(1 for k, _ in a if k.endswith(" " + name)) for name in OPS}
    print(json.dumps({"tool": "ab_train_rows", "lib_a": lib_a, "lib_b": lib_b, "calls": len(a), "calls_per_op": per_op, "tensors": tensors,
                      "differing": len(differ), "first_differing": differ[:8], "equal": not differ and tensors > 0}))
    return 0 if not differ and tensors > 0 else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        sys.exit(record(sys.argv[2]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
