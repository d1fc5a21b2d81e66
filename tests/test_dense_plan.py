"""The k_dense / k_dense2 chooser (laudnet_amd/csrc/ldn_dense_plan.h) on the CPU: tests/dense_plan_cli.cpp, compiled with the host
compiler, runs dense_plan() and the list of built kernels (LDN_DENSE_KERNELS) without HIP.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "golden", "dense_plan_pins.txt")


def _host_compiler():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cxx in (shutil.which("c++"), shutil.which("g++"), os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang++"),
                "/opt/rocm/llvm/bin/clang++"):
        if cxx and os.path.exists(cxx):
            return cxx
    raise AssertionError("no host C++ compiler: neither c++ nor the clang++ that hipcc ships")


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dense_plan") / "dense_plan_cli")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "dense_plan_cli.cpp"), "-o", exe], check=True)
    return exe


def test_every_plan_is_a_built_kernel_and_every_built_kernel_is_chosen(cli):
    """Over the sweep grid (11 input widths x 15 output widths x 7 row counts x counted or not x 5 hints x every form an entry point
    accepts, and the gated form at 4 image sizes): the chooser never names a kernel that is not built -- the launcher would refuse it --
    and the list holds no kernel that the chooser never names."""
    r = subprocess.run([cli, "sweep"], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    unbuilt = [ln for ln in lines if ln.startswith("UNBUILT")]
    assert not unbuilt, f"{len(unbuilt)} plans name a kernel that is not built, e.g. {unbuilt[:3]}"
    rows = dict(ln.rsplit(" ", 1) for ln in lines if ln.startswith("k_dense"))
    assert len(rows) == int(lines[-1].split()[3]) >= 50, f"LDN_DENSE_KERNELS lists a kernel twice: {lines[-1]}"
    dead = [k for k, n in rows.items() if int(n) == 0]
    assert not dead, f"built but never chosen: {dead}"
    assert lines[-1].startswith("cases ") and int(lines[-1].split()[1]) > 150000 and r.returncode == 0, lines[-1:]


def test_chooser_matches_the_pinned_model_shapes(cli):
    """The pin file records the kernel chosen for every shape the shipped models issue; a change of any choice fails here."""
    want = open(PINS).read().splitlines()
    shapes = "\n".join(ln if ln.startswith("#") else ln.rsplit(" ", 1)[0] for ln in want) + "\n"
    got = subprocess.run([cli], input=shapes, capture_output=True, text=True, check=True).stdout.splitlines()
    assert sum(not ln.startswith("#") for ln in want) >= 400
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, f"{len(diff)} pinned choices changed, e.g. {diff[:3]}"


def test_every_built_kernel_is_launched_by_a_gpu_test(cli):
    """golden/dense_plan_gpu_tests.txt maps each kernel of the list to parametrisations of the GPU tests that launch it (fp64 or
    bit-identity checks): the chooser sends every listed shape to the kernel named there, and the map misses no kernel."""
    want = [ln for ln in open(os.path.join(HERE, "golden", "dense_plan_gpu_tests.txt")).read().splitlines() if not ln.startswith("#")]
    shapes = "\n".join(ln.split(" ", 1)[1].rsplit(" ", 1)[0] for ln in want) + "\n"
    got = subprocess.run([cli], input=shapes, capture_output=True, text=True, check=True).stdout.splitlines()
    wrong = [(w, g) for w, g in zip(want, got) if w.split(" ", 1)[1] != g]
    assert len(got) == len(want) and not wrong, f"{len(wrong)} shapes of the map reach another kernel now, e.g. {wrong[:3]}"
    for ln in want:      # the named test exists and is a GPU test module
        mod, fn = ln.split(" ", 1)[0].split("::")
        assert f"def {fn}(" in open(os.path.join(HERE, mod + ".py")).read(), ln
    sweep = subprocess.run([cli, "sweep"], capture_output=True, text=True).stdout.splitlines()
    rows = {ln.rsplit(" ", 1)[0] for ln in sweep if ln.startswith("k_dense")}
    missing = sorted(rows - {ln.rsplit(" ", 1)[1] for ln in want})
    assert not missing, f"no GPU test is recorded for {missing}"
