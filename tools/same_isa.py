#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 device code?  No GPU needed.

    tools/same_isa.py OLD [NEW] [-D NAME[=VALUE] ...] [-j N] [--rename REGEX=REPL ...]

OLD and NEW are directories or git revisions (a revision is exported to a temporary directory); NEW defaults to the working tree.
Every entry of build.SOURCES is compiled device-only with build.FLAGS (+ the -D flags) from both trees, the gfx950 code object is
unbundled, and two things are compared per translation unit: the disassembly (`llvm-objdump -d`, without its file-name line) and
the kernel metadata note (`llvm-readelf --notes`: VGPR / SGPR counts, LDS bytes, scratch, kernarg layout).  The raw objects are
NOT the criterion: hipcc derives a per-compilation id from the source text.  One line per unit; exit status 1 on any difference.

A unit whose text differs is compared again kernel by kernel (by_symbol): instantiating the same templates in another order, or fewer
of them, moves every kernel in the code object.  Per symbol the instruction text is compared without its address column, and without
the literal of the s_add_u32 behind an s_getpc_b64 (the distance to one of the unit's globals, which moves with the layout); per
kernel, its entry of the metadata note.  "same kernels" counts as identical; kernels added, removed or changed are named and do not.

--rename REGEX=REPL (re.sub on OLD's symbols) pairs kernels whose NAME changed on purpose, e.g. a template that gained an argument.  A renamed
kernel is compared by its instruction text and by the resource fields of its metadata entry (registers, LDS, scratch, workgroup size); its
name, symbol and kernel-argument entries are expected to differ and are not compared.  A unit whose only differences are such pairs with the
same text and resources counts as identical and lists them.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "laudnet_amd"))      # build.py alone: importing the package would load torch and the library
import build  # noqa: E402

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def tree_of(spec: str, tmp: str) -> str:
    """A directory as it is; a git revision exported under tmp."""
    if os.path.isdir(spec):
        return os.path.abspath(spec)
    out = os.path.join(tmp, "src_" + spec.replace("/", "_"))
    os.makedirs(out)
    tar = subprocess.run(["git", "-C", REPO, "archive", spec, "include", "laudnet_amd/csrc"], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", out], input=tar, check=True)
    return out


def device_code(tree: str, src: str, defs: list, out: str) -> tuple:
    """(disassembly, metadata note) of one translation unit's gfx950 code object."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sp = os.path.join(tree, "laudnet_amd", "csrc", src)
    subprocess.run([hipcc] + build.FLAGS + defs + ["--cuda-device-only", "-c", "-o", out + ".o", sp], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + out + ".o", "--output=" + out + ".co"], check=True)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", out + ".co"], check=True, capture_output=True, text=True).stdout
    note = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", out + ".co"], check=True, capture_output=True, text=True).stdout
    return [ln for ln in dis.splitlines() if "file format" not in ln], note.splitlines()


SYMBOL = re.compile(r"^[0-9a-f]{16} <(.+)>:$")


def by_symbol(dis: list, note: list) -> dict:
    """{symbol: (instruction text, metadata entry)} of one code object, free of everything that only says where a kernel lies."""
    code, sym, pcrel = {}, None, 0
    for ln in dis:
        m = SYMBOL.match(ln)
        if m:
            sym = m.group(1)
            code[sym] = []
        elif sym is not None and ln.strip() not in ("", "..."):      # ("...": the zero fill behind the last kernel of the section)
            text = ln.split("//")[0].strip()
            if pcrel and text.startswith("s_add_u32 "):
                text, pcrel = text.rsplit(",", 1)[0] + ", <pc-relative>", 0
            else:
                pcrel = 2 if text.startswith("s_getpc_b64") else max(pcrel - 1, 0)
            code[sym].append(text)
    meta, entry = {}, None
    for ln in note:      # the entries of amdhsa.kernels: each begins "  - ." and names its kernel in .name
        if ln.startswith("  - ."):
            entry = [ln]
        elif entry is not None and ln.startswith("    "):
            entry.append(ln)
            if ln.startswith("    .name:"):
                meta[ln.split(":", 1)[1].strip()] = entry
        else:
            entry = None
    return {k: (code[k], meta.get(k)) for k in code}


RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
             ".group_segment_fixed_size", ".max_flat_workgroup_size", ".wavefront_size", ".uses_dynamic_stack")


def resources(entry) -> list:
    """the lines of a kernel's metadata entry that say what it uses, not what it is called or how its arguments are laid out"""
    return sorted(ln.strip() for ln in entry or [] if ln.strip().split(":")[0] in RESOURCES)


def pair_renamed(k0: dict, k1: dict, renames: list) -> list:
    """[(old, new, same)] for OLD's symbols that are gone from NEW and whose renamed form is a symbol only NEW has; both leave k0 / k1"""
    out = []
    for old in sorted(set(k0) - set(k1)):
        new = old
        for rx, repl in renames:
            new = re.sub(rx, repl, new)
        if new != old and new in k1 and new not in k0:
            (c0, m0), (c1, m1) = k0.pop(old), k1.pop(new)
            out.append((old, new, c0 == c1 and resources(m0) == resources(m1)))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new", nargs="?")
    ap.add_argument("-D", dest="defs", action="append", default=[], metavar="NAME[=VALUE]")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    a = ap.parse_args()
    defs = ["-D" + d for d in a.defs]
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max(1, min(a.j, 16))) as pool:
        trees = [tree_of(a.old, tmp), tree_of(a.new, tmp) if a.new else REPO]
        jobs = {(s, i): pool.submit(device_code, t, s, defs, os.path.join(tmp, f"{i}_{s}")) for s in build.SOURCES for i, t in enumerate(trees)}
        print(f"# {a.old} vs {a.new or 'the working tree'}, flags: {' '.join(build.FLAGS + defs)}")
        bad = 0
        for s in build.SOURCES:
            (d0, n0), (d1, n1) = jobs[s, 0].result(), jobs[s, 1].result()
            same = d0 == d1 and n0 == n1
            what, names = "identical", []
            if not same:
                k0, k1 = by_symbol(d0, n0), by_symbol(d1, n1)
                renamed = pair_renamed(k0, k1, renames)
                removed, added = sorted(set(k0) - set(k1)), sorted(set(k1) - set(k0))
                kept = sorted(k for k in set(k0) & set(k1) if k0[k] == k1[k]) + [f"{o} -> {n}" for o, n, ok in renamed if ok]
                changed = sorted(k for k in set(k0) & set(k1) if k0[k] != k1[k]) + [f"{o} -> {n}" for o, n, ok in renamed if not ok]
                same = not (removed or added or changed)
                what = (f"same kernels ({len(kept)})" if same else
                        f"DIFFERENT: {len(removed)} removed, {len(added)} added, {len(changed)} changed, {len(kept)} same")
                names = [f"    {w} {k}" for w, ks in (("removed", removed), ("added", added), ("changed", changed)) for k in ks]
                names += [f"    renamed, same text and resources: {o} -> {n}" for o, n, ok in renamed if ok]
            bad += not same
            print(f"{s:24s} {what:24s} {len(d1)} disassembly lines, {len(n1)} metadata lines", flush=True)
            for ln in names:
                print(ln, flush=True)
        print(f"# {len(build.SOURCES) - bad} of {len(build.SOURCES)} translation units identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
