"""k_head, k_tail (csrc/ldn_tail.hip: head_body, tail_body) and the chained launch (k_chain<NS>, k_chain<NS, F32>, csrc/ldn_chain_ld.h:
k_chain_ld<4|8>) with the per-image channel counts FORCED, against float64.

What a workgroup of these kernels runs is decided by its image's active-channel count Kb, not by the launch: k_head enters a fall-through
switch at nsub = ceil(Kb / 32), stages nw = round_up(max(Kb, 1), 64) / 64 weight DMA instructions per wave and chunk and sizes its ring
(D = 2..4 slots) from them and from the block's pixels; k_tail walks nsub K slices of nine chunks and, at width 256, issues 2 or 4 W2 DMA
instructions per wave (Kp > 128); k_chain_ld packs its W2 / W3 slots densely (Kp / 8 pieces) and takes its ring depths R2 / R3 from Kp, block
after block inside one workgroup.  tests/test_hip_tail.py, tests/test_hip_fused_f32.py and tests/test_hip_ops.py draw their counts (0, all,
Bernoulli(0.62)), tests/test_hip_chain_ops.py lets randomly weighted maskers decide: at width 256 that is nsub 5, nw 3, D 2, n_w2 4 and
little else.

`head_classes`, `tail_class` and `chain_class` restate the kernels' choices in Python with the source lines they come from; a non-GPU test
ties the restated expressions and constants to the source text, `ht_gaps` / `chain_gaps` list what a case table leaves out, and non-GPU
tests prove that the tables below leave nothing out and that the proof notices a removed class.

Per head / tail case and arithmetic mode the GPU test requires: cnt equal to the forced counts; the active columns of h1 within
1e-4 + 1e-4 |ref| per image, the columns up to the next multiple of 32 exactly zero, x untouched; out within 2e-4 + 1e-4 |ref| at every
pixel; colsum summing to the output's sums (atol 1e-2, rtol 1e-5); the in-place residual form bit-identical; the bf16x3 / _f32 form that ran
(dtype spy).  At width 64 the folded-projection pair (bottleneck_head(..., x_split=...) + bottleneck_tail_proj, a bf16x3 form) runs with counts
{2, 30, 32, 34, 62, 64} against the float64 block with the float64 projection added.  Per chained run and mode: masks, counts and lists equal
to the forced ones and to the float64 masker's (the last linear layer is zero, the bias +-4 decides: no margin allowance); the run bit-identical
to masker -> head -> tail block by block; every block within 2e-4 + 1e-4 |ref| of the float64 block started from the kernel's own input;
no hand-off timeout of the loader / consumer form; in-place and repeated runs bit-identical.  The bounds are those of
tests/test_hip_tail.py / tests/test_hip_fused_f32.py / tests/test_hip_chain_ops.py for the same arithmetic.

Measured maximum |error| per case and mode (printed by the GPU tests, run with -s): docs/lab_notebook.md."""
import collections
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fill import seeded_randn
from helpers import apply_math_mode  # noqa: F401  (autouse fixture: a test that takes math_mode runs in that mode)
from helpers import assert_close, bottleneck_stages_f64
from oracle import index_ref as IR
from oracle import torch_ref as TR

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "laudnet_amd", "csrc")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()  # raises if libldn_hip.so is missing -- no fallback
    return _ops


# ------------------------------------------------------------------ the count-dependent choices of the kernels, restated
LDS_BYTES = 160 * 1024       # csrc/ldn_tail.hip:1156 (k_head), :1366 (launch_chain: lds_total)
T_KIDX_BYTES = 1280          # csrc/ldn_tail.hip:104
T_W2_SLOTS = 3               # :105
LD_R2MAX = 4                 # csrc/ldn_chain_ld.h:29
LD_SYNC_OFF = T_KIDX_BYTES   # :30
LD_SYNC_BYTES = 256          # :31


def _round_up(a, b):
    return -(-a // b) * b


def _ceil_div(a, b):
    return -(-a // b)


def head_split(HW):
    """bottleneck_head_impl (csrc/ldn_tail.hip:1210-1214) -> (pix_per_blk, mblocks): workgroups of at most 256 pixels, whole 32-pixel wave
    tiles where that takes no more workgroups."""
    mblocks = _ceil_div(HW, 256)
    pix_per_blk = _ceil_div(HW, mblocks)
    up = _round_up(pix_per_blk, 32)
    if up <= 256 and up * (mblocks - 1) < HW:
        pix_per_blk = up
    return pix_per_blk, mblocks


HeadClass = collections.namedtuple("HeadClass", "nsub nw D kloop")      # of one (image, workgroup)


def head_classes(HW, cin, width, Kb):
    """head_body (csrc/ldn_tail.hip): nsub :882, wrows :883, xrows / slot_bytes :893-894, avail / D :900-901, nchunks :902, nw :904; the chunks
    beyond the K loop re-fetch the last one :932, so cin / 32 < D is a path of its own.  One HeadClass per workgroup of the image (the last
    workgroup may hold fewer pixels and so a deeper ring)."""
    pix_per_blk, mblocks = head_split(HW)
    Nb = min(Kb, width)
    nsub = _ceil_div(Nb, 32)
    wrows = _round_up(max(Nb, 1), 64)
    avail = LDS_BYTES - (T_KIDX_BYTES + 3 * width * 4) - 256
    nchunks = cin // 32
    out = []
    for mb in range(mblocks):
        npix = min(pix_per_blk, HW - mb * pix_per_blk)                    # :877-878
        slot_bytes = (_round_up(npix, 32) + wrows) * 128
        D = min(4, avail // slot_bytes)
        out.append(HeadClass(nsub, wrows // 64, D, "short" if nchunks < D else ("equal" if nchunks == D else "long")))
    return out


TailClass = collections.namedtuple("TailClass", "nsub n_w2 last")


def tail_class(width, gran, Kb):
    """tail_body (csrc/ldn_tail.hip): nsub :211, Kp :212, n_w2 :259 (nchunks = 9 nsub :315; npo[] :261-267 follows 2 v < Kb).  last: the
    fill of the last K slice -- "none" (no channel), "whole", "lone" (one group), "partial"."""
    NS = width // 32
    nsub = _ceil_div(min(Kb, width), 32)
    Kp = nsub * 32
    n_w2 = 1 if NS == 2 else (2 if NS == 4 else (4 if Kp > 128 else 2))
    last = "none" if Kb == 0 else ("whole" if Kb % 32 == 0 else ("lone" if Kb % 32 == gran else "partial"))
    return TailClass(nsub, n_w2, last)


def chain_slice_bytes(HW):
    """launch_chain (csrc/ldn_tail.hip:1365): bytes of an h1 slice slot of a whole-image block."""
    return _round_up((_round_up(HW, 8) + 1) * 128, 1024)


ChainClass = collections.namedtuple("ChainClass", "nsub R2 R3 DX RW")


def chain_class(HW, width, Kb):
    """k_chain_ld (csrc/ldn_chain_ld.h): tail_ld's nsub :411, Kp :412, slot2 / slot3 :414, avail2 / R2 :419-420, avail3 / R3 :421-422 (an
    image without channels returns early with the deepest rings, :211 / :258); head_ld's nwp / wslot :183-184 and DX / RW :195-199."""
    nsub = _ceil_div(min(Kb, width), 32)
    Kp = nsub * 32
    if nsub == 0:
        R2, R3 = LD_R2MAX, 4
    else:
        avail2 = LDS_BYTES - (LD_SYNC_OFF + LD_SYNC_BYTES) - 2 * chain_slice_bytes(HW)
        R2 = min(LD_R2MAX, avail2 // (Kp * 128))
        avail3 = LDS_BYTES - (LD_SYNC_OFF + LD_SYNC_BYTES) - 18 * width * 4 - 7 * 4096
        R3 = min(4, avail3 // (Kp * 128))
    wslot = 4 * max(nsub, 1) * 1024
    avail = LDS_BYTES - (LD_SYNC_OFF + LD_SYNC_BYTES + 3 * width * 4)
    ncomp = _ceil_div(HW, 32)
    DX = 3
    if (avail - ncomp * DX * 4096) // wslot < 3:
        DX = 2
    RW = min(4, (avail - ncomp * DX * 4096) // wslot)
    return ChainClass(nsub, R2, R3, DX, RW)


def expected_chain_kernel(H, Wd, width, f32):
    """launch_chain (csrc/ldn_tail.hip:1369-1392): the loader / consumer form serves bf16x3 at widths 128 / 256 on maps of at most 224 pixels."""
    NS = width // 32
    if not f32 and NS >= 4 and H * Wd <= 224:
        return f"k_chain_ld<{NS}>"
    return f"k_chain<{NS}, F32>" if f32 else f"k_chain<{NS}>"


# the row split of the tail (csrc/ldn_tail.hip:660-697), as tests/test_hip_fused_f32.py restates it: only to name a case's split
def _tail_region_pixels(R, Hi, Wi, st):
    return min(R + 1, (Hi + 1) // 2) * ((Wi - 1) // 2 + 1) if st == 2 else min(R + 2, Hi) * Wi


def tail_rows_per_block(Hi, Wi, NS, st):
    """-> (output rows per workgroup, workgroups per image); (0, 0): the map does not fit."""
    Ho, Wo = (Hi - 1) // st + 1, (Wi - 1) // st + 1
    R = min(256 // Wo, Ho)
    if R < 1:
        return 0, 0

    def fits(r):
        nr = _tail_region_pixels(r, Hi, Wi, st)
        lds2 = (T_KIDX_BYTES + (2 if st == 2 else (1 if NS == 2 else 2)) * _round_up((_round_up(nr, 8) + 1) * 128, 1024)
                + T_W2_SLOTS * 16 * NS * 256)
        return lds2 <= LDS_BYTES and (st == 2 or NS == 2 or _round_up(nr, 8) // 8 <= 72)

    while R > 1 and not fits(R):
        R -= 1
    if not fits(R):
        return 0, 0
    mbk = _ceil_div(Ho, R)
    best, best_waves = _ceil_div(Ho, mbk), 1 << 30
    for r in range(_ceil_div(Ho, mbk), R + 1):
        if r * (mbk - 1) >= Ho:
            break
        waves = sum(_ceil_div(min(r, Ho - r * i) * Wo, 32) for i in range(mbk))
        if waves < best_waves:
            best_waves, best = waves, r
    return best, mbk


# ------------------------------------------------------------------ the case tables: counts are forced per image / per block
SHAPES = {"b": "bottom", "t": "top", "r": "random"}     # which groups an image keeps: the lowest, the highest (the list ends in W - 1), a seeded choice


def _imgs(counts, start=0):
    """(count, list shape) per image: the three list shapes in turn."""
    return tuple((k, "rbt"[(i + start) % 3]) for i, k in enumerate(counts))


Case = collections.namedtuple("Case", "H Wd cin width gran st images")          # cout = 4 * width; st: the stride of the 3x3

HT_CASES = [
    # width 256 on 14 x 14 (one head workgroup): every nsub, nw 1..4 = D 4 / 3 / 2 / 2; cin 96 is a K loop shorter than / equal to / longer than D
    Case(14, 14, 96, 256, 2, 1, _imgs((0, 2, 30, 32, 34, 64, 66, 96, 126, 128, 130, 160, 190, 192, 224, 254, 256))),
    # 324 pixels: two head workgroups (192 + 132 pixels: rings of their own), tail rows 10 + 8; cin / 32 == D at nw 1
    Case(18, 18, 128, 256, 2, 1, _imgs((0, 2, 34, 64, 66, 98, 128, 130, 162, 192, 194, 226, 256), 1)),
    # granularity 4; one K chunk: shorter than every ring
    Case(14, 14, 32, 256, 4, 1, _imgs((0, 4, 28, 32, 36, 64, 100, 128, 132, 188, 252, 256), 2)),
    # width 128: 400 pixels (head 224 + 176, tail 11 + 9 rows) and a non-square 180-pixel map
    Case(20, 20, 96, 128, 2, 1, _imgs((0, 2, 30, 32, 34, 62, 64, 66, 96, 98, 126, 128))),
    Case(9, 20, 256, 128, 2, 1, _imgs((0, 2, 34, 64, 66, 96, 126, 128), 1)),
    # width 64
    Case(14, 14, 32, 64, 2, 1, _imgs((0, 2, 30, 32, 34, 62, 64), 2)),
    Case(11, 25, 128, 64, 2, 1, _imgs((0, 2, 32, 34, 64))),
    # stride 2 at every width: 28 x 28 -> 14 x 14 (four head workgroups), 13 x 13 -> 7 x 7, 16 x 10 -> 8 x 5
    Case(28, 28, 128, 256, 2, 2, _imgs((0, 2, 34, 66, 128, 130, 160, 162, 194, 226, 254, 256), 1)),
    Case(13, 13, 96, 128, 2, 2, _imgs((0, 2, 32, 34, 64, 66, 96, 98, 128), 2)),
    Case(16, 10, 32, 64, 2, 2, _imgs((0, 2, 30, 32, 34, 62, 64))),
]

ProjCase = collections.namedtuple("ProjCase", "H Wd images")                      # cin = width = 64, cout = 256, granularity 2, stride 1
PROJ_COUNTS = (2, 30, 32, 34, 62, 64)
PROJ_CASES = [ProjCase(12, 12, _imgs(PROJ_COUNTS)), ProjCase(17, 19, _imgs(PROJ_COUNTS, 1))]

Run = collections.namedtuple("Run", "B H Wd width gran layers splits blocks")    # C = 4 * width; blocks: (count, list shape) of every image, per block

RUNS = [
    # k_chain_ld<8> (k_chain<8, F32> in fp32): nsub 8, 1, 8, 2, 7, 3, 0, 4, 5, 6; two-layer masker
    Run(3, 14, 14, 256, 2, 2, 8, _imgs((256, 2, 226, 64, 222, 66, 0, 128, 130, 190))),
    # k_chain_ld<4>: nsub 4, 1, 4, 2, 3, 0, 4, 1; one-layer masker; an odd number of GAP splits
    Run(3, 14, 14, 128, 2, 1, 7, _imgs((128, 2, 126, 64, 66, 0, 98, 30), 1)),
    # 225 pixels: the plain k_chain<8> in bf16x3
    Run(2, 15, 15, 256, 2, 2, 8, _imgs((256, 2, 254, 0, 130, 128), 2)),
    # k_chain<2>; granularity 4; one GAP split
    Run(3, 14, 14, 64, 4, 1, 1, _imgs((64, 4, 60, 0, 32, 36))),
]
MODES = ("fp32", "bf16x3")


def case_id(case):
    return f"c{HT_CASES.index(case)}-{case.H}x{case.Wd}x{case.cin}x{case.width}-g{case.gran}-s{case.st}-B{len(case.images)}"


def proj_id(case):
    return f"p{PROJ_CASES.index(case)}-{case.H}x{case.Wd}-B{len(case.images)}"


def run_id(run):
    return f"r{RUNS.index(run)}-{run.B}x{run.H}x{run.Wd}x{run.width}-g{run.gran}-l{run.layers}-n{len(run.blocks)}"


def _count_shape_gaps(what, width, per_case):
    """per_case: [(gran, counts)] of the cases of one width.  The count shapes every width must see."""
    gaps = []
    has = lambda f: any(f(gran, set(counts)) for gran, counts in per_case)
    if not has(lambda g, c: g in c):
        gaps.append(f"{what} width {width}: one group only")
    if not has(lambda g, c: any({32 * k - g, 32 * k, 32 * k + g} <= c for k in range(1, width // 32))):
        gaps.append(f"{what} width {width}: 32 k - gran, 32 k, 32 k + gran for one k")
    if not has(lambda g, c: width - g in c):
        gaps.append(f"{what} width {width}: W - gran")
    if not has(lambda g, c: width in c):
        gaps.append(f"{what} width {width}: W")
    return gaps


def ht_gaps(cases):
    """What a head / tail case table leaves out, as a list of strings (empty: complete).  Everything is asserted on the restated
    quantities of the images, never on a list of counts."""
    gaps = []
    for width in (64, 128, 256):
        NS = width // 32
        mine = [c for c in cases if c.width == width]
        head = [(c, hc) for c in mine for Kb, _ in c.images for hc in head_classes(c.H * c.Wd, c.cin, width, Kb)]
        gaps += [f"k_head width {width}: nsub = {n}" for n in range(NS + 1) if n not in {hc.nsub for _, hc in head}]
        gaps += [f"k_head width {width}: nw = {n}" for n in range(1, width // 64 + 1) if n not in {hc.nw for _, hc in head}]
        for HW in sorted({c.H * c.Wd for c in mine}):
            can = {hc.D for Kb in range(0, width + 1, 2) for hc in head_classes(HW, 32, width, Kb)}
            seen = {hc.D for c, hc in head if c.H * c.Wd == HW}
            gaps += [f"k_head width {width}, {HW} pixels: D = {d}" for d in sorted(can - seen)]
        for st in (1, 2):
            seen = {tail_class(width, c.gran, Kb).nsub for c in mine if c.st == st for Kb, _ in c.images}
            gaps += [f"k_tail width {width} stride {st}: nsub = {n}" for n in range(NS + 1) if n not in seen]
        gaps += _count_shape_gaps("head / tail", width, [(c.gran, [Kb for Kb, _ in c.images]) for c in mine])
        for name in SHAPES.values():
            if not any(SHAPES[s] == name and 0 < Kb < width for c in mine for Kb, s in c.images):
                gaps.append(f"head / tail width {width}: list shape {name}")
    kloops = {hc.kloop for c in cases for Kb, _ in c.images for hc in head_classes(c.H * c.Wd, c.cin, c.width, Kb) if Kb > 0}
    gaps += [f"k_head: cin / 32 {rel} D" for rel, k in (("<", "short"), ("==", "equal"), (">", "long")) if k not in kloops]
    # both n_w2 values of k_tail<8>, on neighbouring images with 128 and 128 + gran channels
    side = False
    for c in cases:
        if c.width == 256:
            cls = [tail_class(256, c.gran, Kb) for Kb, _ in c.images]
            side |= any(c.images[i][0] == 128 and c.images[i + 1][0] == 128 + c.gran and (cls[i].n_w2, cls[i + 1].n_w2) == (2, 4)
                        for i in range(len(cls) - 1))
    if not side:
        gaps.append("k_tail<8>: n_w2 = 2 and 4 side by side (128 and 128 + gran channels)")
    # maps
    splits = [(c, head_split(c.H * c.Wd)[1], tail_rows_per_block(c.H, c.Wd, c.width // 32, c.st)) for c in cases]
    if not any((c.H, c.Wd, c.st) == (14, 14, 1) and hw == 1 for c, hw, _ in splits):
        gaps.append("map: 14 x 14 (one head workgroup)")
    if not any(c.H * c.Wd > 256 and hw == 2 and mbk > 1 and rows * mbk != (c.H - 1) // c.st + 1 for c, hw, (rows, mbk) in splits):
        gaps.append("map: more than 256 pixels with two head workgroups and a ragged tail split")
    if not any((c.H, c.Wd, c.st) == (28, 28, 2) for c in cases):
        gaps.append("map: stride 2, 28 x 28 -> 14 x 14")
    if not any(c.H != c.Wd for c in cases):
        gaps.append("map: non-square")
    gaps += [f"granularity {g}" for g in (2, 4) if g not in {c.gran for c in cases}]
    return gaps


def chain_gaps(runs):
    """What a table of chained runs leaves out."""
    gaps = []
    kernels = {}
    for r in runs:
        for mode in MODES:
            kernels.setdefault(expected_chain_kernel(r.H, r.Wd, r.width, mode == "fp32"), []).append(r)
    for NS in (4, 8):
        mine = kernels.get(f"k_chain_ld<{NS}>", [])
        cls = [chain_class(r.H * r.Wd, r.width, Kb) for r in mine for Kb, _ in r.blocks]
        gaps += [f"k_chain_ld<{NS}>: nsub = {n}" for n in range(1, NS + 1) if n not in {c.nsub for c in cls}]
        for r in mine:
            can = [chain_class(r.H * r.Wd, r.width, 32 * n) for n in range(1, NS + 1)]
            got = [chain_class(r.H * r.Wd, r.width, Kb) for Kb, _ in r.blocks if Kb > 0]
            for axis in ("R2", "R3", "DX", "RW"):
                missing = {getattr(c, axis) for c in can} - {getattr(c, axis) for c in got}
                gaps += [f"k_chain_ld<{NS}> on {r.H} x {r.Wd}: {axis} = {v}" for v in sorted(missing)]
        seqs = [[chain_class(r.H * r.Wd, r.width, Kb).nsub for Kb, _ in r.blocks] for r in mine]
        if not any(0 in s[1:-1] for s in seqs):
            gaps.append(f"k_chain_ld<{NS}>: a block without channels inside a run")
        if not any(s[i:i + 3] == [NS, 1, NS] for s in seqs for i in range(len(s) - 2)):
            gaps.append(f"k_chain_ld<{NS}>: adjacent blocks stepping {NS} -> 1 -> {NS}")
        if len({chain_class(r.H * r.Wd, r.width, Kb).R2 for r in mine for Kb, _ in r.blocks}) < 2 and NS == 8:
            gaps.append("k_chain_ld<8>: a change of ring depth inside a run")
    for k in ("k_chain<8>", "k_chain<2>", "k_chain<2, F32>", "k_chain<4, F32>", "k_chain<8, F32>"):
        if k not in kernels:
            gaps.append(f"a run on {k}")
    gaps += [f"a {n}-layer masker" for n in (1, 2) if n not in {r.layers for r in runs}]
    for width in sorted({r.width for r in runs}):
        mine = [(r.gran, {Kb for Kb, _ in r.blocks}) for r in runs if r.width == width]
        if not any(g in c for g, c in mine):
            gaps.append(f"chain width {width}: one group only")
        if not any(width in c for g, c in mine):
            gaps.append(f"chain width {width}: W")
    return gaps


# ------------------------------------------------------------------ non-GPU: the restatement and the tables
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_restated_expressions_are_the_source():
    """The constants and the expressions restated above, as the source spells them (whitespace aside): a change of any of them must be
    followed here."""
    tail, ld = _source("ldn_tail.hip"), _source("ldn_chain_ld.h")
    const = lambda text, name: re.search(r"constexpr int %s = ([^;]+);" % name, text).group(1).strip()
    assert int(const(tail, "T_KIDX_BYTES")) == T_KIDX_BYTES and int(const(tail, "T_W2_SLOTS")) == T_W2_SLOTS
    assert int(const(ld, "LD_R2MAX")) == LD_R2MAX and int(const(ld, "LD_SYNC_BYTES")) == LD_SYNC_BYTES
    assert const(ld, "LD_SYNC_OFF") == "T_KIDX_BYTES"
    for text, lines in ((tail, (
            "a.mblocks = ceil_div(HW, 256);",
            "a.pix_per_blk = ceil_div(HW, a.mblocks);",
            "if (const int up = round_up(a.pix_per_blk, 32); up <= 256 && (long)up * (a.mblocks - 1) < HW) a.pix_per_blk = up;",
            "const int npix = min(p.pix_per_blk, p.HW - m0);",
            "const int nsub = __builtin_amdgcn_readfirstlane(ceil_div(Nb, 32));",
            "const int wrows = round_up(max(Nb, 1), 64);",
            "const int xrows = round_up(npix, 32);",
            "const int slot_bytes = (xrows + wrows) * 128;",
            "const int avail = lds_total - (T_KIDX_BYTES + 3 * W * 4) - 256;",
            "const int D = min(4, avail / slot_bytes);",
            "const int nchunks = p.cin / 32;",
            "const int nw = wrows / 64;",
            "const int cc = min(c, nchunks - 1);",
            "head_body<NS, F32, true>(p, blockIdx.x % p.B, blockIdx.x / p.B, smem, 160 * 1024, threadIdx.x);",
            "const int nsub = ceil_div(Kb, 32);",
            "const int Kp = nsub * 32;",
            "const int n_w2 = NS == 2 ? 1 : (NS == 4 ? 2 : (Kp > 128 ? 4 : 2));",
            "const int nchunks = nsub * 9;",
            "a.slice_bytes = round_up((round_up(nr, 8) + 1) * 128, 1024); const size_t lds = 160 * 1024;",
            "a.lds_total = (int)lds;",
            "if (use_ld && nr <= 224) {")),
                        (ld, (
            "const int nsub = __builtin_amdgcn_readfirstlane(ceil_div(Kb, 32));",
            "const int Kp = nsub * 32;",
            "const int slot2 = Kp * 128, slot3 = Kp * 128;",
            "const int avail2 = lds_total - (LD_SYNC_OFF + LD_SYNC_BYTES) - 2 * p.slice_bytes;",
            "(nsub > 0 ? min(LD_R2MAX, avail2 / slot2) : LD_R2MAX);",
            "const int avail3 = lds_total - (LD_SYNC_OFF + LD_SYNC_BYTES) - 18 * NP * 4 - 7 * 4096;",
            "(nsub > 0 ? min(4, avail3 / slot3) : 4);",
            "const int nwp = __builtin_amdgcn_readfirstlane(4 * max(nsub, 1));",
            "const int wslot = nwp * 1024;",
            "const int avail = lds_total - (LD_SYNC_OFF + LD_SYNC_BYTES + 3 * W * 4);",
            "if ((avail - ncomp * DX * 4096) / wslot < 3) DX = 2;",
            "(min(4, (avail - ncomp * DX * 4096) / wslot));"))):
        for line in lines:
            assert line in text, f"not in the source any more: {line}"


def test_restated_values_at_the_production_shapes():
    """The values the source gives, written out: k_head's ring at 14 x 14 x 256 per nw, the split of larger maps, k_tail<8>'s n_w2, the
    rings of k_chain_ld at 14 x 14."""
    D = lambda HW, width, Kb: [hc.D for hc in head_classes(HW, 1024, width, Kb)]
    assert [head_classes(196, 1024, 256, Kb)[0][:3] for Kb in (0, 2, 64, 66, 128, 130, 192, 194, 256)] == \
        [(0, 1, 4), (1, 1, 4), (2, 1, 4), (3, 2, 3), (4, 2, 3), (5, 3, 2), (6, 3, 2), (7, 4, 2), (8, 4, 2)]
    assert head_split(196) == (224, 1) and head_split(784) == (224, 4) and head_split(400) == (224, 2) and head_split(324) == (192, 2)
    assert D(324, 256, 128) == [3, 4] and D(400, 128, 128) == [3, 3] and D(784, 256, 128) == [3, 3, 3, 4]          # the last workgroup holds fewer pixels: a deeper ring
    assert [head_classes(196, 32 * n, 256, 2)[0].kloop for n in (1, 3, 4, 5)] == ["short", "short", "equal", "long"]
    assert [tail_class(256, 2, Kb).n_w2 for Kb in (0, 2, 128, 130, 256)] == [2, 2, 2, 4, 4]
    assert {tail_class(128, 2, Kb).n_w2 for Kb in range(0, 129, 2)} == {2} and {tail_class(64, 2, Kb).n_w2 for Kb in range(0, 65, 2)} == {1}
    assert [tail_class(256, 2, Kb).last for Kb in (0, 32, 34, 36, 62)] == ["none", "whole", "lone", "partial", "partial"]
    assert tail_class(256, 4, 36).last == "lone"
    assert chain_slice_bytes(196) == 26624
    assert [chain_class(196, 256, 32 * n)[:3] for n in range(9)] == \
        [(0, 4, 4), (1, 4, 4), (2, 4, 4), (3, 4, 4), (4, 4, 4), (5, 4, 4), (6, 4, 4), (7, 3, 4), (8, 3, 3)]
    assert {chain_class(196, 128, 32 * n)[1:3] for n in range(5)} == {(4, 4)}
    assert tail_rows_per_block(18, 18, 8, 1) == (10, 2) and tail_rows_per_block(20, 20, 4, 1) == (11, 2)
    assert tail_rows_per_block(28, 28, 8, 2) == (14, 1) and tail_rows_per_block(14, 14, 8, 1) == (14, 1)


def test_case_tables_are_complete():
    """Nothing the issue lists is missing from the tables, and every launch is one the library accepts (it loads without a GPU)."""
    from laudnet_amd import ops
    assert ht_gaps(HT_CASES) == []
    assert chain_gaps(RUNS) == []
    for c in HT_CASES:
        assert c.cin in (32, 96, 128, 256) and c.width in (64, 128, 256) and c.gran in (2, 4) and c.st in (1, 2)
        assert 1 <= len(c.images) <= 17 and all(0 <= Kb <= c.width and Kb % c.gran == 0 and s in SHAPES for Kb, s in c.images), c
        rows, mbk = tail_rows_per_block(c.H, c.Wd, c.width // 32, c.st)
        assert rows > 0 and ops.bottleneck_tail_splits(c.H, c.Wd, c.width, c.st) == 8 * mbk, c
    for c in PROJ_CASES:
        assert sorted(Kb for Kb, _ in c.images) == [2, 30, 32, 34, 62, 64] and ops.bottleneck_tail_proj_fits(c.H, c.Wd, 64, 64)
        assert {tail_class(64, 2, Kb).nsub for Kb, _ in c.images} == {1, 2}
    assert {SHAPES[s] for c in PROJ_CASES for _, s in c.images} == set(SHAPES.values())
    assert any(head_split(c.H * c.Wd)[1] == 1 for c in PROJ_CASES) and any(head_split(c.H * c.Wd)[1] == 2 for c in PROJ_CASES)
    for r in RUNS:
        assert ops.bottleneck_chain_fits(r.H, r.Wd, 4 * r.width, r.width, _hidden(r), r.width // r.gran), r
        assert 64 < r.H * r.Wd <= 256 and r.B <= 3 and len(r.blocks) <= 10 and r.width % r.gran == 0 and r.gran % 2 == 0
        assert all(0 <= Kb <= r.width and Kb % r.gran == 0 for Kb, _ in r.blocks)
    seq = [chain_class(196, 256, Kb).nsub for Kb, _ in RUNS[0].blocks]
    assert seq == [8, 1, 8, 2, 7, 3, 0, 4, 5, 6] and expected_chain_kernel(14, 14, 256, False) == "k_chain_ld<8>"


def test_the_completeness_proof_notices_a_removed_class():
    """ht_gaps / chain_gaps have teeth: without the images of one nsub at one width and stride, without a case that is a sole witness, or
    without one block of a run, they name what is missing."""
    drop_images = lambda keep: [c._replace(images=tuple(im for im in c.images if keep(c, im))) for c in HT_CASES]
    for width in (64, 128, 256):
        for st in (1, 2):
            for n in range(width // 32 + 1):
                gaps = ht_gaps(drop_images(lambda c, im: not (c.width == width and c.st == st and _ceil_div(im[0], 32) == n)))
                assert f"k_tail width {width} stride {st}: nsub = {n}" in gaps, (width, st, n)
    assert any("n_w2" in g for g in ht_gaps(drop_images(lambda c, im: im[0] not in (130, 132))))
    assert any("list shape top" in g for g in ht_gaps(drop_images(lambda c, im: im[1] != "t")))
    assert any("one group only" in g for g in ht_gaps(drop_images(lambda c, im: im[0] != c.gran)))
    assert any("W - gran" in g for g in ht_gaps(drop_images(lambda c, im: im[0] != c.width - c.gran)))
    assert any("32 k - gran" in g for g in ht_gaps(drop_images(lambda c, im: im[0] % 32 != 0 or im[0] == c.width)))
    assert any("D = 3" in g for g in ht_gaps(drop_images(lambda c, im: not (c.width == 256 and 64 < im[0] <= 128))))
    without = lambda i: ht_gaps([c for j, c in enumerate(HT_CASES) if j != i])
    assert "granularity 4" in without(2)
    assert "map: stride 2, 28 x 28 -> 14 x 14" in without(7)
    assert "map: 14 x 14 (one head workgroup)" in ht_gaps([c for c in HT_CASES if (c.H, c.Wd, c.st) != (14, 14, 1)])
    assert "map: non-square" in ht_gaps([c for c in HT_CASES if c.H == c.Wd])
    assert any("ragged" in g for g in ht_gaps([c for c in HT_CASES if c.H * c.Wd <= 256 or c.st == 2]))
    assert "k_head: cin / 32 < D" in ht_gaps([c for c in HT_CASES if c.cin >= 128])
    assert "k_head: cin / 32 == D" in ht_gaps([c._replace(cin=256) for c in HT_CASES])
    # the runs: every block of the loader / consumer runs is needed for some class
    drop_block = lambda ri, bi: [r._replace(blocks=r.blocks[:bi] + r.blocks[bi + 1:]) if j == ri else r for j, r in enumerate(RUNS)]
    for ri in (0, 1):
        NS = RUNS[ri].width // 32
        nsubs = [_ceil_div(Kb, 32) for Kb, _ in RUNS[ri].blocks]
        for bi, n in enumerate(nsubs):
            if nsubs.count(n) == 1 or (n == 1 and bi == 1):
                assert chain_gaps(drop_block(ri, bi)) != [], (ri, bi)
        assert f"k_chain_ld<{NS}>: a block without channels inside a run" in chain_gaps(drop_block(ri, nsubs.index(0)))
        assert f"k_chain_ld<{NS}>: adjacent blocks stepping {NS} -> 1 -> {NS}" in chain_gaps(drop_block(ri, 1))
    assert "a run on k_chain<8>" in chain_gaps(RUNS[:2] + RUNS[3:]) and "a run on k_chain<2>" in chain_gaps(RUNS[:3])
    assert "a 2-layer masker" in chain_gaps([r for r in RUNS if r.layers == 1])


# ------------------------------------------------------------------ masks with forced counts
def forced_group_mask(G, gran, images, seed):
    """[len(images), G] {0,1}: image b keeps exactly images[b][0] / gran groups -- the lowest ("b"), the highest ("t") or a seeded choice
    ("r", built as tests/test_hip_small_classes.py builds its masks)."""
    gm = torch.zeros(len(images), G)
    for b, (Kb, shape) in enumerate(images):
        n = Kb // gran
        if shape == "b":
            gm[b, :n] = 1.0
        elif shape == "t":
            gm[b, G - n:] = 1.0
        else:
            gm[b, torch.randperm(G, generator=torch.Generator().manual_seed(seed + 10 + b))[:n]] = 1.0
    return gm


def _check_mask_shapes(gm, width, gran, images):
    idx, cnt = IR.channel_lists(gm.numpy(), width)
    assert cnt.tolist() == [Kb for Kb, _ in images]
    for b, (Kb, shape) in enumerate(images):
        if Kb == 0:
            continue
        lst = idx[b, :Kb]
        if shape == "b":
            assert lst.tolist() == list(range(Kb))
        elif shape == "t":
            assert lst.tolist() == list(range(width - Kb, width)) and lst[-1] == width - 1
        elif 2 * gran <= Kb <= width - 2 * gran:
            assert int(lst[-1] - lst[0]) + 1 > Kb, f"image {b}: a random choice must not be contiguous"


def test_forced_masks_have_the_stated_counts_and_shapes():
    for case in HT_CASES:
        _check_mask_shapes(forced_group_mask(case.width // case.gran, case.gran, case.images, _ht_seed(case)), case.width, case.gran, case.images)
    for case in PROJ_CASES:
        _check_mask_shapes(forced_group_mask(32, 2, case.images, _proj_seed(case)), 64, 2, case.images)
    for run in RUNS:
        _check_mask_shapes(forced_group_mask(run.width // run.gran, run.gran, run.blocks, _run_seed(run)), run.width, run.gran, run.blocks)


# ------------------------------------------------------------------ head and tail: block, input, residual, float64 reference (CPU, seeded)
def _ht_seed(case):
    return 2000 + 19 * HT_CASES.index(case)


def _proj_seed(case):
    return 2600 + 23 * PROJ_CASES.index(case)


def _run_seed(run):
    return 3000 + 41 * RUNS.index(run)


def _he_weights_(convs, g):
    with torch.no_grad():
        for m in convs:
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)


def _ht_kwargs(case):
    return dict(stride=case.st, downsample=None, dyn_mode="channel", channel_dyn_granularity=case.gran, channel_masker="MLP",
                output_size=(case.H - 1) // case.st + 1)


@functools.lru_cache(maxsize=None)
def build_case(case):
    """-> (reference block (float32 parameters), x [B,cin,H,Wd], residual [B,cout,Ho,Wo], group mask [B,G] with the forced counts)."""
    seed = _ht_seed(case)
    B = len(case.images)
    blk = TR.BottleneckRef(case.cin, case.width, **_ht_kwargs(case)).eval()
    TR.randomize_bn_(blk, seed)
    _he_weights_((blk.conv1, blk.conv2, blk.conv3), torch.Generator().manual_seed(seed + 1))
    Ho, Wo = (case.H - 1) // case.st + 1, (case.Wd - 1) // case.st + 1
    x = F.relu(seeded_randn((B, case.cin, case.H, case.Wd), seed + 2))
    ident = F.relu(seeded_randn((B, 4 * case.width, Ho, Wo), seed + 3))     # the residual (a projection's output: cin != cout)
    return blk, x, ident, forced_group_mask(case.width // case.gran, case.gran, case.images, seed)


@functools.lru_cache(maxsize=None)
def reference_f64(case):
    """The channel-mode algebra of oracle.torch_ref.BottleneckRef.forward (laud_resnet.py:115-144: the mask before bn1 / bn2) in float64
    throughout: (h1 [B,width,H,Wd], out [B,Ho,Wo,cout])."""
    blk, x, ident, gm = build_case(case)
    b64 = TR.BottleneckRef(case.cin, case.width, **_ht_kwargs(case)).eval().double()
    b64.load_state_dict(blk.state_dict())
    with torch.no_grad():
        cm = TR.broadcast_channel_mask(gm.double(), case.width)
        h1 = F.relu(b64.bn1(b64.conv1(x.double()) * cm))
        h2 = F.relu(b64.bn2(b64.conv2(h1) * cm))
        out = F.relu(b64.bn3(b64.conv3(h2)) + ident.double()).permute(0, 2, 3, 1).contiguous()
    assert h1.dtype == out.dtype == torch.float64
    return h1, out


# ------------------------------------------------------------------ GPU: head and tail
def _decode_h1(h1, f32):
    """h1 as values: plain floats in the fp32 form; [octet][8 hi | 8 lo] bf16 (hi + lo) in the bf16x3 form."""
    if f32:
        return h1
    B, H, W, ld = h1.shape
    raw = h1.contiguous().view(torch.bfloat16).reshape(B, H, W, ld // 8, 2, 8).float()
    return (raw[..., 0, :] + raw[..., 1, :]).reshape(B, H, W, ld)


class _Spy:
    """Records the dtype of the weight operands of every ops.bottleneck_head / bottleneck_tail / bottleneck_tail_proj call while installed."""

    def __init__(self, ops):
        self.ops, self.head, self.tail, self.proj = ops, [], [], []

    def __enter__(self):
        self._head, self._tail, self._proj = self.ops.bottleneck_head, self.ops.bottleneck_tail, self.ops.bottleneck_tail_proj
        self.ops.bottleneck_head = lambda *a, **k: (self.head.append(a[1].dtype), self._head(*a, **k))[1]
        self.ops.bottleneck_tail = lambda *a, **k: (self.tail.append((a[1].dtype, a[2].dtype)), self._tail(*a, **k))[1]
        self.ops.bottleneck_tail_proj = lambda *a, **k: (self.proj.append((a[1].dtype, a[2].dtype, a[10].dtype)), self._proj(*a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.ops.bottleneck_head, self.ops.bottleneck_tail, self.ops.bottleneck_tail_proj = self._head, self._tail, self._proj


def _check_h1(h1, f32, want_h1, c1, idx, cnt, what):
    """Per image: the active channels' relu(bn1(conv1)) - post_sub1, left-packed, within 1e-4 + 1e-4 |ref|; exact zeros up to the next
    multiple of 32.  -> per-image maximum |error|."""
    dec = _decode_h1(h1, f32).cpu()
    errs = []
    for b in range(dec.shape[0]):
        n = int(cnt[b])
        ch = idx[b, :n].cpu().long()
        want1 = want_h1[b, ch].permute(1, 2, 0) - c1[ch]
        errs.append(assert_close(dec[b, :, :, :n], want1, 1e-4, 1e-4, f"h1 of {what(b)}"))
        pad = (n + 31) // 32 * 32
        assert bool((dec[b, :, :, n:pad] == 0).all()), f"h1 of {what(b)}: columns up to the next multiple of 32 must be zero"
    return errs


@gpu
@pytest.mark.parametrize("case", HT_CASES, ids=case_id)
def test_head_and_tail_forced_counts_vs_float64(ops, case, math_mode):
    from laudnet_amd.laud_resnet import Bottleneck
    H, Wd, cin, width, gran, st, images = case
    f32 = math_mode == "fp32"
    wdtype = torch.float32 if f32 else torch.bfloat16
    B, G, cout = len(images), width // gran, 4 * width
    Ho, Wo = (H - 1) // st + 1, (Wd - 1) // st + 1
    blk, x, ident, gm = build_case(case)
    want_h1, want_out = reference_f64(case)
    hb = Bottleneck(cin, width, **_ht_kwargs(case)).eval()
    hb.load_state_dict(blk.state_dict())
    hb = hb.to(DEV)
    p = hb._prepare(torch.device(DEV))
    w2p, w3p = hb.tail_weights(p)
    w1s = p[hb._w1s_key()]
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, G, gran, mask_in=gm.to(DEV))
    assert cnt.tolist() == [Kb for Kb, _ in images], "the masker must hand the kernels exactly the forced counts"
    widx, _ = IR.channel_lists(gm.numpy(), width)
    for b, (Kb, _) in enumerate(images):
        assert np.array_equal(idx[b, :Kb].cpu().numpy(), widx[b, :Kb]), f"image {b}: the list is not that of the mask"
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    idn = ident.permute(0, 2, 3, 1).contiguous().to(DEV)
    idn_keep = idn.clone()
    splits = ops.bottleneck_tail_splits(H, Wd, width, st)
    assert splits == 8 * tail_rows_per_block(H, Wd, width // 32, st)[1] > 0
    h1 = torch.full((B, H, Wd, width), NAN, device=DEV)
    out = torch.full((B, Ho, Wo, cout), NAN, device=DEV)
    colsum = torch.full((B, splits, cout), NAN, device=DEV)
    with _Spy(ops) as spy:
        ops.bottleneck_head(xn, w1s, idx, cnt, p["s1"], p["t1"], p["c1"], h1)
        ops.bottleneck_tail(h1, w2p, w3p, idx, cnt, p["s2"], p["t2_tab"], p["c2"], p["t3c"], out, residual=idn, colsum=colsum, stride=st)
    torch.cuda.synchronize()
    assert spy.head == [wdtype] and spy.tail == [(wdtype, wdtype)], f"{math_mode} must run the {'fp32' if f32 else 'bf16x3'} forms"
    name = lambda b: (f"image {b} (Kb {images[b][0]} {SHAPES[images[b][1]]}, head {head_classes(H * Wd, cin, width, images[b][0])}, "
                      f"tail {tuple(tail_class(width, gran, images[b][0]))})")
    e1 = _check_h1(h1, f32, want_h1, p["c1"].cpu().double(), idx, cnt, name)
    assert torch.equal(xn.cpu(), x.permute(0, 2, 3, 1)), "the head must not touch its input"
    got = out.cpu()
    eo = [assert_close(got[b], want_out[b], 2e-4, 1e-4, f"out of {name(b)}") for b in range(B)]
    assert torch.allclose(colsum.sum(dim=1).cpu().double(), got.double().sum(dim=(1, 2)), atol=1e-2, rtol=1e-5)
    assert torch.equal(idn, idn_keep), "a residual that is a separate tensor must stay intact"
    # in-place residual stream (out aliases residual): bit-identical, colsum included
    colsum2 = torch.full_like(colsum, NAN)
    ops.bottleneck_tail(h1, w2p, w3p, idx, cnt, p["s2"], p["t2_tab"], p["c2"], p["t3c"], idn, residual=idn, colsum=colsum2, stride=st)
    torch.cuda.synchronize()
    assert torch.equal(idn, out) and torch.equal(colsum2, colsum), "the in-place form must equal the out-of-place one bit for bit"
    print(f"\n[counts] {case_id(case)} {math_mode:6s} max|err| h1 {max(e1):.2e} out {max(eo):.2e}")
    for b, (Kb, s) in enumerate(images):
        hc = head_classes(H * Wd, cin, width, Kb)
        tc = tail_class(width, gran, Kb)
        print(f"    image {b:2d} Kb {Kb:3d} {SHAPES[s]:6s} head nsub {hc[0].nsub} nw {hc[0].nw} D {'/'.join(str(c.D) for c in hc)} kloop "
              f"{'/'.join(c.kloop for c in hc)}; tail n_w2 {tc.n_w2} last {tc.last}; h1 {e1[b]:.2e} out {eo[b]:.2e}")


# ------------------------------------------------------------------ GPU: the folded-projection pair at width 64
def _proj_kwargs(case, cout):
    return dict(stride=1, downsample=nn.Sequential(nn.Conv2d(64, cout, 1, bias=False), nn.BatchNorm2d(cout)), dyn_mode="channel",
                channel_dyn_granularity=2, channel_masker="MLP", channel_masker_layers=2, output_size=case.H)


@functools.lru_cache(maxsize=None)
def build_proj_case(case):
    """Stage 1's first block (64 -> 64 -> 256, stride 1, projection shortcut) -> (reference block, x, group mask, float64 h1 [B,64,H,Wd],
    float64 out [B,H,Wd,256]: the float64 block with the float64 projection added, helpers.bottleneck_stages_f64)."""
    seed = _proj_seed(case)
    B = len(case.images)
    blk = TR.BottleneckRef(64, 64, **_proj_kwargs(case, 256)).eval()
    TR.randomize_bn_(blk, seed)
    _he_weights_((blk.conv1, blk.conv2, blk.conv3, blk.downsample[0]), torch.Generator().manual_seed(seed + 1))
    x = F.relu(seeded_randn((B, 64, case.H, case.Wd), seed + 2))
    gm = forced_group_mask(32, 2, case.images, seed)
    b64 = TR.BottleneckRef(64, 64, **_proj_kwargs(case, 256)).eval().double()
    b64.load_state_dict(blk.state_dict())
    st = bottleneck_stages_f64(b64, x, gm, torch.ones(B, 1, case.H, case.Wd, dtype=torch.float64))
    assert st[3].shape[1] == 256 and st[4].dtype == torch.float64
    return blk, x, gm, st[0], st[4].permute(0, 2, 3, 1).contiguous()


@gpu
@pytest.mark.parametrize("case", PROJ_CASES, ids=proj_id)
def test_folded_projection_forced_counts_vs_float64(ops, case):
    """bottleneck_head(..., x_split=...) + bottleneck_tail_proj called directly (k_tail<2, 1, PROJ>, a bf16x3 form) with forced counts."""
    from laudnet_amd.laud_resnet import Bottleneck
    H, Wd, images = case
    B, cin, width, cout, G, gran = len(images), 64, 64, 256, 32, 2
    blk, x, gm, want_h1, want_out = build_proj_case(case)
    assert ops.bottleneck_tail_proj_fits(H, Wd, width, cin)
    ops.set_math_mode("bf16x3")
    try:
        hb = Bottleneck(cin, width, **_proj_kwargs(case, cout)).eval()
        hb.load_state_dict(blk.state_dict())
        hb = hb.to(DEV)
        p = hb._prepare(torch.device(DEV))
        w2p, w3p = hb.tail_weights(p)
        with torch.no_grad():       # as Bottleneck._run_channel derives them
            wdp = ops.pack_w3_pairs(p["wd"].reshape(cout, cin) * p["sd"].view(-1, 1))
            t3cd = (p["t3c"] + p["td"]).contiguous()
        _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, G, gran, mask_in=gm.to(DEV))
        assert cnt.tolist() == [Kb for Kb, _ in images], "the masker must hand the kernels exactly the forced counts"
        xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
        splits = ops.bottleneck_tail_splits(H, Wd, width, 1)
        h1 = torch.full((B, H, Wd, width), NAN, device=DEV)
        xs = ops.x_split_buffer(B * H * Wd, cin, DEV)
        out = torch.full((B, H, Wd, cout), NAN, device=DEV)
        colsum = torch.full((B, splits, cout), NAN, device=DEV)
        with _Spy(ops) as spy:
            ops.bottleneck_head(xn, p["w1s"], idx, cnt, p["s1"], p["t1"], p["c1"], h1, x_split=xs)
            ops.bottleneck_tail_proj(h1, w2p, w3p, idx, cnt, p["s2"], p["t2_tab"], p["c2"], t3cd, xs, wdp, out, colsum=colsum)
        torch.cuda.synchronize()
        assert spy.head == [torch.bfloat16] and spy.proj == [(torch.bfloat16,) * 3] and spy.tail == []
        name = lambda b: f"image {b} (Kb {images[b][0]} {SHAPES[images[b][1]]}, tail {tuple(tail_class(width, gran, images[b][0]))})"
        e1 = _check_h1(h1, False, want_h1, p["c1"].cpu().double(), idx, cnt, name)
        assert torch.equal(xn.cpu(), x.permute(0, 2, 3, 1)), "the head must not touch its input"
        assert torch.allclose(ops.decode_x_split(xs, B * H * Wd, cin).cpu(), xn.reshape(-1, cin).cpu(), atol=0.0, rtol=2e-5)    # hi + lo = x to 2^-17
        got = out.cpu()
        eo = [assert_close(got[b], want_out[b], 2e-4, 1e-4, f"out of {name(b)}") for b in range(B)]
        assert torch.allclose(colsum.sum(dim=1).cpu().double(), got.double().sum(dim=(1, 2)), atol=1e-2, rtol=1e-5)
        # a second pair of launches into fresh buffers: bit-identical
        out2 = torch.full_like(out, NAN)
        colsum2 = torch.full_like(colsum, NAN)
        ops.bottleneck_tail_proj(h1, w2p, w3p, idx, cnt, p["s2"], p["t2_tab"], p["c2"], t3cd, xs, wdp, out2, colsum=colsum2)
        torch.cuda.synchronize()
        assert torch.equal(out2, out) and torch.equal(colsum2, colsum), "a repeated launch must be bit-identical"
    finally:
        ops.set_math_mode("fp32")
    print(f"\n[counts proj] {proj_id(case)} bf16x3 max|err| h1 {max(e1):.2e} out {max(eo):.2e}; per image out "
          + " ".join(f"{Kb}{s}:{e:.1e}" for (Kb, s), e in zip(images, eo)))


# ------------------------------------------------------------------ the chained launch: blocks whose maskers are decided by their bias
def _hidden(run):
    return max((run.width // run.gran) // 16, 16) if run.layers == 2 else 0       # Masker_channel_MLP: max(groups // reduction, 16)


def _run_kwargs(run):
    return dict(stride=1, downsample=None, dyn_mode="channel", channel_dyn_granularity=run.gran, channel_masker="MLP",
                channel_masker_layers=run.layers, output_size=run.H)


@functools.lru_cache(maxsize=None)
def build_run(run):
    """-> (reference blocks (float32 BottleneckRef), x [B,C,H,Wd], gap_in [B,splits,C], forced masks [nblocks,G]).  Conv weights, BatchNorm
    statistics, bn3.weight x 0.3 and the GAP partials as in tests/test_hip_chain_ops.py.  The masker's last linear layer has ZERO weights
    and the bias +4 / -4 on the keep / drop logit of every kept group (-4 / +4 of every dropped one), in the order of masker_logits_f64:
    the logits are +-4 for every image in float32 and in float64 alike."""
    C, G = 4 * run.width, run.width // run.gran
    seed = _run_seed(run)
    forced = forced_group_mask(G, run.gran, run.blocks, seed)
    blocks = []
    for i in range(len(run.blocks)):
        blk = TR.BottleneckRef(C, run.width, **_run_kwargs(run)).eval()
        TR.randomize_bn_(blk, seed + i)
        g = torch.Generator().manual_seed(seed + 100 + i)
        _he_weights_((blk.conv1, blk.conv2, blk.conv3), g)
        with torch.no_grad():
            blk.bn3.weight.mul_(0.3)
            for prm in blk.masker_channel.parameters():
                prm.copy_(torch.randn(prm.shape, generator=g) * (1.0 if prm.dim() == 2 else 0.5))
            conv = blk.masker_channel.conv
            last = conv if isinstance(conv, nn.Linear) else conv[2]
            last.weight.zero_()
            last.bias[:G] = 8.0 * forced[i] - 4.0
            last.bias[G:] = 4.0 - 8.0 * forced[i]
        blocks.append(blk)
    x = F.relu(seeded_randn((run.B, C, run.H, run.Wd), seed + 7))
    g = torch.Generator().manual_seed(seed + 9)
    assign = torch.randint(run.splits, (run.H * run.Wd,), generator=g)
    assign[:run.splits] = torch.arange(run.splits)                  # every set holds a pixel
    gap = torch.zeros(run.B, run.splits, C).index_add_(1, assign, x.permute(0, 2, 3, 1).reshape(run.B, run.H * run.Wd, C).contiguous())
    return blocks, x, gap, forced


def masker_logits_f64(blk, mean):
    """Masker_channel_MLP's logits (models/utils.py:92-131) from the channel means [B,C], in float64: [B,2,G]."""
    with torch.no_grad():
        conv = blk.masker_channel.conv
        lin = (lambda l, v: v @ l.weight.double().t() + l.bias.double())
        z = lin(conv, mean) if isinstance(conv, nn.Linear) else lin(conv[2], torch.relu(lin(conv[0], mean)))
    return z.reshape(mean.shape[0], 2, -1)


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_forced_maskers_decide_by_their_bias(run):
    """On the CPU: whatever the input, the float64 logits of every block are exactly +-4 and decide the forced mask."""
    blocks, x, gap, forced = build_run(run)
    assert gap.shape == (run.B, run.splits, 4 * run.width)
    assert torch.allclose(gap.sum(1).double(), x.double().sum(dim=(2, 3)), rtol=1e-5, atol=1e-3)
    assert [int(v) * run.gran for v in forced.sum(dim=1)] == [Kb for Kb, _ in run.blocks]
    for i, blk in enumerate(blocks):
        for mean in (gap.double().sum(1) / (run.H * run.Wd), 50.0 * torch.randn(run.B, 4 * run.width, dtype=torch.float64,
                                                                                 generator=torch.Generator().manual_seed(i))):
            z = masker_logits_f64(blk, mean)
            assert bool((z.abs() == 4.0).all()) and torch.equal((z[:, 0] >= z[:, 1]).float(), forced[i].expand(run.B, -1))


def _table_rows(hbs):
    """The rows of ops.chain_table exactly as ResNet._run_chain builds them (laudnet_amd/laud_resnet.py: _run_chain), under the mode in force."""
    rows = []
    for hb in hbs:
        p = hb._prepare(torch.device(DEV))
        mw = hb.masker_channel._weights()
        w2p, w3p = hb.tail_weights(p)
        rows.append((p[hb._w1s_key()], p["s1"], p["t1"], p["c1"], w2p, w3p, p["s2"], p["t2_tab"], p["c2"], p["t3c"], mw[0], mw[1], mw[2], mw[3]))
    return rows


@gpu
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_chain_forced_counts_vs_parts_and_float64(ops, run, math_mode):
    from laudnet_amd.laud_resnet import Bottleneck
    B, H, Wd, width, gran, layers, splits, spec = run
    C, G, HW, nblocks = 4 * width, width // gran, H * Wd, len(spec)
    hidden = _hidden(run)
    f32 = math_mode == "fp32"
    kernel = expected_chain_kernel(H, Wd, width, f32)
    blocks, x, gap_cpu, forced = build_run(run)
    hbs = []
    for blk in blocks:
        hb = Bottleneck(C, width, **_run_kwargs(run)).eval()
        hb.load_state_dict(blk.state_dict())
        hbs.append(hb.to(DEV))
    rows = _table_rows(hbs)
    for r in rows:
        assert r[0].dtype == r[4].dtype == r[5].dtype == (torch.float32 if f32 else torch.bfloat16)     # the mode's own weight layouts
        assert (r[12] is None) == (r[13] is None) == (layers == 1)
    table = ops.chain_table(rows, DEV)
    assert ops.bottleneck_chain_fits(H, Wd, C, width, hidden, G) and ops.bottleneck_tail_splits(H, Wd, width, 1) == 8
    xin = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    gap = gap_cpu.to(DEV)
    keep = xin.clone()
    ops.plan_timeouts(reset=True)

    # ---- the run, out of place (x_work starts as NaN), in place, and again
    work = torch.full_like(xin, NAN)
    masks, idx, cnt, colsum = ops.bottleneck_chain(xin, work, table, width, hidden, G, gran, gap, f32=f32)
    torch.cuda.synchronize()
    assert torch.equal(xin, keep), "x_in must stay intact when x_work is a separate tensor"
    assert tuple(masks.shape) == (nblocks, B, G) and tuple(idx.shape) == (nblocks, B, width) and tuple(cnt.shape) == (nblocks, B)
    assert tuple(colsum.shape) == (B, 8, C) and not bool(torch.isnan(work).any())
    # the kernel's decisions are the forced ones: every image of block i keeps exactly spec[i][0] channels, the groups of forced[i]
    assert cnt.cpu().tolist() == [[Kb] * B for Kb, _ in spec], "cnt must equal the forced counts"
    assert torch.equal(masks.cpu(), forced.unsqueeze(1).expand(nblocks, B, G)), "masks must equal the forced masks"
    widx, _ = IR.channel_lists(forced.numpy(), width)
    idx_c = idx.cpu().numpy()
    for i, (Kb, _) in enumerate(spec):
        for b in range(B):
            assert np.array_equal(idx_c[i, b, :Kb], widx[i, :Kb]), f"block {i}, image {b}: the list is not that of the mask"
    inpl = keep.clone()
    masks_i, idx_i, cnt_i, colsum_i = ops.bottleneck_chain(inpl, inpl, table, width, hidden, G, gran, gap, f32=f32)
    work2 = torch.full_like(xin, NAN)
    masks_2, idx_2, cnt_2, colsum_2 = ops.bottleneck_chain(xin, work2, table, width, hidden, G, gran, gap, f32=f32)
    torch.cuda.synchronize()
    for what, got in (("in place", (inpl, masks_i, idx_i, cnt_i, colsum_i)), ("second run", (work2, masks_2, idx_2, cnt_2, colsum_2))):
        assert torch.equal(got[0], work), f"{what}: x_work differs"
        assert torch.equal(got[1], masks) and torch.equal(got[3], cnt) and torch.equal(got[4], colsum), f"{what}: masks / counts / colsum differ"
        for i, (Kb, _) in enumerate(spec):
            assert torch.equal(got[2][i, :, :Kb], idx[i, :, :Kb]), f"{what}: lists of block {i}"
    if "k_chain_ld" in kernel:
        assert ops.plan_timeouts() == 0, "a hand-off wait of the loader / consumer form ran into its bound"

    # ---- the same run block by block through the stand-alone entry points: bit-identical
    xs = [xin]                      # the float32 input of every block, then the run's output
    gap_i = gap
    for i, r in enumerate(rows):
        mk, ix, ct, _ = ops.channel_masker(None, r[10], r[11], r[12], r[13], G, gran, gap_partial=gap_i, hw=HW)
        assert torch.equal(mk, masks[i]), f"block {i}: the chain's mask differs from ldn_channel_masker's"
        assert torch.equal(ct, cnt[i]), f"block {i}: counts differ"
        assert torch.equal(ix[:, :spec[i][0]], idx[i, :, :spec[i][0]]), f"block {i}: channel lists differ"
        h1 = torch.full((B, H, Wd, width), NAN, device=DEV)
        ops.bottleneck_head(xs[-1], r[0], ix, ct, r[1], r[2], r[3], h1)
        out = torch.full_like(xin, NAN)
        cs = torch.full((B, 8, C), NAN, device=DEV)
        ops.bottleneck_tail(h1, r[4], r[5], ix, ct, r[6], r[7], r[8], r[9], out, residual=xs[-1], colsum=cs)
        xs.append(out)
        gap_i = cs
    torch.cuda.synchronize()
    for i in range(nblocks):
        assert not bool(torch.isnan(xs[i + 1]).any()), f"block {i} executed on its own left an element unwritten"
    diff = (xs[-1] - work).abs().max().item()
    assert torch.equal(xs[-1], work), f"x_work after the run differs from the block-by-block execution (max {diff:.3e})"
    assert torch.equal(gap_i, colsum), "the final colsum differs from the last stand-alone tail's"

    # ---- every block against float64, from the kernel's own input; the float64 masker decides the same mask, without a margin
    errs = []
    for i, blk in enumerate(blocks):
        blk64 = TR.BottleneckRef(C, width, **_run_kwargs(run)).eval().double()
        blk64.load_state_dict(blk.state_dict())
        x_i = xs[i].cpu().permute(0, 3, 1, 2).double()
        mean = gap_cpu.double().sum(1) / HW if i == 0 else x_i.mean(dim=(2, 3))
        z = masker_logits_f64(blk64, mean)
        want_mask = (z[:, 0] >= z[:, 1]).float()
        assert torch.equal(masks[i].cpu(), want_mask), f"block {i}: the kernel's decisions differ from the float64 masker's"
        want = bottleneck_stages_f64(blk64, x_i, want_mask, torch.ones(B, 1, H, Wd, dtype=torch.float64))[4].permute(0, 2, 3, 1)
        cls = chain_class(HW, width, spec[i][0])
        errs.append(assert_close(xs[i + 1], want, 2e-4, 1e-4, f"block {i} of {kernel} (Kb {spec[i][0]} {SHAPES[spec[i][1]]}, {cls})"))
    out64 = work.cpu().double()
    assert torch.allclose(colsum.sum(1).cpu().double(), out64.sum(dim=(1, 2)), atol=1e-2, rtol=1e-5)
    print(f"\n[counts chain] {run_id(run)} {math_mode:6s} {kernel:16s} max|err| {max(errs):.2e}; per block "
          + " ".join(f"{Kb}{s}:{e:.1e}" for (Kb, s), e in zip(spec, errs)))
    if "k_chain_ld" in kernel:
        print("    rings per block (nsub R2 R3 DX RW): " + " ".join("/".join(map(str, chain_class(HW, width, Kb))) for Kb, _ in spec))
