"""ldn_conv_image -- the image form of the per-image channel-subset convolution (include/ldn_hip.h:500-523) -- variant by variant against
float64 (tests/conv_image_ref.py).  The packed-row form of the same three kernels has tests/test_hip_packed.py; this file is its
counterpart for what every channel-mode ResNet block, the RegNet a / c convs, the projection shortcuts and the dense path launch.

a  CPU: `expected_variant` (tests/conv_plan.py: the library's own chooser, conv_plan() of csrc/ldn_conv_plan.h, through a host-only
   program) enumerated over every launch the entry point admits comes to REACHABLE, and the
   case table below runs exactly that set in both arithmetic modes -- every tile shape and weight-staging mode of k_conv_image and
   k_conv_bf3, both wave grids of the 4 x 4 tile, k_conv1x1_stream with and without an input list.
b  The cases are the smallest shapes that still reach each variant, on maps that are never square: wider than high, higher than wide,
   under 32 pixels, one pixel high / wide, stride 2 from odd and from even maps, and for the streaming kernel a last 128-row block that
   holds 2 rows.  Every leading dimension is wider than the tensor it carries, and the padding holds NaN.
c  Per case and mode, every written element against the float64 reference; the zero columns behind an image's count; the padding columns
   untouched; colsum slot by slot; out_format 1 decoded.
d  The argument checks refuse before any launch.

Bounds (the project's own, tests/test_hip_packed.py: float64 reference, O(1) inputs, He-scaled weights, ReLU-ed activations):
1x1 1e-4 + 1e-4 |ref|; 3x3 and anything with a residual 2e-4 + 1e-4 |ref|; a colsum slot the sum of its elements' bounds."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_image_ref as R
import conv_plan
from conv_plan import expected_variant, expected_wave_rows
from fill import seeded_bernoulli, seeded_randn
from helpers import apply_math_mode  # noqa: F401  (autouse fixture: a test that takes math_mode runs in that mode)
from helpers import assert_close

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MATHS = ("fp32", "bf16x3")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()  # raises if libldn_hip.so is missing -- no fallback
    return _ops


# ------------------------------------------------------------------ a: what an image launch can reach
# kind -> (input list, output list); a residual and colsum need a dense output (no output list)
KINDS = {"dense": (False, False), "n": (False, True), "kn": (True, True), "k": (True, False)}
LAUNCH_KINDS = (("dense", 1), ("dense", 9), ("n", 1), ("kn", 9), ("k", 1), ("k", 9))


def launch_kw(kind, taps, rows, cin, cout, kgran=1, residual=False, scale=True, shift_classes=None, out_split=False):
    has_k, has_n = KINDS[kind]
    return dict(packed=False, rows_per_image=rows, cin=cin, cout=cout, taps=taps, has_k=has_k, has_n=has_n, kgran=kgran,
                shift_classes=(16 if taps == 9 else 1) if shift_classes is None else shift_classes, residual=residual, scale=scale,
                out_split=out_split)


def reachable_variants():
    """Every (kernel, MS, NS, BMODE, math, WM) an image launch can run, by ENUMERATION of the chooser over what ldn_conv_image admits: the six
    launch kinds x residual none / with scale / without scale (none with an output list) x list granularity 1 / 2 / 4 x cout 4 .. 2048 x
    Ho * Wo on both sides of every row threshold of the dispatch (64 | 96 | 128 | 256) x cin on both sides of the streaming kernel's 1024 x
    a 1- / 16-class table x out_format 0 / 1 (bf16x3 without a residual only) x both arithmetic modes."""
    couts = sorted(set(range(4, 513, 4)) | {768, 1024, 2048})
    rows = [1, 15, 31, 32, 33, 63, 64, 65, 95, 96, 97, 100, 127, 128, 129, 130, 180, 255, 256, 257, 520, 3136, 12544]
    found = set()
    for math in MATHS:      # one line of the CLI's grid form per (kind, residual, format, table): granularities, widths and row counts as lists
        lines = []
        for kind, taps in LAUNCH_KINDS:
            for residual, scale in ((False, True), (False, False), (True, True), (True, False)):
                if residual and KINDS[kind][1]:
                    continue
                for split in ((False, True) if math == "bf16x3" and not residual else (False,)):
                    for classes in (1, 16):
                        lines.append(conv_plan.shape_line(math=math, **launch_kw(kind, taps, rows, (32, 2048), couts, (1, 2, 4), residual, scale, classes, split)))
        found |= {k[:4] + (math, k[4]) for k in conv_plan.reachable(lines)}
    return found


# What reachable_variants() must come to, written out: every tile shape x every staging mode (no input list: B_NK; an input list alone:
# B_KN4; both lists: B_KN<granularity>) in both modes, the 4 x 4 tile of bf16x3 on both wave grids (2 x 2 behind a residual, which an
# output list excludes: B_NK and B_KN4 only), and the streaming kernel without and with an input list.  fp32 has no 2 x 10 tile and no
# streaming kernel.  16 + 24 instantiations: every row of LDN_CONV_KERNELS.  The last element is WM, the rows of k_conv_bf3's wave grid.
REACHABLE = {
    ("k_conv_image", 6, 2, "B_NK", "fp32", None), ("k_conv_image", 4, 4, "B_NK", "fp32", None), ("k_conv_image", 8, 6, "B_NK", "fp32", None),
    ("k_conv_image", 4, 10, "B_NK", "fp32", None),
    ("k_conv_image", 6, 2, "B_KN1", "fp32", None), ("k_conv_image", 4, 4, "B_KN1", "fp32", None), ("k_conv_image", 8, 6, "B_KN1", "fp32", None),
    ("k_conv_image", 4, 10, "B_KN1", "fp32", None),
    ("k_conv_image", 6, 2, "B_KN2", "fp32", None), ("k_conv_image", 4, 4, "B_KN2", "fp32", None), ("k_conv_image", 8, 6, "B_KN2", "fp32", None),
    ("k_conv_image", 4, 10, "B_KN2", "fp32", None),
    ("k_conv_image", 6, 2, "B_KN4", "fp32", None), ("k_conv_image", 4, 4, "B_KN4", "fp32", None), ("k_conv_image", 8, 6, "B_KN4", "fp32", None),
    ("k_conv_image", 4, 10, "B_KN4", "fp32", None),
    ("k_conv_bf3", 6, 2, "B_NK", "bf16x3", 2), ("k_conv_bf3", 4, 4, "B_NK", "bf16x3", 4), ("k_conv_bf3", 4, 4, "B_NK", "bf16x3", 2), ("k_conv_bf3", 8, 6, "B_NK", "bf16x3", 4),
    ("k_conv_bf3", 4, 10, "B_NK", "bf16x3", 2), ("k_conv_bf3", 2, 10, "B_NK", "bf16x3", 2),
    ("k_conv_bf3", 6, 2, "B_KN1", "bf16x3", 2), ("k_conv_bf3", 4, 4, "B_KN1", "bf16x3", 4), ("k_conv_bf3", 8, 6, "B_KN1", "bf16x3", 4),
    ("k_conv_bf3", 4, 10, "B_KN1", "bf16x3", 2), ("k_conv_bf3", 2, 10, "B_KN1", "bf16x3", 2),
    ("k_conv_bf3", 6, 2, "B_KN2", "bf16x3", 2), ("k_conv_bf3", 4, 4, "B_KN2", "bf16x3", 4), ("k_conv_bf3", 8, 6, "B_KN2", "bf16x3", 4),
    ("k_conv_bf3", 4, 10, "B_KN2", "bf16x3", 2), ("k_conv_bf3", 2, 10, "B_KN2", "bf16x3", 2),
    ("k_conv_bf3", 6, 2, "B_KN4", "bf16x3", 2), ("k_conv_bf3", 4, 4, "B_KN4", "bf16x3", 4), ("k_conv_bf3", 4, 4, "B_KN4", "bf16x3", 2), ("k_conv_bf3", 8, 6, "B_KN4", "bf16x3", 4),
    ("k_conv_bf3", 4, 10, "B_KN4", "bf16x3", 2), ("k_conv_bf3", 2, 10, "B_KN4", "bf16x3", 2),
    ("k_conv1x1_stream", None, None, "B_NK", "bf16x3", None), ("k_conv1x1_stream", None, None, "B_KN4", "bf16x3", None),
}


# ------------------------------------------------------------------ b: the case table
def C(name, B, Hi, Wi, ksize, stride, cin, cout, kind, gran=1, res=None, scale=True, relu=1, ps=False, colsum=False, fmt=0, tab16=None):
    """res: None | "sep" (its own buffer, ldr = cout + 8) | "inplace" (the output buffer itself); tab16: a 16-row shift table (default: every 3x3)."""
    return dict(name=name, B=B, Hi=Hi, Wi=Wi, ksize=ksize, stride=stride, cin=cin, cout=cout, kind=kind, gran=gran, res=res, scale=scale,
                relu=relu, ps=ps, colsum=colsum, fmt=fmt, tab16=(ksize == 3) if tab16 is None else tab16)


# Tiles follow from cout and Ho * Wo alone: cout <= 64 -> 6 x 2; 96 .. 128 -> 4 x 4; 160 .. 192 -> 8 x 6 (up to 128 rows, up to 256 with an
# output list); >= 224 with <= 128 rows -> 4 x 10, with <= 64 rows 2 x 10 in bf16x3; the streaming kernel: cout 256 | 384, >= 96 rows.
CASES = [
    # ---- no input list: B_NK (dense 1x1 / 3x3, output list 1x1)
    C("nk62", 3, 9, 20, 1, 1, 40, 64, "dense", res="sep", colsum=True, tab16=True),       # wider than high; 180 rows: the last colsum run holds 20; two K chunks + tail; a 1x1 handed a 16-row table
    C("nk44", 4, 20, 9, 3, 1, 32, 128, "dense", relu=0, ps=True),                         # higher than wide; 4 x 4 without a residual
    C("nk44r", 4, 13, 21, 1, 2, 32, 96, "dense", res="inplace", scale=False, colsum=True),  # 1x1 stride 2 from an odd map (7 x 11); 4 x 4 with a residual, in place
    C("nk86", 4, 10, 13, 1, 1, 32, 192, "n", gran=1, ps=True),                            # 130 rows with an output list: 8 x 6
    C("nk410", 3, 18, 24, 3, 2, 16, 224, "dense", scale=False, relu=0),                   # 3x3 stride 2 from an even map (9 x 12 = 108 rows)
    C("nk410s", 4, 10, 10, 1, 1, 32, 256, "dense", res="sep", ps=True),                   # scale AND residual: not the streaming kernel
    C("nk95", 3, 5, 19, 1, 1, 32, 256, "dense", relu=0),                                  # 95 rows: one short of the streaming kernel
    C("nk210", 9, 3, 5, 1, 1, 72, 256, "dense", res="sep", scale=False, colsum=True),     # a map under 32 pixels, B = 9 (grid padded to 8); three K chunks + tail
    # ---- the streaming kernel (bf16x3; fp32 runs the same launches on 4 x 10 / 4 x 4)
    C("st100", 4, 10, 10, 1, 1, 32, 256, "dense", ps=True),                               # 100 rows: its row minimum region
    C("st130", 3, 20, 26, 1, 2, 40, 256, "dense", res="sep", scale=False, colsum=True),   # stride 2 onto 10 x 13: the second 128-row block holds 2 rows; K tail
    C("st180", 3, 9, 20, 1, 1, 64, 384, "dense", res="inplace", scale=False, relu=0),     # three N tiles, two row blocks, in place
    C("st_k", 5, 10, 10, 1, 1, 64, 256, "k", gran=2, res="sep", scale=False, colsum=True),  # with an input list: B_KN4
    # ---- an input list alone: B_KN4 whatever the granularity
    C("k62", 4, 1, 7, 1, 1, 64, 64, "k", gran=1, res="sep"),                              # 1 x 7
    C("k44", 4, 7, 1, 3, 1, 32, 128, "k", gran=2, ps=True),                               # 7 x 1: every pixel in the left AND the right class
    C("k410", 4, 14, 22, 1, 2, 32, 224, "k", gran=2, res="inplace", scale=False),         # 1x1 stride 2 from an even map (7 x 11)
    C("k210", 4, 1, 1, 3, 1, 40, 256, "k", gran=1, relu=0),                               # 1 x 1: class 15, one tap inside; K tail with a list
    # ---- both lists (3x3): B_KN<granularity>
    C("kn4_86", 4, 9, 20, 3, 1, 32, 192, "kn", gran=4, ps=True),                          # granularity 4: B_KN4 on 8 x 6
    C("kn2_62", 4, 3, 5, 3, 1, 32, 64, "kn", gran=2, ps=True),
    C("kn2_44", 3, 19, 13, 3, 2, 32, 128, "kn", gran=2, scale=False),                     # 3x3 stride 2 from an odd map (10 x 7)
    C("kn2_86", 4, 9, 12, 3, 1, 16, 160, "kn", gran=2, relu=0),
    C("kn2_410", 3, 10, 10, 3, 1, 16, 256, "kn", gran=2, ps=True),
    C("kn2_210", 4, 5, 9, 3, 1, 16, 224, "kn", gran=2),
    C("kn1_62", 4, 5, 3, 3, 1, 24, 32, "kn", gran=1),
    C("kn1_44", 4, 12, 8, 3, 2, 32, 96, "kn", gran=1, ps=True),                           # 3x3 stride 2 from an even map (6 x 4)
    C("kn1_86", 3, 13, 10, 3, 1, 16, 192, "kn", gran=1, scale=False, ps=True),            # 130 rows: 8 x 6 through the output list
    C("kn1_410", 4, 7, 11, 3, 1, 16, 224, "kn", gran=1, relu=0),
    C("kn1_210", 4, 7, 1, 3, 1, 24, 256, "kn", gran=1, ps=True),
    # ---- out_format 1 (bf16x3 only; fp32 must refuse): with an output list at 6 x 2, 4 x 4, 8 x 6, and the output-dense launch that the
    #      dispatch used to hand to the streaming kernel, whose epilogue stores fp32
    C("ps62", 4, 9, 20, 1, 1, 32, 64, "n", gran=2, ps=True, fmt=1),
    C("ps44", 3, 7, 11, 1, 1, 40, 128, "n", gran=1, ps=True, fmt=1),
    C("ps86", 4, 10, 13, 1, 1, 32, 192, "n", gran=2, fmt=1),
    C("ps_dense", 4, 10, 10, 1, 1, 32, 256, "dense", ps=True, fmt=1),
    # ---- (last, so that the cases above keep their seeds) an input list alone WITH a residual on 4 x 4: the 2 x 2 wave grid of B_KN4
    C("k44r", 4, 6, 11, 1, 1, 32, 128, "k", gran=2, res="sep", scale=False),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_kw(c):
    Ho, Wo = R.out_hw(c["Hi"], c["Wi"], c["stride"])
    return launch_kw(c["kind"], c["ksize"] ** 2, Ho * Wo, c["cin"], c["cout"], c["gran"], c["res"] is not None, c["scale"],
                     16 if c["tab16"] else 1, c["fmt"] == 1)


def case_modes(c):
    return ("bf16x3",) if c["fmt"] == 1 else MATHS          # out_format 1 is refused in fp32: nothing runs


def test_case_table_reaches_every_variant():
    """The set of variants the case table runs equals what the enumeration of the dispatch rule finds (REACHABLE is that set written out) --
    and, branch by branch: every tile shape and staging mode per arithmetic mode, 4 x 4 with and without a residual, the streaming kernel with
    both weight layouts, and the launches that must NOT take it."""
    assert reachable_variants() == REACHABLE and len(REACHABLE) == 16 + 24
    seen, detail = set(), {}
    conv_plan.plans([dict(case_kw(c), math=math) for c in CASES for math in case_modes(c)])      # (one run of the chooser for all)
    for c in CASES:
        for math in case_modes(c):
            v = expected_variant(math=math, **case_kw(c))
            seen.add(v + (math, expected_wave_rows(math=math, **case_kw(c))))
            detail.setdefault((v, math, c["res"] is not None), c["name"])
    assert seen == REACHABLE, f"missing {sorted(map(str, REACHABLE - seen))}, unexpected {sorted(map(str, seen - REACHABLE))}"
    shapes = {m: {(k[0][1], k[0][2]) for k in detail if k[1] == m and k[0][1] is not None} for m in MATHS}
    assert shapes["fp32"] == {(6, 2), (4, 4), (8, 6), (4, 10)}
    assert shapes["bf16x3"] == {(6, 2), (4, 4), (8, 6), (4, 10), (2, 10)}
    for math in MATHS:
        modes = {k[0][3] for k in detail if k[1] == math and k[0][0] != "k_conv1x1_stream"}
        assert modes == {"B_NK", "B_KN1", "B_KN2", "B_KN4"}, (math, modes)
        four = {k[2] for k in detail if k[1] == math and (k[0][1], k[0][2]) == (4, 4)}
        assert four == {False, True}, f"{math}: the 4 x 4 tile must run with and without a residual"
    waves = {expected_wave_rows(math="bf16x3", **case_kw(BY_NAME[name])) for k, name in detail.items() if k[1] == "bf16x3" and (k[0][1], k[0][2]) == (4, 4)}
    assert waves == {4, 2}
    stream = {k[0][3] for k in detail if k[0][0] == "k_conv1x1_stream"}
    assert stream == {"B_NK", "B_KN4"}
    variant = lambda name, math="bf16x3", **over: expected_variant(math=math, **dict(case_kw(BY_NAME[name]), **over))
    for name in ("st100", "st130", "st180", "st_k"):
        assert variant(name)[0] == "k_conv1x1_stream" and variant(name, "fp32")[0] == "k_conv_image"
    assert case_kw(BY_NAME["st100"])["rows_per_image"] == 100 and variant("st100", rows_per_image=95) == ("k_conv_bf3", 4, 10, "B_NK")
    assert case_kw(BY_NAME["nk95"])["rows_per_image"] == 95 and variant("nk95") == ("k_conv_bf3", 4, 10, "B_NK")
    assert variant("nk95", rows_per_image=96)[0] == "k_conv1x1_stream"
    kw = case_kw(BY_NAME["nk410s"])
    assert kw["residual"] and kw["scale"] and variant("nk410s") == ("k_conv_bf3", 4, 10, "B_NK")
    assert variant("nk410s", scale=False)[0] == "k_conv1x1_stream"
    # the pre-split output of an output-dense launch stays with k_conv_bf3, whose epilogue writes it
    assert variant("ps_dense") == ("k_conv_bf3", 4, 10, "B_NK") and variant("ps_dense", out_split=False)[0] == "k_conv1x1_stream"
    assert {case_kw(c)["rows_per_image"] for c in CASES if c["name"].startswith("st")} == {100, 130, 180}
    assert BY_NAME["st130"]["stride"] == 2 and (BY_NAME["st130"]["Hi"], BY_NAME["st130"]["Wi"]) == (20, 26)
    # out_format 1 with an output list at 6 x 2, 4 x 4 and 8 x 6
    assert {variant(n)[1:3] for n in ("ps62", "ps44", "ps86")} == {(6, 2), (4, 4), (8, 6)}


def test_case_table_covers_the_maps_and_terms():
    """The maps, batch sizes, K extents and optional terms section b promises, so that an edit of the table cannot silently lose one."""
    maps = {(c["Hi"], c["Wi"], c["stride"], c["ksize"]) for c in CASES}
    out = {R.out_hw(c["Hi"], c["Wi"], c["stride"]) for c in CASES}
    assert all(h != w or (h, w) in ((1, 1), (10, 10)) for h, w in out)
    assert any(h < w for h, w in out) and any(h > w for h, w in out) and {(9, 20), (20, 9), (3, 5), (1, 7), (7, 1), (1, 1)} <= {m[:2] for m in maps}
    assert any(h * w % 32 for h, w in out) and any(h * w < 32 for h, w in out)
    assert all(h <= 20 and w <= 26 for h, w, _, _ in maps)
    for ksize in (1, 3):
        assert any(m[2] == 2 and m[3] == ksize and m[0] % 2 == 1 and m[1] % 2 == 1 for m in maps), f"{ksize}x{ksize} stride 2 from an odd map"
        assert any(m[2] == 2 and m[3] == ksize and m[0] % 2 == 0 and m[1] % 2 == 0 for m in maps), f"{ksize}x{ksize} stride 2 from an even map"
    assert all(3 <= c["B"] <= 5 or c["B"] == 9 for c in CASES) and sum(c["B"] == 9 for c in CASES) == 1
    assert {(c["kind"], c["ksize"]) for c in CASES} == {(k, 1 if t == 1 else 3) for k, t in LAUNCH_KINDS}
    by_kernel = {}
    for c in CASES:
        for math in case_modes(c):
            by_kernel.setdefault(expected_variant(math=math, **case_kw(c))[0], []).append(c)
    assert set(by_kernel) == {"k_conv_image", "k_conv_bf3", "k_conv1x1_stream"}
    for kernel, cs in by_kernel.items():
        assert all(c["cin"] <= 64 or c["cin"] in (40, 72) for c in cs)
        assert any(c["cin"] in (40, 72) and c["kind"] == "dense" for c in cs), f"{kernel}: more than one K chunk and a K tail"
        assert any(c["res"] == "inplace" for c in cs) and any(c["res"] == "sep" for c in cs), kernel
        assert {c["scale"] for c in cs} == {True, False} and {c["relu"] for c in cs} == {0, 1} and {c["ps"] for c in cs} == {True, False}, kernel
        with_sum = [R.out_hw(c["Hi"], c["Wi"], c["stride"]) for c in cs if c["colsum"]]
        assert with_sum and any(h * w % 32 for h, w in with_sum), f"{kernel}: colsum, on a map whose last run is partial"
    assert all(c["tab16"] for c in CASES if c["ksize"] == 3) and sum(c["tab16"] and c["ksize"] == 1 for c in CASES) == 1
    assert all(c["kind"] in ("dense", "k") for c in CASES if c["res"] or c["colsum"])      # (the entry point refuses them with an output list)


# ------------------------------------------------------------------ the channel lists: forced by construction, asserted on the CPU
def channel_list(B, channels, gran, seed):
    """(idx [B, channels] int32 left-packed ascending in runs of `gran`, cnt [B] int32): image 0 no channel, image 1 every channel,
    Bernoulli draws of whole groups elsewhere -- the first of the seeds seed, seed + 1000, ... whose draw is neither empty nor full and,
    with granularity 1 / 2, has a count that is not a multiple of 4 (check_list_preconditions asserts all of it)."""
    while True:
        gm = seeded_bernoulli((B, channels // gran), 0.6, seed)
        gm[0] = 0.0
        gm[1] = 1.0
        keep = gm.repeat_interleave(gran, dim=1) > 0.5
        n = keep.sum(dim=1)
        if bool(((n[2:] > 0) & (n[2:] < channels)).all()) and (gran == 4 or bool((n % 4 != 0).any())):
            break
        seed += 1000
    idx = torch.zeros(B, channels, dtype=torch.int32)
    for b in range(B):
        ch = torch.nonzero(keep[b]).reshape(-1).to(torch.int32)
        idx[b, :len(ch)] = ch
    return idx, n.to(torch.int32)


def case_lists(c):
    """(k_idx, k_cnt, n_idx, n_cnt) of a case on the CPU; None where its kind has no such list."""
    i = CASES.index(c)
    has_k, has_n = KINDS[c["kind"]]
    k = channel_list(c["B"], c["cin"], c["gran"], 300 + i) if has_k else (None, None)
    n = channel_list(c["B"], c["cout"], c["gran"], 400 + i) if has_n else (None, None)
    return k + n


def check_list_preconditions(c, idx, cnt, channels):
    B, gran = c["B"], c["gran"]
    assert idx.dtype == torch.int32 and cnt.dtype == torch.int32 and tuple(idx.shape) == (B, channels)
    n = cnt.tolist()
    assert n[0] == 0 and n[1] == channels, "image 0 without a channel, image 1 with all of them"
    assert all(0 < n[b] < channels for b in range(2, B)), "the other images' lists are real draws"
    for b in range(B):
        ch = idx[b, :n[b]].long()
        assert n[b] % gran == 0 and bool((ch[1:] > ch[:-1]).all()), "ascending, whole groups"
        runs = ch.view(-1, gran)
        assert bool((runs[:, 0] % gran == 0).all()) and bool((runs == runs[:, :1] + torch.arange(gran)).all()), "aligned runs of consecutive channels"
    if gran in (1, 2):
        assert any(v % 4 for v in n), "granularity 1 / 2: a count that is not a multiple of 4 (zero columns up to the next multiple of 4)"


@pytest.mark.parametrize("c", [c for c in CASES if c["kind"] != "dense"], ids=lambda c: c["name"])
def test_case_lists_hold_their_preconditions(c):
    k_idx, k_cnt, n_idx, n_cnt = case_lists(c)
    assert (k_idx is not None) == KINDS[c["kind"]][0] and (n_idx is not None) == KINDS[c["kind"]][1]
    if k_idx is not None:
        check_list_preconditions(c, k_idx, k_cnt, c["cin"])
        assert c["cin"] % 8 == 0
    if n_idx is not None:
        check_list_preconditions(c, n_idx, n_cnt, c["cout"])


# ------------------------------------------------------------------ inputs and the float64 reference of a case (computed once, never modified)
@functools.lru_cache(maxsize=None)
def _case_reference(name):
    c = BY_NAME[name]
    i = CASES.index(c)
    B, Hi, Wi, cin, cout, T = c["B"], c["Hi"], c["Wi"], c["cin"], c["cout"], c["ksize"] ** 2
    Ho, Wo = R.out_hw(Hi, Wi, c["stride"])
    k_idx, k_cnt, n_idx, n_cnt = case_lists(c)
    x = F.relu(seeded_randn((B, Hi, Wi, cin), 100 + i))
    lda = cin + 8
    a = torch.full((B, Hi, Wi, lda), NAN)                       # what the contract does not name holds NaN
    if k_idx is None:
        a[..., :cin] = x
    else:
        for b in range(B):
            kb = int(k_cnt[b])
            a[b, :, :, :kb] = x[b][:, :, k_idx[b, :kb].long()]    # left-packed
            a[b, :, :, kb:R.round_up(kb, 4)] = 0.0                # as the producing conv leaves them
    w = seeded_randn((cout, T, cin), 200 + i) * (2.0 / (T * cin)) ** 0.5
    if k_idx is not None:
        w = w.permute(1, 2, 0).contiguous()                     # k-major
    g = torch.Generator().manual_seed(500 + i)
    scale = (torch.rand(cout, generator=g) + 0.5) if c["scale"] else None
    shift = torch.randn(16, cout, generator=g) * 0.5 if c["tab16"] else torch.randn(cout, generator=g) * 0.3
    ps = torch.rand(cout, generator=g) * 0.3 if c["ps"] else None
    res = torch.randn(B, Ho, Wo, cout, generator=g) if c["res"] else None
    out, colsum = R.conv_image_f64(a, w, scale, shift, cin=cin, cout=cout, ksize=c["ksize"], stride=c["stride"], k_idx=k_idx, k_cnt=k_cnt,
                                   n_idx=n_idx, n_cnt=n_cnt, post_sub=ps, relu=c["relu"], residual=res, out_format=c["fmt"],
                                   want_colsum=c["colsum"])
    atol = 1e-4 if (T == 1 and res is None) else 2e-4
    sum_bound = None
    if c["colsum"]:                                             # a slot's bound: the element bound summed over its run of <= 32 pixels
        runs = colsum.shape[1]
        eb = torch.zeros(B, runs * 32, cout, dtype=torch.float64)
        eb[:, :Ho * Wo] = (atol + 1e-4 * out.abs()).reshape(B, Ho * Wo, cout)
        sum_bound = eb.reshape(B, runs, 32, cout).sum(dim=2)
    return dict(a=a, w=w, scale=scale, shift=shift, ps=ps, res=res, k_idx=k_idx, k_cnt=k_cnt, n_idx=n_idx, n_cnt=n_cnt, out=out, colsum=colsum,
                sum_bound=sum_bound, atol=atol, Ho=Ho, Wo=Wo)


def _d(t):
    return None if t is None else t.to(DEV)


def _untouched(t):
    """Every word still holds the NaN it was filled with (also true of a pre-split buffer: an fp32 NaN is not a pair the kernel writes)."""
    return bool(torch.isnan(t).all())


# ------------------------------------------------------------------ c: every case, against float64
@gpu
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_conv_image_case_vs_float64(ops, name, math_mode):
    from laudnet_amd import LdnError
    c, ref = BY_NAME[name], _case_reference(name)
    B, cout, Ho, Wo, fmt = c["B"], c["cout"], ref["Ho"], ref["Wo"], c["fmt"]
    width = ref["out"].shape[-1]                                 # cout, or roundup32(cout) with out_format 1
    ldo = width + (32 if fmt == 1 else 4)
    out = torch.full((B, Ho, Wo, ldo), NAN, device=DEV)
    res_d = None
    if c["res"] == "sep":
        res_cpu = torch.full((B, Ho, Wo, cout + 8), NAN)
        res_cpu[..., :cout] = ref["res"]
        res_d = res_cpu.to(DEV)
    elif c["res"] == "inplace":
        out[..., :cout] = ref["res"].to(DEV)
        res_d = out
    colsum = torch.full(tuple(ref["colsum"].shape), NAN, device=DEV) if c["colsum"] else None
    call = lambda: ops.conv_image(_d(ref["a"]), _d(ref["w"]), _d(ref["scale"]), _d(ref["shift"]), out, ksize=c["ksize"], stride=c["stride"],
                                  k_idx=_d(ref["k_idx"]), k_cnt=_d(ref["k_cnt"]), kgran=c["gran"], n_idx=_d(ref["n_idx"]), n_cnt=_d(ref["n_cnt"]),
                                  post_sub=_d(ref["ps"]), relu=c["relu"], residual=res_d, colsum=colsum, out_split=fmt == 1)
    if fmt == 1 and math_mode == "fp32":
        with pytest.raises(LdnError):                            # out_format 1 is bf16x3 arithmetic only: an error, before any launch
            call()
        torch.cuda.synchronize()
        assert _untouched(out), "a refused call must not launch"
        return
    call()
    torch.cuda.synchronize()
    raw = out.cpu()
    assert _untouched(raw[..., width:]), f"columns [{width}, {ldo}) of the output rows were written"
    got = R.decode_split(raw[..., :width]) if fmt == 1 else raw[..., :cout]
    want = ref["out"]
    n_cnt = ref["n_cnt"].tolist() if ref["n_cnt"] is not None else [cout] * B
    worst = 0.0
    for b in range(B):
        n = n_cnt[b]
        worst = max(worst, assert_close(got[b, :, :, :n], want[b, :, :, :n], ref["atol"], 1e-4, f"{name} {math_mode} image {b} ({n} columns)"))
        zero_to = min(R.round_up(n, 32 if fmt == 1 else 4), width)
        assert not bool(torch.isnan(want[b, :, :, n:zero_to]).any()) and bool((got[b, :, :, n:zero_to] == 0).all()), \
            f"{name} image {b}: columns {n}..{zero_to - 1} must be exactly 0"
    if c["res"] == "sep":
        assert torch.equal(res_d.cpu().view(torch.int32), res_cpu.view(torch.int32)), "the out-of-place form must leave the residual alone"
    serr = 0.0
    if c["colsum"]:
        cs = colsum.cpu().double()
        assert not bool(torch.isnan(cs).any()), "a colsum slot was not written"
        excess = (cs - ref["colsum"]).abs() - ref["sum_bound"]
        serr = (cs - ref["colsum"]).abs().max().item()
        at = tuple(int(v) for v in torch.unravel_index(excess.argmax(), excess.shape))
        assert excess.max().item() <= 0, f"{name} colsum: |err| {abs(cs[at] - ref['colsum'][at]).item():.3e} at {at} exceeds the summed element bound {ref['sum_bound'][at].item():.3e}"
    print(f"[conv_image] {name} {math_mode} {expected_variant(math=math_mode, **case_kw(c))}: max |err| {worst:.2e} colsum {serr:.2e}")


# ------------------------------------------------------------------ d: the argument checks
@gpu
def test_argument_checks_refuse_before_any_launch(ops):
    """The checks of ldn_conv_image (csrc/ldn_conv_image.hip, ldn_conv_image): an error code, and neither the output nor colsum is touched."""
    from laudnet_amd import LdnError
    B, Hi, Wi, cin, cout = 2, 4, 6, 32, 32
    a = torch.zeros(B, Hi, Wi, cin, device=DEV)
    w = torch.zeros(cout, 1, cin, device=DEV)
    w9 = torch.zeros(cout, 9, cin, device=DEV)
    sh = torch.zeros(cout, device=DEV)
    out = torch.full((B, Hi, Wi, cout), NAN, device=DEV)
    colsum = torch.full((B, 1, cout), NAN, device=DEV)
    lists = torch.arange(cout, dtype=torch.int32, device=DEV).repeat(B, 1).contiguous()
    counts = torch.full((B,), cout, dtype=torch.int32, device=DEV)
    for shape in ((B, Hi + 1, Wi, cout), (B, Hi, Wi + 1, cout)):       # Ho / Wo beyond the input grid
        tall = torch.full(shape, NAN, device=DEV)
        with pytest.raises(LdnError):
            ops.conv_image(a, w, None, sh, tall)
        with pytest.raises(LdnError):
            ops.conv_image(a, w9, None, sh, tall, ksize=3)
        assert _untouched(tall)
    half = torch.full((B, Hi, Wi // 2 + 1, cout), NAN, device=DEV)     # stride 2: Wo = 4 needs input column 6
    with pytest.raises(LdnError):
        ops.conv_image(a, w, None, sh, half, stride=2)
    with pytest.raises(LdnError):      # colsum with an output-channel list
        ops.conv_image(a, w, None, sh, out, n_idx=lists, n_cnt=counts, colsum=colsum)
    with pytest.raises(LdnError):      # a residual with an output-channel list
        ops.conv_image(a, w, None, sh, out, n_idx=lists, n_cnt=counts, residual=out)
    with pytest.raises(LdnError):      # ldo < cout
        ops.conv_image(a, w, None, sh, torch.full((B, Hi, Wi, cout - 4), NAN, device=DEV))
    with pytest.raises(LdnError):      # out_format 1 with a residual
        ops.conv_image(a, w, None, sh, out, residual=out, math="bf16x3", out_split=True)
    with pytest.raises(LdnError):      # out_format 1 in fp32 arithmetic
        ops.conv_image(a, w, None, sh, out, math="fp32", out_split=True)
    with pytest.raises(LdnError):      # a 3-class shift table
        ops.conv_image(a, w9, None, torch.zeros(3, cout, device=DEV), out, ksize=3)
    torch.cuda.synchronize()
    assert _untouched(out) and _untouched(half) and _untouched(colsum), "a refused call must not launch"
