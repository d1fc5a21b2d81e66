"""The chooser of k_conv_image / k_conv_bf3 / k_conv1x1_stream (laudnet_amd/csrc/ldn_conv_plan.h) on the CPU: tests/conv_plan_cli.cpp,
compiled with the host compiler (tests/conv_plan.py), runs conv_plan() and the list of built kernels (LDN_CONV_KERNELS) without HIP.  No GPU."""
import os
import subprocess

import conv_plan as P

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "golden", "conv_plan_pins.txt")


def test_every_plan_is_a_built_kernel_with_sound_geometry_and_every_built_kernel_is_chosen():
    """Over the sweep grid (packed and image x both arithmetic modes x 1 / 9 taps x 1 / 16 shift classes x the four list kinds x granularity
    1 / 2 / 4 x residual none / with / without scale x out_split x LDN_STREAM_ROWS 0 / 128 / 512 / 1024 x B 1 / 8 / 9 / 256 x 20 row counts
    on both sides of 32 | 64 | 96 | 128 | 256 x 18 widths on both sides of 64 | 128 | 192 | 256, ragged ones among them x 8 input widths up to
    what the LDS and the 32-bit weight offsets refuse; without what the entry points refuse whatever the sizes): the chooser never names a
    kernel that is not built -- the launcher would refuse it --, the list holds no kernel twice and none that the chooser never names, and
    for every admitted shape the block never exceeds its tile (bn <= NS * 32, bm <= MS * 32, whole subtiles of 32; the streaming kernel:
    whole M blocks of ST_BM, at most ST_MAXROWS rows), the blocks cover the rows and the columns, the grid is the padded product and fits
    32 bits, and the LDS fits a CU."""
    r = subprocess.run([P.cli(), "sweep"], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    unbuilt = [ln for ln in lines if ln.startswith("UNBUILT")]
    assert not unbuilt, f"{len(unbuilt)} plans name a kernel that is not built, e.g. {unbuilt[:3]}"
    bad = [ln for ln in lines if ln.startswith("BAD")]
    assert not bad, f"{len(bad)} admitted shapes break a geometry invariant, e.g. {bad[:3]}"
    total = dict(zip(lines[-1].split()[::2], map(int, lines[-1].split()[1::2])))
    rows = dict(ln.rsplit(" ", 1) for ln in lines if ln.startswith("k_conv"))
    assert len(rows) == total["rows"] == total["distinct"] == 16 + 22 + 2, f"LDN_CONV_KERNELS lists a kernel twice, or not the 40: {lines[-1]}"
    dead = [k for k, n in rows.items() if int(n) == 0]
    assert not dead, f"built but never chosen: {dead}"
    assert total["cases"] > 5000000 and total["cases"] > total["admitted"] > 4000000, lines[-1]      # (some shapes are refused: the LDS, the weight offsets)
    assert total["unbuilt"] == total["unreached"] == total["bad"] == 0 and r.returncode == 0, lines[-1]
    # the widest input an input-channel list fits the LDS with, per tile shape: image 1x1 | packed 3x3 with a 16-class table
    maxcin = {ln.split()[1]: tuple(map(int, ln.split()[2:])) for ln in lines if ln.startswith("maxcin")}
    print(maxcin)
    assert maxcin == {"6x2": (23936, 21056), "4x4": (23808, 20608), "8x6": (11008, 5568), "4x10": (10752, 4672), "2x10": (14976, 9536)}


def test_the_rows_a_residual_cannot_reach_are_not_built():
    """k_conv_bf3<4, 4, 2> runs behind a residual only, B_KN2 / B_KN1 with both channel lists only, and both entry points refuse a residual
    with an output list: the chooser does name those two kernels for such a shape, and the list does not hold them."""
    kw = dict(packed=False, math="bf16x3", rows_per_image=196, taps=9, cin=128, cout=128, has_k=True, has_n=True, shift_classes=16,
              residual=True, scale=False)
    got = P.run([P.shape_line(kgran=g, **kw) for g in (1, 2, 4)])
    assert [ln.split()[15] for ln in got] == ["k_conv_bf3<4,4,2,B_KN1>", "k_conv_bf3<4,4,2,B_KN2>", "k_conv_bf3<4,4,2,B_KN4>"]
    assert [ln.endswith(" UNBUILT") for ln in got] == [True, True, False]


def test_chooser_matches_the_pinned_model_shapes():
    """The pin file records the whole plan -- kernel, bn, ntn, bm, mtn, grid, LDS -- for every shape the shipped models issue; any change fails here."""
    want = open(PINS).read().splitlines()
    shapes = [ln if ln.startswith("#") else " ".join(ln.split()[:15]) for ln in want]
    got = P.run(shapes)
    assert sum(not ln.startswith("#") for ln in want) >= 300
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, f"{len(diff)} pinned plans changed, e.g. {diff[:3]}"
    kernels = {ln.split()[15] for ln in want if not ln.startswith("#")}
    assert {k.split("<")[0] for k in kernels} == {"k_conv_image", "k_conv_bf3", "k_conv1x1_stream"}


def test_both_sides_of_every_threshold_of_the_rules():
    """The rules of conv_plan(), threshold by threshold, on the shape to either side: the widths 64 | 96 | 128 | 160 (N subtiles per block), the
    row counts 128 | 129 (wide N blocks) and 256 | 257 (whole 14 x 14 images behind an output list), 64 | 65 rows (the 2 x 10 tile of bf16x3), the
    residual of the 4 x 4 tile, the staging mode by list kind and granularity, and every term of the streaming kernel's predicate."""
    base = dict(packed=False, rows_per_image=3136, taps=1, cin=64, cout=256, has_k=False, has_n=False, kgran=1, shift_classes=1, residual=False,
                scale=True)
    table = [      # (math, overrides, kernel)
        ("fp32", dict(cout=64), "k_conv_image<6,2,B_NK>"), ("fp32", dict(cout=68), "k_conv_image<4,4,B_NK>"),
        ("fp32", dict(cout=128), "k_conv_image<4,4,B_NK>"), ("fp32", dict(cout=132), "k_conv_image<4,4,B_NK>"),
        ("fp32", dict(cout=320, rows_per_image=128), "k_conv_image<4,10,B_NK>"), ("fp32", dict(cout=320, rows_per_image=129), "k_conv_image<4,4,B_NK>"),
        ("fp32", dict(cout=160, rows_per_image=128), "k_conv_image<8,6,B_NK>"), ("fp32", dict(cout=224, rows_per_image=128), "k_conv_image<4,10,B_NK>"),
        ("fp32", dict(cout=320, rows_per_image=256, has_n=True), "k_conv_image<8,6,B_NK>"),
        ("fp32", dict(cout=320, rows_per_image=257, has_n=True), "k_conv_image<4,4,B_NK>"),
        ("fp32", dict(cout=320, rows_per_image=256), "k_conv_image<4,4,B_NK>"),
        ("bf16x3", dict(cout=320, rows_per_image=64), "k_conv_bf3<2,10,2,B_NK>"), ("bf16x3", dict(cout=320, rows_per_image=65), "k_conv_bf3<4,10,2,B_NK>"),
        ("fp32", dict(cout=320, rows_per_image=64), "k_conv_image<4,10,B_NK>"),
        ("bf16x3", dict(cout=128), "k_conv_bf3<4,4,4,B_NK>"), ("bf16x3", dict(cout=128, residual=True), "k_conv_bf3<4,4,2,B_NK>"),
        ("bf16x3", dict(cout=64, residual=True), "k_conv_bf3<6,2,2,B_NK>"), ("bf16x3", dict(cout=192, rows_per_image=100), "k_conv_bf3<8,6,4,B_NK>"),
        # the staging mode: no input list B_NK; an input list alone B_KN4 whatever the granularity; both lists by granularity
        ("fp32", dict(cout=128, has_n=True, kgran=1), "k_conv_image<4,4,B_NK>"), ("fp32", dict(cout=128, has_k=True, kgran=1), "k_conv_image<4,4,B_KN4>"),
        ("fp32", dict(cout=128, has_k=True, has_n=True, kgran=1), "k_conv_image<4,4,B_KN1>"),
        ("fp32", dict(cout=128, has_k=True, has_n=True, kgran=2), "k_conv_image<4,4,B_KN2>"),
        ("fp32", dict(cout=128, has_k=True, has_n=True, kgran=4), "k_conv_image<4,4,B_KN4>"),
        ("fp32", dict(cout=128, has_k=True, has_n=True, kgran=6), "k_conv_image<4,4,B_KN2>"),
        ("fp32", dict(cout=128, has_k=True, has_n=True, kgran=8), "k_conv_image<4,4,B_KN4>"),
        # the streaming kernel, and each term of its predicate alone
        ("bf16x3", dict(), "k_conv1x1_stream<B_NK>"), ("bf16x3", dict(has_k=True), "k_conv1x1_stream<B_KN4>"), ("fp32", dict(), "k_conv_image<4,4,B_NK>"),
        ("bf16x3", dict(rows_per_image=96), "k_conv1x1_stream<B_NK>"), ("bf16x3", dict(rows_per_image=95), "k_conv_bf3<4,10,2,B_NK>"),
        ("bf16x3", dict(cin=1024), "k_conv1x1_stream<B_NK>"), ("bf16x3", dict(cin=1032), "k_conv_bf3<4,4,4,B_NK>"),
        ("bf16x3", dict(cout=128), "k_conv_bf3<4,4,4,B_NK>"), ("bf16x3", dict(cout=320), "k_conv_bf3<4,4,4,B_NK>"), ("bf16x3", dict(cout=384), "k_conv1x1_stream<B_NK>"),
        ("bf16x3", dict(residual=True, scale=False), "k_conv1x1_stream<B_NK>"), ("bf16x3", dict(residual=True), "k_conv_bf3<4,4,2,B_NK>"),
        ("bf16x3", dict(has_n=True), "k_conv_bf3<4,4,4,B_NK>"), ("bf16x3", dict(shift_classes=16), "k_conv_bf3<4,4,4,B_NK>"),
        ("bf16x3", dict(out_split=True), "k_conv_bf3<4,4,4,B_NK>"), ("bf16x3", dict(taps=9), "k_conv_bf3<4,4,4,B_NK>"),
        ("bf16x3", dict(stream_rows=0), "k_conv_bf3<4,4,4,B_NK>"), ("bf16x3", dict(stream_rows=127), "k_conv_bf3<4,4,4,B_NK>"),
        ("bf16x3", dict(stream_rows=128), "k_conv1x1_stream<B_NK>"), ("bf16x3", dict(packed=True), "k_conv1x1_stream<B_NK>"),
    ]
    got = P.run([P.shape_line(math=m, **dict(base, **over)) for m, over, _ in table])
    wrong = [(m, over, want, ln.split()[15]) for (m, over, want), ln in zip(table, got) if ln.split()[15:16] != [want] or "UNBUILT" in ln or "REFUSED" in ln]
    assert not wrong, wrong


def test_geometry_of_hand_computed_launches():
    """bn ntn bm mtn grid lds_bytes of launches worked out by hand from the rules: the balanced M blocks (98 subtiles over 25 blocks of 4; 7 subtiles
    in one 8 x 6 block of 224 rows), the grid padded to the 8 XCDs (B = 9), the streaming kernel's rows per workgroup halved until 512 workgroups
    or 128 rows and its N tiles split while fewer than 512 workgroups, and the LDS with and without the input list and the packed row tables."""
    base = dict(packed=False, rows_per_image=3136, taps=1, cin=64, cout=256, has_k=False, has_n=False, kgran=1, shift_classes=1, residual=False,
                scale=True, B=256)
    lds44 = 2 * 8 * 32 * 32 * 4 + 3 * 128 * 4 + (2 * 128 + 128) * 4      # staging + scale / post_sub / one shift row + pixel, class and column tables
    lds86 = 2 * 14 * 32 * 32 * 4 + (2 + 16) * 192 * 4 + (2 * 256 + 192 + 64) * 4
    stream = (9 * 4096 + 2 * 1024 + 64 + 32) * 4
    table = [
        ("fp32", dict(), f"128 2 128 25 12800 {lds44}"),                                       # 98 subtiles: 25 blocks of 4 (the last holds 2)
        ("fp32", dict(B=9), f"128 2 128 25 464 {lds44}"),                                      # 9 x 25 = 225 units, padded to 232, x 2 N blocks
        ("fp32", dict(packed=True, has_k=True), f"128 2 128 25 12800 {lds44 + 64 * 4 + 128 * 2 * 4}"),   # + the input list + out row and A row per row
        ("fp32", dict(rows_per_image=196, cout=192, cin=64, has_k=True, has_n=True, taps=9, shift_classes=16), f"192 1 224 1 256 {lds86}"),
        ("bf16x3", dict(), f"2 1 512 7 1792 {stream}"),                                        # 256 x 7 blocks of 512 rows >= 512: no halving, no N split
        ("bf16x3", dict(B=1), f"1 2 128 25 50 {stream}"),                                      # 512 -> 256 -> 128 rows; 25 blocks x 2 N tiles, each its own
        ("bf16x3", dict(B=1, cout=2048, rows_per_image=100), f"1 16 128 1 16 {stream}"),       # one row block: the 16 N tiles all split
        ("bf16x3", dict(B=64, rows_per_image=520), f"1 2 128 5 640 {stream}"),                 # 64 x 2 and 64 x 3 blocks < 512: 128 rows, 5 blocks of ceil(104 / 128) x 128; 320 < 512: N split
    ]
    got = P.run([P.shape_line(math=m, **dict(base, **over)) for m, over, _ in table])
    print("\n".join(got))
    wrong = [(over, want, " ".join(ln.split()[16:22])) for (m, over, want), ln in zip(table, got) if " ".join(ln.split()[16:22]) != want or len(ln.split()) != 22]
    assert not wrong, wrong
