"""k_smallmap (csrc/ldn_small.hip: ldn_bottleneck_smallmap, a whole channel-mode bottleneck on a map of at most 64 pixels, one workgroup
per image) over every per-image ring geometry, against float64.

What a workgroup of k_smallmap does depends on its image's active-channel count Kb, not on the launch: the conv2 / conv3 ring geometry
(small_geom), conv1's ring depth and gathers, the per-wave subtile instantiation, the pipelined / single-slot bodies of conv2 and conv3
and conv3's `fast3` body.  tests/test_hip_small.py draws its masks at one keep rate per shape and reaches four of the twelve geometries.

`small_geom`, `small_fits` and `conv1_ring` restate the kernel's choices in Python and `image_class` names the path an image takes; non-GPU
tests compare `small_fits` with ldn_bottleneck_smallmap_fits over a grid and prove on the CPU that the case table below (counts FORCED per
image through mask_in) reaches every geometry -- the set is enumerated, not written down -- and every value of every other axis.

Per case the GPU test requires: out within 2e-4 + 1e-4 |ref| of the block's algebra in float64 (laud_resnet.py:115-144, mask before BN); the
float32 PyTorch block itself sits inside that bound (a non-GPU test: the bound is a condition on the seeds, never fitted to the kernel);
every element written and finite, NaN guards around out / colsum untouched bit for bit; colsum per pixel tile; an empty image exactly
relu(shift3 + residual); a second launch and the in-place launch bit-identical; agreement with ldn_bottleneck_head + ldn_bottleneck_tail
where those cover the shape.  The test prints each case's maximum |error| (kernel and float32 PyTorch against float64) and the class and
errors of every image (run with -s); the class table and the record of those figures: docs/lab_notebook.md."""
import collections
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fill import seeded_randn
from helpers import assert_close
from oracle import torch_ref as TR

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()  # raises if libldn_hip.so is missing -- no fallback
    return _ops


# ------------------------------------------------------------------ the per-image dispatch of k_smallmap, restated
S_LDS = 160 * 1024                   # csrc/ldn_small.hip:57
S_KIDX_BYTES = 2304                  # :63
S_ACT_OFF = S_KIDX_BYTES + 128       # :65
S_TAB1_BYTES = 3 * 512 * 4           # :66

Geom = collections.namedtuple("Geom", "act_bytes ring_off space w2row nks2 slot2 d2 d3")


def _round_up(a, b):
    return -(-a // b) * b


def _cdiv(a, b):
    """C's integer division (truncation towards zero): `space` may be negative for shapes that do not fit."""
    return abs(a) // b * (1 if a >= 0 else -1)


def small_geom(HW, nsub):
    """:145-157: the LDS geometry of an image with nsub K slices of 32 channels on a map of HW pixels."""
    act_bytes = nsub * HW * 128
    ring_off = S_ACT_OFF + act_bytes
    space = S_LDS - ring_off
    w2row = ((nsub + 3) // 4 if nsub > 0 else 1) * 1024
    slot32 = 16 * w2row
    if 3 * slot32 <= space:                          # K32 chunks when three of them fit ...
        nks2, slot2, d2 = 2, slot32, min(_cdiv(space, slot32), 3)
    else:                                            # ... else K16 chunks in a deeper ring
        nks2, slot2 = 1, 8 * w2row
        d2 = min(_cdiv(space, slot2), 4)
    d3 = min(_cdiv(space, 32768), 3)
    return Geom(act_bytes, ring_off, space, w2row, nks2, slot2, d2, d3)


def small_fits(HW, cin, width, cout):
    """:939-948 (ldn_bottleneck_smallmap_fits without its H, Wd >= 1 test)."""
    if HW < 1 or HW > 64 or width < 64 or width > 512 or width % 64 or cin < 32 or cin % 32 or cout < 128 or cout % 128:
        return False
    g = small_geom(HW, width // 32)
    if S_ACT_OFF + g.act_bytes > S_LDS - S_TAB1_BYTES:
        return False
    if g.space < 18 * width * 4:
        return False
    if g.d2 < 1 or g.d3 < 1:
        return False
    return 2 * (64 + width) * 128 <= S_LDS - S_ACT_OFF


def conv1_ring(Kb):
    """:245-248 -> (wrows, slot1, D, nw): conv1's ring slot holds 64 rows of x and the image's weight rows rounded up to 64; every wave
    stages nw pieces of 8 rows per chunk, the pieces beyond four with a second gather (:283)."""
    wrows = _round_up(Kb, 64)
    slot1 = (64 + wrows) * 128
    return wrows, slot1, min(4, (S_LDS - S_ACT_OFF) // slot1), wrows // 64


ImageClass = collections.namedtuple("ImageClass", "empty nks2 d2 d3 nf D1 nw nv last conv3 tiles kloop")


def image_class(HW, cin, width, cout, Kb):
    """The path of an image with Kb active channels (:205-207, 219, 245-248, 288, 410-422, 707-736).  An empty image runs neither conv1 nor
    conv2 (:238): its D1 / nw / nv are 0 and its K loop does not exist; conv3 still walks its groups (without chunks: never `fast`, :735)."""
    assert 0 <= Kb <= width and Kb % 2 == 0
    nsub = -(-Kb // 32)
    g = small_geom(HW, nsub)
    nf = g.w2row // 1024
    if g.d3 == 1:
        conv3 = "single"
    else:
        conv3 = "fast" if (cout % 512 == 0 and nsub > 0) else "general"
    tiles = "1" if HW <= 32 else ("2 full" if HW == 64 else "2 partial")
    if Kb == 0:
        return ImageClass(True, g.nks2, g.d2, g.d3, nf, 0, 0, 0, "none", conv3, tiles, "none")
    _, _, D1, nw = conv1_ring(Kb)
    return ImageClass(False, g.nks2, g.d2, g.d3, nf, D1, nw, min(nsub, 4), "whole" if Kb % 32 == 0 else "partial", conv3, tiles,
                      "short" if cin // 32 < D1 else "long")


def geometry(c):
    return (c.nks2, c.d2, c.d3, c.nf)


@functools.lru_cache(maxsize=None)
def reachable_geometries():
    """Every (nks2, d2, d3, nf) some non-empty image can have in a launch ldn_bottleneck_smallmap accepts (the geometry depends on the map
    and the count only; cin = cout = 4 * width is one shape per (map, width) that passes whenever any does)."""
    seen = set()
    for HW in range(1, 65):
        for width in range(64, 513, 64):
            if small_fits(HW, 4 * width, width, 4 * width):
                seen |= {geometry(image_class(HW, 4 * width, width, 4 * width, Kb)) for Kb in range(2, width + 1, 2)}
    return frozenset(seen)


# ------------------------------------------------------------------ the case table: counts are forced per image
Case = collections.namedtuple("Case", "H Wd cin width cout gran counts residual")     # residual: "x" (cin == cout), "other", "none"

PROD = (7, 7, 2048, 512, 2048, 2)
CASES = [
    # stage 4 of the ResNets, one image per nsub in 0..16 over the two launches, both sides of every multiple of 32 that changes a geometry
    Case(*PROD, (0, 2, 30, 32, 34, 62, 64, 66, 126, 128, 130, 160, 190, 224, 256, 258, 288), "x"),
    Case(*PROD, (320, 322, 352, 384, 386, 416, 448, 480, 482, 510, 512, 0, 96, 290, 200, 444, 2), "x"),
    # 64 pixels at width 448: (1,2,1,3) single-slot conv3, (1,2,2,3), (1,4,2,2)
    Case(8, 8, 1792, 448, 1792, 2, (0, 448, 418, 382, 350, 322, 256, 226, 2), "x"),
    # 33 pixels (one live lane in the second tile), a row and a column: every tap class is a border class; (1,3,3,4)
    Case(3, 11, 2048, 512, 2048, 4, (0, 512, 484, 452, 388, 36), "x"),
    Case(1, 33, 256, 64, 256, 2, (0, 64, 34, 2), "x"),
    Case(33, 1, 512, 128, 640, 2, (0, 128, 98, 30), "other"),
    # one pixel and 16 pixels at width 512: (1,4,3,4), (2,3,3,3)
    Case(1, 1, 2048, 512, 2048, 2, (0, 512, 450, 386, 382, 258, 130, 2), "x"),
    Case(4, 4, 2048, 512, 2048, 2, (0, 512, 482, 386, 322, 66), "x"),
    # a K loop shorter than conv1's ring: cin 32 (one chunk) and 64 (two chunks, rings of three and four)
    Case(7, 7, 32, 512, 128, 2, (0, 512, 386, 322, 258, 130, 62), "other"),
    Case(5, 9, 64, 256, 640, 2, (0, 256, 194, 130, 66, 2), "none"),
    # the general conv3 body with cin != cout at the production width; width 192 below 4 * width
    Case(7, 7, 1024, 512, 640, 2, (0, 512, 330, 290, 34), "other"),
    Case(6, 6, 768, 192, 128, 4, (0, 192, 100, 36), "none"),
]


def case_id(case):
    return f"c{CASES.index(case)}-" + "x".join(str(v) for v in case[:6]) + f"-{case.residual}-B{len(case.counts)}"


def classes_of(case):
    return [image_class(case.H * case.Wd, case.cin, case.width, case.cout, Kb) for Kb in case.counts]


def _all_classes(cases):
    return [c for case in cases for c in classes_of(case)]


def table_gaps(cases):
    """What a case table leaves out, as a list of strings (empty: the table is complete).  (b) every reachable geometry, each with a
    partial last subtile; (c) every value of every other axis; (d) every nsub in 0..16 at the production shape."""
    cls = _all_classes(cases)
    live = [c for c in cls if not c.empty]
    gaps = []
    for g in sorted(reachable_geometries()):
        if not any(geometry(c) == g for c in live):
            gaps.append(f"geometry {g}")
        elif not any(geometry(c) == g and c.last == "partial" for c in live):
            gaps.append(f"geometry {g} with a partial last subtile")
    axes = {"D1": (2, 3, 4), "nw": tuple(range(1, 9)), "nv": (1, 2, 3, 4), "conv3": ("fast", "general", "single"),
            "tiles": ("1", "2 partial", "2 full"), "kloop": ("short", "long"), "last": ("whole", "partial")}
    for axis, values in axes.items():
        have = {getattr(c, axis) for c in live}
        gaps += [f"{axis} = {v}" for v in values if v not in have]
    if not any(c.empty for c in cls):
        gaps.append("an empty image")
    prod_nsub = {-(-Kb // 32) for case in cases if tuple(case[:6]) == PROD for Kb in case.counts}
    gaps += [f"nsub = {n} at the production shape" for n in range(17) if n not in prod_nsub]
    return gaps


def test_small_fits_restated_equals_the_library():
    """(a) The transcription against ldn_bottleneck_smallmap_fits (the library loads without a GPU)."""
    from laudnet_amd import ops
    fit = no = 0
    for HW in range(1, 66):
        for width in range(32, 577, 32):
            for cin in (32, 64, 2048):
                for cout in (128, 256, 640, 2048):
                    want = small_fits(HW, cin, width, cout)
                    assert ops.bottleneck_smallmap_fits(1, HW, cin, width, cout) == want, (HW, cin, width, cout)
                    fit += want
                    no += not want
    assert fit > 3000 and no > 3000
    for H, Wd in ((7, 7), (8, 8), (3, 11), (5, 13), (13, 5), (2, 32)):
        for width in (64, 448, 512):
            assert ops.bottleneck_smallmap_fits(H, Wd, 4 * width, width, 4 * width) == small_fits(H * Wd, 4 * width, width, 4 * width)
    assert not ops.bottleneck_smallmap_fits(0, 7, 2048, 512, 2048) and not ops.bottleneck_smallmap_fits(7, 0, 2048, 512, 2048)
    assert small_fits(49, 2048, 512, 2048) and small_fits(64, 1792, 448, 1792) and not small_fits(64, 2048, 512, 2048)
    for bad in ((49, 16, 512, 2048), (49, 48, 512, 2048), (49, 2048, 512, 64), (49, 2048, 512, 192), (49, 2048, 96, 384)):
        assert not small_fits(*bad)


def test_restated_rings_at_the_production_shape():
    """The values the source gives at 7x7, width 512, written out: the geometry per count (the ranges of the issue that asked for this
    file) and conv1's ring."""
    geo = lambda Kb: geometry(image_class(49, 2048, 512, 2048, Kb))
    assert [geo(k) for k in (2, 128, 130, 256)] == [(2, 3, 3, 1), (2, 3, 3, 1), (2, 3, 3, 2), (2, 3, 3, 2)]
    assert {geo(k) for k in range(258, 321, 2)} == {(1, 4, 3, 3)} and {geo(k) for k in range(322, 385, 2)} == {(1, 3, 2, 3)}
    assert {geo(k) for k in range(386, 481, 2)} == {(1, 2, 2, 4)} and {geo(k) for k in range(482, 513, 2)} == {(1, 1, 1, 4)}
    assert [conv1_ring(k)[2:] for k in (2, 192, 194, 320, 322, 512)] == [(4, 1), (4, 3), (3, 4), (3, 5), (2, 6), (2, 8)]
    assert len(reachable_geometries()) == 12


def test_case_table_is_complete():
    """(b) - (d): nothing is missing from the table, and every launch is one the library accepts."""
    assert table_gaps(CASES) == []
    for case in CASES:
        assert small_fits(case.H * case.Wd, case.cin, case.width, case.cout), case
        assert 1 <= len(case.counts) <= 17 and case.gran % 2 == 0 and case.width % case.gran == 0
        assert all(0 <= k <= case.width and k % case.gran == 0 for k in case.counts), case
        assert case.residual in ("x", "other", "none") and (case.residual != "x" or case.cin == case.cout)
    assert {(1, 1), (4, 4), (1, 33), (33, 1), (3, 11), (8, 8), (7, 7)} <= {(c.H, c.Wd) for c in CASES}
    assert {"x", "other", "none"} == {c.residual for c in CASES}
    assert any(c.cout != 4 * c.width for c in CASES) and any(c.cin != c.cout for c in CASES)
    want = {2, 30, 32, 34, 62, 64, 66, 126, 128, 130, 256, 258, 320, 322, 384, 386, 480, 482, 510, 512}
    assert want <= {k for c in CASES if tuple(c[:6]) == PROD for k in c.counts}


def test_every_sole_witness_is_needed():
    """The completeness check has teeth: without a case that is the only witness of a class, (b) - (d) name what is missing -- the two
    production launches (nsub 0..16), the 64-pixel map (three geometries, the full second tile), the one-pixel map (the K32 ring with
    three DMA instructions per row); and without both short-K-loop cases, that axis."""
    without = lambda *drop: table_gaps([c for i, c in enumerate(CASES) if i not in drop])
    index = lambda **kw: [i for i, c in enumerate(CASES) if all(getattr(c, k) == v for k, v in kw.items())]
    prod = [i for i, c in enumerate(CASES) if tuple(c[:6]) == PROD]
    assert len(prod) == 2 and all(any(g.startswith("nsub = ") for g in without(i)) for i in prod)
    (i88,), (i11,) = index(H=8, Wd=8), index(H=1, Wd=1)
    assert {"geometry (1, 2, 1, 3)", "geometry (1, 2, 2, 3)", "geometry (1, 4, 2, 2)", "tiles = 2 full"} <= set(without(i88))
    assert without(i11) == ["geometry (2, 3, 3, 3)"]
    short = [i for i, c in enumerate(CASES) if c.cin < 128]
    assert len(short) == 2 and without(*short) == ["kloop = short"]
    # every other case alone repeats classes that another shape also reaches: (b) - (d) do not depend on it
    for i in range(len(CASES)):
        assert bool(without(i)) == (i in prod + [i88, i11]), (i, without(i))


# ------------------------------------------------------------------ a case: block, input, residual, masks, references (CPU, seeded)
class _Block(nn.Module):
    """conv1 -> bn1 -> conv2 (3x3) -> bn2 -> conv3 -> bn3 with cout free of the width (BottleneckRef fixes cout = 4 * width)."""

    def __init__(self, cin, width, cout):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width)
        self.conv2, self.bn2 = nn.Conv2d(width, width, 3, padding=1, bias=False), nn.BatchNorm2d(width)
        self.conv3, self.bn3 = nn.Conv2d(width, cout, 1, bias=False), nn.BatchNorm2d(cout)

    def forward(self, x, group_mask, residual):
        """laud_resnet.py:115-144 in channel mode: the mask multiplies conv1's and conv2's output BEFORE the BatchNorm."""
        cm = TR.broadcast_channel_mask(group_mask.to(x.dtype), self.conv1.out_channels)
        h1 = F.relu(self.bn1(self.conv1(x) * cm))
        h2 = F.relu(self.bn2(self.conv2(h1) * cm))
        y = self.bn3(self.conv3(h2))
        return F.relu(y if residual is None else y + residual.to(x.dtype)).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def build_case(case):
    """-> (block (float32), x [B,cin,H,Wd], residual [B,cout,H,Wd] or None, group mask [B,G] with exactly counts[b] / gran groups of image
    b set, chosen by a seeded permutation: the channel lists are sorted but not contiguous)."""
    seed = 900 + 17 * CASES.index(case)
    B, G = len(case.counts), case.width // case.gran
    blk = _Block(case.cin, case.width, case.cout).eval()
    TR.randomize_bn_(blk, seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in (blk.conv1, blk.conv2, blk.conv3):
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
    x = F.relu(seeded_randn((B, case.cin, case.H, case.Wd), seed + 2))
    res = {"x": x, "none": None}[case.residual] if case.residual != "other" else F.relu(seeded_randn((B, case.cout, case.H, case.Wd), seed + 3))
    gm = torch.zeros(B, G)
    for b, Kb in enumerate(case.counts):
        gm[b, torch.randperm(G, generator=torch.Generator().manual_seed(seed + 10 + b))[:Kb // case.gran]] = 1.0
    return blk, x, res, gm


@functools.lru_cache(maxsize=None)
def references(case):
    """(out in float64, out of the same modules in float32 PyTorch), both [B,H,Wd,cout]."""
    blk, x, res, gm = build_case(case)
    b64 = _Block(case.cin, case.width, case.cout).eval().double()
    b64.load_state_dict(blk.state_dict())
    with torch.no_grad():
        want = b64(x.double(), gm, res)
        f32 = blk(x, gm, res)
    assert want.dtype == torch.float64 and f32.dtype == torch.float32
    return want, f32


OUT_ATOL, OUT_RTOL = 2e-4, 1e-4          # the project's bound for this arithmetic (tests/test_hip_small.py), here against float64


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_float32_pytorch_sits_inside_the_bound(case):
    """The bound is a condition on the inputs: plain float32 arithmetic must meet it against float64 with these seeds."""
    blk, x, res, gm = build_case(case)
    assert [int(v) * case.gran for v in gm.sum(dim=1)] == list(case.counts)
    for b, Kb in enumerate(case.counts):
        if 0 < Kb < case.width and case.width // case.gran - Kb // case.gran > 1 and Kb // case.gran > 1:
            on = torch.nonzero(gm[b]).flatten()
            assert int(on[-1] - on[0]) + 1 > len(on), f"image {b}: the groups must not be contiguous"
    want, f32 = references(case)
    err = assert_close(f32, want, OUT_ATOL, OUT_RTOL, "float32 PyTorch")
    assert float(want.abs().max()) > 0.5, "activations of order one"
    print(f"\n[small classes] {case_id(case)} float32 PyTorch max|err| {err:.2e}")


# ------------------------------------------------------------------ GPU
def _device_params(case, blk):
    """The folded parameters and packed weights of the block as Bottleneck._prepare / tail_weights derive them, for any cout."""
    from laudnet_amd import ops
    from laudnet_amd._shared import channel_constants
    from laudnet_amd.laud_resnet import _fold_bn
    with torch.no_grad():
        w1 = blk.conv1.weight.detach().float().reshape(case.width, case.cin)
        w2 = blk.conv2.weight.detach().float()
        w3 = blk.conv3.weight.detach().float().reshape(case.cout, case.width)
        s1, t1 = _fold_bn(blk.bn1)
        s2, t2 = _fold_bn(blk.bn2)
        s3, t3 = _fold_bn(blk.bn3)
        c1, c2, t2_tab, t3c = channel_constants(w2, w3, s2, t2, t1, s3, t3)
        p = dict(w1s=ops.pack_w1_split(w1), w2p=ops.pack_w2_pairs(w2), w3p=ops.pack_w3_pairs(w3 * s3.view(-1, 1)),
                 s1=s1, t1=t1, c1=c1, s2=s2, t2_tab=t2_tab, c2=c2, t3c=t3c)
    return {k: v.detach().contiguous().to(DEV) for k, v in p.items()}, t3c.detach().clone()


def _guarded(shape, per_image):
    """A NaN-filled buffer and a view of `shape` inside it: more than one image's worth of guard on both sides, the view's offset a
    multiple of 16 bytes but not of 32."""
    n = 1
    for v in shape:
        n *= v
    guard = per_image + 4
    buf = torch.full((guard + n + guard,), NAN, device=DEV)
    view = buf[guard:guard + n].view(shape)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view, guard, n


def _guards_intact(buf, guard, n):
    bits = buf.view(torch.int32)
    nan_bits = torch.tensor(NAN).view(torch.int32).item()
    return bool((bits[:guard] == nan_bits).all()) and bool((bits[guard + n:] == nan_bits).all())


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_smallmap_classes_vs_float64(ops, case):
    H, Wd, cin, width, cout, gran, counts, rkind = case
    B, HW, G = len(counts), H * Wd, width // gran
    assert ops.bottleneck_smallmap_fits(H, Wd, cin, width, cout)
    blk, x, res, gm = build_case(case)
    want, f32 = references(case)
    p, t3c_host = _device_params(case, blk)
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, G, gran, mask_in=gm.to(DEV))
    assert cnt.tolist() == list(counts), "the masker must hand the kernel exactly the forced counts"
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    resn = {"x": xn, "none": None}[rkind] if rkind != "other" else res.permute(0, 2, 3, 1).contiguous().to(DEV)
    x_keep = xn.clone()
    res_keep = None if resn is None else resn.clone()

    def launch(out, colsum, x_arg=xn, residual=resn):
        ops.bottleneck_smallmap(x_arg, p["w1s"], p["w2p"], p["w3p"], idx, cnt, p["s1"], p["t1"], p["c1"], p["s2"], p["t2_tab"], p["c2"],
                                p["t3c"], out, residual=residual, colsum=colsum)
        torch.cuda.synchronize()

    obuf, out, og, on = _guarded((B, H, Wd, cout), HW * cout)
    cbuf, colsum, cg, cn = _guarded((B, 2, cout), 2 * cout)
    launch(out, colsum)
    # every element written, nothing outside
    assert bool(torch.isfinite(out).all()), "out: an element was not written (or is not finite)"
    assert bool(torch.isfinite(colsum).all()), "colsum: an element was not written (or is not finite)"
    assert _guards_intact(obuf, og, on), "out: a write outside the tensor"
    assert _guards_intact(cbuf, cg, cn), "colsum: a write outside the tensor"
    assert torch.equal(xn, x_keep) and (rkind != "other" or torch.equal(resn, res_keep)), "inputs of an out-of-place launch must stay intact"
    got = out.cpu()
    # against float64, image by image (the message names the image's class)
    errs = []
    for b, Kb in enumerate(counts):
        cls = image_class(HW, cin, width, cout, Kb)
        errs.append(assert_close(got[b], want[b], OUT_ATOL, OUT_RTOL, f"out of image {b} (Kb {Kb}, {cls})"))
    # an empty image forms no product: exactly relu(shift3 + residual)
    res_host = None if res is None else res.permute(0, 2, 3, 1)
    for b, Kb in enumerate(counts):
        if Kb == 0:
            exact = torch.relu(t3c_host.view(1, 1, cout) + (res_host[b] if res_host is not None else torch.zeros(H, Wd, cout)))
            assert torch.equal(got[b], exact), f"image {b} is empty: out must equal relu(shift3 + residual) exactly"
    # GAP partials per pixel tile: tile t sums the pixels [32 t, 32 t + 32) of the map; a tile without pixels is written as zeros
    flat = got.double().reshape(B, HW, cout)
    tiles = torch.stack((flat[:, :32].sum(dim=1), flat[:, 32:].sum(dim=1)), dim=1)
    assert torch.allclose(colsum.cpu().double(), tiles, atol=1e-2, rtol=1e-5), (colsum.cpu().double() - tiles).abs().max().item()
    if HW <= 32:
        assert bool((colsum[:, 1] == 0).all()), "the second pixel tile holds no pixel: its partial is zero"
    # a second launch into fresh buffers: every sum order is fixed, so bit-identical
    obuf2, out2, _, _ = _guarded((B, H, Wd, cout), HW * cout)
    cbuf2, colsum2, _, _ = _guarded((B, 2, cout), 2 * cout)
    launch(out2, colsum2)
    assert torch.equal(out2, out) and torch.equal(colsum2, colsum), "a repeated launch must be bit-identical"
    assert _guards_intact(obuf2, og, on) and _guards_intact(cbuf2, cg, cn)
    # head + tail on the same lists, where they cover the shape
    err_ht = None
    if width <= 256 and ops.bottleneck_tail_splits(H, Wd, width, 1) > 0:
        h1 = torch.full((B, H, Wd, width), NAN, device=DEV)
        ops.bottleneck_head(xn, p["w1s"], idx, cnt, p["s1"], p["t1"], p["c1"], h1)
        ref = torch.full((B, H, Wd, cout), NAN, device=DEV)
        ops.bottleneck_tail(h1, p["w2p"], p["w3p"], idx, cnt, p["s2"], p["t2_tab"], p["c2"], p["t3c"], ref, residual=resn)
        torch.cuda.synchronize()
        err_ht = assert_close(out, ref.double(), 2e-5, 1e-5, "smallmap vs head + tail")
    # the in-place residual stream (out aliases x and the residual): bit-identical, colsum included
    if rkind == "x":
        xi = xn.clone()
        colsum3 = torch.full((B, 2, cout), NAN, device=DEV)
        launch(xi, colsum3, x_arg=xi, residual=xi)
        assert torch.equal(xi, out) and torch.equal(colsum3, colsum), "the in-place launch must equal the out-of-place one bit for bit"
    err32 = (f32.double() - want).abs().reshape(B, -1).max(dim=1).values.tolist()
    print(f"\n[small classes] {case_id(case)} max|err| kernel {max(errs):.2e} float32 PyTorch {max(err32):.2e}"
          + (f" vs head+tail {err_ht:.2e}" if err_ht is not None else ""))
    for b, Kb in enumerate(counts):
        c = image_class(HW, cin, width, cout, Kb)
        print(f"    image {b:2d} Kb {Kb:3d} geom {geometry(c)} D1 {c.D1} nw {c.nw} nv {c.nv} last {c.last} conv3 {c.conv3} tiles {c.tiles} "
              f"kloop {c.kloop} kernel {errs[b]:.2e} f32 {err32[b]:.2e}")
