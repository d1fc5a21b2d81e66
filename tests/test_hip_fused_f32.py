"""The fused head and tail of a channel-mode bottleneck (ldn_bottleneck_head / ldn_bottleneck_tail and their true-fp32 twins
ldn_bottleneck_head_f32 / ldn_bottleneck_tail_f32, what the `fp32` math mode runs by default: ops.USE_FUSED_F32) in BOTH arithmetic modes,
op by op against float64, on square and non-square maps.

tests/test_hip_tail.py pins bf16x3, compares with float32 PyTorch and runs square maps only.  The fp32 forms have code of their own in
csrc/ldn_tail.hip (LDN_K16's fragment shuffles, the epilogue stores, the A-operand load); a wrong k-slot pairing there was visible only
through a model-level logit tolerance.

`tail_rows_per_block` / `tail_splits` restate the row split of the tail (csrc/ldn_tail.hip:745-784, 823-828) in Python; non-GPU tests compare
them with ldn_bottleneck_tail_splits over a grid and prove that the case table reaches NS in {2, 4, 8} x stride in {1, 2}, each with one
workgroup per image, several workgroups with an even split and several with a shorter last one.

Bounds (tests/test_hip_tail.py, tests/test_hip_packed.py): h1 1e-4 + 1e-4 |ref|, out 2e-4 + 1e-4 |ref|, colsum atol 1e-2, rtol 1e-5.
Measured maximum |error| per case and mode: docs/lab_notebook.md."""
import functools

import pytest
import torch
import torch.nn.functional as F

from fill import seeded_bernoulli, seeded_randn
from helpers import apply_math_mode  # noqa: F401  (autouse fixture: a test that takes math_mode runs in that mode)
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


# ------------------------------------------------------------------ the row split of the tail, restated
T_KIDX_BYTES = 1280      # csrc/ldn_tail.hip:107
T_W2_SLOTS = 3           # :133
LDS_BYTES = 160 * 1024


def _round_up(a, b):
    return -(-a // b) * b


def _ceil_div(a, b):
    return -(-a // b)


def tail_region_pixels(R, Hi, Wi, st):
    """:773-776: pixels resident per slice slot for R output rows (stride 1: the halo'd rows; stride 2: the largest parity plane)."""
    if st == 2:
        return min(R + 1, (Hi + 1) // 2) * ((Wi - 1) // 2 + 1)
    return min(R + 2, Hi) * Wi


def tail_lds2(R, Hi, Wi, NS, st):
    """:779-783: LDS bytes of the conv2 phase."""
    nr = tail_region_pixels(R, Hi, Wi, st)
    slice_bytes = _round_up((_round_up(nr, 8) + 1) * 128, 1024)
    return T_KIDX_BYTES + (2 if st == 2 else (1 if NS == 2 else 2)) * slice_bytes + T_W2_SLOTS * 16 * NS * 256


def tail_rows_per_block(Hi, Wi, NS, st):
    """:786-810 -> (output rows per workgroup, workgroups per image); (0, 0): the map does not fit."""
    Ho, Wo = (Hi - 1) // st + 1, (Wi - 1) // st + 1
    R = 256 // Wo
    if R < 1:
        return 0, 0
    R = min(R, Ho)
    fits = lambda r: (tail_lds2(r, Hi, Wi, NS, st) <= LDS_BYTES
                      and (st == 2 or NS == 2 or _round_up(tail_region_pixels(r, Hi, Wi, st), 8) // 8 <= 72))
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


def tail_splits(H, Wd, width, stride):
    """ldn_bottleneck_tail_splits (:849-854)."""
    if H < 1 or Wd < 1 or stride not in (1, 2) or (Wd - 1) // stride + 1 > 256 or width not in (64, 128, 256):
        return 0
    rows, mbk = tail_rows_per_block(H, Wd, width // 32, stride)
    return 0 if rows == 0 else mbk * 8


def split_class(H, Wd, width, stride):
    """(NS, stride, "single" | "even" | "ragged"): one workgroup per image, several with equal rows, several with a shorter last one."""
    rows, mbk = tail_rows_per_block(H, Wd, width // 32, stride)
    assert rows > 0
    Ho = (H - 1) // stride + 1
    return width // 32, stride, "single" if mbk == 1 else ("even" if rows * mbk == Ho else "ragged")


# (B, H, Wd, cin, width, channel granularity, stride of the 3x3)
CASES = [
    # the shapes of tests/test_hip_tail.py (all have cin % 32 == 0: the fp32 form has k_head as its only conv1)
    (4, 14, 14, 1024, 256, 2, 1), (3, 28, 28, 512, 128, 2, 1), (2, 56, 56, 256, 64, 2, 1), (3, 56, 56, 64, 64, 2, 1),
    (3, 14, 14, 64, 256, 4, 1), (2, 9, 9, 32, 64, 2, 1), (9, 14, 14, 128, 256, 2, 1),
    (3, 56, 56, 256, 128, 2, 2), (3, 28, 28, 512, 256, 2, 2), (2, 13, 13, 64, 64, 2, 2), (2, 30, 30, 64, 128, 4, 2),
    (2, 56, 56, 32, 64, 2, 2), (5, 8, 8, 64, 256, 2, 2),
    # non-square maps
    (3, 9, 20, 512, 128, 2, 1),       # one workgroup per image at width 128
    (3, 15, 17, 1024, 256, 2, 1),     # 8 + 7 rows
    (2, 7, 200, 32, 64, 2, 2), (2, 7, 200, 64, 128, 2, 2), (2, 7, 200, 32, 256, 2, 2),    # 4 x 100 output: 2 + 2 rows / 1 + 1 + 1 + 1 rows
    (3, 20, 9, 64, 64, 2, 2),
    (5, 1, 7, 64, 128, 2, 1),         # a single row; a batch that is not a multiple of 8
    # the rest of (NS, stride, split class)
    (3, 28, 28, 32, 64, 2, 1),        # width 64: 8 + 8 + 8 + 4 rows
    (3, 16, 32, 64, 128, 4, 1),       # width 128: 8 + 8 rows
    (3, 16, 32, 128, 256, 2, 1),      # width 256: 4 x 4 rows
    (3, 24, 48, 64, 256, 2, 2),       # width 256, stride 2: 8 + 4 rows
]


def test_tail_splits_restated_equals_the_library():
    """The transcription against ldn_bottleneck_tail_splits (the library loads without a GPU) over a grid of maps, the three widths and both
    strides, the refusals, and the values the source gives for the maps of the ResNets."""
    from laudnet_amd import ops
    sizes = list(range(1, 41)) + [49, 50, 56, 57, 64, 100, 112, 113, 200, 224, 255, 256, 257, 300, 511, 512, 513]
    zero = nonzero = 0
    for H in sizes:
        for Wd in sizes:
            for width in (64, 128, 256):
                for st in (1, 2):
                    want = tail_splits(H, Wd, width, st)
                    assert ops.bottleneck_tail_splits(H, Wd, width, st) == want, (H, Wd, width, st)
                    zero += want == 0
                    nonzero += want > 0
    assert zero > 500 and nonzero > 5000
    for width in (64, 128, 256):
        assert ops.bottleneck_tail_splits(4, 257, width, 1) == 0 and ops.bottleneck_tail_splits(4, 513, width, 2) == 0    # output wider than 256
        assert ops.bottleneck_tail_splits(4, 256, 64, 1) > 0 and ops.bottleneck_tail_splits(4, 512, 64, 2) > 0
        assert ops.bottleneck_tail_splits(14, 14, width, 3) == 0 and ops.bottleneck_tail_splits(0, 14, width, 1) == 0
    assert ops.bottleneck_tail_splits(112, 112, 256, 1) == 0 and ops.bottleneck_tail_splits(1, 256, 256, 1) == 0
    assert ops.bottleneck_tail_splits(112, 112, 64, 1) > 0 and ops.bottleneck_tail_splits(14, 14, 96, 1) == 0
    rows = lambda H, Wd, st: [tail_rows_per_block(H, Wd, ns, st) for ns in (2, 4, 8)]
    assert rows(28, 28, 1) == [(8, 4), (8, 4), (6, 5)]
    assert rows(56, 56, 1) == [(4, 14), (4, 14), (2, 28)]
    assert rows(56, 56, 2) == [(8, 4), (8, 4), (7, 4)]
    assert rows(15, 17, 1) == [(15, 1), (15, 1), (8, 2)]
    assert rows(7, 200, 2) == [(2, 2), (2, 2), (1, 4)]
    assert rows(14, 14, 1) == [(14, 1)] * 3


def test_case_table_reaches_every_split():
    """NS in {2, 4, 8} x stride in {1, 2} x {one workgroup per image, an even split, a shorter last workgroup}: all eighteen."""
    seen = {}
    for case in CASES:
        B, H, Wd, cin, width, gran, st = case
        assert cin % 32 == 0 and width % gran == 0 and gran % 2 == 0 and B <= 9
        assert tail_splits(H, Wd, width, st) > 0, case
        seen.setdefault(split_class(H, Wd, width, st), case)
    want = {(ns, st, c) for ns in (2, 4, 8) for st in (1, 2) for c in ("single", "even", "ragged")}
    assert set(seen) == want, f"missing {sorted(want - set(seen))}"
    assert split_class(15, 17, 256, 1) == (8, 1, "ragged") and tail_rows_per_block(15, 17, 8, 1) == (8, 2)
    maps = {(c[1], c[2], c[6]) for c in CASES}
    assert {(9, 20, 1), (15, 17, 1), (7, 200, 2), (20, 9, 2), (1, 7, 1)} <= maps
    assert any(c[0] > 8 and c[0] % 8 for c in CASES), "a batch that is not a multiple of 8"


# ------------------------------------------------------------------ a case: block, input, residual, masks, float64 reference (CPU, seeded)
def _ref_block(case):
    B, H, Wd, cin, width, gran, st = case
    return TR.BottleneckRef(cin, width, stride=st, downsample=None, dyn_mode="channel", channel_dyn_granularity=gran,
                            channel_masker="MLP", output_size=(H - 1) // st + 1).eval()


@functools.lru_cache(maxsize=None)
def build_case(case):
    """-> (reference block (float32 parameters), x [B,cin,H,Wd], residual [B,cout,Ho,Wo], group mask [B,G]).  Masks as in
    tests/test_hip_tail.py: image 0 without a channel, image 1 with all, Bernoulli(0.62) draws elsewhere."""
    B, H, Wd, cin, width, gran, st = case
    seed = 500 + 13 * CASES.index(case)
    blk = _ref_block(case)
    TR.randomize_bn_(blk, seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in (blk.conv1, blk.conv2, blk.conv3):
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
    Ho, Wo = (H - 1) // st + 1, (Wd - 1) // st + 1
    x = F.relu(seeded_randn((B, cin, H, Wd), seed + 2))
    ident = F.relu(seeded_randn((B, 4 * width, Ho, Wo), seed + 3))      # the residual (x itself when cin == cout, else a projection's output)
    gm = seeded_bernoulli((B, width // gran), 0.62, seed + 4)
    gm[0] = 0.0
    gm[1] = 1.0
    return blk, x, ident, gm


@functools.lru_cache(maxsize=None)
def reference_f64(case):
    """The channel-mode algebra of oracle.torch_ref.BottleneckRef.forward (laud_resnet.py:115-144: the mask before bn1 / bn2) in float64
    throughout: (h1 [B,width,H,Wd], out [B,Ho,Wo,cout])."""
    blk, x, ident, gm = build_case(case)
    b64 = _ref_block(case).double()
    b64.load_state_dict(blk.state_dict())
    with torch.no_grad():
        cm = TR.broadcast_channel_mask(gm.double(), b64.conv1.out_channels)
        h1 = F.relu(b64.bn1(b64.conv1(x.double()) * cm))
        h2 = F.relu(b64.bn2(b64.conv2(h1) * cm))
        out = F.relu(b64.bn3(b64.conv3(h2)) + ident.double()).permute(0, 2, 3, 1).contiguous()
    return h1, out


def test_mask_preconditions():
    """Image 0 keeps no channel, image 1 every channel; every other image of the table keeps some but not all, and together they draw
    between 45 % and 80 % of their groups."""
    kept = total = 0
    for case in CASES:
        gm = build_case(case)[3]
        assert float(gm[0].sum()) == 0 and float(gm[1].sum()) == gm.shape[1]
        for b in range(2, gm.shape[0]):
            assert 0 < float(gm[b].sum()) < gm.shape[1], (case, b)
            kept += float(gm[b].sum())
            total += gm.shape[1]
    assert total > 2000 and 0.45 < kept / total < 0.8


# ------------------------------------------------------------------ GPU
def _decode_h1(h1, f32):
    """h1 as values: plain floats in the fp32 form; [octet][8 hi | 8 lo] bf16 (hi + lo) in the bf16x3 form."""
    if f32:
        return h1
    B, H, W, ld = h1.shape
    raw = h1.contiguous().view(torch.bfloat16).reshape(B, H, W, ld // 8, 2, 8).float()
    return (raw[..., 0, :] + raw[..., 1, :]).reshape(B, H, W, ld)


def _hip_block(case, blk):
    from laudnet_amd.laud_resnet import Bottleneck
    B, H, Wd, cin, width, gran, st = case
    hb = Bottleneck(cin, width, stride=st, downsample=None, dyn_mode="channel", channel_dyn_granularity=gran,
                    channel_masker="MLP", output_size=(H - 1) // st + 1).eval()
    hb.load_state_dict(blk.state_dict())
    return hb.to(DEV)


class _Spy:
    """Records the dtype of the weight operand of every ops.bottleneck_head / ops.bottleneck_tail call while installed."""

    def __init__(self, ops):
        self.ops, self.head, self.tail = ops, [], []

    def __enter__(self):
        self._head, self._tail = self.ops.bottleneck_head, self.ops.bottleneck_tail
        self.ops.bottleneck_head = lambda *a, **k: (self.head.append(a[1].dtype), self._head(*a, **k))[1]
        self.ops.bottleneck_tail = lambda *a, **k: (self.tail.append((a[1].dtype, a[2].dtype)), self._tail(*a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.ops.bottleneck_head, self.ops.bottleneck_tail = self._head, self._tail


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_and_tail_vs_float64(ops, case, math_mode):
    B, H, Wd, cin, width, gran, st = case
    f32 = math_mode == "fp32"
    wdtype = torch.float32 if f32 else torch.bfloat16
    G, cout = width // gran, 4 * width
    Ho, Wo = (H - 1) // st + 1, (Wd - 1) // st + 1
    blk, x, ident, gm = build_case(case)
    want_h1, want_out = reference_f64(case)
    hb = _hip_block(case, blk)
    p = hb._prepare(torch.device(DEV))
    w2p, w3p = hb.tail_weights(p)
    w1s = p[hb._w1s_key()]
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, G, gran, mask_in=gm.to(DEV))
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    idn = ident.permute(0, 2, 3, 1).contiguous().to(DEV)
    idn_keep = idn.clone()
    splits = ops.bottleneck_tail_splits(H, Wd, width, st)
    assert splits == tail_splits(H, Wd, width, st) > 0
    h1 = torch.full((B, H, Wd, width), NAN, device=DEV)
    out = torch.full((B, Ho, Wo, cout), NAN, device=DEV)
    colsum = torch.full((B, splits, cout), NAN, device=DEV)
    with _Spy(ops) as spy:
        ops.bottleneck_head(xn, w1s, idx, cnt, p["s1"], p["t1"], p["c1"], h1)
        ops.bottleneck_tail(h1, w2p, w3p, idx, cnt, p["s2"], p["t2_tab"], p["c2"], p["t3c"], out, residual=idn, colsum=colsum, stride=st)
    torch.cuda.synchronize()
    assert spy.head == [wdtype] and spy.tail == [(wdtype, wdtype)], f"{math_mode} must run the {'fp32' if f32 else 'bf16x3'} forms"
    # h1: the active channels' relu(bn1(conv1)) - post_sub1, left-packed; zero up to the next multiple of 32
    dec = _decode_h1(h1, f32).cpu()
    c1 = p["c1"].cpu().double()
    err_h1 = 0.0
    for b in range(B):
        n = int(cnt[b])
        ch = idx[b, :n].cpu().long()
        want1 = want_h1[b, ch].permute(1, 2, 0) - c1[ch]
        err_h1 = max(err_h1, assert_close(dec[b, :, :, :n], want1, 1e-4, 1e-4, f"h1 of image {b}"))
        pad = (n + 31) // 32 * 32
        assert bool((dec[b, :, :, n:pad] == 0).all()), f"h1 of image {b}: columns up to the next multiple of 32 must be zero"
    assert torch.equal(xn.cpu(), x.permute(0, 2, 3, 1)), "the head must not touch its input"
    # out: every pixel
    err_out = assert_close(out, want_out, 2e-4, 1e-4, "out")
    assert torch.allclose(colsum.sum(dim=1).cpu().double(), out.cpu().double().sum(dim=(1, 2)), atol=1e-2, rtol=1e-5)
    assert torch.equal(idn, idn_keep), "a residual that is a separate tensor must stay intact"
    # in-place residual stream (out aliases residual): bit-identical, colsum included
    colsum2 = torch.full_like(colsum, NAN)
    ops.bottleneck_tail(h1, w2p, w3p, idx, cnt, p["s2"], p["t2_tab"], p["c2"], p["t3c"], idn, residual=idn, colsum=colsum2, stride=st)
    torch.cuda.synchronize()
    assert torch.equal(idn, out) and torch.equal(colsum2, colsum), "the in-place form must equal the out-of-place one bit for bit"
    print(f"\n[fused] {'x'.join(map(str, case))} {math_mode:6s} {split_class(H, Wd, width, st)} max|err| h1 {err_h1:.2e} out {err_out:.2e}")


@gpu
def test_tail_refuses_mixed_weight_layouts(ops):
    """A bf16 w2_pairs with an fp32 w3_pairs (or the reverse) is an argument error and writes nothing."""
    from laudnet_amd._lib import LdnError
    case = CASES[5]
    B, H, Wd, cin, width, gran, st = case
    blk, x, ident, gm = build_case(case)
    hb = _hip_block(case, blk)
    p = hb._prepare(torch.device(DEV))
    weights = {}
    for mode in ("fp32", "bf16x3"):
        ops.set_math_mode(mode)
        try:
            weights[mode] = hb.tail_weights(p)
        finally:
            ops.set_math_mode("fp32")
    assert weights["fp32"][0].dtype == torch.float32 and weights["bf16x3"][0].dtype == torch.bfloat16
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, width // gran, gran, mask_in=gm.to(DEV))
    h1 = torch.zeros(B, H, Wd, width, device=DEV)
    idn = ident.permute(0, 2, 3, 1).contiguous().to(DEV)
    for w2p, w3p in ((weights["bf16x3"][0], weights["fp32"][1]), (weights["fp32"][0], weights["bf16x3"][1])):
        out = torch.full((B, H, Wd, 4 * width), NAN, device=DEV)
        colsum = torch.full((B, ops.bottleneck_tail_splits(H, Wd, width, st), 4 * width), NAN, device=DEV)
        with pytest.raises(LdnError):
            ops.bottleneck_tail(h1, w2p, w3p, idx, cnt, p["s2"], p["t2_tab"], p["c2"], p["t3c"], out, residual=idn, colsum=colsum, stride=st)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(colsum).all()), "a refused call must write nothing"


# (B, H, Wd, cin = cout, width, granularity): identity-shortcut blocks on maps of more than 64 pixels (smaller ones run the dense execution)
BLOCK_CASES = [(3, 14, 14, 256, 64, 2), (3, 9, 20, 512, 128, 2), (3, 15, 17, 1024, 256, 4)]


@gpu
@pytest.mark.parametrize("B,H,Wd,cin,width,gran", BLOCK_CASES)
def test_fp32_block_runs_the_fused_forms_exactly_when_switched_on(ops, B, H, Wd, cin, width, gran):
    """In the fp32 math mode a channel-mode Bottleneck with forced masks runs ldn_bottleneck_head_f32 / ldn_bottleneck_tail_f32 when
    ops.USE_FUSED_F32 is on and the three-launch path when it is off; both within the tail's bound of the float64 block."""
    from helpers import bottleneck_stages_f64, start_state
    from laudnet_amd.laud_resnet import Bottleneck
    kw = dict(stride=1, downsample=None, dyn_mode="channel", channel_dyn_granularity=gran, channel_masker="MLP", output_size=H)
    ref = TR.BottleneckRef(cin, width, **kw).eval()
    TR.randomize_bn_(ref, 11 + H)
    g = torch.Generator().manual_seed(12 + H)
    with torch.no_grad():
        for m in (ref.conv1, ref.conv2, ref.conv3):
            fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
    hb = Bottleneck(cin, width, **kw).eval()
    hb.load_state_dict(ref.state_dict())
    hb = hb.to(DEV)
    gm = seeded_bernoulli((B, width // gran), 0.62, 13 + H)
    gm[0] = 0.0
    gm[1] = 1.0
    assert 0 < float(gm[2].sum()) < gm.shape[1]
    x = F.relu(seeded_randn((B, cin, H, Wd), 14 + H))
    b64 = TR.BottleneckRef(cin, width, **kw).eval().double()
    b64.load_state_dict(ref.state_dict())
    want = bottleneck_stages_f64(b64, x, gm, torch.ones(B, 1, H, Wd, dtype=torch.float64))[4]
    hb.forced_channel_mask = gm.to(DEV)
    flag = ops.USE_FUSED_F32
    ops.set_math_mode("fp32")
    errs = {}
    try:
        for fused in (True, False):
            ops.USE_FUSED_F32 = fused
            with _Spy(ops) as spy:
                with torch.no_grad():
                    out = hb(start_state(x.to(DEV)), 1.0)[0]
            torch.cuda.synchronize()
            if fused:
                assert spy.head == [torch.float32] and spy.tail == [(torch.float32, torch.float32)], "the fp32 fused forms must run"
            else:
                assert spy.head == [] and spy.tail == [], "with the switch off the block must run the three-launch path"
            errs[fused] = assert_close(out, want, 2e-4, 1e-4, f"fused={fused}")
    finally:
        ops.USE_FUSED_F32 = flag
        ops.set_math_mode("fp32")
    print(f"\n[fused block] {B}x{H}x{Wd}x{cin}x{width} fp32 max|err| fused {errs[True]:.2e} three launches {errs[False]:.2e}")
