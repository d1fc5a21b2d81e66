"""GPU tests of the matrix-core packed-row grouped 3x3 at group widths 56 and 112 (ops.grouped_wide_conv3x3_rows ->
ldn_grouped_wide_conv3x3_rows, k_grouped_wide_rows, bf16x3; the fragments of ops.pack_grouped_wide_weights) against
F.conv2d(groups = C / gw) in float64 at the kept pixels, bound 1e-4 max(1, |want|max): the project's bound for every matrix-core grouped
kernel (tests/test_hip_grouped_mfma.py, tests/test_hip_grouped_wide.py).  The construction of tests/test_hip_grouped_mfma.py: the lists of
ops.mask_to_index, NaN in the input rows past the dilated list, sentinels in the pad columns of a (lda = C + 8) and of out (ldo = C + 4), zero
and negative scales, with and without ReLU, twice, bit for bit.  One group and several, less than one row tile, ragged last tiles, more
tiles than one workgroup holds, one kept pixel, a device-side count of zero, no count at all -- every case through the launch plan's own choice
of pixel tiles per wave (one at these sizes: ldn_grouped_wide_rows_tiles, whose thresholds tests/test_grouped_wide_rows_abi.py pins) and
through both forms the plan can choose, forced by LDN_GROUPED_WIDE_ROWS_FORM = b1 / b2 (b2 is what the model shapes with many rows launch).
Refusals leave the output untouched.  Then
the dispatch: with laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS on a layer-skip block runs conv b on the new op and not on the VALU one, with it
off the reverse, and the two outputs agree; with the default switch the new op is never called."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0

# (gw, B, Ho, stride, C, keep)
CASES = [(56, 1, 5, 1, 56, 1.0),        # one group, 25 rows: less than one tile
         (56, 2, 7, 2, 168, 0.6),       # 3 groups
         (56, 3, 14, 1, 224, 0.5),      # ragged last tile
         (112, 1, 5, 1, 112, 1.0),      # one group, 25 rows: less than one tile
         (112, 2, 7, 2, 224, 0.6),
         (112, 3, 14, 1, 336, 0.5),
         # A wave keeps 1 or 2 pixel tiles of 32 rows, a workgroup's 4 waves 4 or 8 = at most 256 rows, and the grid's x dimension walks the
         # tiles (there is no loop inside the kernel: csrc/ldn_grouped_wide_rows.hip, launch_grouped_wide_rows).  A whole 17 x 17 image is
         # 289 rows = 10 tiles: the smallest square map past 256 rows.  With two tiles per wave the second workgroup's first wave holds a
         # full tile and one of a single row and its other three waves have nothing and leave; with one tile per wave the third workgroup
         # has two live waves.
         (56, 1, 17, 1, 56, 1.0),
         (112, 1, 17, 1, 112, 1.0)]


@pytest.fixture(autouse=True)
def _bf16x3():
    from laudnet_amd import ops
    ops.set_math_mode("bf16x3")
    yield
    ops.set_math_mode("fp32")


@pytest.fixture(params=[None, "b1", "b2"], ids=["plan", "one_tile", "two_tiles"])
def form(request, monkeypatch):
    """pixel tiles per wave: the launch plan's choice, or one of the two forms it chooses between"""
    if request.param is None:
        monkeypatch.delenv("LDN_GROUPED_WIDE_ROWS_FORM", raising=False)
    else:
        monkeypatch.setenv("LDN_GROUPED_WIDE_ROWS_FORM", request.param)
    return request.param


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()
    return _ops


@functools.lru_cache(maxsize=None)
def _problem(gw, B, Ho, stride, C, keep, single=False):
    """-> (ix, n3, a [cap1, C + 8] on the device, w [C, 9, gw], scale, shift, y64 [n3, C] = scale conv + shift in float64 at the kept pixels);
    built once per case and shared by the ReLU / no-ReLU runs, never modified"""
    from laudnet_amd import ops
    Hi = Ho * stride
    if single:
        patch = torch.zeros(B, Ho, Ho)
        patch[B - 1, Ho // 2, 1] = 1.0
    else:
        patch = seeded_bernoulli((B, Ho, Ho), keep, 191 + C)
    ix = ops.mask_to_index(patch.to(DEV), Ho, Ho, stride)
    n3, n1 = int(ix.cnt[0].item()), int(ix.cnt[1].item())
    x = seeded_randn((B, C, Hi, Hi), 192 + C)
    w = seeded_randn((C, gw, 3, 3), 193 + C) * 0.1
    scale = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(194))
    scale[0::5] = 0.0
    scale[1::5] = -scale[1::5]
    shift = 0.1 * seeded_randn((C,), 195)
    idx1, idx3 = ix.idx1[:n1].long().cpu(), ix.idx3[:n3].long().cpu()
    m1 = torch.zeros(B * Hi * Hi, dtype=torch.bool)
    m1[idx1] = True
    xm = (x * m1.view(B, 1, Hi, Hi)).double()            # the packed input holds the dilated-list pixels only; the others read as zero
    y = F.conv2d(xm, w.double(), None, stride, 1, 1, C // gw) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    y64 = y.permute(0, 2, 3, 1).reshape(B * Ho * Ho, C)[idx3]
    a = torch.full((ix.cap1, C + 8), float("nan"))        # rows outside the dilated list: NaN
    a[:n1] = SENTINEL * 1e6                               # the pad columns of the listed rows
    a[:n1, :C] = x.permute(0, 2, 3, 1).reshape(B * Hi * Hi, C)[idx1]
    return ix, n3, a.to(DEV), w.permute(0, 2, 3, 1).reshape(C, 9, gw).contiguous(), scale, shift, y64


def _run(ops, prob, gw, relu, m_count="list"):
    ix, n3, a, w, scale, shift, _ = prob
    C = w.shape[0]
    frag = ops.pack_grouped_wide_weights(w.to(DEV), gw)
    out = torch.full((ix.cap3, C + 4), SENTINEL, device=DEV)
    cnt = ix.cnt[0:1] if m_count == "list" else m_count
    ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag, gw, scale.to(DEV), shift.to(DEV), out[:, :C], m_count=cnt, m_cap=ix.cap3, relu=relu)
    torch.cuda.synchronize()
    return out


def _check(ops, prob, gw, relu):
    ix, n3, a, w, scale, shift, y64 = prob
    C = w.shape[0]
    assert a.stride(0) == C + 8
    out = _run(ops, prob, gw, relu)
    want = torch.relu(y64) if relu else y64
    got = out[:n3, :C].cpu()
    assert torch.isfinite(got).all()
    err, bound = (got.double() - want).abs().max().item(), 1e-4 * max(1.0, want.abs().max().item())
    print(f"grouped_wide_rows gw {gw} C {C} rows {n3} relu {relu}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    assert bool((out[n3:] == SENTINEL).all()), "rows at or past the device-side count must not be written"
    assert bool((out[:, C:] == SENTINEL).all()), "columns past C must not be written"
    if not relu:
        assert bool((got < 0).any())
        zero = scale == 0
        assert torch.equal(got[:, zero], shift[zero].expand(n3, -1)), "a zero scale leaves the shift"
    assert torch.equal(_run(ops, prob, gw, relu), out), "two runs differ"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gw,B,Ho,stride,C,keep", CASES)
def test_grouped_wide_conv3x3_rows_vs_float64(ops, form, gw, B, Ho, stride, C, keep, relu):
    from laudnet_amd import _lib
    assert ops.grouped_wide_rows_ok(C, gw)
    prob = _problem(gw, B, Ho, stride, C, keep)
    ix, n3 = prob[0], prob[1]
    assert _lib.load().ldn_grouped_wide_rows_tiles(C, gw, ix.cap3) == 1, "the plan's own choice at these sizes"
    if keep < 1:
        assert 0 < n3 < ix.cap3
    else:
        assert n3 == ix.cap3
    if Ho == 17:
        assert n3 == 289 and 256 < n3, "more rows than one workgroup holds"
    if Ho == 14:
        assert n3 % 32, "a ragged last tile"
    _check(ops, prob, gw, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gw,C", [(56, 112), (112, 224)])
def test_one_kept_pixel(ops, form, gw, C, relu):
    prob = _problem(gw, 2, 5, 1, C, 0.0, single=True)
    assert prob[1] == 1
    _check(ops, prob, gw, relu)


@pytest.mark.parametrize("gw,B,Ho,stride,C,keep", [CASES[1], CASES[4]])
def test_a_device_side_count_of_zero_writes_nothing(ops, form, gw, B, Ho, stride, C, keep):
    prob = _problem(gw, B, Ho, stride, C, keep)
    out = _run(ops, prob, gw, 1, m_count=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("gw,B,Ho,stride,C,keep", [CASES[1], CASES[4]])
def test_no_count_means_m_cap_rows(ops, form, gw, B, Ho, stride, C, keep):
    """the rows past the list read whatever their table entries name, so they are pointed at the zero row: exactly relu(shift)"""
    ix, n3, a, w, scale, shift, y64 = _problem(gw, B, Ho, stride, C, keep)
    assert 0 < n3 < ix.cap3
    nbr = ix.nbr.view(-1, 9).clone()
    nbr[n3:] = -1
    frag = ops.pack_grouped_wide_weights(w.to(DEV), gw)
    out = torch.full((ix.cap3, C), SENTINEL, device=DEV)
    ops.grouped_wide_conv3x3_rows(a[:, :C], nbr.reshape(-1).contiguous(), frag, gw, scale.to(DEV), shift.to(DEV), out, relu=1)
    torch.cuda.synchronize()
    assert (out[:n3].cpu().double() - torch.relu(y64)).abs().max().item() < 1e-4 * max(1.0, torch.relu(y64).abs().max().item())
    assert torch.equal(out[n3:].cpu(), torch.relu(shift).expand(ix.cap3 - n3, -1))


def test_refusals(ops):
    from laudnet_amd._lib import LdnError
    prob = _problem(*CASES[1])
    ix, n3, a, w, scale, shift, _ = prob
    C = w.shape[0]
    frag = ops.pack_grouped_wide_weights(w.to(DEV), 56)
    out = torch.full((ix.cap3, C), SENTINEL, device=DEV)
    args = (scale.to(DEV), shift.to(DEV), out)
    kw = dict(m_count=ix.cnt[0:1], m_cap=ix.cap3)
    with pytest.raises(LdnError):                   # truncated by 16 bytes
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag.reshape(-1)[:-8], 56, *args, **kw)
    with pytest.raises(LdnError):                   # fragments of the other width
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag, 112, *args, **kw)
    with pytest.raises(LdnError):                   # fp32 fragments
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag.float(), 56, *args, **kw)
    with pytest.raises(LdnError, match="not built"):        # width 24
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, ops.pack_grouped_mfma_weights(torch.zeros(C, 9, 24, device=DEV), 24), 24, *args, **kw)
    assert not ops.grouped_wide_rows_ok(C, 24)
    with pytest.raises(LdnError):                   # a row stride that is no multiple of 4: refused by the entry point itself
        wide = torch.full((ix.cap3, C + 2), SENTINEL, device=DEV)
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag, 56, scale.to(DEV), shift.to(DEV), wide[:, :C], **kw)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((wide == SENTINEL).all())


# ------------------------------------------------------------------ the dispatch switch
def _counted(ops, monkeypatch):
    """counting wrappers around the new op and the VALU op it replaces -> (calls of the new one, calls of the old one), group widths"""
    new, old = [], []
    real_new, real_old = ops.grouped_wide_conv3x3_rows, ops.grouped_conv3x3_rows

    def counted_new(a2d, nbr, w_frag, group_width, *args, **kwargs):
        new.append(group_width)
        return real_new(a2d, nbr, w_frag, group_width, *args, **kwargs)

    def counted_old(a2d, nbr, w, group_width, *args, **kwargs):
        old.append(group_width)
        return real_old(a2d, nbr, w, group_width, *args, **kwargs)
    monkeypatch.setattr(ops, "grouped_wide_conv3x3_rows", counted_new)
    monkeypatch.setattr(ops, "grouped_conv3x3_rows", counted_old)
    return new, old


def _block_out(gw, stride, on, monkeypatch, ops):
    """one seeded layer-skip ResBottleneckBlock 2 gw -> 2 gw (w_b = 2 gw: two groups), output 7 x 7, a forced per-image mask with a skipped
    image between kept ones -> (output, new calls, old calls); on = None leaves the switch as the module has it"""
    from laudnet_amd import laud_regnet
    if on is not None:
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE_ROWS", on)
    W = 2 * gw
    blk = laud_regnet.ResBottleneckBlock(W, W, stride, lambda c: nn.BatchNorm2d(c, eps=1e-5, momentum=0.1), nn.ReLU, group_width=gw,
                                         bottleneck_multiplier=1.0, se_ratio=0.25, output_size=7, mask_spatial_granularity=7,
                                         dyn_mode="spatial").eval()
    assert (blk.proj is not None) == (stride == 2) and blk.f.group_width == gw and blk.f.w_b == W and blk.f.mask_size == 1
    blk.load_state_dict(fill_state_dict(blk.state_dict(), 77 + gw))
    blk = blk.to(DEV)
    B = 4
    blk.f.forced_spatial_mask = torch.tensor([1.0, 0.0, 1.0, 1.0]).view(B, 1, 1, 1)
    x = torch.relu(seeded_randn((B, W, 7 * stride, 7 * stride), 700 + gw)).to(DEV)
    new, old = _counted(ops, monkeypatch)
    with torch.no_grad():
        out, stats = blk.run_dynamic(x)
    torch.cuda.synchronize()
    return out.clone(), list(new), list(old)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("gw", [56, 112])
def test_block_dispatch_at_widths_56_and_112(ops, monkeypatch, gw, stride):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS is False
    on, new, old = _block_out(gw, stride, True, monkeypatch, ops)
    assert new == [gw] and old == [], (new, old)
    monkeypatch.undo()
    off, new, old = _block_out(gw, stride, False, monkeypatch, ops)
    assert new == [] and old == [gw], (new, old)
    err, bound = (on - off).abs().max().item(), 1e-4 * max(1.0, off.abs().max().item())
    print(f"layer-skip block gw {gw} stride {stride}: switch on vs off max |diff| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(on).all() and err < bound


@pytest.mark.parametrize("gw", [56, 112])
def test_default_switch_never_calls_the_new_op(ops, monkeypatch, gw):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS is False
    _, new, old = _block_out(gw, 1, None, monkeypatch, ops)
    assert new == [] and old == [gw], (new, old)
