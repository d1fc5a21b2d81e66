"""GPU tests of the matrix-core packed-row grouped 3x3 at group width 232, the width of lad_regnet_y_32gf (ops.grouped_wide_conv3x3_rows ->
ldn_grouped_wide_conv3x3_rows, k_grouped_wide_rows<232>, bf16x3) against F.conv2d(groups = C / 232) in float64 at the kept pixels, bound
1e-4 max(1, |want|max): the project's bound for every matrix-core grouped kernel.  The construction of tests/test_hip_grouped_wide_rows.py:
the lists of ops.mask_to_index, NaN in the input rows past the dilated list, sentinels in the pad columns of a (lda = C + 8) and of out, zero
and negative scales, with and without ReLU, twice, bit for bit.  What this width adds: the eighth row tile holds 24 pad out channels
(232-255) and K ends in a pad octet (261).  The output buffer is ldo = C + 32 wide, so a pad channel that were stored would land INSIDE it (in
a non-last group: in the next group's columns, which are checked group by group against float64).  Every case runs through the plan's own
form and through each form compiled for this width ("b1" = every row tile in one wave, one pixel tile; "a" = one row tile x four pixel tiles
per wave); "b2" / "b4" are not compiled at this width and must give the plan's result bit for bit.  Then the dispatch of a layer-skip block
with w_b = 464."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
GW = 232
PAD = 32                   # out's pad columns: more than the 24 pad out channels of the last row tile

# (gw, B, Ho, stride, C, keep)
CASES = [(232, 1, 5, 1, 232, 1.0),        # one group, 25 rows: less than one tile
         (232, 2, 7, 2, 464, 0.6),        # two groups, stride 2
         (232, 3, 14, 1, 464, 0.5),       # ragged last tile
         # One pixel tile of 32 rows per wave at this width (two would be 256 accumulator registers), four waves per workgroup = 128 rows; the
         # "a" form keeps four tiles per wave = 512 rows.  12 x 12 = 144 rows = 5 tiles is the smallest square map past the 128 rows of the
         # launched form (the second workgroup has one live wave); 17 x 17 = 289 rows = 10 tiles (three workgroups, the last with two live
         # waves) is the case of the other widths; 23 x 23 = 529 rows is the smallest square map past the 512 rows of the "a" form.
         (232, 1, 12, 1, 232, 1.0),
         (232, 1, 17, 1, 232, 1.0),
         (232, 1, 23, 1, 232, 1.0),
         (232, 1, 4, 1, 3712, 1.0)]       # the 16 groups of the model's stage 4


@pytest.fixture(autouse=True)
def _bf16x3():
    from laudnet_amd import ops
    ops.set_math_mode("bf16x3")
    yield
    ops.set_math_mode("fp32")


@pytest.fixture(params=[None, "b1", "a"], ids=["plan", "all_row_tiles", "one_row_tile"])
def form(request, monkeypatch):
    """the launch plan's choice, or one of the two forms compiled at this width"""
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
    built once per case and shared by every run, never modified"""
    from laudnet_amd import ops
    Hi = Ho * stride
    if single:
        patch = torch.zeros(B, Ho, Ho)
        patch[B - 1, Ho // 2, 1] = 1.0
    else:
        patch = seeded_bernoulli((B, Ho, Ho), keep, 291 + C)
    ix = ops.mask_to_index(patch.to(DEV), Ho, Ho, stride)
    n3, n1 = int(ix.cnt[0].item()), int(ix.cnt[1].item())
    x = seeded_randn((B, C, Hi, Hi), 292 + C)
    w = seeded_randn((C, gw, 3, 3), 293 + C) * 0.05
    scale = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(294))
    scale[0::5] = 0.0
    scale[1::5] = -scale[1::5]
    shift = 0.1 * seeded_randn((C,), 295)
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


@functools.lru_cache(maxsize=None)
def _frag(gw, B, Ho, stride, C, keep, single=False):
    from laudnet_amd import ops
    return ops.pack_grouped_wide_weights(_problem(gw, B, Ho, stride, C, keep, single)[3].to(DEV), gw)


def _run(ops, prob, frag, relu, m_count="list"):
    ix, n3, a, w, scale, shift, _ = prob
    C = w.shape[0]
    out = torch.full((ix.cap3, C + PAD), SENTINEL, device=DEV)
    cnt = ix.cnt[0:1] if m_count == "list" else m_count
    ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag, GW, scale.to(DEV), shift.to(DEV), out[:, :C], m_count=cnt, m_cap=ix.cap3, relu=relu)
    torch.cuda.synchronize()
    return out


def _check(ops, prob, frag, relu):
    ix, n3, a, w, scale, shift, y64 = prob
    C = w.shape[0]
    assert a.stride(0) == C + 8
    out = _run(ops, prob, frag, relu)
    assert out.stride(0) == C + PAD
    want = torch.relu(y64) if relu else y64
    got = out[:n3, :C].cpu()
    assert torch.isfinite(got).all()
    bound = 1e-4 * max(1.0, want.abs().max().item())
    for g in range(C // GW if C // GW <= 2 else 1):           # two groups: each group's columns on their own
        cols = slice(g * GW, (g + 1) * GW) if C // GW <= 2 else slice(0, C)
        err = (got[:, cols].double() - want[:, cols]).abs().max().item()
        print(f"grouped_wide_rows gw {GW} C {C} rows {n3} relu {relu} columns {cols.start}:{cols.stop}: max |err| {err:.3e} (bound {bound:.3e})")
        assert err < bound
    assert bool((out[n3:] == SENTINEL).all()), "rows at or past the device-side count must not be written"
    assert bool((out[:, C:] == SENTINEL).all()), "columns past C (where the pad out channels 232-255 of the last group would land) must not be written"
    if not relu:
        assert bool((got < 0).any())
        zero = scale == 0
        assert torch.equal(got[:, zero], shift[zero].expand(n3, -1)), "a zero scale leaves the shift"
    assert torch.equal(_run(ops, prob, frag, relu), out), "two runs differ"
    return out


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gw,B,Ho,stride,C,keep", CASES)
def test_grouped_wide_conv3x3_rows_232_vs_float64(ops, form, gw, B, Ho, stride, C, keep, relu):
    from laudnet_amd import _lib
    assert ops.grouped_wide_rows_ok(C, gw)
    prob = _problem(gw, B, Ho, stride, C, keep)
    ix, n3 = prob[0], prob[1]
    assert _lib.load().ldn_grouped_wide_rows_tiles(C, gw, ix.cap3) == 1, "one pixel tile per wave at this width"
    if keep < 1:
        assert 0 < n3 < ix.cap3
    else:
        assert n3 == ix.cap3
    if Ho == 12:
        assert n3 == 144 and 11 * 11 <= 4 * 32 < n3, "the smallest square map with more rows than one workgroup of the launched form holds (4 waves x 1 tile of 32)"
    if Ho == 17:
        assert n3 == 289 and n3 > 2 * 4 * 32, "more than two workgroups of the launched form"
    if Ho == 23:
        assert n3 == 529 and n3 > 4 * 4 * 32, "more rows than one workgroup of the 'a' form holds (4 waves x 4 tiles of 32)"
    if Ho == 14:
        assert n3 % 32, "a ragged last tile"
    _check(ops, prob, _frag(gw, B, Ho, stride, C, keep), relu)


@pytest.mark.parametrize("uncompiled", ["b2", "b4"])
@pytest.mark.parametrize("gw,B,Ho,stride,C,keep", [CASES[2], CASES[4]])
def test_a_form_that_is_not_compiled_at_this_width_runs_the_plans_choice(ops, monkeypatch, uncompiled, gw, B, Ho, stride, C, keep):
    prob, frag = _problem(gw, B, Ho, stride, C, keep), _frag(gw, B, Ho, stride, C, keep)
    monkeypatch.delenv("LDN_GROUPED_WIDE_ROWS_FORM", raising=False)
    plan = _run(ops, prob, frag, 1)
    monkeypatch.setenv("LDN_GROUPED_WIDE_ROWS_FORM", uncompiled)
    got = _check(ops, prob, frag, 1)
    assert torch.equal(got, plan)


@pytest.mark.parametrize("relu", [1, 0])
def test_one_kept_pixel(ops, form, relu):
    prob = _problem(GW, 2, 5, 1, 464, 0.0, single=True)
    assert prob[1] == 1
    _check(ops, prob, _frag(GW, 2, 5, 1, 464, 0.0, single=True), relu)


def test_a_device_side_count_of_zero_writes_nothing(ops, form):
    prob = _problem(*CASES[1])
    out = _run(ops, prob, _frag(*CASES[1]), 1, m_count=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert bool((out == SENTINEL).all())


def test_no_count_means_m_cap_rows(ops, form):
    """the rows past the list read whatever their table entries name, so they are pointed at the zero row: exactly relu(shift)"""
    ix, n3, a, w, scale, shift, y64 = _problem(*CASES[1])
    C = w.shape[0]
    assert 0 < n3 < ix.cap3
    nbr = ix.nbr.view(-1, 9).clone()
    nbr[n3:] = -1
    out = torch.full((ix.cap3, C + PAD), SENTINEL, device=DEV)
    ops.grouped_wide_conv3x3_rows(a[:, :C], nbr.reshape(-1).contiguous(), _frag(*CASES[1]), GW, scale.to(DEV), shift.to(DEV), out[:, :C], relu=1)
    torch.cuda.synchronize()
    assert (out[:n3, :C].cpu().double() - torch.relu(y64)).abs().max().item() < 1e-4 * max(1.0, torch.relu(y64).abs().max().item())
    assert torch.equal(out[n3:, :C].cpu(), torch.relu(shift).expand(ix.cap3 - n3, -1))
    assert bool((out[:, C:] == SENTINEL).all())


def test_refusals(ops):
    from laudnet_amd._lib import LdnError
    ix, n3, a, w, scale, shift, _ = _problem(*CASES[1])
    C = w.shape[0]
    frag = _frag(*CASES[1])
    out = torch.full((ix.cap3, C), SENTINEL, device=DEV)
    args = (scale.to(DEV), shift.to(DEV), out)
    kw = dict(m_count=ix.cnt[0:1], m_cap=ix.cap3)
    with pytest.raises(LdnError):                   # truncated by 16 bytes
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag.reshape(-1)[:-8], GW, *args, **kw)
    with pytest.raises(LdnError):                   # fragments of another width of the family
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag, 112, *args, **kw)
    with pytest.raises(LdnError):                   # fp32 fragments
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag.float(), GW, *args, **kw)
    with pytest.raises(LdnError, match="not built"):        # width 116: half of this one
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag, 116, *args, **kw)
    with pytest.raises(LdnError, match="not built"):        # width 264 (RegNetY-128GF)
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag, 264, *args, **kw)
    assert not ops.grouped_wide_rows_ok(C, 116) and not ops.grouped_wide_rows_ok(240, GW) and not ops.grouped_wide_rows_ok(528, 264)
    with pytest.raises(LdnError):                   # a row stride that is no multiple of 4: refused by the entry point itself
        wide = torch.full((ix.cap3, C + 2), SENTINEL, device=DEV)
        ops.grouped_wide_conv3x3_rows(a[:, :C], ix.nbr, frag, GW, scale.to(DEV), shift.to(DEV), wide[:, :C], **kw)
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


def _block_out(stride, on, monkeypatch, ops):
    """one seeded layer-skip ResBottleneckBlock 464 -> 464 (w_b = 464: two groups of 232), output 7 x 7, a forced per-image mask with a skipped
    image between kept ones -> (output, new calls, old calls); on = None leaves the switch as the module has it"""
    from laudnet_amd import laud_regnet
    if on is not None:
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDE_ROWS", on)
    W = 2 * GW
    blk = laud_regnet.ResBottleneckBlock(W, W, stride, lambda c: nn.BatchNorm2d(c, eps=1e-5, momentum=0.1), nn.ReLU, group_width=GW,
                                         bottleneck_multiplier=1.0, se_ratio=0.25, output_size=7, mask_spatial_granularity=7,
                                         dyn_mode="spatial").eval()
    assert (blk.proj is not None) == (stride == 2) and blk.f.group_width == GW and blk.f.w_b == W and blk.f.mask_size == 1
    blk.load_state_dict(fill_state_dict(blk.state_dict(), 77 + GW))
    blk = blk.to(DEV)
    B = 4
    blk.f.forced_spatial_mask = torch.tensor([1.0, 0.0, 1.0, 1.0]).view(B, 1, 1, 1)
    x = torch.relu(seeded_randn((B, W, 7 * stride, 7 * stride), 700 + GW)).to(DEV)
    new, old = _counted(ops, monkeypatch)
    with torch.no_grad():
        out, stats = blk.run_dynamic(x)
    torch.cuda.synchronize()
    return out.clone(), list(new), list(old)


@pytest.mark.parametrize("stride", [1, 2])
def test_block_dispatch_at_width_232(ops, monkeypatch, stride):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS is False
    on, new, old = _block_out(stride, True, monkeypatch, ops)
    assert new == [GW] and old == [], (new, old)
    monkeypatch.undo()
    off, new, old = _block_out(stride, False, monkeypatch, ops)
    assert new == [] and old == [GW], (new, old)
    err, bound = (on - off).abs().max().item(), 1e-4 * max(1.0, off.abs().max().item())
    print(f"layer-skip block gw {GW} stride {stride}: switch on vs off max |diff| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(on).all() and err < bound


def test_default_switch_never_calls_the_new_op(ops, monkeypatch):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS is False
    _, new, old = _block_out(1, None, monkeypatch, ops)
    assert new == [] and old == [GW], (new, old)
