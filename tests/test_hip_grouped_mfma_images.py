"""GPU tests of the whole-image and SE-fused matrix-core grouped 3x3 at group widths 8 and 24 (ops.grouped_mfma_conv3x3_images[_gap] ->
ldn_grouped_mfma_conv3x3_images[_gap], k_grouped_gw_img; bf16x3).

1. against F.conv2d(groups = C / gw) in float64 at the kept images, bound 1e-4 max(1, |want|max) -- the bound of every kernel of this family
   (tests/test_hip_grouped_mfma.py) -- on inputs built as that file builds them: NaN in the rows outside the list, sentinel pad columns,
   lda = C + 8, ldo = C + 4, zero and negative scales; with and without ReLU; twice, bit for bit; nothing kept writes nothing;
2. bit-identical to ops.grouped_mfma_conv3x3_rows over the same lists' neighbour table;
3. the _gap form: the plain form's output bit for bit, gap [B, bands, C] bit-identical over two launches and within 1e-5 max(1, |ref|max)
   (tests/test_hip_se_fused.py) of the float64 sums of the kernel's own output -- with negative scales and no ReLU, so a padded lane or a
   dropped accumulator quad that added its value would show;
4. refusals raise LdnError and write nothing;
5. a layer-skip ResBottleneckBlock at RegNetY-400MF / -1.6GF shapes: the three-launch b -> SE -> c against today's path, and the image form
   against the row form bit for bit;
6. regnet_tiny.pt (group width 8) with both switches on, through the comparison of tests/test_hip_grouped_mfma.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0

# (gw, B, Ho, Wo, stride, C, keep)
CASES = [(8, 2, 5, 5, 1, 8, 1.0),          # one group, 25 pixels: one full and one partial tile
         (8, 4, 7, 7, 1, 440, 0.5),        # 55 groups, several chunks
         (8, 5, 14, 14, 2, 208, 0.4),      # stride 2, whole image
         (8, 3, 28, 28, 1, 104, 0.6),      # 13 groups, odd count
         (8, 3, 56, 56, 2, 48, 0.7),       # banded, stride 2 from 112 x 112
         (8, 2, 6, 10, 1, 24, 1.0),        # non-square
         (24, 2, 5, 5, 1, 24, 1.0),        # one group, less than one 32-pixel tile
         (24, 4, 7, 7, 1, 888, 0.5),       # 37 groups
         (24, 5, 14, 14, 2, 336, 0.4),     # stride 2
         (24, 3, 28, 28, 1, 120, 0.6),     # 5 groups
         (24, 2, 56, 56, 1, 48, 1.0),      # banded, stride 1
         (24, 3, 56, 56, 2, 48, 0.7),      # banded, stride 2
         (24, 2, 10, 6, 2, 72, 1.0),       # non-square, stride 2
         (8, 4, 9, 9, 2, 24, 0.0),         # nothing kept
         (24, 4, 9, 9, 2, 48, 0.0)]        # nothing kept
BANDED = {(8, 56, 2), (24, 56, 1), (24, 56, 2)}      # (gw, Ho, stride) of the cases the plan cuts into bands


@pytest.fixture(autouse=True)
def _bf16x3():
    from laudnet_amd import ops
    ops.set_math_mode("bf16x3")
    yield
    ops.set_math_mode("fp32")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()
    return _ops


@functools.lru_cache(maxsize=None)
def _problem(gw, B, Ho, Wo, stride, C, keep):
    """-> (ix, kept, a [cap1, C + 8] on the device, w [C, 9, gw], scale, shift, y64 [kept Ho Wo, C] = scale conv + shift in float64 at the kept
    images); built once per case and shared by every test, never modified"""
    from laudnet_amd import ops
    Hi, Wi = Ho * stride, Wo * stride
    patch = seeded_bernoulli((B, 1, 1), keep, 320 + C + B + gw)
    ix = ops.mask_to_index(patch.to(DEV), Ho, Wo, stride)
    n3, n1 = int(ix.cnt[0].item()), int(ix.cnt[1].item())
    kept = int(patch.sum().item())
    assert n3 == kept * Ho * Wo and n1 == kept * Hi * Wi and ix.cap3 == B * Ho * Wo and ix.cap1 == B * Hi * Wi
    x = seeded_randn((B, C, Hi, Wi), 292 + C)
    w = seeded_randn((C, gw, 3, 3), 293 + C) * 0.1
    scale = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(294))
    scale[0::5] = 0.0
    scale[1::5] = -scale[1::5]
    shift = 0.1 * seeded_randn((C,), 295)
    xk = x[patch.view(B) > 0]                               # the kept images, in order: image k of them owns the rows [k Hi Wi, (k + 1) Hi Wi)
    if kept:
        y = F.conv2d(xk.double(), w.double(), None, stride, 1, 1, C // gw) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        y64 = y.permute(0, 2, 3, 1).reshape(kept * Ho * Wo, C)
    else:
        y64 = torch.zeros(0, C, dtype=torch.float64)
    a = torch.full((ix.cap1, C + 8), float("nan"))        # rows outside the list: NaN
    a[:n1] = SENTINEL * 1e6                               # the pad columns of the listed rows
    a[:n1, :C] = xk.permute(0, 2, 3, 1).reshape(kept * Hi * Wi, C)
    return ix, kept, a.to(DEV), w.permute(0, 2, 3, 1).reshape(C, 9, gw).contiguous(), scale, shift, y64


def _images(case):
    gw, B, Ho, Wo, stride, C, keep = case
    return (B, Ho * stride, Wo * stride, Ho, Wo, stride)


def _run(ops, case, relu, form="images"):
    """-> out [cap3, C + 4] (sentinel outside what the kernel writes), and gap for form 'gap'"""
    gw = case[0]
    ix, kept, a, w, scale, shift, _ = _problem(*case)
    C = w.shape[0]
    frag = ops.pack_grouped_mfma_weights(w.to(DEV), gw)
    out = torch.full((ix.cap3, C + 4), SENTINEL, device=DEV)
    gap = None
    if form == "rows":
        ops.grouped_mfma_conv3x3_rows(a[:, :C], ix.nbr, frag, gw, scale.to(DEV), shift.to(DEV), out[:, :C], m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=relu)
    elif form == "gap":
        gap = ops.grouped_mfma_conv3x3_images_gap(a[:, :C], frag, gw, scale.to(DEV), shift.to(DEV), out[:, :C], m_count=ix.cnt[0:1],
                                                  images=_images(case), relu=relu)
    else:
        ops.grouped_mfma_conv3x3_images(a[:, :C], frag, gw, scale.to(DEV), shift.to(DEV), out[:, :C], m_count=ix.cnt[0:1], images=_images(case), relu=relu)
    torch.cuda.synchronize()
    return out, gap


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_images_vs_float64(ops, case, relu):
    gw, B, Ho, Wo, stride, C, keep = case
    ix, kept, a, w, scale, shift, y64 = _problem(*case)
    assert ops.grouped_mfma_images_fit(Ho * stride, Wo * stride, C, gw) > 0
    bands = ops.grouped_mfma_images_bands(Ho * stride, Wo * stride, Ho, stride, C, gw)
    assert (bands >= 2) == ((gw, Ho, stride) in BANDED), bands
    assert kept == (B if keep == 1.0 else 0) or 0 < kept < B
    assert a.stride(0) == C + 8
    n3 = kept * Ho * Wo
    out, _ = _run(ops, case, relu)
    assert bool((out[n3:] == SENTINEL).all()), "rows at or past the device-side count must not be written"
    assert bool((out[:, C:] == SENTINEL).all()), "columns past C must not be written"
    assert torch.equal(_run(ops, case, relu)[0], out), "two runs differ"
    if keep == 0.0:
        assert n3 == 0 and bool((out == SENTINEL).all())
        return
    want = torch.relu(y64) if relu else y64
    got = out[:n3, :C].cpu()
    assert torch.isfinite(got).all()
    err, bound = (got.double() - want).abs().max().item(), 1e-4 * max(1.0, want.abs().max().item())
    print(f"grouped_mfma images gw {gw} C {C} {Ho}x{Wo} s{stride} rows {n3} relu {relu}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    if not relu:
        assert bool((got < 0).any())
        zero = scale == 0
        assert torch.equal(got[:, zero], shift[zero].expand(n3, -1)), "a zero scale leaves the shift"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_images_are_bit_identical_to_the_row_form(ops, case, relu):
    assert torch.equal(_run(ops, case, relu)[0], _run(ops, case, relu, form="rows")[0])


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_gap_form_leaves_the_channel_sums_of_its_output(ops, case, relu):
    """relu 0 with the negative scales: the sums are of signed values, and a lane without output (width 8: kg >= 2; width 24: quad 3) that added
    the value it computed -- the shift of a channel that is not its own, at the least -- would move them past the bound."""
    gw, B, Ho, Wo, stride, C, keep = case
    kept = _problem(*case)[1]
    n3 = kept * Ho * Wo
    want, _ = _run(ops, case, relu)
    got, gap = _run(ops, case, relu, form="gap")
    gap2 = _run(ops, case, relu, form="gap")[1]
    assert torch.equal(got, want)
    bands = ops.grouped_mfma_images_bands(Ho * stride, Wo * stride, Ho, stride, C, gw)
    assert gap.shape == (B, bands, C) and bands >= 1
    assert torch.equal(gap[:kept], gap2[:kept])
    if kept:
        ref = got[:n3, :C].double().view(kept, Ho * Wo, C).sum(dim=1)
        err, bound = (gap[:kept].double().sum(dim=1) - ref).abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item())
        print(f"grouped_mfma images gap gw {gw} C {C} {Ho}x{Wo} s{stride} bands {bands} relu {relu}: max |err| {err:.3e} (bound {bound:.3e})")
        assert err < bound
        if not relu:
            assert bool((ref < 0).any())


def test_refusals(ops):
    from laudnet_amd._lib import LdnError
    case = CASES[5]                                       # (8, 2, 6, 10, 1, 24, 1.0)
    ix, kept, a, w, scale, shift, _ = _problem(*case)
    C, images = w.shape[0], _images(case)
    frag = ops.pack_grouped_mfma_weights(w.to(DEV), 8)
    out = torch.full((ix.cap3, C), SENTINEL, device=DEV)
    sc, sh = scale.to(DEV), shift.to(DEV)
    kw = dict(m_count=ix.cnt[0:1], images=images)
    for f in (ops.grouped_mfma_conv3x3_images, ops.grouped_mfma_conv3x3_images_gap):
        with pytest.raises(LdnError):
            f(a[:, :C], frag, 24, sc, sh, out, **kw)                                   # fragments of the other width
        with pytest.raises(LdnError):
            f(a[:, :C], frag.reshape(-1)[:-16], 8, sc, sh, out, **kw)                  # truncated
        with pytest.raises(LdnError):
            f(a[:, :C], frag.float(), 8, sc, sh, out, **kw)
        with pytest.raises(LdnError):
            f(a[:, :C], ops.pack_grouped16_weights(torch.zeros(32, 9, 16, device=DEV)), 16, sc, sh, out, **kw)
        with pytest.raises(LdnError):                                                  # a row stride that is no multiple of 4: the entry point itself
            wide = torch.full((ix.cap3, C + 2), SENTINEL, device=DEV)
            f(a[:, :C], frag, 8, sc, sh, wide[:, :C], **kw)
        with pytest.raises(LdnError):
            f(a[:ix.cap1 - 1, :C], frag, 8, sc, sh, out, **kw)                         # a / out shorter than B whole images
        with pytest.raises(LdnError):
            f(a[:, :C], frag, 8, sc, sh, out[:ix.cap3 - 1], **kw)
        with pytest.raises(LdnError):
            f(a[:, :C], frag, 8, sc, sh, out, m_count=ix.cnt[0:1], images=(2, 6, 10, 6, 10, 3))      # stride 3
        with pytest.raises(LdnError):
            f(a[:, :C], frag, 8, sc, sh, out, m_count=ix.cnt[0:1], images=(2, 6, 10, 5, 10, 1))      # Ho of another geometry
        # a map of which three input rows do not fit the LDS
        Wi = 1 << 14
        assert ops.grouped_mfma_images_fit(3, Wi, C, 8) == 0
        big_a, big_out = torch.zeros(3 * Wi, C, device=DEV), torch.full((3 * Wi, C), SENTINEL, device=DEV)
        with pytest.raises(LdnError):
            f(big_a, frag, 8, sc, sh, big_out, m_count=ix.cnt[0:1], images=(1, 3, Wi, 3, Wi, 1))
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((wide == SENTINEL).all()) and bool((big_out == SENTINEL).all())


# ------------------------------------------------------------------ a layer-skip block: b -> SE -> c in three launches
def _block(gw, stride, Hi, w_in, w_out):
    import torch.nn as nn
    from functools import partial
    from laudnet_amd import laud_regnet
    Ho = Hi // stride
    blk = laud_regnet.ResBottleneckBlock(w_in, w_out, stride, partial(nn.BatchNorm2d), nn.ReLU, group_width=gw, bottleneck_multiplier=1.0,
                                         se_ratio=0.25, output_size=Ho, mask_spatial_granularity=Ho, dyn_mode="spatial").eval()
    blk.load_state_dict(fill_state_dict(blk.state_dict(), 51))
    blk = blk.to(DEV)
    B = 12
    x = torch.relu(seeded_randn((B, w_in, Hi, Hi), 52)).to(DEV).contiguous(memory_format=torch.channels_last)
    blk.f.forced_spatial_mask = seeded_bernoulli((B, 1, 1, 1), 0.6, 53).to(DEV)
    return blk, x


def _count(ops, monkeypatch, names):
    calls = {n: 0 for n in names}

    def wrap(name, real):
        def counted(*args, **kwargs):
            calls[name] += 1
            return real(*args, **kwargs)
        return counted
    for n in names:
        monkeypatch.setattr(ops, n, wrap(n, getattr(ops, n)))
    return calls


OPS = ("grouped_mfma_conv3x3_images_gap", "grouped_mfma_conv3x3_images", "grouped_mfma_conv3x3_rows", "se_gate_slots", "conv_rows_gated", "se_packed")


@pytest.mark.parametrize("gw,stride,Hi,w_in,w_out", [(24, 1, 14, 336, 336), (24, 2, 28, 120, 336), (24, 1, 7, 888, 888),
                                                     (8, 1, 14, 208, 208), (8, 2, 28, 104, 208), (8, 1, 7, 440, 440)])
def test_block_with_folded_se_matches_todays_path(ops, monkeypatch, gw, stride, Hi, w_in, w_out):
    """the new switch on against off (LDN_GROUPED_MFMA_WIDTHS on in both): equal to the fp32 rounding of the two orders of the channel sums, the
    bound of tests/test_hip_se_fused.py; and with LDN_SE_FUSED off in both runs the image form against the row form, bit for bit"""
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS", True)
    blk, x = _block(gw, stride, Hi, w_in, w_out)
    calls = _count(ops, monkeypatch, OPS)

    def run(images_on, se_fused):
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS_IMAGES", images_on)
        monkeypatch.setattr(laud_regnet, "USE_SE_FUSED", se_fused)
        for n in calls:
            calls[n] = 0
        with torch.no_grad():
            y, _ = blk.run_dynamic(x)
        torch.cuda.synchronize()
        return y.clone(), dict(calls)
    y_new, c_new = run(True, True)
    y_old, c_old = run(False, True)
    assert c_new == dict(grouped_mfma_conv3x3_images_gap=1, grouped_mfma_conv3x3_images=0, grouped_mfma_conv3x3_rows=0, se_gate_slots=1,
                         conv_rows_gated=1, se_packed=0), c_new
    assert c_old == dict(grouped_mfma_conv3x3_images_gap=0, grouped_mfma_conv3x3_images=0, grouped_mfma_conv3x3_rows=1, se_gate_slots=0,
                         conv_rows_gated=0, se_packed=1), c_old
    assert torch.isfinite(y_new).all()
    err, bound = (y_new - y_old).abs().max().item(), 1e-5 * max(1.0, y_old.abs().max().item())
    print(f"block gw {gw} stride {stride} {Hi}x{Hi} {w_in}->{w_out}: fused vs today's path max |delta| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    y_img, c_img = run(True, False)
    y_row, c_row = run(False, False)
    assert c_img["grouped_mfma_conv3x3_images"] == 1 and c_img["grouped_mfma_conv3x3_rows"] == 0 and c_img["se_packed"] == 1, c_img
    assert c_row["grouped_mfma_conv3x3_images"] == 0 and c_row["grouped_mfma_conv3x3_rows"] == 1 and c_row["se_packed"] == 1, c_row
    assert torch.equal(y_img, y_row)


# ------------------------------------------------------------------ the dispatch switches on regnet_tiny.pt (group width 8)
@pytest.mark.parametrize("case,run", [("layerskip", "injected_run"), ("layerskip", "masker_run"), ("spatial_g2", "injected_run")])
def test_regnet_tiny_on_the_image_form(ops, monkeypatch, case, run):
    """the comparison and the bounds of tests/test_hip_grouped_mfma.py::_regnet_run, both switches on"""
    import test_hip_grouped_mfma as rows_tests
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS", True)
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS_IMAGES", True)
    calls = _count(ops, monkeypatch, OPS)
    rows_tests._regnet_run(case, run, run == "injected_run")
    print(f"regnet_tiny {case} {run}: {calls}")
    assert calls["grouped_mfma_conv3x3_images_gap"] + calls["grouped_mfma_conv3x3_images"] >= 1, calls
    if case == "layerskip":
        assert calls["grouped_mfma_conv3x3_images_gap"] >= 1 and calls["grouped_mfma_conv3x3_rows"] == 0, calls
