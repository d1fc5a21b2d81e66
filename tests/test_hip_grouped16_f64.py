"""k_grouped16_mfma and k_grouped16_img (csrc/ldn_grouped.hip: the width-16 matrix-core conv b of LAD-RegNet, the only one on by default)
against float64 at their edges, through the C ABI on buffers the test owns.

What tests/test_hip_ops.py and tests/test_hip_se_fused.py leave open: a wave of the row kernel never takes a second tile there (the launch
caps the grid at a few workgroups per CU, so that needs hundreds of thousands of rows); lda == ldo == C; ReLU always on; scales in
[0.5, 1.5]; always a device-side count below m_cap; square maps with Hi = Ho * stride.  Here:
  rows    neighbour tables of ops.mask_to_index (1 .. 49 groups, one kept pixel), tables with no geometry behind them (a row names one
          input row in several taps, any order), counts of zero / one / NULL / above m_cap, and row counts sized from the device's CU count
          so that every wave takes a second tile and some a third;
  images  non-square maps, odd heights and widths at stride 2, 1 .. 8 bands, one pixel, nothing kept, images_cap below the count, more than
          eight (image, band) pairs; the _gap form's output equal to the plain form's bit for bit, its sums per band; the image form equal
          to the row kernel bit for bit over the table of the same geometry;
  refusals leave the output as it was.
Inputs: lda = C + 8 with a large finite sentinel in the pad columns of the listed rows, NaN in every row that no table entry or kept image
names, ldo = C + 4, scale[0::5] = 0, scale[1::5] < 0; ReLU on and off; every launch twice, bit for bit.  `out` and `gap` sit inside larger
flat tensors between guards of 4096 floats filled with a sentinel and are NaN before each launch: afterwards the guards are bit-identical,
the columns C .. ldo of every row and the rows at or past the count still hold that NaN, and everything that must be written is free of it.

Reference: tests/grouped16_ref.py in float64 from the float32 tensors the kernel receives (tests/test_grouped16_ref.py ties its two forms
together on the CPU).  Bounds:
  output  |got - ref| <= 1e-4 max(1, |ref|max)    the family's bound (tests/test_hip_ops.py::test_grouped16_conv3x3_rows_mfma_vs_torch);
          the bf16x3 arithmetic alone, emulated on the CPU over the inputs of the small cases, reaches 0.07 of it
          (tests/test_grouped16_pack.py::test_the_arithmetic_alone_is_inside_the_gpu_bound)
  gap     |sum over bands - float64 sum of the kernel's own output| <= 1e-5 max(1, |sum|max) per image (tests/test_hip_se_fused.py), and
          per band |gap - float64 band sum of the reference| <= pixels of the band * 1e-4 max(1, |ref|max): the per-pixel bound summed
          (tests/test_hip_stem_f64.py)
Measured on an MI355X (256 CUs) when these tests were written: worst error / bound 0.069 for k_grouped16_mfma (0.049 and 0.065 on the
multi-tile cases: 611 737 rows at C = 64 in 0.3 s, 101 913 rows at C = 400 in less than 0.1 s, reference included), 0.059 for
k_grouped16_img, 0.025 for its channel sums against its own output and 0.044 against the reference's band sums.  No defect: every test
passed on the library as it was."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

import grouped16_cases as K
import grouped16_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                     # floats in front of and behind every payload (16 KiB: payload offsets stay 16-byte aligned)
SENTINEL = -7.25e5               # the guards: finite, exactly representable, far from every value of the tests
PAD_IN = -7.0e6                  # the pad columns C .. lda of the listed input rows
NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _lib():
    import laudnet_amd._lib as L
    from laudnet_amd import load_library
    load_library()
    return L, L.load()


@functools.lru_cache(maxsize=None)
def _cus():
    _, lib = _lib()
    c = ctypes.c_int(0)
    assert lib.ldn_device_cus(ctypes.byref(c)) == 0 and c.value > 0
    return c.value


class _Banded:
    """n floats on the device between two guards: payload NaN, guards SENTINEL."""

    def __init__(self, n):
        self.n = n
        self.flat = torch.full((GUARD + n + GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
        self.flat[GUARD:GUARD + n] = float("nan")
        assert self.flat.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def ptr(self, byte_offset=0):
        return ctypes.c_void_p(self.flat.data_ptr() + 4 * GUARD + byte_offset)

    def fetch(self, on_device=False):
        """-> the payload (a copy on the CPU, or the device's own); asserts that the guards are bit-identical to the sentinel"""
        torch.cuda.synchronize()
        want = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device=DEV).view(torch.int32)
        assert torch.equal(self.flat[:GUARD].view(torch.int32), want), "the guard in front of the payload was written"
        assert torch.equal(self.flat[GUARD + self.n:].view(torch.int32), want), "the guard behind the payload was written"
        payload = self.flat[GUARD:GUARD + self.n]
        return payload if on_device else payload.cpu()


def _untouched(t):
    """every element still holds the NaN it held before the launch, bit for bit"""
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Prob:
    """A problem on the device: a [rows_in, C + 8] (NaN outside `listed`, PAD_IN in the pad columns of the listed rows), the fragments, scale, shift"""

    def __init__(self, p, rows, rows_in, listed=None):
        from laudnet_amd import ops
        self.C = C = p["w"].shape[0]
        a = torch.full((rows_in, C + 8), float("nan"))
        listed = torch.arange(rows.shape[0]) if listed is None else listed
        assert rows.shape[0] == len(listed) <= rows_in
        a[listed] = PAD_IN
        a[listed, :C] = rows
        self.a = a.to(DEV)
        self.frag = ops.pack_grouped16_weights(p["w"].to(DEV))
        self.sc, self.sh = p["scale"].to(DEV).contiguous(), p["shift"].to(DEV).contiguous()
        self.scale, self.shift = p["scale"], p["shift"]
        assert self.a.stride(0) == C + 8 and self.a.data_ptr() % 16 == 0


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def _launch_rows(pr, relu, nbr, cnt, m_cap, out_rows, on_device=False):
    """ldn_grouped16_conv3x3_rows on a NaN-filled guard-banded out [out_rows, C + 4] -> the payload"""
    L, lib = _lib()
    ldo = pr.C + 4
    out = _Banded(out_rows * ldo)
    rc = lib.ldn_grouped16_conv3x3_rows(L.ptr(pr.a), pr.a.stride(0), L.ptr(nbr), L.ptr(cnt), m_cap, L.ptr(pr.frag), pr.C, L.ptr(pr.sc),
                                        L.ptr(pr.sh), relu, out.ptr(), ldo, L.stream_ptr())
    assert rc == 0, lib.ldn_last_error()
    return out.fetch(on_device).view(out_rows, ldo)


def _launch_images(pr, geom, relu, cnt, images_cap, bands=None):
    """ldn_grouped16_conv3x3_images, or _images_gap with bands -> (out [B Ho Wo, C + 4], gap [B, bands, C] or None)"""
    L, lib = _lib()
    B, Hi, Wi, stride = geom
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    ldo = pr.C + 4
    out = _Banded(B * Ho * Wo * ldo)
    head = (L.ptr(pr.a), pr.a.stride(0), L.ptr(cnt), images_cap, Hi, Wi, Ho, Wo, stride, L.ptr(pr.frag), pr.C, L.ptr(pr.sc), L.ptr(pr.sh), relu,
            out.ptr(), ldo)
    if bands is None:
        rc = lib.ldn_grouped16_conv3x3_images(*head, L.stream_ptr())
        assert rc == 0, lib.ldn_last_error()
        return out.fetch().view(B * Ho * Wo, ldo), None
    gap = _Banded(B * bands * pr.C)
    rc = lib.ldn_grouped16_conv3x3_images_gap(*head, gap.ptr(), L.stream_ptr())
    assert rc == 0, lib.ldn_last_error()
    return out.fetch().view(B * Ho * Wo, ldo), gap.fetch().view(B, bands, pr.C)


def _check(got, n, pr, y64, relu, tag):
    """got [out_rows, C + 4] after a launch that must write the rows [0, n): pads and later rows untouched, no NaN, within the bound of the
    float64 reference y64 [n, C] (before the ReLU).  -> error / bound"""
    C = pr.C
    assert _untouched(got[:, C:]), f"{tag}: columns C .. ldo were written"
    assert _untouched(got[n:]), f"{tag}: rows at or past the count were written"
    if n == 0:
        return 0.0
    val = got[:n, :C]
    nan = torch.isnan(val)
    assert not nan.any(), f"{tag}: {int(nan.sum())} elements were never written (or are NaN), first at {nan.nonzero()[0].tolist()}"
    want = y64.to(val.device)
    want = want.clamp(min=0) if relu else want
    err = (val.double() - want).abs().max().item()
    bound = 1e-4 * max(1.0, want.abs().max().item())
    print(f"[grouped16 f64] {tag} relu {relu}: rows {n} max |err| {err:.3e} (error / bound {err / bound:.3f})")
    assert err <= bound, f"{tag}: error / bound = {err / bound:.3f}"
    if not relu:
        assert bool((val < 0).any())
        zero = (pr.scale == 0).to(val.device)
        assert torch.equal(val[:, zero], pr.shift[zero.cpu()].to(val.device).expand(n, -1)), f"{tag}: a zero scale leaves the shift"
    else:
        assert bool((val == 0).any()) and bool((val >= 0).all())
    return err / bound


# ---------------------------------------------------------------------------------------------------------------- 3a: tables of mask_to_index
@functools.lru_cache(maxsize=None)
def _row_case(case, single=False):
    """-> (problem on the device, ix of ops.mask_to_index, n3, the table on the device with exactly n3 rows, y64 [n3, C]); built once, shared"""
    from laudnet_amd import ops
    p = K.row_problem(*case, single=single)
    B, Ho, stride = case[:3]
    ix = ops.mask_to_index(p["patch"].to(DEV), Ho, Ho, stride)
    n3, n1 = int(ix.cnt[0].item()), int(ix.cnt[1].item())
    assert n3 == len(p["idx3"]) and n1 == len(p["idx1"]) and ix.cap1 == B * Ho * Ho * stride * stride
    assert np.array_equal(ix.idx1[:n1].cpu().numpy(), p["idx1"])
    assert torch.equal(ix.nbr.view(-1, 9)[:n3].cpu(), p["nbr"]), "the device's neighbour table is the index oracle's"
    y64 = R.rows_ref64(p["rows"], p["nbr"], p["w"], p["scale"], p["shift"], 0)
    return _Prob(p, p["rows"], ix.cap1), ix, n3, p["nbr"].to(DEV).contiguous(), y64


ROW_IDS = ["-".join(str(v) for v in c) for c in K.ROW_CASES]


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", K.ROW_CASES, ids=ROW_IDS)
def test_rows_vs_float64(case, relu):
    pr, ix, n3, _, y64 = _row_case(case)
    assert n3 == ix.cap3 if case[4] == 1.0 else 0 < n3 < ix.cap3
    got = _launch_rows(pr, relu, ix.nbr, ix.cnt[0:1], ix.cap3, ix.cap3)
    _check(got, n3, pr, y64, relu, f"rows {case}")
    assert _bits_equal(_launch_rows(pr, relu, ix.nbr, ix.cnt[0:1], ix.cap3, ix.cap3), got), "two launches differ"


@pytest.mark.parametrize("relu", [1, 0])
def test_rows_one_kept_pixel(relu):
    pr, ix, n3, _, y64 = _row_case(K.SINGLE + (0.0,), single=True)
    assert n3 == 1
    got = _launch_rows(pr, relu, ix.nbr, ix.cnt[0:1], ix.cap3, ix.cap3)
    C = pr.C
    assert _untouched(got[:, C:]) and _untouched(got[1:]) and not torch.isnan(got[0, :C]).any()
    want = y64.clamp(min=0) if relu else y64
    assert (got[:1, :C].double() - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())
    assert _bits_equal(_launch_rows(pr, relu, ix.nbr, ix.cnt[0:1], ix.cap3, ix.cap3), got)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", K.ROW_CASES[1:3], ids=ROW_IDS[1:3])
def test_rows_counts(case, relu):
    """a device-side count of zero, of one, none at all (m_cap rows), and one above m_cap (clamped)"""
    pr, ix, n3, nbr, y64 = _row_case(case)
    assert n3 > 40
    got = _launch_rows(pr, relu, ix.nbr, _count(0), ix.cap3, ix.cap3)
    assert _untouched(got), "a count of zero writes nothing"
    got = _launch_rows(pr, relu, nbr, _count(1), n3, n3)
    _check_few(got, 1, pr, y64, relu, "count 1")
    got = _launch_rows(pr, relu, nbr, None, n3, n3 + 3)                       # m_count = NULL: m_cap is the count
    _check(got, n3, pr, y64, relu, f"rows {case} without a count")
    m_cap = n3 - 21                                                          # a ragged last tile that is not the list's
    short = nbr[:m_cap].clone()                                              # a table of exactly m_cap rows
    assert short.numel() == 9 * m_cap and m_cap % 16 != 0
    got = _launch_rows(pr, relu, short, _count(n3 + 100), m_cap, n3)
    _check(got, m_cap, pr, y64[:m_cap], relu, f"rows {case} count above m_cap")
    got = _launch_rows(pr, relu, short, _count(2 ** 31 - 1), m_cap, n3)
    _check(got, m_cap, pr, y64[:m_cap], relu, f"rows {case} count INT_MAX")


def _check_few(got, n, pr, y64, relu, tag):
    """_check without its demands on the values' signs (too few rows for them)"""
    C = pr.C
    assert _untouched(got[:, C:]) and _untouched(got[n:]), f"{tag}: pads or rows at or past the count were written"
    assert not torch.isnan(got[:n, :C]).any(), tag
    want = y64[:n].clamp(min=0) if relu else y64[:n]
    err, bound = (got[:n, :C].double() - want).abs().max().item(), 1e-4 * max(1.0, want.abs().max().item())
    assert err <= bound, f"{tag}: error / bound = {err / bound:.3f}"


# ---------------------------------------------------------------------------------------------------------------- 3b: hand-built tables
def _hand_build(case, ref_on_device=False, cached=True):
    C, rows, rows_in, seed = case
    p = K.hand_problem(*case) if cached else K.hand_problem.__wrapped__(*case)
    assert bool((p["nbr"][0::4, 0] == p["nbr"][0::4, 3]).any()), "some rows name one input row in several taps"
    pr = _Prob(p, p["rows"][p["named"]], rows_in, listed=p["named"])
    nbr = p["nbr"].to(DEV).contiguous()
    if ref_on_device:          # float64 torch on the device: independent of the kernel
        y64 = R.rows_ref64(pr.a, nbr, p["w"], p["scale"], p["shift"], 0)
    else:
        y64 = R.rows_ref64(p["rows"], p["nbr"], p["w"], p["scale"], p["shift"], 0)
    return pr, nbr, y64


_hand_case = functools.lru_cache(maxsize=None)(_hand_build)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", K.HAND_CASES, ids=lambda c: f"C{c[0]}")
def test_rows_hand_built_table_vs_float64(case, relu):
    rows = case[1]
    pr, nbr, y64 = _hand_case(case)
    assert torch.isnan(pr.a[3]).all() and rows % 16 != 0
    got = _launch_rows(pr, relu, nbr, _count(rows), rows, rows + 2)
    _check(got, rows, pr, y64, relu, f"hand-built table C {pr.C}")
    assert _bits_equal(_launch_rows(pr, relu, nbr, _count(rows), rows, rows + 2), got), "two launches differ"


# ---------------------------------------------------------------------------------------------------------------- 3c: several tiles per wave
@pytest.mark.parametrize("C", [64, 400])
def test_rows_second_and_third_tile_per_wave(C):
    """csrc/ldn_grouped.hip, ldn_grouped16_conv3x3_rows:
        nchunks = ceil(G / 12); gchunk = ceil(G / nchunks); lds = gchunk * 10240
        cap = max(1, (cus * (lds <= 80 * 1024 ? 2 : 1) * 4) / nchunks);  grid = (min(ceil(tiles / 8), cap), nchunks) workgroups of 8 waves
    and in k_grouped16_mfma a wave walks `for (tile = blockIdx.x * 8 + wave; tile < ntiles; tile += gridDim.x * 8)`.  With
    tiles = 2 * 8 cap + 8 cap / 3 + 5 every wave of every workgroup takes a second tile -- re-deriving aoff[] and restarting the two-slot
    prefetch -- about a third of them a third, and the last tile is ragged.  C = 64: one chunk of 4 groups, two workgroups per CU;
    C = 400: 3 chunks of 9 groups, 90 KB of LDS, one workgroup per CU.  A launch that sizes its grid otherwise makes the assertion on
    `tiles` below fail or skip: then this test no longer bites and must be re-derived."""
    t0 = time.perf_counter()
    cus, G = _cus(), C // 16
    nchunks = -(-G // 12)
    gchunk = -(-G // nchunks)
    lds = gchunk * 10240
    assert (nchunks, gchunk) == {64: (1, 4), 400: (3, 9)}[C] and (lds <= 80 * 1024) == (C == 64)
    cap = max(1, cus * (2 if lds <= 80 * 1024 else 1) * 4 // nchunks)
    tiles = 2 * 8 * cap + 8 * cap // 3 + 5
    if not tiles > 8 * cap:
        pytest.skip(f"{tiles} tiles do not give a wave of {cap} workgroups a second tile")
    assert tiles > 2 * 8 * cap and tiles < 3 * 8 * cap
    rows = tiles * 16 - 7
    pr, nbr, y64 = _hand_build((C, rows, 1000, 13 + C), ref_on_device=True, cached=False)      # (not kept: hundreds of MB on the device)
    assert y64.is_cuda and tuple(y64.shape) == (rows, C)
    got = _launch_rows(pr, 1, nbr, _count(rows), rows, rows + 1, on_device=True)
    ratio = _check(got, rows, pr, y64, 1, f"{tiles} tiles on {cus} CUs (cap {cap}) C {C}")
    print(f"[grouped16 f64] multi-tile C {C}: {rows} rows, error / bound {ratio:.3f}, {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------------------------- 3d: the image form
IMG_IDS = ["-".join(str(v) for v in c[:6]) for c in K.IMAGE_CASES]


@functools.lru_cache(maxsize=None)
def _image_case(case):
    """-> (problem on the device, kept, y64 [kept, C, Ho, Wo] before the ReLU, the table of the geometry on the device, bands of the gap form)"""
    B, Hi, Wi, stride, C, keep, want_bands = case
    _, lib = _lib()
    p = K.image_problem(B, Hi, Wi, stride, C, keep)
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    assert lib.ldn_grouped16_images_fit(Hi, Wi, C) > 0
    bands = lib.ldn_grouped16_images_bands(Hi, Wi, Ho, stride, C)
    assert 1 <= bands <= Ho and (want_bands is None or bands == want_bands), bands
    pr = _Prob(p, R.to_rows(p["x"]), B * Hi * Wi)
    y64 = R.images_ref64(p["x"], p["w"], p["scale"], p["shift"], stride, 0)
    return pr, p["kept"], y64, p["nbr"].to(DEV).contiguous(), bands


@functools.lru_cache(maxsize=None)
def _image_run(case, relu):
    """every launch of one (case, ReLU): the plain form twice, the gap form twice, the row kernel over the geometry's table"""
    B, Hi, Wi, stride = case[:4]
    pr, kept, _, nbr, bands = _image_case(case)
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    n3 = kept * Ho * Wo
    cnt, geom = _count(n3), (B, Hi, Wi, stride)
    plain = [_launch_images(pr, geom, relu, cnt, B)[0] for _ in range(2)]
    fused = [_launch_images(pr, geom, relu, cnt, B, bands) for _ in range(2)]
    rows = _launch_rows(pr, relu, nbr, cnt, n3, B * Ho * Wo) if n3 else None
    return dict(plain=plain, fused=fused, rows=rows, n3=n3)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", K.IMAGE_CASES, ids=IMG_IDS)
def test_images_vs_float64(case, relu):
    pr, kept, y64, _, _ = _image_case(case)
    r = _image_run(case, relu)
    got = r["plain"][0]
    if kept == 0:
        assert _untouched(got), "nothing kept writes nothing"
    elif r["n3"] < 16:
        _check_few(got, r["n3"], pr, R.to_rows(y64), relu, f"images {case[:6]}")
    else:
        _check(got, r["n3"], pr, R.to_rows(y64), relu, f"images {case[:6]}")
    assert _bits_equal(r["plain"][1], got), "two launches differ"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", K.IMAGE_CASES, ids=IMG_IDS)
def test_images_are_bit_identical_to_the_row_kernel(case, relu):
    pr, kept, _, _, _ = _image_case(case)
    r = _image_run(case, relu)
    if kept:
        assert _untouched(r["rows"][:, pr.C:]) and _untouched(r["rows"][r["n3"]:])
        assert _bits_equal(r["plain"][0][:r["n3"], :pr.C], r["rows"][:r["n3"], :pr.C])


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", K.IMAGE_CASES, ids=IMG_IDS)
def test_gap_form_leaves_the_band_sums_of_its_output(case, relu):
    """relu 0 with the negative scales: the sums are of signed values, and a lane of a partial tile that added the value it computed for no
    pixel -- the shift, at the least -- would move them past the bound."""
    B, Hi, Wi, stride, C = case[:5]
    pr, kept, y64, _, bands = _image_case(case)
    r = _image_run(case, relu)
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    (out, gap), (out2, gap2) = r["fused"]
    assert _bits_equal(out, r["plain"][0]), "the output of the launch with gap differs from the launch without"
    assert _bits_equal(out2, out) and _bits_equal(gap2, gap), "two launches differ"
    assert tuple(gap.shape) == (B, bands, C)
    assert _untouched(gap[kept:]), "the sums of images past the count were written"
    if kept == 0:
        return
    nan = torch.isnan(gap[:kept])
    assert not nan.any(), f"{int(nan.sum())} sums were never written, first at [image, band, channel] = {nan.nonzero()[0].tolist()}"
    own = out[:r["n3"], :C].double().view(kept, Ho * Wo, C).sum(dim=1)
    err, bound = (gap[:kept].double().sum(dim=1) - own).abs().max().item(), 1e-5 * max(1.0, own.abs().max().item())
    want = y64.clamp(min=0) if relu else y64
    berr = (gap[:kept].double() - R.band_sums(want, bands)).abs()
    bbound = (R.band_pixels(Ho, Wo, bands) * 1e-4 * max(1.0, want.abs().max().item())).view(1, bands, 1)
    print(f"[grouped16 f64] gap {case[:6]} relu {relu} bands {bands}: own sums error / bound {err / bound:.3f}, "
          f"reference band sums error / bound {(berr / bbound).max().item():.3f}")
    assert err <= bound, f"error / bound = {err / bound:.3f}"
    assert bool((berr <= bbound).all()), f"per band: error / bound = {(berr / bbound).max().item():.3f}, first at {(berr > bbound).nonzero()[0].tolist()}"
    if not relu and Ho * Wo >= 16:
        assert bool((own < 0).any())


def test_images_cap_below_the_count():
    """the count names three images, the launch covers two: only those are written -- rows and sums"""
    case = K.IMAGE_CASES[4]
    B, Hi, Wi, stride, C = case[:5]
    pr, kept, y64, _, bands = _image_case(case)
    assert kept == 3 and B == 3
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    full = _image_run(case, 0)["plain"][0]
    for cap in (1, 2):
        n = cap * Ho * Wo
        for b in (None, bands):
            out, gap = _launch_images(pr, (B, Hi, Wi, stride), 0, _count(kept * Ho * Wo), cap, b)
            _check(out, n, pr, R.to_rows(y64)[:n], 0, f"images_cap {cap}")
            assert _bits_equal(out[:n], full[:n])
            if b:
                assert _untouched(gap[cap:]) and not torch.isnan(gap[:cap]).any()


def test_more_than_eight_pairs_in_a_ragged_last_eight():
    """the workgroup id decodes (image, band) pairs in eights: 11 pairs here, 6 and 24 among the cases above"""
    case = next(c for c in K.IMAGE_CASES if c[0] == 11)
    assert _image_case(case)[1] * _image_case(case)[4] == 11
    pairs = sorted(c[0] * _image_case(c)[4] for c in K.IMAGE_CASES)
    assert any(p < 8 for p in pairs) and any(p > 8 and p % 8 for p in pairs) and any(p > 8 and p % 8 == 0 for p in pairs), pairs


# ---------------------------------------------------------------------------------------------------------------- 3e: refusals
def test_refusals_write_nothing():
    """Each is refused with an error code and its text, and nothing is launched: the NaN payloads and the guards stay as they were.  (Were
    one of them launched after all, it would still write inside the payload and the guards: the excess of the wrong Ho is B Wo ldo floats.)"""
    L, lib = _lib()
    case = K.IMAGE_CASES[2]                                   # (2, 6, 10, 1, 48): both images kept
    B, Hi, Wi, stride, C = case[:5]
    pr, kept, _, nbr, bands = _image_case(case)
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    n3, ldo = kept * Ho * Wo, C + 4
    assert B * Wo * ldo < GUARD
    out, gap = _Banded(B * Ho * Wo * ldo), _Banded(B * bands * C)
    cnt, st = _count(n3), L.stream_ptr()

    def refused(rc, *words):
        msg = lib.ldn_last_error() or b""
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    def rows(C=C, ldo=ldo, outp=None):
        return lib.ldn_grouped16_conv3x3_rows(L.ptr(pr.a), C + 8, L.ptr(nbr), L.ptr(cnt), n3, L.ptr(pr.frag), C, L.ptr(pr.sc), L.ptr(pr.sh), 1,
                                              outp or out.ptr(), ldo, st)

    refused(rows(ldo=C + 2), b"strides must be multiples of 4")
    refused(rows(ldo=C - 4), b"strides")
    refused(rows(outp=out.ptr(4)), b"16-byte aligned")
    refused(rows(C=40), b"multiple of the group width 16", b"40")
    for name, extra in (("ldn_grouped16_conv3x3_images", ()), ("ldn_grouped16_conv3x3_images_gap", (gap.ptr(),))):
        f = getattr(lib, name)

        def images(C=C, ldo=ldo, outp=None, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, count=cnt, extra=extra):
            return f(L.ptr(pr.a), C + 8, L.ptr(count), B, Hi, Wi, Ho, Wo, stride, L.ptr(pr.frag), C, L.ptr(pr.sc), L.ptr(pr.sh), 1,
                     outp or out.ptr(), ldo, *extra, st)
        refused(images(ldo=C + 2), b"strides must be multiples of 4")
        refused(images(ldo=C - 4), b"strides")
        refused(images(outp=out.ptr(4)), b"16-byte aligned")
        refused(images(Ho=Ho + 1), b"is not a 3x3 / pad 1 / stride 1 geometry")
        refused(images(C=40), b"multiple of the group width 16", b"40")
        # a map of which three rows do not fit (no buffer of that size behind it: the count is zero, should it ever be launched)
        refused(images(Hi=8, Wi=1 << 20, Ho=8, Wo=1 << 20, count=_count(0)), b"do not fit the LDS")
        if extra:
            refused(images(extra=(None,)), b"ldn_grouped16_conv3x3_images_gap: null pointer")
    assert _untouched(out.fetch()) and _untouched(gap.fetch())
