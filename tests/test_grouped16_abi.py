"""CPU checks of the host side of the width-16 matrix-core grouped 3x3 (csrc/ldn_grouped.hip): the plan of the whole-image form
(ldn_grouped16_images_fit, ldn_grouped16_images_bands) is host arithmetic and answers without a GPU -- for every conv b of RegNetY-800MF, for
non-square maps, and over a sweep of maps on which it is held to a model of the documented plan and to the LDS it may use; the entry points
refuse bad arguments before any launch, with the texts they have today.

The bands query sizes the buffer of the _gap form, so it must answer for THAT form: the channel-sum scratch counts against the budgets, and a
map near a limit is cut differently with it (16 x 111 at stride 1: one band without, four with)."""
import ctypes

import pytest

KB = 1024
FRAG = 5 * 64 * 32              # bytes of one group's fragments
MAXG = 12                       # groups per workgroup at the most


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


def _bytes(ng, in_rows, Wi, out_rows, Wo, gap):
    """LDS of a workgroup: fragments ng * 10240, staged pixels (in_rows Wi + 1) (16 ng + 4) floats, sums ng ceil(out_rows Wo / 16) * 64"""
    return ng * FRAG + (in_rows * Wi + 1) * (16 * ng + 4) * 4 + (ng * -(-(out_rows * Wo) // 16) * 64 if gap else 0)


def _plan(Hi, Wi, Ho, stride, G, gap):
    """The documented plan -> (groups per workgroup, output rows per workgroup) or None.  A whole image per workgroup when one group's share
    fits 150 KB, then as many groups (at most 12) as keep it within 80 KB -- two workgroups per CU -- spread evenly over the chunks; otherwise
    one group and bands of R output rows, the largest R whose (R - 1) stride + 3 input rows fit 80 KB, evened out over the bands."""
    Wo = (Wi - 1) // stride + 1
    if _bytes(1, Hi, Wi, Ho, Wo, gap) <= 150 * KB:
        ng = 1
        while ng < G and ng < MAXG and _bytes(ng + 1, Hi, Wi, Ho, Wo, gap) <= 80 * KB:
            ng += 1
        return -(-G // -(-G // ng)), Ho
    R = 0
    while R < Ho and _bytes(1, R * stride + 3, Wi, R + 1, Wo, gap) <= 80 * KB:
        R += 1
    if R < 1:
        return None
    return 1, -(-Ho // -(-Ho // R))


def _model_shapes():
    """(C, Hi, stride) of conv b of every stage of RegNetY-800MF at 224 px -- the stride-2 first block and the stride-1 blocks"""
    from laudnet_amd import laud_regnet
    params = laud_regnet.BlockParams.from_init_params(se_ratio=0.25, **laud_regnet._Y["800mf"])
    shapes, size = [], 112                                 # the stem halves 224
    for width, stride, depth, gw, mult in params._get_expanded_params():
        w_b = int(round(width * mult))
        assert stride == 2 and gw == 16 and w_b % 16 == 0
        shapes.append((w_b, size, 2))
        size //= 2
        if depth > 1:
            shapes.append((w_b, size, 1))
    assert size == 7
    return shapes


def test_every_conv_b_of_regnety_800mf_fits(lib):
    shapes = _model_shapes()
    assert len(shapes) >= 7 and {s[0] for s in shapes} == {64, 144, 320, 784}
    for C, Hi, s in shapes:
        Ho = (Hi - 1) // s + 1
        ng = lib.ldn_grouped16_images_fit(Hi, Hi, C)
        nb = lib.ldn_grouped16_images_bands(Hi, Hi, Ho, s, C)
        assert 1 <= ng <= min(C // 16, MAXG), (C, Hi, s, ng)
        assert 1 <= nb <= Ho, (C, Hi, s, nb)
        if Ho in (14, 7):
            assert nb == 1, (C, Hi, s, nb)                 # the small maps are whole images
        if Hi == 112:
            assert nb >= 2, (C, Hi, s, nb)                 # 112 x 112 -> 56 x 56 is banded
    assert lib.ldn_grouped16_images_bands(112, 112, 112, 1, 64) >= 2


def test_non_square_maps_are_planned(lib):
    fit, bands = lib.ldn_grouped16_images_fit, lib.ldn_grouped16_images_bands
    assert fit(6, 10, 48) > 0 and bands(6, 10, 6, 1, 48) == 1
    assert fit(20, 12, 208) > 0 and bands(20, 12, 10, 2, 208) == 1
    assert fit(13, 9, 208) > 0 and bands(13, 9, 7, 2, 208) == 1              # odd height and width at stride 2
    assert bands(7, 280, 7, 1, 16) == 7                                 # a wide, low map: banded although it has few rows
    assert bands(56, 40, 56, 1, 32) == 3 and bands(55, 41, 28, 2, 32) == 3 and bands(111, 57, 56, 2, 48) == 8
    # the query answers for the gap form: without the channel-sum scratch this map would be one band
    assert _plan(16, 111, 16, 1, 1, gap=False) == (1, 16) and _plan(16, 111, 16, 1, 1, gap=True) == (1, 4)
    assert bands(16, 111, 16, 1, 16) == 4


def test_refusals_answer_zero(lib):
    fit, bands = lib.ldn_grouped16_images_fit, lib.ldn_grouped16_images_bands
    for C in (100, 8, 24, 0, -16):                                             # C % 16 != 0, C <= 0
        assert fit(14, 14, C) == 0 and bands(14, 14, 14, 1, C) == 0, C
    assert fit(0, 14, 32) == 0 and fit(14, 0, 32) == 0 and fit(-1, 14, 32) == 0
    assert bands(0, 14, 1, 1, 32) == 0 and bands(14, 0, 14, 1, 32) == 0 and bands(14, 14, 0, 1, 32) == 0
    assert bands(14, 14, 14, 0, 32) == 0 and bands(14, 14, 14, -1, 32) == 0
    assert fit(8, 1 << 20, 32) == 0                                            # three rows do not fit: an answer, not an error
    assert bands(8, 1 << 20, 8, 1, 32) == 0 and bands(8, 1 << 20, 4, 2, 32) == 0
    assert fit(14, 14, 32) > 0 and bands(14, 14, 14, 1, 32) == 1 and bands(14, 14, 7, 2, 32) == 1      # ... and the map next to them is taken
    assert lib.ldn_grouped16_weight_bytes(32) == 2 * FRAG and lib.ldn_grouped16_weight_bytes(24) == 0 and lib.ldn_grouped16_weight_bytes(0) == 0


def test_entry_points_refuse_before_any_launch(lib):
    d = ctypes.c_void_p(256)
    rows = lib.ldn_grouped16_conv3x3_rows

    def call_rows(a=d, lda=48, nbr=d, m_cap=4, C=48, out=d, ldo=48, scale=d):
        return rows(a, lda, nbr, None, m_cap, d, C, scale, d, 1, out, ldo, None)
    assert call_rows(a=None) == -1 and b"ldn_grouped16_conv3x3_rows: null pointer" in lib.ldn_last_error()
    assert call_rows(nbr=None) == -1 and b"null pointer" in lib.ldn_last_error()
    assert call_rows(out=None) == -1 and b"null pointer" in lib.ldn_last_error()
    for C in (40, 0, -16):
        assert call_rows(C=C) == -1 and b"multiple of the group width 16" in lib.ldn_last_error(), C
    assert b"(got -16)" in lib.ldn_last_error()
    assert call_rows(lda=50) == -1 and b"strides must be multiples of 4" in lib.ldn_last_error()
    assert call_rows(ldo=50) == -1 and b"strides" in lib.ldn_last_error()
    assert call_rows(ldo=44) == -1 and b"strides" in lib.ldn_last_error()                  # ldo < C
    assert call_rows(lda=32) == -1 and b"strides" in lib.ldn_last_error()                  # lda < C
    assert call_rows(out=ctypes.c_void_p(260)) == -1 and b"16-byte aligned" in lib.ldn_last_error()
    assert call_rows(a=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.ldn_last_error()
    assert call_rows(scale=ctypes.c_void_p(260)) == -1 and b"aligned" in lib.ldn_last_error()
    assert call_rows(m_cap=0) == 0 and call_rows(m_cap=-3) == 0                            # no rows: nothing to launch
    for name, extra in (("ldn_grouped16_conv3x3_images", ()), ("ldn_grouped16_conv3x3_images_gap", (d,))):
        f = getattr(lib, name)

        def call(a=d, lda=48, cnt=d, cap=2, Hi=7, Wi=7, Ho=7, Wo=7, stride=1, C=48, out=d, ldo=48, extra=extra):
            return f(a, lda, cnt, cap, Hi, Wi, Ho, Wo, stride, d, C, d, d, 1, out, ldo, *extra, None)
        assert call(a=None) == -1 and b"ldn_grouped16_conv3x3_images: null pointer" in lib.ldn_last_error()
        assert call(cnt=None) == -1 and b"null pointer" in lib.ldn_last_error()            # this form has no count-less launch
        if extra:
            assert call(extra=(None,)) == -1 and b"ldn_grouped16_conv3x3_images_gap: null pointer" in lib.ldn_last_error()
        for C in (40, 0):
            assert call(C=C) == -1 and b"multiple of the group width 16" in lib.ldn_last_error(), C
        assert call(lda=50) == -1 and b"strides must be multiples of 4" in lib.ldn_last_error()
        assert call(ldo=50) == -1 and b"strides" in lib.ldn_last_error()
        assert call(ldo=44) == -1 and b"strides" in lib.ldn_last_error()
        assert call(out=ctypes.c_void_p(260)) == -1 and b"16-byte aligned" in lib.ldn_last_error()
        assert call(Ho=6) == -1 and b"7x7 -> 6x7 is not a 3x3 / pad 1 / stride 1 geometry" in lib.ldn_last_error()
        assert call(Wo=8) == -1 and b"geometry" in lib.ldn_last_error()
        assert call(stride=0) == -1 and b"geometry" in lib.ldn_last_error()
        assert call(stride=2, Ho=3, Wo=4) == -1 and b"geometry" in lib.ldn_last_error()    # 7 -> 4 at stride 2, not 3
        assert call(Hi=0, Ho=0) == -1 and b"geometry" in lib.ldn_last_error()
        assert call(Hi=8, Wi=1 << 20, Ho=8, Wo=1 << 20) == -1 and b"do not fit the LDS (ldn_grouped16_images_fit)" in lib.ldn_last_error()
        assert call(cap=0) == 0 and call(cap=-1) == 0                                      # no images: nothing to launch


@pytest.mark.parametrize("G", [1, 3, 13])
def test_the_plan_is_consistent_over_a_sweep(lib, G):
    """Hi, Wi in 1 .. 120, both strides: the bands the library answers are the documented plan's for the GAP form, 1 <= bands <= Ho, the LDS of
    that plan (recomputed here from the layout) stays within the 160 KB of a CU, and a map that fits is banded at both strides."""
    fit, bands = lib.ldn_grouped16_images_fit, lib.ldn_grouped16_images_bands
    C = 16 * G
    banded = whole = differ = 0
    for Hi in range(1, 121):
        for Wi in range(1, 121):
            nb = {}
            for stride in (1, 2):
                Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
                nb[stride] = bands(Hi, Wi, Ho, stride, C)
                plan = _plan(Hi, Wi, Ho, stride, G, gap=True)
                assert plan is not None and nb[stride] == -(-Ho // plan[1]), (Hi, Wi, stride, nb[stride], plan)
                assert 1 <= nb[stride] <= Ho, (Hi, Wi, stride, nb[stride])
                ng, R = plan
                assert 1 <= ng <= min(G, MAXG) and (ng == 1 or R == Ho)
                in_rows = Hi if R == Ho else min(Hi, (R - 1) * stride + 3)
                lds = _bytes(ng, in_rows, Wi, R, Wo, gap=True)
                assert lds <= 160 * KB, (Hi, Wi, stride, ng, R, lds)
                assert lds <= 80 * KB or ng == 1, (Hi, Wi, stride, ng, R, lds)           # several groups only where two workgroups share a CU
                plain = _plan(Hi, Wi, Ho, stride, G, gap=False)
                assert -(-Ho // plain[1]) <= nb[stride]                                 # the plain form never needs more bands than the buffer has
                differ += -(-Ho // plain[1]) != nb[stride]
                banded += nb[stride] > 1
                whole += nb[stride] == 1
            ng1 = fit(Hi, Wi, C)
            assert ng1 == _plan(Hi, Wi, Hi, 1, G, gap=True)[0], (Hi, Wi, ng1)
            assert ng1 > 0 and nb[1] > 0 and nb[2] > 0
    assert banded > 1000 and whole > 1000 and differ > 0, (banded, whole, differ)
