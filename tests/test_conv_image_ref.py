"""CPU checks of tests/conv_image_ref.py, the float64 restatement of ldn_conv_image's contract that tests/test_hip_conv_image.py holds the
kernels against: it equals F.conv2d where the contract is a plain convolution, the channel lists mean "the dropped channels are zero",
the border class of a pixel is the set of taps that fall outside, and the out_format 1 decoder inverts a plain hi / lo split.  The maps are
non-square throughout, so a reference that confused rows with columns, or one class with another, would fail here.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_image_ref as R
from fill import seeded_bernoulli, seeded_randn

# (Hi, Wi, stride): wider than high, higher than wide, odd, stride 2 from an odd and from an even map, one pixel high / wide, one pixel
MAPS = [(9, 20, 1), (20, 9, 1), (3, 5, 1), (13, 21, 2), (20, 26, 2), (12, 7, 2), (1, 7, 1), (7, 1, 1), (1, 7, 2), (1, 1, 1), (2, 6, 2)]
IDS = [f"{h}x{w}s{s}" for h, w, s in MAPS]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _dense(x, w, ksize, stride):
    """F.conv2d in float64 of NCHW x with n-major w [cout, T, cin] -> NHWC."""
    cout, T, cin = w.shape
    w4 = w.double().reshape(cout, ksize, ksize, cin).permute(0, 3, 1, 2)
    return _nhwc(F.conv2d(x.double(), w4, stride=stride, padding=ksize // 2))


@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("Hi,Wi,stride", MAPS, ids=IDS)
def test_plain_launch_equals_conv2d(Hi, Wi, stride, ksize):
    """No lists, one shift class: scale * conv2d + shift (+ residual), ReLU, - post_sub; a is read through a wider, NaN-padded stride."""
    B, cin, cout = 2, 8, 12
    x = seeded_randn((B, cin, Hi, Wi), 1)
    w = seeded_randn((cout, ksize * ksize, cin), 2)
    scale, shift, ps = seeded_randn((cout,), 3), seeded_randn((cout,), 4), seeded_randn((cout,), 5)
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    res = seeded_randn((B, Ho, Wo, cout + 4), 6)
    a = torch.full((B, Hi, Wi, cin + 4), float("nan"))
    a[..., :cin] = _nhwc(x)
    conv = _dense(x, w, ksize, stride)
    assert conv.shape == (B, Ho, Wo, cout)
    got, _ = R.conv_image_f64(a, w, scale, shift, cin=cin, cout=cout, ksize=ksize, stride=stride, relu=0)
    assert torch.allclose(got, conv * scale.double() + shift.double(), rtol=0, atol=1e-12)
    got, colsum = R.conv_image_f64(a, w, None, shift, cin=cin, cout=cout, ksize=ksize, stride=stride, relu=1, residual=res, post_sub=ps,
                                   want_colsum=True)
    want = torch.relu(conv + shift.double() + res[..., :cout].double()) - ps.double()
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    runs = -(-Ho * Wo // 32)
    assert colsum.shape == (B, runs, cout)
    flat = want.reshape(B, Ho * Wo, cout)
    for r in range(runs):
        assert torch.allclose(colsum[:, r], flat[:, 32 * r:32 * r + 32].sum(dim=1), rtol=0, atol=1e-11)


@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("Hi,Wi,stride", MAPS[:6], ids=IDS[:6])
def test_lists_mean_dropped_channels_are_zero(Hi, Wi, stride, ksize):
    """Input list + k-major weights, output list: the packed columns of the dense convolution whose dropped input channels are zeroed."""
    B, cin, cout = 4, 8, 12
    x = seeded_randn((B, cin, Hi, Wi), 7)
    w = seeded_randn((cout, ksize * ksize, cin), 8)
    scale, shift, ps = seeded_randn((cout,), 9), seeded_randn((cout,), 10), seeded_randn((cout,), 11)
    km, nm = seeded_bernoulli((B, cin), 0.6, 12).bool(), seeded_bernoulli((B, cout), 0.6, 13).bool()
    km[0], km[1], nm[0], nm[1] = False, True, False, True
    k_idx, n_idx = torch.zeros(B, cin, dtype=torch.int32), torch.zeros(B, cout, dtype=torch.int32)
    k_cnt, n_cnt = km.sum(dim=1).to(torch.int32), nm.sum(dim=1).to(torch.int32)
    a = torch.full((B, Hi, Wi, cin), float("nan"))
    for b in range(B):
        kk, nn_ = torch.nonzero(km[b]).reshape(-1), torch.nonzero(nm[b]).reshape(-1)
        k_idx[b, :len(kk)], n_idx[b, :len(nn_)] = kk.to(torch.int32), nn_.to(torch.int32)
        a[b, :, :, :len(kk)] = _nhwc(x)[b][:, :, kk]                     # left-packed; NaN behind the count: never read
    dense = _dense(x * km.view(B, cin, 1, 1), w, ksize, stride) * scale.double() + shift.double()
    dense = torch.relu(dense) - ps.double()
    for fmt, mult in ((0, 4), (1, 32)):
        got, _ = R.conv_image_f64(a, w.permute(1, 2, 0).contiguous(), scale, shift, cin=cin, cout=cout, ksize=ksize, stride=stride, k_idx=k_idx,
                                  k_cnt=k_cnt, n_idx=n_idx, n_cnt=n_cnt, post_sub=ps, relu=1, out_format=fmt)
        width = got.shape[-1]
        assert width == (cout if fmt == 0 else 32)
        for b in range(B):
            n = int(n_cnt[b])
            assert torch.allclose(got[b, :, :, :n], dense[b][:, :, n_idx[b, :n].long()], rtol=0, atol=1e-12)
            zero_to = min(R.round_up(n, mult), width)
            assert bool((got[b, :, :, n:zero_to] == 0).all()) and bool(torch.isnan(got[b, :, :, zero_to:]).all())
    # an input list alone (n-major rows are not gathered: every output channel)
    got, _ = R.conv_image_f64(a, w.permute(1, 2, 0).contiguous(), scale, shift, cin=cin, cout=cout, ksize=ksize, stride=stride, k_idx=k_idx,
                              k_cnt=k_cnt, post_sub=ps, relu=1)
    assert torch.allclose(got, dense, rtol=0, atol=1e-12)


def _outside_taps(Hi, Wi, stride):
    """[9, Ho, Wo] bool: tap t of the 3x3 (pad 1) at this output pixel falls outside the map -- by convolving an all-ones map with one-hot kernels."""
    onehot = torch.eye(9, dtype=torch.float64).reshape(9, 1, 3, 3)
    inside = F.conv2d(torch.ones(1, 1, Hi, Wi, dtype=torch.float64), onehot, stride=stride, padding=1)[0]
    return inside == 0


@pytest.mark.parametrize("Hi,Wi,stride", MAPS, ids=IDS)
def test_border_class_is_the_set_of_taps_outside(Hi, Wi, stride):
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    out = _outside_taps(Hi, Wi, stride)
    assert out.shape == (9, Ho, Wo)
    top, bottom, left, right = out[1].long(), out[7].long(), out[3].long(), out[5].long()       # taps (0,1), (2,1), (1,0), (1,2)
    cls = R.border_class(Hi, Wi, Ho, Wo, stride)
    assert torch.equal(cls, (top | bottom << 1) * 4 + (left | right << 1))
    # a tap is outside exactly when its row or its column is: the four bits say everything
    rows, cols = (top.bool(), torch.zeros_like(top).bool(), bottom.bool()), (left.bool(), torch.zeros_like(left).bool(), right.bool())
    for t in range(9):
        assert torch.equal(out[t], rows[t // 3] | cols[t % 3])
    assert not bool(R.border_class(Hi, Wi, Ho, Wo, stride, ksize=1).any()), "a 1x1 has no tap outside"
    if (Hi, Wi, stride) == (1, 7, 1):
        assert cls.tolist() == [[13, 12, 12, 12, 12, 12, 14]]
    if (Hi, Wi, stride) == (7, 1, 1):
        assert cls.reshape(-1).tolist() == [7, 3, 3, 3, 3, 3, 11]
    if (Hi, Wi, stride) == (1, 1, 1):
        assert cls.tolist() == [[15]]
    if (Hi, Wi, stride) == (20, 26, 2):
        assert set(cls.reshape(-1).tolist()) == {0, 1, 4, 5}, "stride 2 on an even map: the bottom / right bit is never set"
    if (Hi, Wi, stride) == (13, 21, 2):
        assert set(cls.reshape(-1).tolist()) == {0, 1, 2, 4, 5, 6, 8, 9, 10}


@pytest.mark.parametrize("Hi,Wi,stride", MAPS, ids=IDS)
def test_shift_table_row_is_the_class_of_the_pixel(Hi, Wi, stride):
    """conv3x3(x + c) with zero padding = conv3x3(x) + (the sum of w . c over the taps INSIDE the map): a 16-row table built from the meaning
    of the four class bits makes the reference reproduce F.conv2d of the shifted input.  A wrong class, or two table rows swapped, does not."""
    B, cin, cout = 2, 4, 8
    x = seeded_randn((B, cin, Hi, Wi), 14)
    w = seeded_randn((cout, 9, cin), 15)
    c = seeded_randn((cin,), 16)
    wc = (w.double() * c.double()).sum(dim=2)                                  # [cout, 9]
    table = torch.zeros(16, cout, dtype=torch.float64)
    for cls in range(16):
        top, bottom, left, right = cls >> 2 & 1, cls >> 3 & 1, cls & 1, cls >> 1 & 1
        for t in range(9):
            ky, kx = t // 3, t % 3
            if not ((ky == 0 and top) or (ky == 2 and bottom) or (kx == 0 and left) or (kx == 2 and right)):
                table[cls] += wc[:, t]
    got, _ = R.conv_image_f64(_nhwc(x), w, None, table, cin=cin, cout=cout, ksize=3, stride=stride, relu=0)
    want = _dense(x.double() + c.double().view(1, cin, 1, 1), w, 3, stride)
    assert torch.allclose(got, want, rtol=0, atol=1e-11)
    # a 1x1 launch that is handed a 16-row table uses row 0 only
    w1 = seeded_randn((cout, 1, cin), 17)
    rnd = seeded_randn((16, cout), 18)
    got1, _ = R.conv_image_f64(_nhwc(x), w1, None, rnd, cin=cin, cout=cout, ksize=1, stride=stride, relu=0)
    assert torch.allclose(got1, _dense(x, w1, 1, stride) + rnd[0].double(), rtol=0, atol=1e-12)


def test_decoder_inverts_a_plain_split():
    v = seeded_randn((3, 5, 64), 19) * torch.logspace(-6, 3, 64)
    v[0, 0, :8] = 0.0
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    stored = torch.stack((hi.reshape(3, 5, 8, 8), lo.reshape(3, 5, 8, 8)), dim=3).reshape(3, 5, 128).view(torch.float32)
    assert stored.shape == v.shape and torch.equal(stored, R.encode_split(v))
    dec = R.decode_split(stored)
    assert dec.shape == v.shape and torch.equal(dec, hi.float() + lo.float())
    assert bool(((dec - v).abs() <= 2.0 ** -16 * v.abs()).all())              # hi + lo = v to 2^-17 relative (two roundings to 8 bits)
    assert bool((dec[0, 0, :8] == 0).all())
