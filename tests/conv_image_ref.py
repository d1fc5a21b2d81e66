"""The contract of ldn_conv_image (include/ldn_hip.h:500-523) restated as ONE plain float64 torch function with every optional term: the
per-image input list (k-major weights), the output list, scale or NULL, the 1- or 16-class border shift table, residual, ReLU, post_sub,
the zero columns behind an image's count and the colsum by-product; and the decoder of out_format 1.  Nothing of the kernels' structure is
in it (no tiles, no split products, no F.conv2d: the taps are gathered one by one).  tests/test_conv_image_ref.py checks it on the CPU,
tests/test_hip_conv_image.py compares the kernels with it.  No CUDA here."""
from __future__ import annotations

import torch


def round_up(n, m):
    return -(-n // m) * m


def out_hw(Hi, Wi, stride):
    """The output map of a 1x1 (pad 0) or 3x3 (pad 1) convolution with this stride."""
    return (Hi - 1) // stride + 1, (Wi - 1) // stride + 1


def tap_source(Hi, Wi, Ho, Wo, stride, ky, kx, pad):
    """Input pixel (iy [Ho,1], ix [1,Wo]) of tap (ky, kx) for every output pixel, and whether it lies inside the Hi x Wi map [Ho,Wo]."""
    iy = (torch.arange(Ho) * stride + ky - pad).view(Ho, 1)
    ix = (torch.arange(Wo) * stride + kx - pad).view(1, Wo)
    inside = (iy >= 0) & (iy < Hi) & (ix >= 0) & (ix < Wi)
    return iy, ix, inside


def border_class(Hi, Wi, Ho, Wo, stride, ksize=3):
    """[Ho, Wo] class of every output pixel: (top | bottom << 1) * 4 + (left | right << 1) of the taps that fall outside the input map
    (pad 1 for a 3x3; a 1x1 has no tap outside: class 0 everywhere, whatever table it is given)."""
    pad = ksize // 2
    oy, ox = torch.arange(Ho).view(Ho, 1), torch.arange(Wo).view(1, Wo)
    top, bottom = (oy * stride - pad < 0).long(), (oy * stride + pad >= Hi).long()
    left, right = (ox * stride - pad < 0).long(), (ox * stride + pad >= Wi).long()
    return (top | bottom << 1) * 4 + (left | right << 1)


def conv_image_f64(a, w, scale, shift, *, cin, cout, ksize=1, stride=1, k_idx=None, k_cnt=None, n_idx=None, n_cnt=None, post_sub=None,
                   relu=1, residual=None, out_format=0, want_colsum=False):
    """a [B,Hi,Wi,lda >= cin] (only the columns the contract names are read: the first Kb of an image), w [cout,T,cin] without k_idx /
    [T,cin,cout] with it, shift [cout] or [16,cout], residual [B,Ho,Wo,ldr >= cout].
    -> (out [B,Ho,Wo,width] float64, colsum [B,ceil(Ho*Wo/32),cout] float64 or None); width = cout (out_format 0) / roundup32(cout)
    (out_format 1).  Columns the contract is silent on -- behind roundup4(Nb) (roundup32 with out_format 1) -- hold NaN."""
    f64 = torch.float64
    B, Hi, Wi, _ = a.shape
    T = ksize * ksize
    pad = ksize // 2
    Ho, Wo = out_hw(Hi, Wi, stride)
    assert tuple(w.shape) == ((T, cin, cout) if k_idx is not None else (cout, T, cin))
    assert not (want_colsum and n_idx is not None) and not (residual is not None and n_idx is not None)
    w_ntk = (w.permute(2, 0, 1) if k_idx is not None else w).double()                     # [cout][T][cin], whatever the layout in memory
    sh = shift.double().view(-1, cout)
    assert sh.shape[0] in (1, 16)
    cls = border_class(Hi, Wi, Ho, Wo, stride, ksize) if sh.shape[0] == 16 else torch.zeros(Ho, Wo, dtype=torch.long)
    width = cout if out_format == 0 else round_up(cout, 32)
    out = torch.full((B, Ho, Wo, width), float("nan"), dtype=f64)
    for b in range(B):
        Kb = int(k_cnt[b]) if k_idx is not None else cin
        Nb = int(n_cnt[b]) if n_idx is not None else cout
        ks = k_idx[b, :Kb].long() if k_idx is not None else torch.arange(cin)             # channel of A's column i
        os_ = n_idx[b, :Nb].long() if n_idx is not None else torch.arange(cout)           # channel of the output's column j
        ab = a[b, :, :, :Kb].double()
        wb = w_ntk[os_][:, :, ks]                                                         # [Nb][T][Kb]
        acc = torch.zeros(Ho, Wo, Nb, dtype=f64)
        for t in range(T):
            iy, ix, inside = tap_source(Hi, Wi, Ho, Wo, stride, t // ksize, t % ksize, pad)
            src = ab[iy.clamp(0, Hi - 1), ix.clamp(0, Wi - 1)]                            # [Ho,Wo,Kb]
            src = torch.where(inside.unsqueeze(-1), src, torch.zeros((), dtype=f64))
            acc += src @ wb[:, t, :].t()
        v = acc * scale.double()[os_] if scale is not None else acc
        v = v + sh[cls][:, :, os_]
        if residual is not None:
            v = v + residual[b, :, :, :Nb].double()
        if relu:
            v = v.clamp(min=0)
        if post_sub is not None:
            v = v - post_sub.double()[os_]
        out[b, :, :, :Nb] = v
        out[b, :, :, Nb:min(round_up(Nb, 32 if out_format == 1 else 4), width)] = 0.0
    colsum = None
    if want_colsum:
        HW = Ho * Wo
        runs = -(-HW // 32)
        flat = torch.zeros(B, runs * 32, cout, dtype=f64)
        flat[:, :HW] = out.reshape(B, HW, cout)
        colsum = flat.reshape(B, runs, 32, cout).sum(dim=2)
    return out, colsum


def decode_split(h1s):
    """[..., ld] fp32-typed storage of [octet][8 hi | 8 lo] bf16 (out_format 1) -> fp32 values hi + lo, same shape."""
    shape = h1s.shape
    raw = h1s.contiguous().view(torch.bfloat16).reshape(*shape[:-1], shape[-1] // 8, 2, 8).float()
    return (raw[..., 0, :] + raw[..., 1, :]).reshape(shape)


def encode_split(v):
    """The plain split out_format 1 stores: hi = bf16(v), lo = bf16(v - hi), per octet [8 hi | 8 lo], as fp32-typed storage [..., ld]."""
    v = v.float()
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    shape = v.shape
    pair = torch.stack((hi.reshape(*shape[:-1], shape[-1] // 8, 8), lo.reshape(*shape[:-1], shape[-1] // 8, 8)), dim=-2)
    return pair.reshape(*shape[:-1], 2 * shape[-1]).contiguous().view(torch.float32).reshape(shape)
