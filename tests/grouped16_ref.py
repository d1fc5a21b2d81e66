"""The contract of the width-16 grouped 3x3 (include/ldn_hip.h: ldn_grouped16_conv3x3_rows / _images / _images_gap) restated as plain float64
torch: the packed-row form through a neighbour table, the whole-image form through F.conv2d(groups = C / 16), the band sums of the _gap form,
and the neighbour table of whole images built from the geometry alone.  Nothing of the kernels' structure is in it (no tiles, no fragments, no
split products).  tests/test_grouped16_ref.py ties the two forms together on the CPU; tests/test_hip_grouped16_f64.py compares the kernels
with them.  The functions run on whatever device their tensors are on."""
from __future__ import annotations

import torch
import torch.nn.functional as F

GW = 16


def out_hw(Hi, Wi, stride):
    """The output map of a 3x3 / pad 1 convolution with this stride."""
    return (Hi - 1) // stride + 1, (Wi - 1) // stride + 1


def rows_ref64(a, nbr, w, scale, shift, relu, chunk_bytes=64 << 20):
    """out[r, 16 g + n] = act(scale * sum_t sum_i a[nbr[r, t], 16 g + i] * w[16 g + n, t, i] + shift) in float64.
    a [rows_in, >= C] float32 (only the first C columns are read), nbr [R, 9] integers (a negative entry is a zero row), w [C, 9, 16],
    scale / shift [C].  Rows of `a` that no entry names are never touched (they may hold NaN).  Works in chunks of rows so that the gathered
    taps [chunk, 9, C] in float64 stay within chunk_bytes.  -> [R, C] float64 on a's device."""
    C = w.shape[0]
    assert C % GW == 0 and tuple(w.shape[1:]) == (9, GW) and nbr.dim() == 2 and nbr.shape[1] == 9 and a.shape[1] >= C
    G, R, dev = C // GW, nbr.shape[0], a.device
    wk = w.to(dev).double().view(G, GW, 9 * GW).transpose(1, 2).contiguous()            # [g][t * 16 + i][n]
    sc, sh = scale.to(dev).double(), shift.to(dev).double()
    out = torch.empty(R, C, dtype=torch.float64, device=dev)
    step = max(1, chunk_bytes // (9 * C * 8))
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for r0 in range(0, R, step):
        nb = nbr[r0:r0 + step].to(dev).long()                                           # [r, 9]
        taps = a[nb.clamp(min=0).reshape(-1), :C].double().view(-1, 9, G, GW)
        taps = torch.where((nb >= 0).view(-1, 9, 1, 1), taps, zero)
        x = taps.permute(2, 0, 1, 3).reshape(G, -1, 9 * GW)                             # [g][r][t * 16 + i]
        v = torch.bmm(x, wk).permute(1, 0, 2).reshape(-1, C) * sc + sh
        out[r0:r0 + step] = v.clamp(min=0) if relu else v
    return out


def images_ref64(x_kept, w, scale, shift, stride, relu):
    """x_kept [K, C, Hi, Wi] float32 (the kept images, in order), w [C, 9, 16] -> [K, C, Ho, Wo] float64 through F.conv2d(groups = C / 16)."""
    K, C = x_kept.shape[:2]
    assert C % GW == 0 and tuple(w.shape) == (C, 9, GW)
    w4 = w.double().view(C, 3, 3, GW).permute(0, 3, 1, 2)
    y = F.conv2d(x_kept.double(), w4, None, stride, 1, 1, C // GW)
    y = y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return y.clamp(min=0) if relu else y


def to_rows(y):
    """[K, C, H, W] -> [K H W, C]: image k owns the rows [k H W, (k + 1) H W), pixels row-major."""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def band_sums(y, bands):
    """y [K, C, Ho, Wo] -> [K, bands, C]: channel sums over bands of R = ceil(Ho / bands) output rows (the last band holds what is left)."""
    K, C, Ho, Wo = y.shape
    R = -(-Ho // bands)
    assert bands >= 1 and -(-Ho // R) == bands
    return torch.stack([y[:, :, b * R:min((b + 1) * R, Ho)].sum(dim=(2, 3)) for b in range(bands)], dim=1)


def band_pixels(Ho, Wo, bands):
    """[bands] number of output pixels of every band of band_sums"""
    R = -(-Ho // bands)
    return torch.tensor([(min((b + 1) * R, Ho) - b * R) * Wo for b in range(bands)], dtype=torch.float64)


def full_table(K, Hi, Wi, stride):
    """The neighbour table of K whole images from the geometry alone: row k Ho Wo + oy Wo + ox, tap t = 3 ky + kx names the input row
    k Hi Wi + iy Wi + ix with (iy, ix) = (oy stride - 1 + ky, ox stride - 1 + kx), or -1 outside the Hi x Wi map.  -> int32 [K Ho Wo, 9]."""
    Ho, Wo = out_hw(Hi, Wi, stride)
    k = torch.arange(K).view(K, 1, 1, 1)
    oy, ox = torch.arange(Ho).view(1, Ho, 1, 1), torch.arange(Wo).view(1, 1, Wo, 1)
    t = torch.arange(9).view(1, 1, 1, 9)
    iy, ix = oy * stride - 1 + t // 3, ox * stride - 1 + t % 3
    inside = (iy >= 0) & (iy < Hi) & (ix >= 0) & (ix < Wi)
    rows = k * (Hi * Wi) + iy * Wi + ix
    return torch.where(inside, rows, torch.full_like(rows, -1)).reshape(K * Ho * Wo, 9).to(torch.int32)
