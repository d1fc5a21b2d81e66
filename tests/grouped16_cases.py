"""The cases of tests/test_hip_grouped16_f64.py and their inputs, built on the CPU (no CUDA here): tests/test_grouped16_pack.py runs the
bf16x3 emulation of the kernel's contraction over the same inputs, to show that the arithmetic alone stays inside the GPU file's bound.
Every builder is cached: a problem is built once, shared, and never modified."""
import functools

import numpy as np
import torch

from fill import seeded_bernoulli, seeded_randn
from oracle import index_ref as IR

import grouped16_ref as R

# 3a -- (B, Ho, stride, C, keep): square maps, spatial masks, the neighbour table of ops.mask_to_index
ROW_CASES = [(1, 5, 1, 16, 1.0),         # one group, 25 rows, ragged last tile
             (2, 7, 2, 48, 0.6),         # 3 groups: an odd count in the two-per-trip loop
             (3, 14, 1, 208, 0.5),       # 13 groups: 2 chunks of 7
             (2, 9, 2, 784, 0.4)]        # 49 groups: 5 chunks of 10
SINGLE = (2, 5, 1, 48)                   # (B, Ho, stride, C) of the case with one kept pixel

# 3b -- (C, rows, rows of a, seed): tables with no geometry behind them
HAND_CASES = [(64, 333, 1000, 11), (400, 205, 1000, 12)]

# 3d -- (B, Hi, Wi, stride, C, keep, bands of the gap form or None where the issue's table gives none)
IMAGE_CASES = [(2, 5, 5, 1, 16, 1.0, None),       # two tiles, one partial
               (4, 7, 7, 1, 784, 0.5, None),      # several groups per workgroup, several chunks; plain and gap take different chunk sizes
               (2, 6, 10, 1, 48, 1.0, None),      # non-square
               (2, 10, 6, 2, 208, 1.0, None),     # non-square, stride 2
               (3, 13, 9, 2, 208, 1.0, None),     # odd Hi and Wi at stride 2
               (2, 9, 15, 2, 400, 1.0, None),     # odd Hi and Wi at stride 2
               (2, 56, 40, 1, 32, 1.0, 3),        # 3 bands, non-square
               (2, 55, 41, 2, 32, 1.0, 3),        # 3 bands, odd height, stride 2: a band's last halo row is clipped by Hi
               (3, 111, 57, 2, 48, 0.7, 8),       # 8 bands
               (2, 1, 1, 1, 16, 1.0, None),       # one pixel
               (2, 2, 3, 2, 32, 1.0, None),       # one output row of two pixels at stride 2
               (4, 9, 9, 2, 48, 0.0, None),       # nothing kept
               (11, 5, 4, 1, 208, 1.0, None)]     # 11 (image, band) pairs: more than eight, and a ragged last eight; several chunks


def affine(C, seed):
    """BN scale / shift with zero and negative scales (tests/test_hip_grouped_mfma.py)"""
    scale = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed))
    scale[0::5] = 0.0
    scale[1::5] = -scale[1::5]
    return scale, 0.1 * seeded_randn((C,), seed + 1)


@functools.lru_cache(maxsize=None)
def row_problem(B, Ho, stride, C, keep, single=False):
    """-> dict: patch [B, Ho, Ho] float, idx3 / idx1 (the kept output pixels / the dilated input list, flat and row-major), nbr [n3, 9] int32
    into the packed input, rows [n1, C] float32 (the packed input), w [C, 9, 16], scale, shift"""
    Hi = Ho * stride
    if single:
        patch = torch.zeros(B, Ho, Ho)
        patch[B - 1, Ho // 2, 1] = 1.0
    else:
        patch = seeded_bernoulli((B, Ho, Ho), keep, 191 + C)
    m3 = patch.numpy() > 0.5
    m1 = IR.dilate_mask(m3, stride, 1)
    idx3, idx1 = IR.nonzero_rows(m3)[0], IR.nonzero_rows(m1)[0]
    nbr = torch.from_numpy(IR.neighbour_table(m3, m1, stride).astype(np.int32))
    x = seeded_randn((B, C, Hi, Hi), 192 + C)
    rows = x.permute(0, 2, 3, 1).reshape(B * Hi * Hi, C)[torch.from_numpy(idx1.astype(np.int64))].contiguous()
    scale, shift = affine(C, 194)
    return dict(patch=patch, idx3=idx3, idx1=idx1, nbr=nbr, rows=rows, w=seeded_randn((C, 9, 16), 193 + C) * 0.1, scale=scale, shift=shift)


def hand_table(rows, rows_in, seed):
    """[rows, 9] int32: entries anywhere in [0, rows_in), about a fifth of them -1; every fourth row names one input row in several taps"""
    g = torch.Generator().manual_seed(seed)
    nbr = torch.randint(0, rows_in, (rows, 9), generator=g, dtype=torch.int32)
    nbr[0::4, 3] = nbr[0::4, 0]
    nbr[0::4, 8] = nbr[0::4, 0]
    nbr[torch.rand(rows, 9, generator=g) < 0.2] = -1
    return nbr


@functools.lru_cache(maxsize=None)
def hand_problem(C, rows, rows_in, seed):
    """-> dict as row_problem's: a table with no image behind it.  The entries skip every seventh row of `a`, which therefore is named by no
    entry (the GPU file fills those rows with NaN)."""
    nbr = hand_table(rows, rows_in, seed)
    live = torch.tensor([r for r in range(rows_in) if r % 7 != 3], dtype=torch.int32)
    nbr = torch.where(nbr >= 0, live[nbr.long().clamp(min=0) % len(live)], nbr)
    assert 0.1 < (nbr < 0).float().mean().item() < 0.3
    scale, shift = affine(C, seed + 40)
    return dict(nbr=nbr, rows=seeded_randn((rows_in, C), seed + 20), named=live.long(), w=seeded_randn((C, 9, 16), seed + 30) * 0.1,
                scale=scale, shift=shift)


@functools.lru_cache(maxsize=None)
def image_problem(B, Hi, Wi, stride, C, keep):
    """-> dict: kept (number of kept images), x [kept, C, Hi, Wi] (the kept images in order), nbr [kept Ho Wo, 9] from the geometry,
    w [C, 9, 16], scale, shift"""
    patch = seeded_bernoulli((B,), keep, 320 + C + B + Hi)
    kept = int(patch.sum().item())
    assert kept == (B if keep == 1.0 else 0) or 0 < kept < B
    x = seeded_randn((B, C, Hi, Wi), 292 + C + Wi)[patch > 0]
    scale, shift = affine(C, 294)
    return dict(kept=kept, x=x, nbr=R.full_table(kept, Hi, Wi, stride), w=seeded_randn((C, 9, 16), 293 + C) * 0.1, scale=scale, shift=shift)
