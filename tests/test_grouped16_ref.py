"""CPU checks of tests/grouped16_ref.py: on whole images the packed-row form through a neighbour table built from the geometry alone equals
the F.conv2d form to 1e-12 relative -- square, non-square, odd heights and widths at stride 2 -- which is what entitles
tests/test_hip_grouped16_f64.py to hand-built tables; the table agrees with the index oracle; negative entries are zero rows; rows no entry
names are never read; the chunking changes nothing; the band sums add up to the image sums."""
import numpy as np
import pytest
import torch

from fill import seeded_randn
from oracle import index_ref as IR

import grouped16_ref as R

# (K, Hi, Wi, stride, C)
GEOM = [(2, 5, 5, 1, 16), (2, 6, 10, 1, 48), (2, 10, 6, 2, 32), (3, 13, 9, 2, 48), (2, 9, 15, 2, 16), (1, 55, 41, 2, 16), (2, 1, 1, 1, 16),
        (2, 2, 3, 2, 32), (1, 7, 1, 2, 16)]


def _inputs(K, Hi, Wi, C, seed):
    x = seeded_randn((K, C, Hi, Wi), seed)
    w = seeded_randn((C, 9, 16), seed + 1) * 0.1
    scale = seeded_randn((C,), seed + 2)
    scale[0::5] = 0.0
    return x, w, scale, seeded_randn((C,), seed + 3) * 0.1


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("K,Hi,Wi,stride,C", GEOM)
def test_rows_form_equals_images_form_on_whole_images(K, Hi, Wi, stride, C, relu):
    x, w, scale, shift = _inputs(K, Hi, Wi, C, 7 + Hi + Wi)
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    nbr = R.full_table(K, Hi, Wi, stride)
    assert tuple(nbr.shape) == (K * Ho * Wo, 9) and nbr.dtype == torch.int32
    want = R.images_ref64(x, w, scale, shift, stride, relu)
    assert tuple(want.shape) == (K, C, Ho, Wo) and want.dtype == torch.float64
    got = R.rows_ref64(R.to_rows(x), nbr, w, scale, shift, relu)
    assert got.dtype == torch.float64
    assert (got - R.to_rows(want)).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    if not relu:
        assert bool((got < 0).any())


@pytest.mark.parametrize("K,Hi,Wi,stride,C", GEOM)
def test_full_table_agrees_with_the_index_oracle(K, Hi, Wi, stride, C):
    Ho, Wo = R.out_hw(Hi, Wi, stride)
    want = IR.neighbour_table(np.ones((K, Ho, Wo), dtype=bool), np.ones((K, Hi, Wi), dtype=bool), stride)
    assert np.array_equal(R.full_table(K, Hi, Wi, stride).numpy(), want)
    if stride == 2 and Hi % 2 == 1:
        assert bool((want[-1, 6:] < 0).all())        # odd height: the last output row's bottom taps fall outside the map ...
    if stride == 2 and Hi % 2 == 0:
        assert bool((want[-1, 6:] >= 0).any())       # ... even height: they are inside


def test_negative_entries_are_zero_rows_and_unnamed_rows_are_not_read():
    C, rows_in = 32, 20
    a = seeded_randn((rows_in, C + 8), 1)
    a[:, C:] = float("nan")                          # columns past C
    a[5] = float("nan")                              # a row that no entry names
    w, scale, shift = seeded_randn((C, 9, 16), 2), seeded_randn((C,), 3), seeded_randn((C,), 4)
    g = torch.Generator().manual_seed(5)
    nbr = torch.randint(0, rows_in, (40, 9), generator=g, dtype=torch.int32)
    nbr[nbr == 5] = 6
    nbr[torch.rand(40, 9, generator=g) < 0.3] = -1
    nbr[7] = -1                                      # a row with no tap at all: act(shift)
    got = R.rows_ref64(a, nbr, w, scale, shift, 0)
    assert torch.isfinite(got).all()
    assert torch.equal(got[7], shift.double())
    # against the definition, tap by tap
    want = torch.zeros(40, C, dtype=torch.float64)
    for r in range(40):
        for t in range(9):
            if nbr[r, t] >= 0:
                row = a[nbr[r, t], :C].double().view(C // 16, 1, 16)
                want[r] += (w[:, t, :].double().view(C // 16, 16, 16) * row).sum(-1).reshape(C)
    want = want * scale.double() + shift.double()
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert torch.equal(R.rows_ref64(a, nbr, w, scale, shift, 1), got.clamp(min=0))
    # one row per chunk, and a table of another integer type: the same numbers
    assert torch.equal(R.rows_ref64(a, nbr.long(), w, scale, shift, 0, chunk_bytes=1), got)
    assert tuple(R.rows_ref64(a, nbr[:0], w, scale, shift, 0).shape) == (0, C)


@pytest.mark.parametrize("Ho,Wo,bands", [(7, 5, 1), (10, 3, 3), (28, 21, 3), (56, 29, 8), (5, 2, 5)])
def test_band_sums(Ho, Wo, bands):
    y = seeded_randn((2, 16, Ho, Wo), Ho).double()
    s = R.band_sums(y, bands)
    assert tuple(s.shape) == (2, bands, 16)
    assert (s.sum(dim=1) - y.sum(dim=(2, 3))).abs().max().item() < 1e-12 * Ho * Wo
    Rr = -(-Ho // bands)
    assert torch.equal(s[:, 0], y[:, :, :Rr].sum(dim=(2, 3)))
    px = R.band_pixels(Ho, Wo, bands)
    assert px.sum().item() == Ho * Wo and bool((px > 0).all())
    assert torch.equal(R.band_sums(torch.ones_like(y), bands)[0, :, 0], px)
