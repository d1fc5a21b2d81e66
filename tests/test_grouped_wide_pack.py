"""CPU check of ops.pack_grouped_wide_weights (the streamed fragments of k_grouped_wide<56 | 112>): the tensor is unpacked by the index
formula of the docstring, element by element in plain Python loops over (step, row tile, lane) -- not by inverting the permutation the
packer uses -- and compared with the weights: hi is the bf16 rounding of w, hi + lo reproduces w to bf16x2 precision
(|w - (hi + lo)| <= 2^-16 |w|), every pad element is zero; bad shapes and widths are refused."""
import pytest
import torch

from fill import seeded_randn

WIDE = {56: (32, 2), 112: (63, 4)}


def _unpack(frag, gw):
    """-> (hi, lo [C, 9, gw] float32, number of pad elements, whether they are all zero), by the docstring's formula"""
    steps, mt = WIDE[gw]
    G = frag.shape[0]
    Q = gw // 8
    f = frag.float()
    assert tuple(f.shape) == (G, steps, mt, 64, 2, 8)
    hi, lo = torch.full((G * gw, 9, gw), float("nan")), torch.full((G * gw, 9, gw), float("nan"))
    pads, pads_zero = 0, True
    for s in range(steps):
        for m in range(mt):
            for l in range(64):
                q, i = 2 * s + (l >> 5), 32 * m + (l & 31)
                v = f[:, s, m, l]                       # [G, 2, 8]
                if i >= gw or q >= 9 * Q:
                    pads += v.numel()
                    pads_zero = pads_zero and bool((v == 0).all())
                    continue
                tap, o = q // Q, q % Q
                for g in range(G):
                    hi[g * gw + i, tap, 8 * o:8 * o + 8] = v[g, 0]
                    lo[g * gw + i, tap, 8 * o:8 * o + 8] = v[g, 1]
    return hi, lo, pads, pads_zero


@pytest.mark.parametrize("gw,C", [(56, 56), (56, 168), (112, 112), (112, 224)])
def test_fragments_by_the_index_formula(gw, C):
    from laudnet_amd import ops
    w = seeded_randn((C, 9, gw), 900 + gw + C) * (2.0 / (9 * gw)) ** 0.5
    w[0, 0, 0] = 0.0
    w[1, 4, 5] = 1.0 + 2.0 ** -9                       # needs its lo part
    frag = ops.pack_grouped_wide_weights(w, gw)
    steps, mt = WIDE[gw]
    assert frag.dtype == torch.bfloat16 and frag.is_contiguous() and tuple(frag.shape) == (C // gw, steps, mt, 64, 2, 8)
    hi, lo, pads, pads_zero = _unpack(frag, gw)
    assert not torch.isnan(hi).any() and not torch.isnan(lo).any(), "the formula must reach every weight"
    assert torch.equal(hi, w.to(torch.bfloat16).float()), "hi is the bf16 rounding of w"
    assert torch.equal(lo, (w - hi).to(torch.bfloat16).float()), "lo is the bf16 rounding of w - hi"
    err = (w.double() - (hi.double() + lo.double())).abs()
    assert bool((err <= 2.0 ** -16 * w.double().abs()).all()), err.max().item()
    assert hi[1, 4, 5] == 1.0 and lo[1, 4, 5] == 2.0 ** -9
    assert pads_zero, "pad rows and the pad octet are zeros"
    assert pads == (C // gw) * 16 * (steps * mt * 64 - gw * 9 * gw // 8), "every element is a weight or a pad"


def test_bad_shapes_and_widths_are_refused():
    from laudnet_amd import ops
    from laudnet_amd._lib import LdnError
    for shape, gw in [((48, 9, 24), 24), ((64, 9, 16), 16), ((80, 9, 40), 40), ((100, 9, 56), 56), ((112, 9, 112), 56), ((112, 9, 56), 112),
                      ((112, 8, 56), 56), ((0, 9, 56), 56), ((112, 9 * 56), 56)]:
        with pytest.raises(LdnError):
            ops.pack_grouped_wide_weights(torch.zeros(*shape), gw)
