"""CPU checks of ops.pack_grouped16_weights, the fragment layout of the width-16 matrix-core grouped 3x3 (k_grouped16_mfma / k_grouped16_img):
the kernel's contraction emulated from the fragments with the lane map csrc/ldn_grouped.hip documents -- lane = out channel i + 16 kg; step s,
k-group kg is tap 2 s + (kg >> 1), channels 8 (kg & 1) .. + 7 of the group; the second half of step 4 is zeros -- accumulating
hi.hi + hi.lo + lo.hi in float64 exactly as tests/test_grouped_mfma_pack.py does for widths 8 and 24, against the float64 definition with
that file's bound.  Then the same emulation over the inputs of the small cases of tests/test_hip_grouped16_f64.py: the arithmetic alone must
stay inside the GPU file's bound 1e-4 max(1, |ref|max), and the worst ratio is the one that file's docstring quotes."""
import pytest
import torch

from fill import seeded_randn
from test_grouped_mfma_pack import _definition, _split

import grouped16_cases as K
import grouped16_ref as R

STEPS = 5


def _tap(s, kg):
    """step s, k-group kg -> (tap, first channel of the group), None for the padding half of step 4"""
    t = 2 * s + (kg >> 1)
    return (t, 8 * (kg & 1)) if t < 9 else None


def _emulate16(frag, a, nbr):
    """out[r, c] (no scale / shift) as the kernel forms it, all rows at once: per step and k-group, the A fragment of lane i + 16 kg is what the
    packer put there, the B fragment of row r is eight consecutive channels of the neighbour row the lane map names (zeros for a negative
    entry or the padding half-step); hi.hi + hi.lo + lo.hi accumulated in float64."""
    G, rows = frag.shape[0], nbr.shape[0]
    acc = torch.zeros(rows, G, 16, dtype=torch.float64)
    nb = nbr.long()
    for s in range(STEPS):
        for kg in range(4):
            lanes = torch.arange(16) + 16 * kg
            ah, al = frag[:, s, lanes, 0].double(), frag[:, s, lanes, 1].double()          # [G, 16 (out channel i), 8]
            tap = _tap(s, kg)
            if tap is None:
                b = torch.zeros(rows, G, 8)
            else:
                t, ch = tap
                b = a[nb[:, t].clamp(min=0)][:, :G * 16].reshape(rows, G, 16)[:, :, ch:ch + 8]
                b = torch.where((nb[:, t] >= 0).view(rows, 1, 1), b, torch.zeros(()))
            bh, bl = _split(b)
            acc += torch.einsum("gne,rge->rgn", ah, bh) + torch.einsum("gne,rge->rgn", ah, bl) + torch.einsum("gne,rge->rgn", al, bh)
    return acc.reshape(rows, G * 16)


@pytest.mark.parametrize("C", [16, 48, 208])
def test_fragments_reproduce_the_definition(C):
    from laudnet_amd import _lib, ops
    G = C // 16
    w = seeded_randn((C, 9, 16), 3 + C) * 0.2
    frag = ops.pack_grouped16_weights(w)
    assert frag.dtype == torch.bfloat16 and frag.is_contiguous() and tuple(frag.shape) == (G, STEPS, 64, 2, 8)
    assert frag.numel() * 2 == _lib.load().ldn_grouped16_weight_bytes(C)
    # hi + lo reproduces the fp32 weight to 2^-16 relative, where the lane map says the weight sits; the padding half-step is exact zeros
    seen = torch.zeros(C, 9, 16, dtype=torch.bool)
    for s in range(STEPS):
        for kg in range(4):
            blk = frag[:, s, 16 * kg: 16 * (kg + 1)].float()                    # [G, 16 (out channel i), 2, 8]
            tap = _tap(s, kg)
            if tap is None:
                assert s == 4 and kg >= 2
                assert bool((blk == 0).all()), "the second half of step 4 is padding"
                continue
            t, ch = tap
            want = w[:, t, ch:ch + 8].view(G, 16, 8).double()
            got = blk[:, :, 0].double() + blk[:, :, 1].double()
            assert bool(((got - want).abs() <= 2.0 ** -16 * want.abs()).all())
            assert torch.equal(blk[:, :, 0], w[:, t, ch:ch + 8].view(G, 16, 8).to(torch.bfloat16).float()), "hi is the bf16 rounding of the weight"
            assert not seen[:, t, ch:ch + 8].any()
            seen[:, t, ch:ch + 8] = True
    assert bool(seen.all()), "every weight sits in exactly one place, the one the lane map names"
    # the contraction, on a small neighbour table with zero rows
    rows, rows_in = 7, 11
    a = seeded_randn((rows_in, C), 5 + C)
    nbr = torch.randint(-3, rows_in, (rows, 9), generator=torch.Generator().manual_seed(7 + C))
    nbr[nbr < 0] = -1
    assert bool((nbr < 0).any()) and bool((nbr >= 0).any())
    got = _emulate16(frag, a, nbr)
    want = _definition(w, 16, a, nbr)
    size = _definition(w, 16, a, nbr, absolute=True)
    # bf16x3 drops lo.lo (2^-18 of a product) and the two residuals of the splits (2^-18 each): 2^-16 of the absolute sum covers them
    assert bool(((got - want).abs() <= 2.0 ** -16 * size + 1e-30).all()), float(((got - want).abs() / (size + 1e-30)).max())
    assert float(want.abs().max()) > 0.1
    # ... and the plain reference of the GPU file is that definition
    one, zero = torch.ones(C), torch.zeros(C)
    assert (R.rows_ref64(a, nbr, w, one, zero, 0) - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def _ratio(p, relu):
    """worst |emulation - float64 reference| / (1e-4 max(1, |ref|max)) of one problem of tests/grouped16_cases.py"""
    from laudnet_amd import ops
    frag = ops.pack_grouped16_weights(p["w"])
    a = p["rows"] if "rows" in p else R.to_rows(p["x"])
    acc = _emulate16(frag, a, p["nbr"])
    got = acc * p["scale"].double() + p["shift"].double()                           # the epilogue, in float64: the float32 one adds 2^-24 relative
    got = got.clamp(min=0) if relu else got
    want = R.rows_ref64(a, p["nbr"], p["w"], p["scale"], p["shift"], relu)
    return (got - want).abs().max().item() / (1e-4 * max(1.0, want.abs().max().item()))


def _small_problems():
    yield from (("rows", c, K.row_problem(*c)) for c in K.ROW_CASES)
    yield "single", K.SINGLE, K.row_problem(*K.SINGLE, 0.0, single=True)
    yield from (("hand", c, K.hand_problem(*c)) for c in K.HAND_CASES)
    for c in K.IMAGE_CASES:
        if c[1] * c[2] <= 400 and c[5] > 0:                # the small maps; the banded ones add pixels, not arithmetic
            yield "images", c, K.image_problem(*c[:6])


def test_the_arithmetic_alone_is_inside_the_gpu_bound():
    """bf16x3 on the inputs of the GPU file's small cases: the worst error / bound, before any kernel runs"""
    worst = 0.0
    for kind, case, p in _small_problems():
        for relu in (1, 0):
            r = _ratio(p, relu)
            print(f"[grouped16 emulation] {kind} {case} relu {relu}: error / bound {r:.4f}")
            assert r < 1.0, (kind, case, relu, r)
            worst = max(worst, r)
    print(f"[grouped16 emulation] worst error / bound {worst:.4f}")
