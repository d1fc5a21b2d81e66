"""CPU checks of the matrix-core grouped 3x3 for group widths 8 and 24 (ldn_grouped_mfma_conv3x3_rows): the fragment layout of
ops.pack_grouped_mfma_weights, pinned by emulating the kernel's contraction from the fragments with the documented lane maps of
v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16 against the float64 definition; the shape predicate; and the dispatch switch
(laud_regnet.USE_GROUPED_MFMA_WIDTHS), which is off by default and then changes nothing."""
import pytest
import torch

from fill import seeded_randn

# (tile rows = out channels of an MFMA, K steps, chunks of 8 k-values per step)
GEOM = {24: (32, 14, 2), 8: (16, 3, 4)}


def _chunk(gw, s, kg):
    """chunk q of step s, k-group kg -> (tap, first channel of the group), None for a padding chunk"""
    if gw == 24:
        q = 2 * s + kg
        return (q // 3, 8 * (q % 3)) if q < 27 else None
    q = 4 * s + kg
    return (q, 0) if q < 9 else None


def _split(x):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


def _emulate(frag, gw, a, nbr):
    """out[r, c] (no scale / shift) as the kernel forms it: per group and K step, lane l = i + rows * kg holds the A fragment (weights of
    out channel i, k-group kg) where the packer put it, and the B fragment of tile column r is eight consecutive channels of the neighbour
    row the lane map names (zeros for a negative entry or a padding chunk); hi.hi + hi.lo + lo.hi accumulated in float64."""
    rows, steps, per = GEOM[gw]
    G, R = frag.shape[0], nbr.shape[0]
    out = torch.zeros(R, G * gw, dtype=torch.float64)
    zero8 = torch.zeros(8)
    for g in range(G):
        acc = torch.zeros(rows, R, dtype=torch.float64)           # D[out channel i][tile column r]
        for s in range(steps):
            for kg in range(per):
                lanes = torch.arange(rows) + rows * kg
                ah, al = frag[g, s, lanes, 0].double(), frag[g, s, lanes, 1].double()      # [rows, 8]
                ck = _chunk(gw, s, kg)
                b = torch.stack([a[nbr[r, ck[0]], g * gw + ck[1]: g * gw + ck[1] + 8] if ck is not None and nbr[r, ck[0]] >= 0 else zero8
                                 for r in range(R)])                                          # [R, 8]
                bh, bl = _split(b)
                acc += ah @ bh.t() + ah @ bl.t() + al @ bh.t()
        assert bool((acc[gw:] == 0).all()), "the unused rows of the tile must stay zero"
        out[:, g * gw:(g + 1) * gw] = acc[:gw].t()
    return out


def _definition(w, gw, a, nbr, absolute=False):
    """sum_t sum_i a[nbr[r, t], (c / gw) gw + i] w[c, t, i] in float64 (absolute: of the absolute values -- the size the error bound scales with)"""
    C, R = w.shape[0], nbr.shape[0]
    wd, ad = w.double(), a.double()
    if absolute:
        wd, ad = wd.abs(), ad.abs()
    out = torch.zeros(R, C, dtype=torch.float64)
    for r in range(R):
        for t in range(9):
            if nbr[r, t] < 0:
                continue
            row = ad[nbr[r, t]].view(C // gw, 1, gw)                      # [g][1][i]
            out[r] += (wd[:, t, :].view(C // gw, gw, gw) * row).sum(-1).reshape(C)
    return out


@pytest.mark.parametrize("gw,C", [(8, 8), (8, 24), (8, 104), (24, 24), (24, 72), (24, 120)])
def test_fragments_reproduce_the_definition(gw, C):
    from laudnet_amd import _lib, ops
    rows, steps, per = GEOM[gw]
    G = C // gw
    w = seeded_randn((C, 9, gw), 3 + C) * 0.2
    frag = ops.pack_grouped_mfma_weights(w, gw)
    assert frag.dtype == torch.bfloat16 and frag.is_contiguous() and tuple(frag.shape) == (G, steps, 64, 2, 8)
    assert frag.numel() * 2 == _lib.load().ldn_grouped_mfma_weight_bytes(C, gw)
    # hi + lo reproduces the fp32 weight to 2^-16 relative, where the lane map says the weight sits; padding entries are exact zeros
    seen = torch.zeros(C, 9, gw, dtype=torch.bool)
    for s in range(steps):
        for kg in range(per):
            ck = _chunk(gw, s, kg)
            blk = frag[:, s, rows * kg: rows * (kg + 1)].float()           # [G, rows (out channel i), 2, 8]
            assert bool((blk[:, gw:] == 0).all()), "out channels past the group width are padding"
            if ck is None:
                assert bool((blk == 0).all()), "chunks past the ninth tap are padding"
                continue
            t, ch = ck
            want = w[:, t, ch:ch + 8].view(G, gw, 8)
            got = blk[:, :gw, 0].double() + blk[:, :gw, 1].double()
            assert bool(((got - want.double()).abs() <= 2.0 ** -16 * want.double().abs()).all())
            seen[:, t, ch:ch + 8] = True
    assert bool(seen.all()), "every weight sits in exactly the chunks the lane map names"
    # the contraction, on a small neighbour table with zero rows
    R, Rin = 7, 11
    a = seeded_randn((Rin, C), 5 + C)
    gen = torch.Generator().manual_seed(7 + C)
    nbr = torch.randint(-3, Rin, (R, 9), generator=gen)
    nbr[nbr < 0] = -1
    assert bool((nbr < 0).any()) and bool((nbr >= 0).any())
    got = _emulate(frag, gw, a, nbr)
    want = _definition(w, gw, a, nbr)
    size = _definition(w, gw, a, nbr, absolute=True)
    # bf16x3 drops lo.lo (2^-18 of a product) and the two residuals of the splits (2^-18 each): 2^-16 of the absolute sum covers them
    assert bool(((got - want).abs() <= 2.0 ** -16 * size + 1e-30).all()), float(((got - want).abs() / (size + 1e-30)).max())
    assert float(want.abs().max()) > 0.1


def test_weight_bytes_and_ok_truth_table():
    from laudnet_amd import _lib, ops
    lib = _lib.load()
    for C, gw, ok in [(8, 8, True), (104, 8, True), (440, 8, True), (24, 24, True), (120, 24, True), (888, 24, True), (1512, 24, True),
                      (32, 16, False), (24, 12, False), (56, 56, False), (112, 56, False), (100, 8, False), (100, 24, False), (32, 24, False),
                      (0, 8, False), (-24, 24, False), (24, 0, False)]:
        assert ops.grouped_mfma_ok(C, gw) is ok, (C, gw)
        steps = 14 if gw == 24 else 3
        assert lib.ldn_grouped_mfma_weight_bytes(C, gw) == (C // gw * steps * 64 * 32 if ok else 0), (C, gw)


@pytest.mark.parametrize("C,gw", [(32, 16), (24, 12), (56, 56), (20, 8), (40, 24)])
def test_refusals(C, gw):
    import ctypes
    from laudnet_amd import _lib, ops
    with pytest.raises(_lib.LdnError):
        ops.pack_grouped_mfma_weights(torch.zeros(C, 9, gw), gw)
    with pytest.raises(_lib.LdnError):
        ops.pack_grouped_mfma_weights(torch.zeros(24, 9, 8), 24)          # the weight's own width disagrees
    # the entry point refuses the shape before any launch, and names the width
    lib, dummy = _lib.load(), ctypes.c_void_p(16)
    assert lib.ldn_grouped_mfma_conv3x3_rows(dummy, C, dummy, None, 4, dummy, C, gw, dummy, dummy, 1, dummy, C, None) == -1
    assert f"width {gw}".encode() in lib.ldn_last_error()
    assert lib.ldn_grouped_mfma_conv3x3_rows(None, 24, None, None, 4, None, 24, 24, None, None, 1, None, 24, None) == -1
    assert b"null" in lib.ldn_last_error()
    assert lib.ldn_grouped_mfma_conv3x3_rows(dummy, 26, dummy, None, 4, dummy, 24, 24, dummy, dummy, 1, dummy, 24, None) == -1
    assert b"strides" in lib.ldn_last_error()


def _transform(gw, w_b):
    from torch import nn
    from laudnet_amd import laud_regnet
    torch.manual_seed(0)
    return laud_regnet.BottleneckTransform(w_b, w_b, 1, nn.BatchNorm2d, nn.ReLU, gw, 1.0, 0.25, output_size=8, dyn_mode="spatial").eval()


@pytest.mark.parametrize("gw,w_b", [(8, 24), (24, 48), (16, 32)])
def test_switch_is_off_by_default_and_then_changes_nothing(gw, w_b, monkeypatch):
    from laudnet_amd import laud_regnet, ops, training
    assert laud_regnet.USE_GROUPED_MFMA_WIDTHS is False
    before = ops.get_math_mode()
    ops.set_math_mode("bf16x3")
    try:
        p = _transform(gw, w_b).prepared("cpu")
        assert "wb_frag_gw" not in p and ("wb_frag" in p) == (gw == 16)
        assert not laud_regnet.grouped_mfma_widths_on(w_b, gw)
        sb, tb = torch.ones(w_b), torch.zeros(w_b)
        pb = training._conv_b_params(p["wb"], sb, tb, gw)
        assert sorted(pb) == (["sb", "tb", "wb", "wb_frag"] if gw == 16 else ["sb", "tb", "wb"])
        assert pb["wb"] is p["wb"] and pb["sb"] is sb and pb["tb"] is tb
        # on: widths 8 and 24 get their fragments, width 16 keeps its own; fp32 mode or USE_GROUPED_MFMA off turn it off again
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS", True)
        assert laud_regnet.grouped_mfma_widths_on(w_b, gw) == (gw != 16)
        p = _transform(gw, w_b).prepared("cpu")
        assert ("wb_frag_gw" in p) == (gw != 16) and ("wb_frag" in p) == (gw == 16)
        pb = training._conv_b_params(p["wb"], sb, tb, gw)
        assert ("wb_frag_gw" in pb) == (gw != 16) and ("wb_frag" in pb) == (gw == 16)
        if gw != 16:
            assert torch.equal(pb["wb_frag_gw"], ops.pack_grouped_mfma_weights(p["wb"], gw)) and torch.equal(pb["wb_frag_gw"], p["wb_frag_gw"])
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", False)
        assert not laud_regnet.grouped_mfma_widths_on(w_b, gw)
        monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA", True)
        ops.set_math_mode("fp32")
        assert not laud_regnet.grouped_mfma_widths_on(w_b, gw)
        assert "wb_frag_gw" not in training._conv_b_params(p["wb"], sb, tb, gw)
    finally:
        ops.set_math_mode(before if before != ops.get_math_mode() else None)
        ops.set_math_mode(None)
