"""-m gpu: the optional epilogue terms of the shared-weight row convolution (ops.conv_rows on k_dense / k_dense2, csrc/ldn_dense.hip) against
the float64 restatement of the contract in tests/dense_rows_ref.py, kernel by kernel: post_sub, the per-image channel mask (image of the
DESTINATION row), the 16-class border shift table through pix_map, the LayerNorm fold (statistics of the SOURCE row) and the exact GELU.
tests/test_dense_rows_ref.py proves on the CPU that the cases reach every kernel that carries the terms and that their inputs move by more than
100 x the bound under each of eight plausible mistakes.

Every case runs on column slices of wider matrices (lda = cin + 8, ldo = cout + 4, ldr = cout + 8) with NaN wherever the contract reads
nothing: the pad columns of A and the residual, A / ln_stats rows that no list names within the count, residual rows that are no destination,
the mask row behind the last image; list entries behind the count are out-of-range garbage.  The output starts as NaN on the rows that are no
destination, a sentinel on the destinations and another in the pad columns: every written cell must be finite and within the bound, every
other cell bitwise unchanged, masked channels exactly 0, and a second launch must give the same bits.

Bounds (the project's op-level bounds of this kernel, none taken from what it gives here): affine / ReLU / post_sub / mask forms
max |got - ref| < 1e-4 max(1, |ref|max) in both arithmetic modes (test_hip_se_fused.py, test_hip_rows_ps.py, test_conv_rows_f32_kernel_vs_fp64);
LayerNorm and GELU forms 2e-4 absolute on the inputs of test_hip_adavit.py::test_layernorm_and_gelu_as_epilogue_terms (a quarter of the rows
with mean / std = 3).  Each test prints its figure before it asserts.

Measured on one MI355X (largest max |got - ref| per kernel family, affine + mask form / LayerNorm + GELU form; docs/lab_notebook.md has the table):
k_dense2 whole tiles 2.99e-5 / 6.30e-5, k_dense2 ragged 3.76e-5 / 7.11e-5, k_dense bf16x3 1x1 3.50e-5 / 1.07e-4, bf16x3 3x3 2.18e-5,
fp32 1x1 1.38e-6 / 2.67e-6, fp32 3x3 2.26e-6; the q / k / v call 6.98e-5 (bf16x3) and 5.21e-6 (fp32); the conv1 -> conv2 pair 2.31e-5 and 1.38e-6."""
import inspect

import pytest
import torch

import dense_rows_ref as R
from fill import seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
DST_SENTINEL, PAD_SENTINEL = -12345.0, 7777.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _window(rows, width, left, right, fill):
    """A [rows, width] column slice of a wider matrix filled with `fill`, 16-byte aligned (left % 4 == 0) -> (the wide matrix, the slice)"""
    big = torch.full((rows, left + width + right), fill, dtype=torch.float32)
    return big, big[:, left:left + width]


def _launch(ops, c, inp, mode):
    """One launch of the case on freshly built device buffers -> (the whole output matrix before, after; both on the CPU)"""
    p = R.poisoned(inp)
    r = p["ref"]
    cin, cout, n = c["cin"], c["cout"], inp["count"]
    a_big, a = _window(inp["a_total"], cin, 4, 4, NAN)
    a.copy_(p["a"])
    o_big, o = _window(inp["out_total"], cout, 0, 4, NAN)
    o[r["out_rows"][:n].long()] = DST_SENTINEL
    o_big[:, cout:] = PAD_SENTINEL
    res = None
    if r["residual"] is not None:
        r_big, rs = _window(inp["out_total"], cout, 4, 4, NAN)
        rs.copy_(r["residual"])
        res = r_big.to(DEV)[:, 4:4 + cout]
    cm = torch.cat((r["chan_mask"], torch.full((1, cout), NAN)), 0).to(DEV)[: inp["B"]]      # the row behind the last image: NaN
    dev = lambda t: None if t is None else t.to(DEV)
    out_dev = o_big.to(DEV)
    ops.conv_rows(a_big.to(DEV)[:, 4:4 + cin], dev(inp["w"]), dev(inp["scale"]), dev(inp["shift"]), out_dev[:, :cout],
                  a_rows=dev(r["a_rows"].reshape(-1)), taps=c["taps"], m_count=torch.tensor([n], dtype=torch.int32, device=DEV) if c["counted"] else None,
                  m_cap=c["m_cap"], relu=c["relu"], rows_hint=c["hint"] if c["hint"] >= 0 else None, relu_if_neg=dev(r["relu_if_neg"]),
                  out_rows=dev(r["out_rows"]), residual2d=res, math=mode, post_sub=dev(r["post_sub"]), chan_mask=cm, rows_per_image=c["rows_per_image"],
                  pix_map=dev(r["pix_map"]), geom=c["geom"], ln_stats=dev(r["ln_stats"]), ln_c1=dev(r["ln_c1"]))
    torch.cuda.synchronize()
    return o_big, out_dev.cpu()


def _check(ops, monkeypatch, c, count=None):
    mode = "fp32" if c["form"].startswith("f32") else "bf16x3"
    monkeypatch.setattr(ops, "USE_DENSE_F32", True)       # (the fp32 row kernel is opt-in: without it ops.conv_rows refuses the terms in fp32 mode)
    assert ops.dense_kernel_ok(mode)
    inp = R.build_inputs(c, count)
    assert c["counted"] or inp["count"] == c["m_cap"]
    ref, written = R.reference(c, inp)
    before, after = _launch(ops, c, inp, mode)
    cout = c["cout"]
    wr_big = torch.zeros_like(before, dtype=torch.bool)
    wr_big[:, :cout] = written
    same = _bits(before) == _bits(after)
    assert same[~wr_big].all(), f"{(~same[~wr_big]).sum().item()} cells that the contract does not write have changed"
    got = after[:, :cout].double()
    err = 0.0
    if written.any():
        assert torch.isfinite(got[written]).all(), "a written cell is not finite: a poisoned row, mask row or pad column was read"
        err = (got[written] - ref[written]).abs().max().item()
        tol = R.tolerance(c, ref[written].abs().max().item())
        print(f"dense terms {c['id']} count {inp['count']} {c['kernel']} {mode}: max err {err:.3e} bound {tol:.3e} |ref|max {ref[written].abs().max().item():.3f}")
        n, r = inp["count"], inp["ref"]
        dst = r["out_rows"][:n].long()
        dropped = torch.zeros_like(written)
        dropped[dst] = r["chan_mask"][dst // c["rows_per_image"]] == 0
        assert dropped.any() and (got[dropped] == 0).all(), "a masked channel is not exactly 0"
        assert err < tol, (err, tol)
    _, again = _launch(ops, c, inp, mode)
    assert torch.equal(_bits(again), _bits(after)), "a second launch on the same inputs gives other bits"
    return err


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import load_library, ops as _ops
    load_library()
    return _ops


@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_terms_vs_fp64(ops, monkeypatch, c):
    """Every case of the table: `feat` cases in bf16x3, `f32+feat` cases in true fp32."""
    _check(ops, monkeypatch, c)


@pytest.mark.parametrize("count", R.COUNTS)
@pytest.mark.parametrize("family", sorted(R.COUNT_FAMILIES))
def test_device_side_counts(ops, monkeypatch, family, count):
    """Device-side counts 0 (nothing is written), 1, 257 (a second tile of one row) and m_cap (no entry is garbage), one case per kernel family."""
    c = R.case_by_id(R.COUNT_FAMILIES[family])
    _check(ops, monkeypatch, c, c["m_cap"] if count == "m_cap" else count)


# ---- the two compositions as the product issues them --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
def test_token_skip_qkv_call(ops, monkeypatch, mode):
    """norm1 + q / k / v of a token-skipping block as adavit.py issues it: the kept-token list of ops.token_lists as gather AND scatter list, the
    list form of ops.row_stats, the head-keep mask repeated over q, k and v with rows_per_image = Lt, no activation, into a sentinel-filled
    qkv buffer.  Against layer_norm -> linear -> mask in float64 (the statistics of the reference are its own); bound 2e-4 absolute."""
    monkeypatch.setattr(ops, "USE_DENSE_F32", True)
    B, Lt, dim, heads, eps = 3, 197, 128, 2, 1e-5
    rows, cout = B * Lt, 3 * dim
    keep = seeded_bernoulli((B, Lt), 0.6, 41)
    keep[:, 0] = 1.0
    tok_rows, _, count = ops.token_lists(keep.to(DEV))
    n = int(count.item())
    kept = torch.nonzero(keep.reshape(-1) > 0.5).reshape(-1)
    assert n == kept.numel() and torch.equal(tok_rows[:n].long().cpu(), kept) and 0.4 * rows < n < 0.8 * rows
    x = seeded_randn((rows, dim), 42)
    x[: rows // 4] += 3.0
    gamma, beta = seeded_randn((dim,), 43) * 0.2 + 1.0, seeded_randn((dim,), 44) * 0.1
    w0, b0 = seeded_randn((cout, dim), 45) * (1.0 / dim) ** 0.5, seeded_randn((cout,), 46) * 0.1
    wg = w0.double() * gamma.double().view(1, -1)
    wq, bq, cq = wg.float().reshape(cout, 1, dim).contiguous(), (w0.double() @ beta.double() + b0.double()).float(), wg.sum(1).float()
    head_keep = torch.tensor([[1.0, 0.0], [0.0, 0.0], [0.0, 1.0]])
    hk3 = head_keep.repeat_interleave(dim // heads, dim=1).repeat(1, 3).contiguous()
    is_kept = keep.reshape(-1) > 0.5
    x_big, xw = _window(rows, dim, 4, 4, NAN)
    xw.copy_(torch.where(is_kept.view(-1, 1), x, torch.full((), NAN)))                  # a dropped token's row is never read
    x_dev = x_big.to(DEV)[:, 4:4 + dim]
    st = ops.row_stats(x_dev, eps, rows=tok_rows, count=count)
    st[(~is_kept).to(DEV)] = NAN                                                        # (the list form leaves these entries uninitialised)
    q_big, _ = _window(rows, cout, 0, 4, DST_SENTINEL)
    q_big[:, cout:] = PAD_SENTINEL
    q_dev = q_big.to(DEV)
    cm = torch.cat((hk3, torch.full((1, cout), NAN)), 0).to(DEV)[:B]
    ops.conv_rows(x_dev, wq.to(DEV), None, bq.to(DEV), q_dev[:, :cout], a_rows=tok_rows, out_rows=tok_rows, taps=1, m_count=count, m_cap=rows, relu=0,
                  ln_stats=st, ln_c1=cq.to(DEV), chan_mask=cm, rows_per_image=Lt, math=mode)
    torch.cuda.synchronize()
    after = q_dev.cpu()
    xd = x.double()
    stats = torch.stack((xd.mean(1), (xd.var(1, unbiased=False) + eps).rsqrt()), 1)
    lists = torch.cat((kept, torch.full((rows - n,), -7))).to(torch.int32)
    ref, written = R.conv_rows_f64(x, wq, None, bq, n, rows, a_rows=lists, out_rows=lists, relu=0, chan_mask=hk3, rows_per_image=Lt, ln_stats=stats, ln_c1=cq)
    direct = torch.nn.functional.linear(torch.nn.functional.layer_norm(xd[kept], (dim,), gamma.double(), beta.double(), eps), w0.double(), b0.double())
    direct = direct * hk3.double()[kept // Lt]
    assert (ref[kept] - direct).abs().max().item() < 1e-5          # (the fold of the contract is the LayerNorm: fp32 rounding of w', c1 and the constant)
    wr_big = torch.zeros_like(q_big, dtype=torch.bool)
    wr_big[:, :cout] = written
    assert (_bits(q_big) == _bits(after))[~wr_big].all(), "rows of dropped tokens or pad columns of qkv have changed"
    got = after[:, :cout].double()
    assert torch.isfinite(got[written]).all()
    err = (got[written] - direct.reshape(-1)).abs().max().item()
    print(f"dense terms qkv composition {mode}: max err {err:.3e} bound 2e-4")
    assert (got[kept][hk3[kept // Lt] == 0] == 0).all()
    assert err < 2e-4, err


def _neighbour_table(B, Hi, Wi, Ho, Wo, stride):
    """nbr [B * Ho * Wo, 9] of an all-active batch: flat input pixel (oy * stride - 1 + ky, ox * stride - 1 + kx) of the image, -1 out of bounds"""
    b, oy, ox, ky, kx = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), torch.arange(3), torch.arange(3), indexing="ij")
    iy, ix = oy * stride - 1 + ky, ox * stride - 1 + kx
    ok = (iy >= 0) & (iy < Hi) & (ix >= 0) & (ix < Wi)
    return torch.where(ok, b * Hi * Wi + iy * Wi + ix, torch.full((), -1)).reshape(B * Ho * Wo, 9).to(torch.int32)


@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
@pytest.mark.parametrize("geom", [(7, 7, 7, 7, 1), (14, 14, 7, 7, 2)], ids=["7x7", "14to7"])
def test_dense_channel_conv1_conv2_pair(ops, monkeypatch, geom, mode):
    """The dense execution of channel mode as _shared.dense_channel_convs issues it: conv1 with post_sub + chan_mask over row tiles that span
    images, then the 3x3 over the neighbour table and idx3 of ops.mask_to_index with a [16, cout] shift table, post_sub and chan_mask; conv2 reads
    the h1 that conv1 left.  Against the float64 chain; bound 1e-4 max(1, |ref|max) on both outputs."""
    monkeypatch.setattr(ops, "USE_DENSE_F32", True)
    Hi, Wi, Ho, Wo, stride = geom
    B, cin, W = 3, 64, 64
    rows1, rows3 = B * Hi * Wi, B * Ho * Wo
    ix = ops.mask_to_index(torch.ones(B, 1, 1, device=DEV), Ho, Wo, stride)
    nbr = _neighbour_table(B, Hi, Wi, Ho, Wo, stride)
    assert (ix.cap1, ix.cap3) == (rows1, rows3) and torch.equal(ix.nbr.cpu().reshape(rows3, 9), nbr) and torch.equal(ix.idx3.cpu(), torch.arange(rows3, dtype=torch.int32))
    x = seeded_randn((rows1, cin), 51)
    w1, w2 = seeded_randn((W, 1, cin), 52) * (1.0 / cin) ** 0.5, seeded_randn((W, 9, W), 53) * (1.0 / (9 * W)) ** 0.5
    s1, t1, c1 = 0.75 + 0.5 * torch.rand(W, generator=torch.Generator().manual_seed(54)), seeded_randn((W,), 55) * 0.1, 0.5 + torch.rand(W, generator=torch.Generator().manual_seed(56))
    s2, tab, c2 = 0.75 + 0.5 * torch.rand(W, generator=torch.Generator().manual_seed(57)), seeded_randn((16, W), 58) * 0.5, 0.5 + torch.rand(W, generator=torch.Generator().manual_seed(59))
    chm = seeded_bernoulli((B, W), 0.5, 60)
    chm[1] = 0.0
    d = lambda t: t.contiguous().to(DEV)
    h1 = torch.full((rows1, W), NAN, device=DEV)
    ops.conv_rows(d(x), d(w1), d(s1), d(t1), h1, taps=1, m_cap=ix.cap1, relu=1, post_sub=d(c1), chan_mask=d(chm), rows_per_image=Hi * Wi, math=mode)
    h2 = torch.full((rows3, W), NAN, device=DEV)
    ops.conv_rows(h1, d(w2), d(s2), d(tab), h2, a_rows=ix.nbr, taps=9, m_cap=ix.cap3, pix_map=ix.idx3, geom=geom, post_sub=d(c2), relu=1,
                  chan_mask=d(chm), rows_per_image=Ho * Wo, math=mode)
    torch.cuda.synchronize()
    ref1, wr1 = R.conv_rows_f64(x, w1, s1, t1, rows1, rows1, relu=1, post_sub=c1, chan_mask=chm, rows_per_image=Hi * Wi)
    ref2, wr2 = R.conv_rows_f64(ref1, w2, s2, tab, rows3, rows3, taps=9, a_rows=nbr, relu=1, post_sub=c2, chan_mask=chm, rows_per_image=Ho * Wo,
                                pix_map=torch.arange(rows3, dtype=torch.int32), geom=geom)
    assert wr1.all() and wr2.all()
    for name, got, ref, rpi in (("h1", h1, ref1, Hi * Wi), ("h2", h2, ref2, Ho * Wo)):
        got = got.cpu().double()
        assert torch.isfinite(got).all()
        err, tol = (got - ref).abs().max().item(), 1e-4 * max(1.0, ref.abs().max().item())
        print(f"dense terms channel pair {geom} {mode} {name}: max err {err:.3e} bound {tol:.3e}")
        assert (got.view(B, rpi, W)[chm.view(B, 1, W).expand(B, rpi, W) == 0] == 0).all()
        assert err < tol, (name, err, tol)


# ---- refusals: LdnError before any launch ------------------------------------------------------------------------------------------------
def _refusal_args(taps=1):
    rows, cin, cout = 64, 64, 64
    a = torch.ones(rows, cin, device=DEV)
    w = torch.ones(cout, taps, cin, device=DEV)
    out = torch.full((rows, cout), DST_SENTINEL, device=DEV)
    kw = dict(taps=taps, m_cap=rows, math="bf16x3")
    if taps == 9:
        kw["a_rows"] = torch.zeros(rows * 9, dtype=torch.int32, device=DEV)
    return a, w, out, kw


def _refused(call, out):
    from laudnet_amd import LdnError
    with pytest.raises(LdnError):
        call()
    torch.cuda.synchronize()
    assert (out == DST_SENTINEL).all(), "a refused call has written"


def test_refusals(ops):
    """Argument combinations the contract excludes, each refused with LdnError and nothing written: chan_mask without rows_per_image; ln_stats
    without ln_c1; ln_stats with taps == 9; a 16-row shift table without pix_map, and with taps == 1; the GELU with taps == 9 in bf16x3; the
    only term conv_rows_ps can be handed at all (the GELU: its signature has no post_sub / chan_mask / ln_stats / pix_map); a misaligned post_sub."""
    zeros = lambda *s: torch.zeros(*s, device=DEV)
    pix, g = torch.zeros(64, dtype=torch.int32, device=DEV), (8, 8, 8, 8, 1)
    a, w, out, kw = _refusal_args()
    sh = zeros(64)
    _refused(lambda: ops.conv_rows(a, w, None, sh, out, chan_mask=torch.ones(1, 64, device=DEV), **kw), out)
    _refused(lambda: ops.conv_rows(a, w, None, sh, out, ln_stats=zeros(64, 2), **kw), out)
    _refused(lambda: ops.conv_rows(a, w, None, sh, out, ln_c1=zeros(64), **kw), out)
    _refused(lambda: ops.conv_rows(a, w, None, zeros(16, 64), out, pix_map=pix, geom=g, **kw), out)
    _refused(lambda: ops.conv_rows(a, w, None, sh, out, post_sub=zeros(68)[1:65], **kw), out)
    assert not {"post_sub", "chan_mask", "ln_stats", "ln_c1", "pix_map", "rows_per_image"} & set(inspect.signature(ops.conv_rows_ps).parameters)
    _refused(lambda: ops.conv_rows_ps(a, w, None, sh, out, out_presplit=True, m_cap=64, relu=3), out)
    _refused(lambda: ops.conv_rows_ps(ops.presplit_rows(a), w, None, sh, out, a_presplit=True, m_cap=64, relu=3), out)
    a, w, out, kw = _refusal_args(taps=9)
    _refused(lambda: ops.conv_rows(a, w, None, sh, out, ln_stats=zeros(64, 2), ln_c1=zeros(64), **kw), out)
    _refused(lambda: ops.conv_rows(a, w, None, zeros(16, 64), out, geom=g, **kw), out)
    _refused(lambda: ops.conv_rows(a, w, None, sh, out, relu=3, **kw), out)
