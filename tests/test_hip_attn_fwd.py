"""ldn_packed_mha / ldn_packed_mha_heads up to 256 tokens per image (k_packed_mha, csrc/ldn_attn.hip) against the float64 restatement of
tests/attn_fwd_ref.py, at the places the kernel can go wrong without the four randn cases of tests/test_hip_adavit.py noticing: every chunk
(32 keys) and wave (32 queries) seam in one launch, max_tokens BELOW an image's count (the first max_tokens tokens attend among themselves,
the later packed rows are not written, and ops.packed_mha_bwd differentiates that same function), dropped tokens' q / k / v poisoned, qkv as
a column window of a wider matrix, an explicit scale, the running softmax under large / shifted / monotone logits, head skipping at op
level, determinism and the argument errors.  "Not written" is asserted on a sentinel-filled `out` through the C ABI.

Bounds.  Unit-scale inputs: the project's forward bound, 2e-5 * max(1, |want|max) against float64.  The scale and stress cases:
max(that, 64 * E_f32), E_f32 = the error of plain fp32 dense attention on the CPU against float64 on the same inputs -- bf16x3 drops the
lo * lo product, about 2^-18 of a term, where fp32 rounds at 2^-24: a factor 64.  Each such case prints the kernel's error, E_f32 and their
ratio.  No bound here was taken from those figures.

Measured on one MI355X (max |err| against float64; docs/lab_notebook.md has the same table):
    seams 1.29e-5; max_tokens below the count, (kept, max_tokens): (60, 40) 9.0e-6, (40, 32) 9.3e-6, (200, 64) 9.4e-6, (50, 1) 7.6e-6,
    (256, 255) 1.0e-5; their backward, max |err| / max |want|: 9.2e-6, 5.9e-6, 1.0e-5, 3.1e-6, 1.1e-5 (bound 1e-3)
    case              kernel err   E_f32     ratio   bound     |want|max
    scale 1.0         8.89e-5      6.78e-6   13.1    4.34e-4   3.45
    scale 0.03        1.45e-5      1.41e-7   103     4.74e-5   2.37      (the 2e-5 |want|max term decides: E_f32 is one fp32 rounding of |want|max)
    x4        L=96    5.48e-4      1.09e-5   50.5    6.95e-4   4.03
    x4        L=200   1.96e-4      1.67e-5   11.8    1.07e-3   4.35
    shift6    L=96    2.27e-4      8.59e-5   2.6     5.50e-3   3.11
    shift6    L=200   4.98e-4      1.28e-4   3.9     8.18e-3   3.37
    ascending L=96    3.26e-5      4.00e-6   8.2     2.56e-4   1.06
    ascending L=200   2.01e-5      3.63e-6   5.6     2.32e-4   0.72
    descending L=96   3.68e-5      4.29e-6   8.6     2.75e-4   1.19
    descending L=200  1.99e-5      2.95e-6   6.8     1.89e-4   0.81
The seams launch holds 10 images (one per count), one more than the other cases' B <= 9: the counts belong in ONE launch."""
import pytest
import torch

from attn_bwd_ref import BOUND, grad_err, keep_pattern
from attn_fwd_ref import attending, mha_packed_f64
from fill import seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0


def keep_counts(L, counts, seed):
    """[len(counts), L] keep masks with exactly counts[b] kept tokens in image b, the CLS token among them (counts[b] = 0: none)"""
    keep = torch.zeros(len(counts), L)
    for b, n in enumerate(counts):
        if n > 0:
            perm = torch.randperm(L - 1, generator=torch.Generator().manual_seed(seed + b))[: n - 1] + 1
            keep[b, 0] = 1.0
            keep[b, perm] = 1.0
    assert keep.sum(1).tolist() == [float(n) for n in counts]
    return keep


def lists(keep):
    """ops.token_lists on the device, checked against the mask -> (tok_rows, prefix, n)"""
    from laudnet_amd import ops, load_library
    load_library()
    tok_rows, prefix, count = ops.token_lists(keep.to(DEV))
    n = int(count.item())
    assert n == int(keep.sum().item())
    assert torch.equal(tok_rows[:n].long().cpu(), torch.nonzero(keep.reshape(-1) > 0.5).reshape(-1))
    return tok_rows, prefix, n


def launch(qd, tok_rows, prefix, B, heads, max_tokens, scale=None, head_keep=None, head_dim=64, ld=None, expect_error=False):
    """The C entry points on a SENTINEL-filled out [rows of qd, heads * head_dim] -> out on the CPU.  qd: a 2-D device tensor, possibly a
    column window of a wider one (its row stride is passed as ld_qkv)."""
    from laudnet_amd import LdnError, _lib as L_, load_library
    lib = load_library()
    dim = heads * head_dim
    out = torch.full((qd.shape[0], dim), SENTINEL, device=DEV)
    scale = float(head_dim ** -0.5 if scale is None else scale)
    ld = qd.stride(0) if ld is None else ld
    if head_keep is None:
        status = lib.ldn_packed_mha(L_.ptr(qd), ld, L_.ptr(tok_rows), L_.ptr(prefix), B, heads, head_dim, max_tokens, scale, L_.ptr(out), dim,
                                    L_.stream_ptr(out))
    else:
        hk = head_keep.to(DEV).float().contiguous()
        status = lib.ldn_packed_mha_heads(L_.ptr(qd), ld, L_.ptr(tok_rows), L_.ptr(prefix), B, heads, head_dim, max_tokens, scale, L_.ptr(hk),
                                          L_.ptr(out), dim, L_.stream_ptr(out))
    if expect_error:
        with pytest.raises(LdnError):
            L_.check(status, "ldn_packed_mha")
    else:
        L_.check(status, "ldn_packed_mha")
    return out.cpu()


def unit_bound(want):
    return 2e-5 * max(1.0, want.abs().max().item())


def check_rows(out, want, written, bound, label):
    """out [cap, dim] from a sentinel-filled launch; want [n, dim] float64 packed; written: the packed rows the contract writes.
    Those rows within `bound` of float64, EVERY other row of out still the sentinel -> the error."""
    mask = torch.zeros(out.shape[0], dtype=torch.bool)
    mask[written] = True
    err = (out[written].double() - want[written]).abs().max().item() if written.numel() else 0.0
    assert err < bound, (label, err, bound)
    assert torch.equal(out[~mask], torch.full_like(out[~mask], SENTINEL)), label
    return err


# ---------------------------------------------------------------------------------------------- chunk and wave seams
def test_every_chunk_and_wave_seam_in_one_launch():
    """0 / 1 / 31 / 32 / 33 / 63 / 64 / 65 / 255 / 256 kept tokens of L = 256 in one launch (LDS sized for 256 tokens, every image its own
    padded length): an image without tokens, one key, one below / at / one past a chunk and a wave, two chunks, the full tile."""
    counts = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256]
    B, L, heads = len(counts), 256, 1
    qkv = seeded_randn((B, L, 192), 101)
    keep = keep_counts(L, counts, 102)
    tok_rows, prefix, n = lists(keep)
    pre = [0]
    for c in counts:
        pre.append(pre[-1] + c)
    assert prefix.cpu().tolist() == pre and n == pre[-1] == 800
    want, written = mha_packed_f64(qkv, keep, heads)
    assert torch.equal(written, torch.arange(n))
    out = launch(qkv.reshape(B * L, 192).to(DEV), tok_rows, prefix, B, heads, L)
    err = check_rows(out, want, written, unit_bound(want), "seams")                  # rows past the total count keep the sentinel
    print(f"[attn_fwd] seams: max |err| vs float64 = {err:.3e}")
    for b, c in enumerate(counts):                                                    # the one-key image: softmax = 1, out = v up to bf16x3's 16 bits
        if c == 1:
            v = qkv[b, 0, 128:]
            assert (out[pre[b]] - v).abs().max().item() <= 2.0 ** -15 * v.abs().max().item()


# ---------------------------------------------------------------------------------------------- max_tokens below the count
CUT_CASES = [(60, 40, 64), (40, 32, 64), (200, 64, 256), (50, 1, 64), (256, 255, 256)]      # (kept, max_tokens, L)
_CUT = {}


def cut_case(kept, mt, L):
    """Image 0 keeps `kept` > max_tokens, image 1 stays under the bound, image 2 keeps nothing; 2 heads.  Computed once, left unchanged."""
    key = (kept, mt, L)
    if key not in _CUT:
        B, heads = 3, 2
        qkv = seeded_randn((B, L, 3 * 64 * heads), 200 + kept + mt)
        under = max(1, mt - 7)
        keep = keep_counts(L, [kept, under, 0], 300 + kept + mt)
        hk = torch.tensor([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0]])                       # drops head 0 of the over-full image
        want, written = mha_packed_f64(qkv, keep, heads, max_tokens=mt)
        want_hk, written_hk = mha_packed_f64(qkv, keep, heads, max_tokens=mt, head_keep=hk)
        assert torch.equal(written, written_hk)
        assert written.tolist() == list(range(mt)) + list(range(kept, kept + under))  # the first mt rows of image 0, all of image 1
        _CUT[key] = (qkv, keep, hk, want, want_hk, written)
    return _CUT[key]


@pytest.mark.parametrize("kept,mt,L", CUT_CASES)
def test_max_tokens_below_the_count_forward(kept, mt, L):
    """The first max_tokens packed rows of the over-full image = float64 attention among those tokens ONLY; its later rows keep the sentinel."""
    qkv, keep, hk, want, want_hk, written = cut_case(kept, mt, L)
    B, heads = 3, 2
    tok_rows, prefix, n = lists(keep)
    qd = qkv.reshape(B * L, -1).to(DEV)
    out = launch(qd, tok_rows, prefix, B, heads, mt)
    err = check_rows(out, want, written, unit_bound(want), (kept, mt))
    print(f"[attn_fwd] kept {kept} max_tokens {mt}: max |err| vs float64 = {err:.3e}")
    # a head of the over-full image dropped: exact zeros on the written rows, the sentinel beyond them
    out_hk = launch(qd, tok_rows, prefix, B, heads, mt, head_keep=hk)
    check_rows(out_hk, want_hk, written, unit_bound(want), (kept, mt, "head_keep"))
    assert torch.equal(out_hk[:mt, :64], torch.zeros(mt, 64))
    assert torch.equal(out_hk[mt:kept], torch.full((kept - mt, 128), SENTINEL))
    assert torch.equal(out_hk[:mt, 64:], out[:mt, 64:])                                # the head that stays: the floats of the plain run
    assert torch.equal(out_hk[kept:n], out[kept:n])                                    # image 1 keeps both heads


@pytest.mark.parametrize("kept,mt,L", CUT_CASES)
def test_max_tokens_below_the_count_backward_is_the_same_function(kept, mt, L):
    """ops.packed_mha_bwd on the same lists and max_tokens against float64 autograd of the TRUNCATED reference, at the bound of
    tests/test_hip_attn_bwd.py: forward and backward describe one function."""
    from laudnet_amd import ops
    qkv, keep, hk, _, _, written = cut_case(kept, mt, L)
    B, heads = 3, 2
    dim = 64 * heads
    tok_rows, prefix, n = lists(keep)
    d_out = seeded_randn((B * L, dim), 400 + kept + mt)                                # packed: row n = the gradient of packed row n
    for head_keep in (None, hk):
        x = qkv.double().requires_grad_(True)
        ref, _ = mha_packed_f64(x, keep, heads, max_tokens=mt, head_keep=head_keep)
        (ref * d_out[:n].double()).sum().backward()
        got = ops.packed_mha_bwd(qkv.reshape(B * L, -1).to(DEV), tok_rows, prefix, B, heads, mt, d_out.to(DEV),
                                 head_keep=None if head_keep is None else head_keep.to(DEV)).view(B, L, -1).cpu()
        err = grad_err(got, x.grad)
        print(f"[attn_fwd] kept {kept} max_tokens {mt} head_keep {head_keep is not None}: backward max |err| / max |want| = {err:.3e}")
        assert err < BOUND, err
        idle = ~attending(keep, mt)                                                    # dropped tokens and the cut ones: no gradient, not written
        assert torch.equal(x.grad[idle], torch.zeros_like(x.grad[idle])) and torch.equal(got[idle], torch.zeros_like(got[idle]))


# ---------------------------------------------------------------------------------------------- rows that must not be read
@pytest.mark.parametrize("mt", [None, 40])
def test_unlisted_rows_are_never_read(mt):
    """q, k and v of every dropped token NaN, then +-3e38: the outputs are the bits of the run with zeros there.  With max_tokens = 40 the
    tokens past the bound (listed, but neither attended to nor written) are poisoned as well."""
    B, L, heads = 4, 64, 2
    qkv = seeded_randn((B, L, 3 * 64 * heads), 501)
    keep = keep_counts(L, [60, 17, 0, 33], 502)
    tok_rows, prefix, n = lists(keep)
    unread = ~attending(keep, mt)
    assert int(unread.sum()) > B * L - n or mt is None
    big = torch.where(seeded_bernoulli((B, L, 3 * 64 * heads), 0.5, 503) > 0.5, 3e38, -3e38)
    outs = []
    for poison in (torch.zeros_like(qkv), torch.full_like(qkv, float("nan")), big):
        x = torch.where(unread[:, :, None], poison, qkv)
        outs.append(launch(x.reshape(B * L, -1).to(DEV), tok_rows, prefix, B, heads, L if mt is None else mt))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    want, written = mha_packed_f64(qkv, keep, heads, max_tokens=mt)
    check_rows(outs[1], want, written, unit_bound(want), "poisoned")


def test_qkv_as_a_column_window_of_a_wider_matrix():
    """ld_qkv = 3 dim + 24, the window 8 floats in, NaN in the surrounding columns: the bits of the contiguous run."""
    B, L, heads = 3, 70, 2
    dim = 64 * heads
    qkv = seeded_randn((B, L, 3 * dim), 511)
    keep = keep_pattern(B, L, 0.6, 512)
    tok_rows, prefix, n = lists(keep)
    dense = launch(qkv.reshape(B * L, 3 * dim).to(DEV), tok_rows, prefix, B, heads, L)
    wide = torch.full((B * L, 3 * dim + 24), float("nan"), device=DEV)
    window = wide[:, 8:8 + 3 * dim]
    window.copy_(qkv.reshape(B * L, 3 * dim))
    assert window.stride(0) == 3 * dim + 24 and window.data_ptr() % 16 == 0 and torch.isnan(wide[:, :8]).all() and torch.isnan(wide[:, 8 + 3 * dim:]).all()
    strided = launch(window, tok_rows, prefix, B, heads, L)
    assert torch.equal(strided, dense)
    want, written = mha_packed_f64(qkv, keep, heads)
    check_rows(strided, want, written, unit_bound(want), "strided")


# ---------------------------------------------------------------------------------------------- scale; the running softmax under stress
def dense32(qkv, att, heads, scale):
    """The yardstick of the scale / stress cases: plain fp32 dense masked attention on the CPU -> [B * L, dim] (rows of non-attending tokens unused)"""
    B, L, _ = qkv.shape
    q, k, v = qkv.float().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~att[:, None, None, :], float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B * L, 64 * heads)


def run_against_f32_yardstick(label, qkv, keep, heads, scale):
    B, L, _ = qkv.shape
    tok_rows, prefix, n = lists(keep)
    want, written = mha_packed_f64(qkv, keep, heads, scale=scale)
    rows = tok_rows[:n].long().cpu()
    e32 = (dense32(qkv, keep > 0.5, heads, 64 ** -0.5 if scale is None else scale)[rows].double() - want).abs().max().item()
    wmax = want.abs().max().item()
    bound = max(2e-5 * max(1.0, wmax), 64.0 * e32)
    out = launch(qkv.reshape(B * L, -1).to(DEV), tok_rows, prefix, B, heads, L, scale=scale)
    assert torch.isfinite(out).all(), label
    err = (out[:n].double() - want).abs().max().item()
    print(f"[attn_fwd] {label}: kernel err {err:.3e}  E_f32 {e32:.3e}  ratio {err / e32:.2f}  bound {bound:.3e}  |want|max {wmax:.2f}")
    check_rows(out, want, written, bound, label)
    return err


@pytest.mark.parametrize("scale", [1.0, 0.03])
def test_explicit_scale(scale):
    B, L, heads = 3, 70, 2
    qkv = seeded_randn((B, L, 3 * 64 * heads), 601)
    keep = keep_pattern(B, L, 0.6, 602)
    run_against_f32_yardstick(f"scale {scale}", qkv, keep, heads, scale)
    if scale == 0.03:       # ... and it is not ignored: the default scale gives other floats
        tok_rows, prefix, n = lists(keep)
        qd = qkv.reshape(B * L, -1).to(DEV)
        assert not torch.equal(launch(qd, tok_rows, prefix, B, heads, L, scale=scale), launch(qd, tok_rows, prefix, B, heads, L))


def stress_inputs(kind, L):
    """B = 2 (image 0 keeps all L tokens: 3 chunks at L = 96, 7 at L = 200; image 1 Bernoulli 0.7), 2 heads -> (qkv, keep)"""
    B, heads = 2, 2
    x = seeded_randn((B, L, 3, heads, 64), 700 + L)
    keep = torch.ones(B, L)
    keep[1] = seeded_bernoulli((L,), 0.7, 701 + L)
    keep[1, 0] = 1.0
    if kind == "x4":                    # logits 16 times those of randn: a peaked softmax, real rescaling between chunks
        x[:, :, :2] *= 4.0
    elif kind == "shift6":              # logits near 0.125 * 64 * 36 = 288 and nearly equal: exp overflows without the max subtraction
        x[:, :, :2] += 6.0
    else:                               # q = u, k_j = ramp_j * 160 u (+ noise): scores 0 .. 20 monotone in key order, steps of 20 / L
        u = seeded_randn((heads, 64), 702)
        u = u / u.norm(dim=1, keepdim=True)
        j = torch.arange(L, dtype=torch.float32)
        ramp = (j if kind == "ascending" else (L - 1 - j)) / L
        x[:, :, 0] = u + 0.02 * x[:, :, 0]
        x[:, :, 1] = ramp[None, :, None, None] * 160.0 * u + 0.02 * x[:, :, 1]
        s = torch.einsum("bihd,bjhd->bhij", x[:, :, 0].double(), x[:, :, 1].double())
        step = s[..., 1:] - s[..., :-1]             # ascending: every chunk raises the running max; descending: alpha = 1 after the first
        assert (step > 0).all() if kind == "ascending" else (step < 0).all()
    return x.reshape(B, L, 3 * 64 * heads), keep


@pytest.mark.parametrize("L", [96, 200])
@pytest.mark.parametrize("kind", ["x4", "shift6", "ascending", "descending"])
def test_running_softmax_under_stress(kind, L):
    qkv, keep = stress_inputs(kind, L)
    run_against_f32_yardstick(f"{kind} L={L}", qkv, keep, 2, None)


# ---------------------------------------------------------------------------------------------- head skipping, determinism, refusals
def test_head_skipping_at_op_level():
    """3 heads, mixed head_keep, ragged counts through ops.packed_mha: a dropped (image, head) is exact zeros on the image's live rows, the
    kept heads are the floats of the run without head_keep."""
    from laudnet_amd import ops
    B, L, heads = 5, 80, 3
    dim = 64 * heads
    qkv = seeded_randn((B, L, 3 * dim), 801)
    keep = keep_counts(L, [80, 1, 33, 0, 47], 802)
    hk = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
    tok_rows, prefix, n = lists(keep)
    qd = qkv.reshape(B * L, 3 * dim).to(DEV)
    full = ops.packed_mha(qd, tok_rows, prefix, B, heads, L).cpu()
    got = ops.packed_mha(qd, tok_rows, prefix, B, heads, L, head_keep=hk.to(DEV)).cpu()
    img = tok_rows[:n].long().cpu() // L
    for b in range(B):
        live, ref = got[:n][img == b], full[:n][img == b]
        for h in range(heads):
            cols = slice(64 * h, 64 * h + 64)
            if hk[b, h] < 0.5:
                assert torch.equal(live[:, cols], torch.zeros_like(live[:, cols])), (b, h)
            else:
                assert torch.equal(live[:, cols], ref[:, cols]), (b, h)
    want, _ = mha_packed_f64(qkv, keep, heads, head_keep=hk)
    assert (got[:n].double() - want).abs().max().item() < unit_bound(want)


def test_two_launches_are_bit_identical():
    B, L, heads = 4, 197, 3
    qkv = seeded_randn((B, L, 3 * 64 * heads), 811)
    keep = keep_pattern(B, L, 0.5, 812)
    tok_rows, prefix, n = lists(keep)
    qd = qkv.reshape(B * L, -1).to(DEV)
    hk = seeded_bernoulli((B, heads), 0.6, 813)
    assert torch.equal(launch(qd, tok_rows, prefix, B, heads, L), launch(qd, tok_rows, prefix, B, heads, L))
    assert torch.equal(launch(qd, tok_rows, prefix, B, heads, L, head_keep=hk), launch(qd, tok_rows, prefix, B, heads, L, head_keep=hk))


def test_refusals():
    """LdnError before any launch (the sentinel-filled out is untouched), from the library and from ops.packed_mha's own checks."""
    from laudnet_amd import LdnError, ops
    B, L, heads = 2, 40, 2
    dim = 64 * heads
    keep = keep_pattern(B, L, 0.5, 821)
    tok_rows, prefix, n = lists(keep)
    qd = seeded_randn((B * L, 3 * dim), 822).to(DEV)
    untouched = torch.full((B * L, dim), SENTINEL)
    assert torch.equal(launch(qd, tok_rows, prefix, B, 4, L, head_dim=32, expect_error=True), untouched)          # head_dim 32
    assert torch.equal(launch(qd, tok_rows, prefix, B, heads, 0, expect_error=True), untouched)                   # max_tokens 0
    wide = torch.zeros(B * L, 3 * dim + 2, device=DEV)
    assert torch.equal(launch(wide[:, :3 * dim], tok_rows, prefix, B, heads, L, expect_error=True), untouched)    # ld_qkv % 4 != 0
    with pytest.raises(LdnError):
        ops.packed_mha(torch.zeros(B * L, 3 * 4 * 32, device=DEV), tok_rows, prefix, B, 4, L)
    with pytest.raises(LdnError):
        ops.packed_mha(qd, tok_rows, prefix, B, heads, 0)
    with pytest.raises(LdnError):
        ops.packed_mha(wide[:, :3 * dim], tok_rows, prefix, B, heads, L)
    with pytest.raises(LdnError, match="head_keep"):
        ops.packed_mha(qd, tok_rows, prefix, B, heads, L, head_keep=torch.ones(B, heads + 1, device=DEV))
    with pytest.raises(LdnError, match="head_keep"):
        ops.packed_mha(qd, tok_rows, prefix, B, heads, L, head_keep=torch.ones(B + 1, heads, device=DEV))
    with pytest.raises(LdnError, match="prefix"):
        ops.packed_mha(qd, tok_rows, prefix[:B], B, heads, L)
    with pytest.raises(LdnError, match="prefix"):
        ops.packed_mha(qd, tok_rows, torch.cat((prefix, prefix[-1:])), B, heads, L)
    for bad_heads in (0, -2):
        with pytest.raises(LdnError):
            ops.packed_mha(qd, tok_rows, prefix, B, bad_heads, L)
    ops.packed_mha(qd, tok_rows, prefix, B, heads, L)                                   # ... and the same arguments, right, run
