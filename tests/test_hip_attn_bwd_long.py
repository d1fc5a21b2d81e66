"""ops.packed_mha_bwd_long (ldn_packed_mha_bwd_long: k_packed_mha_bwd_q + k_packed_mha_bwd_kv, the attention backward tiled by 256 queries / keys)
against float64 autograd of the dense masked restatement (tests/attn_bwd_ref.py) at every seam of the tiling, bit-identity with the one-launch
kernel on images of at most 256 kept tokens, a ragged batch with a poisoned workspace and poisoned guard rows, head skipping across tiles, and
the argument checks.  Bound: every element within 1e-3 of the tensor's own maximum (BOUND; the one-launch kernel measures 5e-6 to 1e-5).  Every
image of a reference-compared case keeps at least its CLS token (softmax over no key is NaN in the dense reference); the empty image is checked
with sentinels.  `measure` returns the figures without asserting (tools/train_adavit_grad_err.py records them)."""
import pytest
import torch

from attn_bwd_ref import BOUND, grad_err, mha_bwd_autograd
from fill import seeded_bernoulli, seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25

# (L, kept tokens per image, heads): one token past a tile, a one-token image, an exactly full tile, a tile plus one chunk | exactly two tiles,
# two tiles plus one, a short image in a long launch, three tiles with a ragged last one | the 384 px shape
SEAMS = [(320, (257, 1, 256, 288), 1), (600, (512, 513, 33, 600), 1), (577, (300, 40, 577), 2)]
_CASES = {}


def _keep_counts(L, counts, seed):
    """[len(counts), L] keep masks with exactly counts[b] kept tokens in image b, the CLS token among them (counts[b] = 0: none)
    (tests/test_hip_adavit_long.py's helper)."""
    keep = torch.zeros(len(counts), L)
    for b, n in enumerate(counts):
        if n > 0:
            perm = torch.randperm(L - 1, generator=torch.Generator().manual_seed(seed + b))[: n - 1] + 1
            keep[b, 0] = 1.0
            keep[b, perm] = 1.0
    assert keep.sum(1).tolist() == [float(n) for n in counts]
    return keep


def _inputs(keep, heads):
    B, L = keep.shape
    qkv = seeded_randn((B, L, 192 * heads), 3 + L)
    d_out = seeded_randn((B, L, 64 * heads), 7 + L) * keep[..., None]
    return qkv, d_out


def case(L, counts, heads):
    """(qkv [B, L, 3 dim] fp32, keep, d_out dense fp32 (zero at dropped tokens), want float64), computed once per shape and left unchanged"""
    key = (L, counts, heads)
    if key not in _CASES:
        keep = _keep_counts(L, counts, 5 + L)
        qkv, d_out = _inputs(keep, heads)
        _CASES[key] = (qkv, keep, d_out, mha_bwd_autograd(qkv.double(), keep, heads, d_out.double()))
    return _CASES[key]


def run(qkv, keep, heads, d_out, max_tokens=None, head_keep=None, out=None, ws=None, op="packed_mha_bwd_long", poison=False):
    """-> (d_qkv [B * L, 3 dim] on the device, the kept tokens' flat rows).  poison: the packed rows of d_out at and past the count are NaN."""
    from laudnet_amd import ops
    B, L, three = qkv.shape
    tok_rows, prefix, count = ops.token_lists(keep.to(DEV))
    n = int(count.item())
    rows = tok_rows[:n].long()
    packed = torch.full((B * L, three // 3), float("nan") if poison else 0.0, device=DEV)
    packed[:n] = d_out.reshape(B * L, -1).to(DEV)[rows]
    kw = {} if ws is None else {"ws": ws}
    got = getattr(ops, op)(qkv.reshape(B * L, three).to(DEV), tok_rows, prefix, B, heads, L if max_tokens is None else max_tokens, packed,
                           head_keep=None if head_keep is None else head_keep.to(DEV), out=out, **kw)
    return got, rows


def measure(L, counts, heads):
    qkv, keep, d_out, want = case(L, counts, heads)
    got, _ = run(qkv, keep, heads, d_out)
    ref32 = mha_bwd_autograd(qkv.to(DEV), keep.to(DEV), heads, d_out.to(DEV))
    return {"d_qkv": grad_err(got.view(len(counts), L, -1), want)}, {"d_qkv": grad_err(ref32, want)}


def _thirds(got, want, heads):
    errs = {"d_qkv": grad_err(got, want)}
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(64 * heads * i, 64 * heads * (i + 1))
        errs[name] = grad_err(got[..., sl], want[..., sl])                # each third against its own maximum
    return errs


@pytest.mark.parametrize("L,counts,heads", SEAMS)
def test_packed_mha_bwd_long_vs_float64(L, counts, heads):
    qkv, keep, d_out, want = case(L, counts, heads)
    got, _ = run(qkv, keep, heads, d_out)
    got = got.view(len(counts), L, -1).cpu()
    errs = _thirds(got, want, heads)
    print(f"packed_mha_bwd_long {(L, counts, heads)}: max |err| / max |want| = {errs}")
    assert all(e < BOUND for e in errs.values()), errs
    assert torch.equal(got[keep < 0.5], torch.zeros_like(got[keep < 0.5]))   # the default buffer is zeroed; dropped tokens are not written
    for b, n in enumerate(counts):
        if n == 1:       # the one-token image: P = 1, so dQ = dK = 0 and dV = dO
            g = got[b, 0].reshape(3, -1)
            tol = 2.0 ** -15 * d_out[b, 0].abs().max().item()                 # bf16x3 carries dO with 16 mantissa bits (hi + lo)
            assert g[0].abs().max().item() <= tol and g[1].abs().max().item() <= tol and (g[2] - d_out[b, 0]).abs().max().item() <= tol


def test_long_pair_is_bit_identical_to_the_short_kernel_up_to_256_kept():
    B, L, heads = 4, 320, 2
    keep = _keep_counts(L, [256, 1, 200, 33], 5 + L)
    qkv, d_out = _inputs(keep, heads)
    short, rows = run(qkv, keep, heads, d_out, max_tokens=256, op="packed_mha_bwd")
    assert rows.numel() == 490 and short[rows].abs().max().item() > 0
    long_, _ = run(qkv, keep, heads, d_out, max_tokens=L)
    assert torch.equal(long_, short)                                          # every row: the kept ones the same floats, the others zero
    long256, _ = run(qkv, keep, heads, d_out, max_tokens=256)
    assert torch.equal(long256, short)
    want = mha_bwd_autograd(qkv.double(), keep, heads, d_out.double())
    assert grad_err(long_.view(B, L, -1), want) < BOUND


def test_ragged_batch_guard_rows_poison_and_determinism():
    """300, 40, 0 and 577 kept tokens at L = 577 in one call.  The workspace and the packed rows of d_out past the count are NaN: an entry the
    first launch did not write, or a row past the count, must never be loaded (NaN * 0 is NaN)."""
    B, L, heads = 4, 577, 2
    dim = 64 * heads
    keep = _keep_counts(L, [300, 40, 0, 577], 5 + L)
    qkv, d_out = _inputs(keep, heads)
    live = [0, 1, 3]
    want = mha_bwd_autograd(qkv[live].double(), keep[live], heads, d_out[live].double())      # images are independent
    poisoned_ws = lambda: torch.full((3 * heads * B * L,), float("nan"), device=DEV)
    out = torch.full((B * L, 3 * dim), SENTINEL, device=DEV)
    got, rows = run(qkv, keep, heads, d_out, out=out, ws=poisoned_ws(), poison=True)
    assert got.data_ptr() == out.data_ptr() and rows.numel() == 917
    dropped = (keep.reshape(-1) < 0.5).to(DEV)
    assert torch.equal(out[dropped], torch.full_like(out[dropped], SENTINEL))      # dropped tokens and all of image 2 are untouched
    assert torch.equal(out.view(B, L, -1)[2], torch.full_like(out.view(B, L, -1)[2], SENTINEL))
    assert torch.isfinite(out[rows]).all() and not (out[rows] == SENTINEL).any()   # every column of every kept row is written
    o = out.view(B, L, -1).cpu()
    kept = keep[live] > 0.5
    errs = _thirds(torch.where(kept[..., None], o[live], torch.zeros(())), want, heads)
    print(f"ragged batch: {errs}")
    assert all(e < BOUND for e in errs.values()), errs
    again = torch.full((B * L, 3 * dim), SENTINEL, device=DEV)
    run(qkv, keep, heads, d_out, out=again, ws=poisoned_ws(), poison=True)
    assert torch.equal(again, out)                                                 # two runs are bit-identical
    # max_tokens = 300 on the same lists: image 3's kept tokens number 300 and above are neither read nor written
    out3 = torch.full((B * L, 3 * dim), SENTINEL, device=DEV)
    run(qkv, keep, heads, d_out, max_tokens=300, out=out3, ws=poisoned_ws(), poison=True)
    o3 = out3.view(B, L, -1).cpu()
    idx3 = torch.nonzero(keep[3] > 0.5).reshape(-1)
    assert torch.equal(o3[3, idx3[300:]], torch.full_like(o3[3, idx3[300:]], SENTINEL))
    keep_t = keep[live].clone()
    keep_t[2, idx3[300:]] = 0.0
    assert keep_t.sum(1).tolist() == [300.0, 40.0, 300.0]
    want_t = mha_bwd_autograd(qkv[live].double(), keep_t, heads, (d_out[live] * keep_t[..., None]).double())
    errs = _thirds(torch.where((keep_t > 0.5)[..., None], o3[live], torch.zeros(())), want_t, heads)
    print(f"max_tokens 300: {errs}")
    assert all(e < BOUND for e in errs.values()), errs
    assert torch.isfinite(o3[live][keep_t > 0.5]).all() and not (o3[live][keep_t > 0.5] == SENTINEL).any()


def test_head_skipping_across_tiles():
    B, L, heads = 2, 300, 3
    keep = torch.ones(B, L)
    keep[1] = seeded_bernoulli((L,), 0.93, 92)
    keep[1, 0] = 1.0
    assert int(keep[1].sum().item()) > 256
    qkv, d_out = _inputs(keep, heads)
    hk = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    want = mha_bwd_autograd(qkv.double(), keep, heads, d_out.double(), hk)
    plain, _ = run(qkv, keep, heads, d_out)
    got, _ = run(qkv, keep, heads, d_out, head_keep=hk)
    assert grad_err(got.view(B, L, -1), want) < BOUND
    g = got.view(B, L, 3, heads, 64).cpu()
    pl = plain.view(B, L, 3, heads, 64).cpu()
    for b in range(B):
        kept = keep[b] > 0.5
        assert int(kept.sum()) > 256
        for h in range(heads):
            if hk[b, h] < 0.5:       # the dropped head's 3 x 64 columns: exact zeros on every kept row, rows >= 256 of the image included
                assert torch.equal(g[b, kept][:, :, h], torch.zeros_like(g[b, kept][:, :, h]))
            else:                    # the other heads: the run without head_keep, bit for bit
                assert torch.equal(g[b, :, :, h], pl[b, :, :, h])
    # dropped heads leave their rows alone in a caller's buffer except for the zeros: written, not skipped
    out = torch.full((B * L, 3 * 64 * heads), SENTINEL, device=DEV)
    run(qkv, keep, heads, d_out, head_keep=hk, out=out)
    o = out.view(B, L, 3, heads, 64).cpu()
    assert torch.equal(o[1, keep[1] > 0.5][:, :, 0], torch.zeros_like(o[1, keep[1] > 0.5][:, :, 0]))


def test_packed_mha_bwd_long_argument_errors():
    from laudnet_amd import LdnError, ops
    B, L, heads = 2, 300, 1
    keep = torch.ones(B, L)
    tok_rows, prefix, _ = ops.token_lists(keep.to(DEV))
    qkv = torch.zeros(B * L, 192, device=DEV)
    d_out = torch.zeros(B * L, 64, device=DEV)
    ops.packed_mha_bwd_long(qkv, tok_rows, prefix, B, heads, L, d_out)
    ops.packed_mha_bwd_long(qkv, tok_rows, prefix, B, heads, L, d_out, ws=torch.empty(3 * B * L, device=DEV))
    with pytest.raises(LdnError):
        ops.packed_mha_bwd_long(qkv.double(), tok_rows, prefix, B, heads, L, d_out)
    with pytest.raises(LdnError):
        ops.packed_mha_bwd_long(qkv, tok_rows, prefix, B, heads, L, d_out.half())
    with pytest.raises(LdnError):
        ops.packed_mha_bwd_long(qkv, tok_rows, prefix, B, heads, L, d_out[:, :32])
    with pytest.raises(LdnError):
        ops.packed_mha_bwd_long(qkv[:, :100], tok_rows, prefix, B, heads, L, d_out)
    with pytest.raises(LdnError):
        ops.packed_mha_bwd_long(qkv, tok_rows.long(), prefix, B, heads, L, d_out)
    with pytest.raises(LdnError):
        ops.packed_mha_bwd_long(qkv, tok_rows, prefix, B, heads, L, d_out, head_keep=torch.ones(B, 2, device=DEV))
    with pytest.raises(LdnError):
        ops.packed_mha_bwd_long(qkv, tok_rows, prefix, B, heads, L, d_out, out=torch.zeros(B * L, 64, device=DEV))
    with pytest.raises(LdnError, match="ws"):
        ops.packed_mha_bwd_long(qkv, tok_rows, prefix, B, heads, L, d_out, ws=torch.empty(3 * B * L - 1, device=DEV))
    with pytest.raises(LdnError, match="256"):                                   # the one-launch op keeps its limit
        ops.packed_mha_bwd(qkv, tok_rows, prefix, B, heads, 257, d_out)
