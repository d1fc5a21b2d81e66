"""ops.packed_mha_bwd (ldn_packed_mha_bwd) against float64 autograd of the dense masked restatement of ops.packed_mha
(tests/attn_bwd_ref.py: test_packed_mha_vs_dense_masked_attention's, in float64).  Bound: every element of the gradient within 1e-3 of the
tensor's own maximum -- the strict statement of tests/test_hip_training_f64.py, no allowance (there are no ReLU ties here).  `measure`
returns the figure without asserting (tools/train_adavit_grad_err.py records it, beside fp32 autograd of the same restatement on the GPU)."""
import pytest
import torch

from attn_bwd_ref import BOUND, grad_err, keep_pattern, mha_bwd_autograd
from fill import seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, L, heads, keep probability): ragged counts that are no multiple of 32 + a one-token image + a full image | one key past a 32-key chunk |
# image 0 forced to keep all 256: the full tile | the DeiT-S shape
SHAPES = [(3, 40, 2, 0.5), (2, 33, 1, 1.0), (2, 256, 1, 0.7), (4, 197, 6, 0.5)]
_CASES = {}


def case(B, L, heads, p):
    """(qkv [B, L, 3 dim] fp32, keep, d_out dense fp32 (zero at dropped tokens), want float64), computed once per shape and left unchanged"""
    key = (B, L, heads, p)
    if key not in _CASES:
        dim = 64 * heads
        qkv = seeded_randn((B, L, 3 * dim), 3 + L)
        keep = keep_pattern(B, L, p, 5 + L)
        if L == 256:
            keep[0] = 1.0
        d_out = seeded_randn((B, L, dim), 7 + L) * keep[:, :, None]
        want = mha_bwd_autograd(qkv.double(), keep, heads, d_out.double())
        _CASES[key] = (qkv, keep, d_out, want)
    return _CASES[key]


def run(qkv, keep, heads, d_out, head_keep=None, out=None, max_tokens=None):
    """-> (d_qkv [B * L, 3 dim] on the device, the kept tokens' flat rows)"""
    from laudnet_amd import ops
    B, L, three = qkv.shape
    tok_rows, prefix, count = ops.token_lists(keep.to(DEV))
    n = int(count.item())
    rows = tok_rows[:n].long()
    packed = torch.zeros(B * L, three // 3, device=DEV)
    packed[:n] = d_out.reshape(B * L, -1).to(DEV)[rows]
    got = ops.packed_mha_bwd(qkv.reshape(B * L, three).to(DEV), tok_rows, prefix, B, heads, L if max_tokens is None else max_tokens, packed,
                             head_keep=None if head_keep is None else head_keep.to(DEV), out=out)
    return got, rows


def measure(B, L, heads, p):
    qkv, keep, d_out, want = case(B, L, heads, p)
    got, _ = run(qkv, keep, heads, d_out)
    ref32 = mha_bwd_autograd(qkv.to(DEV), keep.to(DEV), heads, d_out.to(DEV))
    return {"d_qkv": grad_err(got.view(B, L, -1), want)}, {"d_qkv": grad_err(ref32, want)}


@pytest.mark.parametrize("B,L,heads,p", SHAPES)
def test_packed_mha_bwd_vs_float64(B, L, heads, p):
    qkv, keep, d_out, want = case(B, L, heads, p)
    got, _ = run(qkv, keep, heads, d_out)
    got = got.view(B, L, -1).cpu()
    err = grad_err(got, want)
    print(f"packed_mha_bwd {(B, L, heads, p)}: max |err| / max |want| = {err:.3e}")
    assert err < BOUND, err
    for name, sl in (("dq", slice(0, 64 * heads)), ("dk", slice(64 * heads, 128 * heads)), ("dv", slice(128 * heads, 192 * heads))):
        assert grad_err(got[..., sl], want[..., sl]) < BOUND, name           # each third against its own maximum
    assert torch.equal(got[keep < 0.5], torch.zeros_like(got[keep < 0.5]))   # the default buffer is zeroed; dropped tokens are not written
    if B > 1:        # the one-token image: P = 1, so dQ = dK = 0 and dV = dO
        g = got[1, 0].reshape(3, -1)
        tol = 2.0 ** -15 * d_out[1, 0].abs().max().item()                     # bf16x3 carries dO with 16 mantissa bits (hi + lo)
        assert g[0].abs().max().item() <= tol and g[1].abs().max().item() <= tol and (g[2] - d_out[1, 0]).abs().max().item() <= tol


def test_packed_mha_bwd_head_keep():
    B, L, heads, p = 3, 40, 2, 0.5
    qkv, keep, d_out, _ = case(B, L, heads, p)
    hk = torch.tensor([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0]])
    want = mha_bwd_autograd(qkv.double(), keep, heads, d_out.double(), hk)
    plain, _ = run(qkv, keep, heads, d_out)
    got, _ = run(qkv, keep, heads, d_out, head_keep=hk)
    assert grad_err(got.view(B, L, -1), want) < BOUND
    g = got.view(B, L, 3, heads, 64).cpu()
    pl = plain.view(B, L, 3, heads, 64).cpu()
    for b in range(B):
        kept = keep[b] > 0.5
        for h in range(heads):
            if hk[b, h] < 0.5:       # the dropped head's 3 x 64 columns: exact zeros on the image's kept rows
                assert torch.equal(g[b, kept][:, :, h], torch.zeros_like(g[b, kept][:, :, h]))
            else:                    # the other heads: the run without head_keep, bit for bit
                assert torch.equal(g[b, :, :, h], pl[b, :, :, h])


def test_packed_mha_bwd_writes_kept_rows_only_and_is_deterministic():
    from laudnet_amd import ops
    B, L, heads, p = 3, 40, 2, 0.5
    qkv, keep, d_out, want = case(B, L, heads, p)
    sentinel = -7.25
    out = torch.full((B * L, 3 * 64 * heads), sentinel, device=DEV)
    got, rows = run(qkv, keep, heads, d_out, out=out)
    assert got.data_ptr() == out.data_ptr()
    dropped = (keep.reshape(-1) < 0.5).to(DEV)
    assert torch.equal(out[dropped], torch.full_like(out[dropped], sentinel))      # rows of dropped tokens are untouched
    assert not (out[rows] == sentinel).any()                                       # every column of every kept row is written
    again, _ = run(qkv, keep, heads, d_out)
    assert torch.equal(again[rows], out[rows])                                     # two runs are bit-identical
    # an image with no listed tokens (a skipped attention sub-block) is not written
    keep0 = keep.clone()
    keep0[2] = 0.0
    out2 = torch.full((B * L, 3 * 64 * heads), sentinel, device=DEV)
    run(qkv, keep0, heads, d_out * keep0[:, :, None], out=out2)
    assert torch.equal(out2.view(B, L, -1)[2], torch.full_like(out2.view(B, L, -1)[2], sentinel))
    assert torch.equal(out2.view(B, L, -1)[:2], out.view(B, L, -1)[:2])            # the other images do not depend on it
    # tokens of an image past max_tokens are neither read nor written: image 2 keeps 40, max_tokens 32
    out3 = torch.full((B * L, 3 * 64 * heads), sentinel, device=DEV)
    run(qkv, keep, heads, d_out, out=out3, max_tokens=32)
    o3 = out3.view(B, L, -1)
    assert torch.equal(o3[2, 32:], torch.full_like(o3[2, 32:], sentinel)) and not (o3[2, :32] == sentinel).any()


def test_packed_mha_bwd_argument_errors():
    from laudnet_amd import LdnError, ops
    B, L, heads = 2, 300, 1
    keep = torch.ones(B, L)
    tok_rows, prefix, _ = ops.token_lists(keep.to(DEV))
    qkv = torch.zeros(B * L, 192, device=DEV)
    d_out = torch.zeros(B * L, 64, device=DEV)
    with pytest.raises(LdnError, match="256"):
        ops.packed_mha_bwd(qkv, tok_rows, prefix, B, heads, 257, d_out)
    ops.packed_mha_bwd(qkv, tok_rows, prefix, B, heads, 256, d_out)                 # the first 256 tokens of each image
    with pytest.raises(LdnError):
        ops.packed_mha_bwd(qkv.double(), tok_rows, prefix, B, heads, 256, d_out)
    with pytest.raises(LdnError):
        ops.packed_mha_bwd(qkv, tok_rows, prefix, B, heads, 256, d_out.half())
    with pytest.raises(LdnError):
        ops.packed_mha_bwd(qkv, tok_rows, prefix, B, heads, 256, d_out[:, :32])
    with pytest.raises(LdnError):
        ops.packed_mha_bwd(qkv[:, :100], tok_rows, prefix, B, heads, 256, d_out)
    with pytest.raises(LdnError):
        ops.packed_mha_bwd(qkv, tok_rows.long(), prefix, B, heads, 256, d_out)
    with pytest.raises(LdnError):
        ops.packed_mha_bwd(qkv, tok_rows, prefix, B, heads, 256, d_out, head_keep=torch.ones(B, 2, device=DEV))
    with pytest.raises(LdnError):
        ops.packed_mha_bwd(qkv, tok_rows, prefix, B, heads, 256, d_out, out=torch.zeros(B * L, 64, device=DEV))
