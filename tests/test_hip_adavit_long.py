"""Token skipping with MORE than 256 kept tokens per image (k_packed_mha_long: query tiles of 256, keys streamed through LDS in tiles
of 256 under one running softmax).  The attention alone against float64 dense masked attention at every seam of the tiling (one
token past a tile, a tile plus one chunk, exactly two tiles, three tiles with a ragged last one), bit-identity with k_packed_mha on
images of at most 256 kept tokens, a ragged batch (300 / 40 / 0 / 577 kept) in one launch with a guard region, head skipping
across query tiles, then one block and a two-block trunk at the 384 px shape (577 tokens) against oracle/adavit_ref.py
(self-consistency: parity unpinned, see the oracle's header)."""
import pytest
import torch

from fill import seeded_bernoulli, seeded_randn
from oracle import adavit_ref as AR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0


def _attention64(qkv, keep, heads):
    """float64 dense masked attention on the CPU: qkv [B, L, 3 * dim], keep [B, L] -> [B * L, dim] (rows of dropped tokens and of
    images without a kept token are meaningless: never compared)."""
    B, L, _ = qkv.shape
    q, k, v = qkv.double().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 64 ** -0.5
    s = s.masked_fill(keep[:, None, None, :] < 0.5, float("-inf"))
    return torch.nan_to_num(s.softmax(-1) @ v).transpose(1, 2).reshape(B * L, 64 * heads)


def _keep_counts(L, counts, seed):
    """[len(counts), L] keep masks with exactly counts[b] kept tokens in image b, the CLS token among them (counts[b] = 0: none)."""
    keep = torch.zeros(len(counts), L)
    for b, n in enumerate(counts):
        if n > 0:
            perm = torch.randperm(L - 1, generator=torch.Generator().manual_seed(seed + b))[: n - 1] + 1
            keep[b, 0] = 1.0
            keep[b, perm] = 1.0
    assert keep.sum(1).tolist() == [float(n) for n in counts]
    return keep


def _run(qkv, keep, heads, max_tokens, head_keep=None):
    """ops.packed_mha on the device -> (packed rows [capacity, dim] on the CPU, kept rows [n], n)."""
    from laudnet_amd import ops, load_library
    load_library()
    B, L, _ = qkv.shape
    tok_rows, prefix, count = ops.token_lists(keep.to(DEV))
    got = ops.packed_mha(qkv.reshape(B * L, -1).to(DEV), tok_rows, prefix, B, heads, max_tokens,
                         head_keep=None if head_keep is None else head_keep.to(DEV))
    n = int(count.item())
    assert n == int(keep.sum().item())
    rows = tok_rows[:n].long().cpu()
    assert torch.equal(rows, torch.nonzero(keep.reshape(-1)).reshape(-1))
    return got.cpu(), rows, n


def _seam_keep(B, L, pattern, seed):
    keep = torch.ones(B, L)
    if pattern != "all":                       # image 0 keeps everything, image 1 its CLS token only, image 2 Bernoulli(pattern)
        keep[1, 1:] = 0.0
        keep[2] = seeded_bernoulli((L,), pattern, seed)
        keep[2, 0] = 1.0
    return keep


@pytest.mark.parametrize("B,L,heads,pattern", [(3, 257, 1, 0.5), (2, 288, 2, "all"), (2, 512, 1, "all"), (3, 577, 2, 0.6)])
def test_packed_mha_long_vs_float64_dense_masked_attention(B, L, heads, pattern):
    """Max abs error against float64 below the project's 2e-5 (the bound of test_packed_mha_vs_dense_masked_attention on the same
    randn inputs: a softmax-weighted mean of unit-variance values does not grow with L).  These shapes were refused (LdnError)
    before k_packed_mha_long."""
    qkv = seeded_randn((B, L, 3 * 64 * heads), 3 + L)
    keep = _seam_keep(B, L, pattern, 5 + L)
    want = _attention64(qkv, keep, heads)
    got, rows, n = _run(qkv, keep, heads, L)
    err = (got[:n].double() - want[rows]).abs().max().item()
    print(f"[mha_long] B={B} L={L} heads={heads}: max |err| vs float64 = {err:.3e}")
    assert err < 2e-5, err


def test_long_kernel_is_bit_identical_to_k_packed_mha_up_to_256_kept():
    """Keys in ascending 32-key chunks with the per-chunk arithmetic of k_packed_mha: images with <= 256 kept tokens (one exactly 256,
    one its CLS token only) get the same floats from either kernel."""
    B, L, heads = 4, 320, 2
    qkv = seeded_randn((B, L, 3 * 64 * heads), 71)
    keep = _keep_counts(L, [256, 1, 200, 33], 72)
    short, rows_s, n = _run(qkv, keep, heads, 256)        # k_packed_mha
    long_, rows_l, n_l = _run(qkv, keep, heads, L)        # k_packed_mha_long: identical work
    assert n == n_l == 490 and torch.equal(rows_s, rows_l)
    assert torch.equal(long_[:n], short[:n])
    err = (long_[:n].double() - _attention64(qkv, keep, heads)[rows_l]).abs().max().item()
    assert err < 2e-5, err


def test_ragged_batch_in_one_launch_and_guard_rows():
    """300, 40, 0 and 577 kept tokens at L = 577 in one launch: workgroups whose query tile lies past their image's count (and all
    three of the image without a kept token) return at once, the others stream 2, 1 and 3 key tiles.  Rows of `out` past `count`
    keep their sentinel."""
    from laudnet_amd import _lib as L_, ops, load_library
    lib = load_library()
    B, L, heads = 4, 577, 2
    dim = 64 * heads
    qkv = seeded_randn((B, L, 3 * dim), 81)
    keep = _keep_counts(L, [300, 40, 0, 577], 82)
    want = _attention64(qkv, keep, heads)
    tok_rows, prefix, count = ops.token_lists(keep.to(DEV))
    assert prefix.cpu().tolist() == [0, 300, 340, 340, 917]
    n = int(count.item())
    assert n == 917
    qd = qkv.reshape(B * L, 3 * dim).to(DEV)
    out = torch.full((B * L, dim), SENTINEL, device=DEV)
    L_.check(lib.ldn_packed_mha(L_.ptr(qd), 3 * dim, L_.ptr(tok_rows), L_.ptr(prefix), B, heads, 64, L, 64 ** -0.5, L_.ptr(out), dim,
                                L_.stream_ptr(out)), "ldn_packed_mha")
    out = out.cpu()
    rows = tok_rows[:n].long().cpu()
    err = (out[:n].double() - want[rows]).abs().max().item()
    assert err < 2e-5, err
    assert torch.equal(out[n:], torch.full((B * L - n, dim), SENTINEL))


def test_head_skipping_across_query_tiles():
    """A dropped (image, head) writes exact zeros to its 64 columns on EVERY live row (both query tiles: rows >= 256 of the image
    too); the kept heads are the floats of the run without head_keep."""
    B, L, heads = 2, 300, 3
    qkv = seeded_randn((B, L, 3 * 64 * heads), 91)
    keep = torch.ones(B, L)
    keep[1] = seeded_bernoulli((L,), 0.93, 92)
    keep[1, 0] = 1.0
    assert int(keep[1].sum().item()) > 256
    hk = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    full, rows, n = _run(qkv, keep, heads, L)
    got, _, _ = _run(qkv, keep, heads, L, head_keep=hk)
    img = rows // L
    for b in range(B):
        live = got[:n][img == b]
        assert live.shape[0] > 256
        for hd in range(heads):
            cols = slice(64 * hd, 64 * hd + 64)
            if hk[b, hd] < 0.5:
                assert torch.equal(live[:, cols], torch.zeros_like(live[:, cols])), (b, hd)
            else:
                assert torch.equal(live[:, cols], full[:n][img == b][:, cols]), (b, hd)


def _keep(B, L, p, seed):
    k = seeded_bernoulli((B, L), p, seed)
    k[:, 0] = 1.0            # CLS
    if B > 1:
        k[1, 1:] = 0.0       # an image that keeps only CLS
    if B > 2:
        k[2] = 1.0           # an image that keeps everything
    return k


def test_token_skip_block_300_tokens_vs_oracle():
    from laudnet_amd import ops
    from laudnet_amd.adavit import TokenSkipBlock
    B, L, dim, heads = 3, 300, 128, 2
    ref = AR.TokenSkipBlockRef(dim, heads).eval()
    torch.manual_seed(7)
    for p_ in ref.parameters():
        torch.nn.init.normal_(p_, std=0.05) if p_.dim() > 1 else torch.nn.init.normal_(p_, mean=0.0, std=0.1)
    hip = TokenSkipBlock(dim, heads).eval()
    hip.load_state_dict(ref.state_dict())
    hip = hip.to(DEV)
    x = seeded_randn((B, L, dim), 21)
    keep = _keep(B, L, 0.5, 22)                  # Bernoulli 0.5 / CLS only / all 300 (two query tiles, two key tiles)
    with torch.no_grad():
        want = ref.double()(x.double(), keep.double()).float()
    ops.set_math_mode("bf16x3")
    try:
        with torch.no_grad():
            got = hip(x.to(DEV), keep.to(DEV)).cpu()
    finally:
        ops.set_math_mode("fp32")
    dropped = keep < 0.5
    assert torch.equal(got[dropped], x[dropped])                     # skipped tokens pass through bit-exactly
    err = (got - want).abs().max().item()
    assert err < 1e-4 * max(1.0, want.abs().max().item()), err


def test_token_skip_trunk_384px_shape():
    """DeiT-S at 384 px: 577 tokens, keep 0.7 per block (about 404 kept: two query tiles, two key tiles); the second block also
    drops heads per image, skips image 1's attention (no token in the attention list: Lb = 0 in the kernel) and image 0's MLP."""
    from laudnet_amd import ops
    from laudnet_amd.adavit import TokenSkipViT
    B, L, dim, heads, depth = 2, 577, 384, 6, 2
    ref = AR.TokenSkipViTRef(depth, dim, heads).eval()
    torch.manual_seed(11)
    for p_ in ref.parameters():
        if p_.dim() > 1:
            torch.nn.init.normal_(p_, std=0.03)
    hip = TokenSkipViT(depth, dim, heads).eval()
    hip.load_state_dict(ref.state_dict())
    hip = hip.to(DEV)
    x = seeded_randn((B, L, dim), 31)
    keeps = []
    for i in range(depth):
        k = seeded_bernoulli((B, L), 0.7, 40 + i)
        k[:, 0] = 1.0
        keeps.append(k)
    hks = [None, torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0, 1.0, 1.0]])]
    aks = [None, torch.tensor([1.0, 0.0])]
    mks = [None, torch.tensor([0.0, 1.0])]
    with torch.no_grad():
        want = ref.double()(x.double(), [k.double() for k in keeps], hks, aks, mks).float()
    dev = lambda seq: [None if t is None else t.to(DEV) for t in seq]
    ops.set_math_mode("bf16x3")
    try:
        with torch.no_grad():
            got = hip(x.to(DEV), dev(keeps), dev(hks), dev(aks), dev(mks)).cpu()
    finally:
        ops.set_math_mode("fp32")
    err = (got - want).abs().max().item()
    assert err < 1e-3 * max(1.0, want.abs().max().item()), err
