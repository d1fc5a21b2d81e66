"""What ldn_packed_mha / ldn_packed_mha_heads compute, restated as dense masked attention in float64 torch on the host
(tests/test_attn_fwd_ref.py checks it against torch's scaled_dot_product_attention, against attn_bwd_ref.mha_dense and against a hand-written
example of the max_tokens rule; tests/test_hip_attn_fwd.py compares the kernels with it): per (image, head)
    out_i = sum_j softmax_j(scale q_i . k_j) v_j      i, j over the image's ATTENDING tokens,
the attending tokens being the image's kept tokens, cut to the first max_tokens of them in ascending row order (the order of ops.token_lists)
when max_tokens is given.  The later kept tokens keep their place in the packed row numbering (the prefix counts every kept token) but are
neither keys nor queries, and their packed rows are not written."""
import torch


def attending(keep, max_tokens=None):
    """keep [B, L] {0,1} -> the same mask with every image cut to its first max_tokens kept tokens (ascending row order)"""
    att = keep > 0.5
    if max_tokens is not None:
        att = att & (att.cumsum(1) <= max_tokens)
    return att


def mha_packed_f64(qkv, keep, heads, scale=None, max_tokens=None, head_keep=None):
    """qkv [B, L, 3 dim] (q | k | v, each [heads][head_dim]), keep [B, L] {0,1}, head_keep [B, heads] {0,1} or None
    -> (packed [N, dim] float64, written [W] int64): N = the number of kept tokens, packed row n belongs to the n-th kept token in image-major
    ascending order (tok_rows[n] of ops.token_lists); `written` lists, ascending, the packed rows the contract says are written -- those of the
    attending tokens.  The other rows of `packed` are zero and mean nothing.  A dropped (image, head) gives zeros on the written rows.
    Differentiable in qkv (float64 in, float64 autograd out)."""
    B, L, three = qkv.shape
    dim = three // 3
    hd = dim // heads
    assert three == 3 * dim and dim == heads * hd
    scale = hd ** -0.5 if scale is None else scale
    x = qkv.double()
    kept = keep > 0.5
    att = attending(keep, max_tokens)
    pieces, written, n0 = [], [], 0
    for b in range(B):
        idx = torch.nonzero(kept[b]).reshape(-1)                             # ascending rows: the image's packed rows n0 .. n0 + count - 1
        out_b = torch.zeros(idx.numel(), dim, dtype=torch.float64)
        live = att[b, idx]                                                   # a prefix of the image's kept tokens
        if live.any():
            q, k, v = x[b].reshape(L, 3, heads, hd).permute(1, 2, 0, 3)      # [heads, L, hd]
            s = (q @ k.transpose(-1, -2)) * scale                            # dense [heads, L, L]: every token queries ...
            s = s.masked_fill(~att[b][None, None, :], float("-inf"))         # ... the attending keys only
            o = s.softmax(-1) @ v                                            # [heads, L, hd]
            if head_keep is not None:
                o = o * (head_keep[b] > 0.5).double()[:, None, None]
            o = o.transpose(0, 1).reshape(L, dim)[idx]                       # the kept tokens' rows
            out_b = torch.where(live[:, None], o, out_b)
            written.append(n0 + torch.nonzero(live).reshape(-1))
        pieces.append(out_b)
        n0 += idx.numel()
    packed = torch.cat(pieces) if pieces else torch.zeros(0, dim, dtype=torch.float64)
    written = torch.cat(written) if written else torch.zeros(0, dtype=torch.int64)
    return packed, written
