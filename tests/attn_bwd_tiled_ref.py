"""The two-launch scheme of ldn_packed_mha_bwd_long (k_packed_mha_bwd_q + k_packed_mha_bwd_kv) restated in float64 torch on the host, with the
kernels' loop structure: tiles of 256 tokens, chunks of 32, the running {m, l, sum e dP} of a query carried across the key tiles, the
statistics {m, 1 / l, D} handed from the first launch to the second through an array indexed by packed row and head, dK / dV accumulated
over the query tiles in ascending order.  tests/test_attn_bwd_tiled_ref.py checks it against autograd; the kernel author debugs against it."""
import torch

TILE, CHUNK = 256, 32


def _chunks(lo, hi):
    """the 32-token chunks of the tile [lo, hi) in ascending order, the last one ragged"""
    return [(c, min(c + CHUNK, hi)) for c in range(lo, hi, CHUNK)]


def launch_q(Q, K, V, dO, scale, ws, n0, hd):
    """One (image, head) of k_packed_mha_bwd_q: Q / K / V / dO [n, 64] of the kept tokens -> dQ [n, 64]; writes ws[hd, :, n0 + query]."""
    n = Q.shape[0]
    dQ = torch.zeros_like(Q)
    for q0 in range(0, n, TILE):                              # one workgroup per query tile
        q1 = min(q0 + TILE, n)
        q, g = Q[q0:q1], dO[q0:q1]
        m = torch.full((q1 - q0,), float("-inf"), dtype=Q.dtype)
        l = torch.zeros(q1 - q0, dtype=Q.dtype)
        d = torch.zeros(q1 - q0, dtype=Q.dtype)
        for k0 in range(0, n, TILE):                          # pass 1: the key tiles streamed in ascending order
            for c0, c1 in _chunks(k0, min(k0 + TILE, n)):
                s = (q @ K[c0:c1].T) * scale
                dp = g @ V[c0:c1].T
                m_new = torch.maximum(m, s.max(1).values)
                alpha = torch.exp(m - m_new)
                e = torch.exp(s - m_new[:, None])
                l = l * alpha + e.sum(1)
                d = d * alpha + (e * dp).sum(1)
                m = m_new
        inv = 1.0 / l
        dd = d * inv
        ws[hd, 0, n0 + q0:n0 + q1], ws[hd, 1, n0 + q0:n0 + q1], ws[hd, 2, n0 + q0:n0 + q1] = m, inv, dd
        acc = torch.zeros_like(q)
        for k0 in range(0, n, TILE):                          # pass 2: the key tiles again
            for c0, c1 in _chunks(k0, min(k0 + TILE, n)):
                p = torch.exp((q @ K[c0:c1].T) * scale - m[:, None]) * inv[:, None]
                ds = p * (g @ V[c0:c1].T - dd[:, None])
                acc = acc + ds @ K[c0:c1]
        dQ[q0:q1] = acc * scale
    return dQ


def launch_kv(Q, K, V, dO, scale, ws, n0, hd):
    """One (image, head) of k_packed_mha_bwd_kv: -> (dK, dV) [n, 64]; reads ws[hd, :, n0 + query]."""
    n = Q.shape[0]
    dK, dV = torch.zeros_like(K), torch.zeros_like(V)
    for k0 in range(0, n, TILE):                              # one workgroup per key tile
        k1 = min(k0 + TILE, n)
        k, v = K[k0:k1], V[k0:k1]
        ak, av = torch.zeros_like(k), torch.zeros_like(v)
        for q0 in range(0, n, TILE):                          # the query tiles streamed in ascending order
            for c0, c1 in _chunks(q0, min(q0 + TILE, n)):
                m, inv, dd = ws[hd, 0, n0 + c0:n0 + c1], ws[hd, 1, n0 + c0:n0 + c1], ws[hd, 2, n0 + c0:n0 + c1]
                p = torch.exp((Q[c0:c1] @ k.T) * scale - m[:, None]) * inv[:, None]
                ds = p * (dO[c0:c1] @ v.T - dd[:, None])
                av = av + p.T @ dO[c0:c1]
                ak = ak + ds.T @ Q[c0:c1]
        dK[k0:k1], dV[k0:k1] = ak * scale, av
    return dK, dV


def mha_bwd_tiled(qkv, keep, heads, d_out, head_keep=None):
    """d L / d qkv [B, L, 3 dim] (tests/attn_bwd_ref.py: mha_bwd_closed_form's contract) by the two launches: every (image, head) of the first,
    then every (image, head) of the second.  The workspace starts as NaN: an entry the first launch did not write must not be used."""
    B, L, three = qkv.shape
    dim = three // 3
    scale = 64 ** -0.5
    idx = [torch.nonzero(keep[b] > 0.5).reshape(-1) for b in range(B)]
    prefix = [0]
    for i in idx:
        prefix.append(prefix[-1] + i.numel())
    ws = torch.full((heads, 3, max(prefix[-1], 1)), float("nan"), dtype=qkv.dtype)
    out = torch.zeros_like(qkv)
    live = lambda b, hd: idx[b].numel() > 0 and (head_keep is None or head_keep[b, hd] > 0.5)
    rows = lambda b, part, hd: qkv[b, idx[b], part * dim + 64 * hd:part * dim + 64 * hd + 64]
    for launch in (0, 1):
        for b in range(B):
            for hd in range(heads):
                if not live(b, hd):
                    continue                                  # a dropped head: zeros (out is zeroed), no statistics written or read
                Q, K, V = rows(b, 0, hd), rows(b, 1, hd), rows(b, 2, hd)
                dO = d_out[b, idx[b], 64 * hd:64 * hd + 64]
                if launch == 0:
                    out[b, idx[b], 64 * hd:64 * hd + 64] = launch_q(Q, K, V, dO, scale, ws, prefix[b], hd)
                else:
                    dK, dV = launch_kv(Q, K, V, dO, scale, ws, prefix[b], hd)
                    out[b, idx[b], dim + 64 * hd:dim + 64 * hd + 64] = dK
                    out[b, idx[b], 2 * dim + 64 * hd:2 * dim + 64 * hd + 64] = dV
    return out
