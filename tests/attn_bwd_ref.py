"""The formulas ldn_packed_mha_bwd and ldn_rows_ln_bwd implement, restated in float64 torch on the host (tests/test_attn_bwd_ref.py checks them
against autograd; the GPU tests use the autograd references, the kernel author debugs against these): per (image, head) over the image's
kept tokens
    P = softmax(scale Q K^T)   dV = P^T dO   dP = dO V^T   D_i = sum_j P_ij dP_ij (= sum_d dO_id O_id)   dS = P o (dP - D)
    dQ = scale dS K            dK = scale dS^T Q
and per row of a LayerNorm  y = gamma x^ + beta,  x^ = (x - mean) rstd:
    g = dy gamma   dx = rstd (g - mean_k(g) - x^ mean_k(g x^))   d_gamma = sum_rows dy x^   d_beta = sum_rows dy."""
import torch

BOUND = 1e-3      # every element of a gradient within BOUND of the tensor's own maximum (tests/test_hip_training_f64.py's strict statement)


def keep_pattern(B, L, p, seed):
    """tests/test_hip_adavit.py's _keep: CLS always kept, image 1 keeps only CLS, image 2 keeps everything"""
    from fill import seeded_bernoulli
    k = seeded_bernoulli((B, L), p, seed)
    k[:, 0] = 1.0
    if B > 1:
        k[1, 1:] = 0.0
    if B > 2:
        k[2] = 1.0
    return k


def mha_dense(qkv, keep, heads, head_keep=None):
    """The dense masked restatement of ops.packed_mha (test_packed_mha_vs_dense_masked_attention): qkv [B, L, 3 dim], keep [B, L] -> [B, L, dim]
    (rows of dropped tokens hold values too: a dropped token still queries the kept keys; the caller reads the kept rows)."""
    B, L, three = qkv.shape
    dim = three // 3
    q, k, v = qkv.reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 64 ** -0.5
    s = s.masked_fill(keep[:, None, None, :] < 0.5, float("-inf"))
    a = s.softmax(-1) @ v
    if head_keep is not None:
        a = a * head_keep.to(a.dtype)[:, :, None, None]
    return a.transpose(1, 2).reshape(B, L, dim)


def mha_bwd_autograd(qkv, keep, heads, d_out, head_keep=None):
    """d L / d qkv [B, L, 3 dim] by autograd of mha_dense for L = sum(out o d_out), d_out [B, L, dim] ZERO at the dropped tokens (then the
    gradient's rows of dropped tokens are zero as well: they are neither queries with a gradient nor keys with a weight)."""
    x = qkv.detach().clone().requires_grad_(True)
    (mha_dense(x, keep, heads, head_keep) * d_out).sum().backward()
    return x.grad


def mha_bwd_closed_form(qkv, keep, heads, d_out, head_keep=None):
    """The same gradient from the closed form, image by image on the kept tokens (what the kernel computes)."""
    B, L, three = qkv.shape
    dim = three // 3
    scale = 64 ** -0.5
    out = torch.zeros_like(qkv)
    for b in range(B):
        idx = torch.nonzero(keep[b] > 0.5).reshape(-1)
        n = idx.numel()
        if n == 0:
            continue
        Q, K, V = qkv[b, idx].reshape(n, 3, heads, 64).permute(1, 2, 0, 3)          # [heads, n, 64]
        dO = d_out[b, idx].reshape(n, heads, 64).permute(1, 0, 2)
        if head_keep is not None:
            dO = dO * head_keep[b].to(dO.dtype)[:, None, None]
        P = ((Q @ K.transpose(-1, -2)) * scale).softmax(-1)
        dV = P.transpose(-1, -2) @ dO
        dP = dO @ V.transpose(-1, -2)
        D = (P * dP).sum(-1, keepdim=True)
        dS = P * (dP - D)
        dQ = scale * (dS @ K)
        dK = scale * (dS.transpose(-1, -2) @ Q)
        out[b, idx] = torch.stack((dQ, dK, dV)).permute(2, 0, 1, 3).reshape(n, 3 * dim)
    return out


def ln_bwd_closed_form(x, gamma, dy, eps=1e-5):
    """x, dy [rows, C] -> (dx [rows, C], d_gamma [C], d_beta [C]) of y = LayerNorm(x) (biased variance)"""
    mean = x.mean(1, keepdim=True)
    rstd = (x.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def grad_err(got, want):
    """max |got - want| / max |want| (the bound's left side); a zero reference must be met exactly"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    top = want.abs().max().item()
    err = (got - want).abs().max().item()
    return err / top if top > 0 else (0.0 if err == 0 else float("inf"))
