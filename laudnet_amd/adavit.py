"""Token skipping on the HIP path (BASELINE config 5: AdaViT / DeiT-S shaped blocks, "dynamic-token packed MHA").

The reference ships no model for this configuration, only the latency model of its operators
(DyNetSimulator/adavit/simulate_adavit.py:77-182): q / k / v, attention among the SELECTED tokens, projection /
MLP / residual updates on the selected tokens only (the latency model prices q / k / v on every token, :90-93; a dropped token is neither
query nor key, so they are computed for the attending tokens only -- TokenSkipBlock.qkv_kept_only).  This module executes that operator list on PACKED token lists with the
kernels of libldn_hip.so: the keep mask becomes a row list (ldn_mask_to_index on a [B, L, 1] mask), the linears are the packed-row
1x1 kernel (k_dense: gather rows in, scatter-add rows out, fused bias + residual), the attention is ldn_packed_mha (one workgroup
per image and head over the image's kept tokens; beyond 256 tokens per image, e.g. the 577 of a 384 px input, one workgroup per image,
head and tile of 256 queries, the keys streamed through LDS 256 at a time -- any sequence length).  HEAD skipping (a per-image head mask: q / k / v masked in the linear's epilogue, the
dropped heads' attention workgroups compute nothing) and LAYER skipping (per-image decisions for the attention and the MLP sub-block: the
image has no tokens in that sub-block's list) of simulate_adavit.py:81-88,140-182 ride on the same lists.  LayerNorm and GELU are epilogue terms of the linears (ldn_row_stats + the ln_* / relu-mode-3 arguments of ldn_conv_rows_split).  Parity is UNPINNED (there is
nothing in the reference to pin it to): tests compare against oracle/adavit_ref.py, a dense masked restatement of the same operator
list.  The modules are eval-only; no CPU fallback.

TRAINING goes through block_train / train_forward below (forward + backward on the same packed lists, one autograd.Function per block): the
forward runs the inference kernels and keeps each sub-block's input rows, the backward is ldn_packed_mha_bwd (attention), ldn_rows_ln_bwd (both
LayerNorms), the transposed linears on ldn_conv_rows (gather in, scatter out) and the weight gradients on ldn_wgrad_rows.  A dropped token's
gradient passes through untouched.  Sequences of more than 256 tokens (384 px: 577) train behind USE_LONG_BWD (env LDN_MHA_BWD_LONG=1; default
off): their attention backward is ldn_packed_mha_bwd_long, two launches over tiles of 256 queries / keys.  Not built (LdnError): more than 256
kept tokens per image with the switch off, gradients of the keep masks, q / k / v of unattending tokens (qkv_kept_only = False), dropout /
drop-path."""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import training as _tr
from ._lib import LdnError


class TokenSkipBlock(nn.Module):
    """Pre-norm transformer block (DeiT layout: norm1, attn.qkv / proj, norm2, mlp.fc1 / fc2) that updates only the kept tokens."""

    def __init__(self, dim=384, heads=6, mlp_ratio=4.0):
        super().__init__()
        if dim % heads or dim // heads != 64:
            raise LdnError("TokenSkipBlock: head dimension must be 64 (DeiT / AdaViT: dim = 64 * heads)")
        hidden = int(dim * mlp_ratio)
        if dim % 32 or hidden % 32:
            raise LdnError("TokenSkipBlock: dim and the MLP width must be multiples of 32")
        self.dim, self.heads = dim, heads
        self.norm1 = nn.LayerNorm(dim)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim)
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)
        self._w = None

    def invalidate(self):
        """Drop the folded weights (after an edit their key cannot see: through `p.data`, or of a parameter that is an inference tensor --
        the blind spots of laud_resnet._PrepCache; a replaced parameter object IS seen here, the key walks the module on every call)."""
        self._w = None

    def _weights(self, dev):
        """Linear weights as k_dense wants them ([out, 1, in] fp32).  The two LayerNorms are folded into the linears that follow them
        (ldn_conv_rows_split: LN(x) . w + b = rstd (x . (gamma * w) - mean c1) + (w . beta + b)): qkv and fc1 carry gamma-scaled
        weights, c1 = their row sums and the constant as bias; only the rows' {mean, rstd} are computed per call (ldn_row_stats).
        Kept until a parameter changes: keyed on (data_ptr, version) of every parameter, the LayerNorms' included."""
        key = ops.version_key(tuple(self.parameters()))
        if self._w is None or self._w[0] != key:
            with torch.no_grad():
                def plain(lin):
                    return (lin.weight.detach().float().reshape(lin.out_features, 1, lin.in_features).contiguous().to(dev),
                            lin.bias.detach().float().contiguous().to(dev))

                def after_ln(lin, ln):
                    w = lin.weight.detach().double()
                    g, be = ln.weight.detach().double(), ln.bias.detach().double()
                    wg = (w * g.view(1, -1)).float()
                    # c1 multiplies the row MEAN and cancels against the GEMM's large term when |mean| >> std: it must be the row sum
                    # of the weights the kernel actually multiplies with (the bf16 hi + lo split of wg, ~16 mantissa bits), not of
                    # the exact products -- the mismatch would be amplified by rstd
                    hi, lo = ops._hi_lo(wg)
                    c1 = (hi.double() + lo.double()).sum(dim=1)
                    return (wg.reshape(lin.out_features, 1, lin.in_features).contiguous().to(dev),
                            (w @ be + lin.bias.detach().double()).float().contiguous().to(dev), c1.float().contiguous().to(dev))
                self._w = (key, after_ln(self.qkv, self.norm1), plain(self.proj), after_ln(self.fc1, self.norm2), plain(self.fc2))
        return self._w[1:]

    qkv_kept_only = True      # class-level switch (A/B, tests): False = q / k / v for the rows of `qkv_rows` (every token of the running images)

    def run_packed(self, x2d, tok_rows, prefix, count, B, max_tokens, head_keep=None, mlp_lists=None, qkv_rows=None):
        """x2d [B*L, dim] fp32, updated IN PLACE on the kept tokens; tok_rows / prefix / count from ops.token_lists (the attention
        sub-block's token list).  Head and layer skipping (simulate_adavit.py:81-88,140-182), all optional:
          head_keep [B, heads] {0,1}  heads each image attends with: q / k / v of a dropped head are masked in the linear's epilogue,
                                      its attention workgroup computes nothing and contributes zeros to the projection;
          mlp_lists (rows, prefix, count)  the MLP sub-block's own token list (layer skipping decides the two sub-blocks separately:
                                      an image whose attention / MLP is skipped simply has no tokens in that list);
          qkv_rows (rows, count)      (only with qkv_kept_only = False) token rows q / k / v are computed for; by default they are
                                      computed for the attention list itself."""
        if self.training:
            raise LdnError("laudnet_amd implements the eval-mode (inference) hot path only")
        if ops.get_math_mode() != "bf16x3":
            raise LdnError("TokenSkipBlock runs in the bf16x3 arithmetic mode (ops.set_math_mode('bf16x3'))")
        (wq, bq, cq), (wp, bp), (w1, b1, c1), (w2, b2) = self._weights(x2d.device)
        rows = x2d.shape[0]
        Lt = rows // B
        q_rows, q_count = qkv_rows if qkv_rows is not None and not self.qkv_kept_only else (tok_rows, count)
        st = ops.row_stats(x2d, self.norm1.eps, rows=q_rows, count=q_count)                     # {mean, rstd} of the attending tokens (norm1)
        qkv = torch.empty(rows, 3 * self.dim, device=x2d.device, dtype=torch.float32)
        hk3 = None
        if head_keep is not None:     # [B, 3 * dim]: the head's decision over its 64 channels of q, k and v
            hk = head_keep.float().reshape(B, self.heads)
            hk3 = hk.repeat_interleave(self.dim // self.heads, dim=1).repeat(1, 3).contiguous()
        # norm1 + q / k / v of the tokens that attend (the attention list: a dropped token is neither query nor key,
        # simulate_adavit.py:96-109) -- not of every token: at keep 0.5 that is half of the widest linear of the block
        m_rows, _, m_count = mlp_lists if mlp_lists is not None else (tok_rows, prefix, count)
        # list lengths of this block's previous forward (pinned memory, no synchronisation): the tile-width hint of the row kernels
        hint = getattr(self, "_rows_hint", None)
        if hint is None:
            hint = self._rows_hint = ops.RowsHint(3)
        nq, na, nm = hint.get(0), hint.get(1), hint.get(2)
        hint.update(q_count, count, m_count)
        ops.conv_rows(x2d, wq, None, bq, qkv, a_rows=q_rows, out_rows=q_rows, taps=1, m_count=q_count, m_cap=rows, relu=0,
                      ln_stats=st, ln_c1=cq, chan_mask=hk3, rows_per_image=Lt if hk3 is not None else 0, rows_hint=nq)
        att = ops.packed_mha(qkv, tok_rows, prefix, B, self.heads, max_tokens,
                             head_keep=None if head_keep is None else head_keep.float().reshape(B, self.heads).contiguous())   # [capacity, dim], packed
        ops.conv_rows(att, wp, None, bp, x2d, taps=1, m_count=count, m_cap=rows, relu=0, out_rows=tok_rows, residual2d=x2d, rows_hint=na)
        st = ops.row_stats(x2d, self.norm2.eps, rows=m_rows, count=m_count)                     # norm2 (after the attention update)
        hid = torch.empty(rows, w1.shape[0], device=x2d.device, dtype=torch.float32)
        ops.conv_rows(x2d, w1, None, b1, hid, a_rows=m_rows, taps=1, m_count=m_count, m_cap=rows, relu=3, ln_stats=st, ln_c1=c1, rows_hint=nm)   # norm2 + fc1 + GELU
        ops.conv_rows(hid, w2, None, b2, x2d, taps=1, m_count=m_count, m_cap=rows, relu=0, out_rows=m_rows, residual2d=x2d, rows_hint=nm)
        return x2d

    @staticmethod
    def skip_lists(keep, attn_keep=None, mlp_keep=None):
        """Token lists of a block under token + layer skipping: keep [B, L] {0,1}; attn_keep / mlp_keep [B] {0,1} (None = run).
        -> (attention list (rows, prefix, count), MLP list or None, q/k/v rows (rows, count) or None)."""
        B, Lt = keep.shape
        ka = keep if attn_keep is None else keep * attn_keep.view(B, 1).to(keep.dtype)
        a_list = ops.token_lists(ka.contiguous())
        # the MLP sub-block has its OWN list whenever either decision is given: with attn_keep alone the attention list above has lost the
        # images whose attention is skipped, but their MLP still runs (mlp_keep None = run: the MLP list is then the plain token list)
        if mlp_keep is not None:
            m_list = ops.token_lists((keep * mlp_keep.view(B, 1).to(keep.dtype)).contiguous())
        else:
            m_list = None if attn_keep is None else ops.token_lists(keep.contiguous())
        q_rows = None
        if attn_keep is not None:
            r, _, c = ops.token_lists(attn_keep.view(B, 1).to(keep.dtype).expand(B, Lt).contiguous())
            q_rows = (r, c)
        return a_list, m_list, q_rows

    def forward(self, x, keep, head_keep=None, attn_keep=None, mlp_keep=None):
        """x [B, L, dim], keep [B, L] {0,1} -> new [B, L, dim] (kept tokens updated, the others passed through).  head_keep [B, heads],
        attn_keep / mlp_keep [B]: head and layer skipping (see run_packed).  Any L: ldn_packed_mha tiles sequences beyond 256 tokens."""
        B, Lt, D = x.shape
        x2d = x.reshape(B * Lt, D).clone()
        (tok_rows, prefix, count), m_list, q_rows = self.skip_lists(keep, attn_keep, mlp_keep)
        self.run_packed(x2d, tok_rows, prefix, count, B, Lt, head_keep=head_keep, mlp_lists=m_list, qkv_rows=q_rows)
        return x2d.view(B, Lt, D)


class TokenSkipViT(nn.Module):
    """A trunk of token-skipping blocks (DeiT-S: depth 12, dim 384, 6 heads, MLP x4; 197 tokens at 224 px, 577 at 384 px -- the
    sequence length is free).  forward(x, keeps): keeps[i] is the [B, L] keep mask of block i (the CLS token must be kept).  The residual stream is one [B*L, dim] buffer updated in place."""

    def __init__(self, depth=12, dim=384, heads=6, mlp_ratio=4.0):
        super().__init__()
        self.blocks = nn.ModuleList(TokenSkipBlock(dim, heads, mlp_ratio) for _ in range(depth))

    @staticmethod
    def blocks_qkv_kept_only():
        """Do the blocks compute q / k / v for the attending tokens only (the class-level switch of TokenSkipBlock)?"""
        return bool(TokenSkipBlock.qkv_kept_only)

    def forward(self, x, keeps, head_keeps=None, attn_keeps=None, mlp_keeps=None):
        """keeps[i] [B, L]; optional per-block head_keeps[i] [B, heads], attn_keeps[i] / mlp_keeps[i] [B] (head / layer skipping)."""
        B, Lt, D = x.shape
        x2d = x.reshape(B * Lt, D).clone()
        pick = lambda seq, i: None if seq is None else seq[i]
        for i, (blk, keep) in enumerate(zip(self.blocks, keeps)):
            (tok_rows, prefix, count), m_list, q_rows = blk.skip_lists(keep, pick(attn_keeps, i), pick(mlp_keeps, i))
            blk.run_packed(x2d, tok_rows, prefix, count, B, Lt, head_keep=pick(head_keeps, i), mlp_lists=m_list, qkv_rows=q_rows)
        return x2d.view(B, Lt, D)


# ------------------------------------------------------------------------------------------------------------------ training
BWD_MAX_TOKENS = 256      # kept tokens per image ldn_packed_mha_bwd (the one-launch kernel) takes
# sequences beyond BWD_MAX_TOKENS on ldn_packed_mha_bwd_long (LDN_MHA_BWD_LONG=1).  Off by default: block_train refuses them as before; up to
# BWD_MAX_TOKENS the one-launch kernel runs either way (the dispatch is by L, the floats do not change)
USE_LONG_BWD = os.environ.get("LDN_MHA_BWD_LONG", "0") == "1"


def _wgrad_T(dy, a2d, a_rows, count, cap, valid):
    """sum_{r < count} dy[r, n] * a2d[src(r), k] -> [n, k] (src = a_rows[r], or r): ldn_wgrad_rows, or the gather + GEMM path for shapes outside its
    predicate and with training.USE_WGRAD_KERNEL off.  dy [cap, n] packed; rows past the device-side count may hold recycled memory: the
    kernel does not read them, the GEMM path selects them away (valid [cap, 1] bool)."""
    n, k = dy.shape[1], a2d.shape[1]
    if _tr.USE_WGRAD_KERNEL and ops.wgrad_rows_ok(k, n, 1):
        return ops.wgrad_rows(dy, a2d, a_rows=a_rows, taps=1, m_count=count, m_cap=cap).view(n, k)
    zero = dy.new_zeros(1)
    if a_rows is not None:
        src = torch.where(valid.view(-1), a_rows[:cap].long(), torch.zeros_like(a_rows[:cap], dtype=torch.long)).clamp(0, a2d.shape[0] - 1)
        a2d = a2d[src]
    return torch.where(valid, dy[:cap], zero).t() @ torch.where(valid, a2d[:cap], zero)


def _linear_T(dy, lin_weight, out_cols, *, a_rows=None, count, cap):
    """The transposed linear on listed rows: out[r] = dy[src(r)] . W for r < count (W = the nn.Linear weight [cols of dy, out_cols]), packed."""
    out = torch.empty(cap, out_cols, device=dy.device, dtype=torch.float32)
    wT = lin_weight.t().reshape(out_cols, 1, lin_weight.shape[0]).contiguous()
    ops.conv_rows(dy, wT, None, torch.zeros(out_cols, device=dy.device), out, a_rows=a_rows, taps=1, m_count=count, m_cap=cap, relu=0)
    return out


class _TokenSkipBlockFn(torch.autograd.Function):
    """One token-skipping block on packed lists (TokenSkipBlock.run_packed with the sub-blocks' inputs kept): differentiable in x and the
    block's twelve parameter tensors.  lists = TokenSkipBlock.skip_lists(...); ka / km [B * L, 1] bool = the rows of the two lists."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qw, qb, pw, pb, n2w, n2b, f1w, f1b, f2w, f2b, block, lists, head_keep, ka, km):
        B, Lt, D = x.shape
        dev, rows = x.device, B * Lt
        (wq, bq, cq), (wp, bp), (w1, b1, c1), (w2, b2) = block._weights(dev)
        (a_rows, prefix, a_count), m_list, _ = lists
        m_rows, _, m_count = m_list if m_list is not None else (a_rows, prefix, a_count)
        x0 = x.detach().reshape(rows, D).float().contiguous()
        hk = hk3 = None
        if head_keep is not None:
            hk = head_keep.detach().float().reshape(B, block.heads).contiguous()
            hk3 = hk.repeat_interleave(D // block.heads, dim=1).repeat(1, 3).contiguous()
        st1 = ops.row_stats(x0, block.norm1.eps, rows=a_rows, count=a_count)
        qkv = torch.empty(rows, 3 * D, device=dev, dtype=torch.float32)
        ops.conv_rows(x0, wq, None, bq, qkv, a_rows=a_rows, out_rows=a_rows, taps=1, m_count=a_count, m_cap=rows, relu=0, ln_stats=st1, ln_c1=cq,
                      chan_mask=hk3, rows_per_image=Lt if hk3 is not None else 0)
        att = ops.packed_mha(qkv, a_rows, prefix, B, block.heads, Lt, head_keep=hk)                      # [capacity, dim], packed
        x1 = x0.clone()                                            # the MLP sub-block's input: x0 stays what norm1's backward reads
        ops.conv_rows(att, wp, None, bp, x1, taps=1, m_count=a_count, m_cap=rows, relu=0, out_rows=a_rows, residual2d=x0)
        st2 = ops.row_stats(x1, block.norm2.eps, rows=m_rows, count=m_count)
        pre = torch.empty(rows, w1.shape[0], device=dev, dtype=torch.float32)                       # fc1 WITHOUT the GELU epilogue: the backward needs z
        ops.conv_rows(x1, w1, None, b1, pre, a_rows=m_rows, taps=1, m_count=m_count, m_cap=rows, relu=0, ln_stats=st2, ln_c1=c1)
        hid = F.gelu(pre)                                          # rows past the count hold recycled memory on both sides; fc2 does not read them
        x2 = x1.clone()
        ops.conv_rows(hid, w2, None, b2, x2, taps=1, m_count=m_count, m_cap=rows, relu=0, out_rows=m_rows, residual2d=x1)
        f32 = lambda t: t.detach().float().contiguous()
        ctx.save_for_backward(x0, x1, st1, st2, qkv, att, pre, a_rows, prefix, a_count, m_rows, m_count, ka, km,
                              f32(n1w), f32(n1b), f32(qw), f32(pw), f32(n2w), f32(n2b), f32(f1w), f32(f2w))
        ctx.hk, ctx.geom, ctx.heads = hk, (B, Lt, D), block.heads
        ctx.math_mode = ops.get_math_mode()
        return x2.view(B, Lt, D)

    @staticmethod
    @_tr._in_forward_mode
    def backward(ctx, g):
        (x0, x1, st1, st2, qkv, att, pre, a_rows, prefix, a_count, m_rows, m_count, ka, km,
         n1w, n1b, qw, pw, n2w, n2b, f1w, f2w) = ctx.saved_tensors
        B, Lt, D = ctx.geom
        dev, rows, H = g.device, B * Lt, f1w.shape[0]
        zero = torch.zeros(1, device=dev)
        ar = torch.arange(rows, device=dev).unsqueeze(1)
        va, vm = ar < a_count, ar < m_count                        # [rows, 1] bool: the packed rows in front of each device-side count
        gx = g.detach().reshape(rows, D).float().clone()           # d L / d (residual stream), walked backwards in place: dropped tokens keep g

        # ---- MLP sub-block: x2 = x1 + fc2(gelu(fc1(norm2(x1)))) on the rows of the MLP list
        g_f2b = torch.where(km, gx, zero).sum(0)
        g_f2w = _wgrad_T(F.gelu(pre), gx, m_rows, m_count, rows, vm).t()                                    # [dim, hidden]
        dhid = _linear_T(gx, f2w, H, a_rows=m_rows, count=m_count, cap=rows)                       # [capacity, hidden], packed
        z = pre
        dgelu = 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327
        dpre = torch.where(vm, dhid * dgelu, zero)                 # select, do not multiply: rows past the count are recycled memory
        g_f1b = dpre.sum(0)
        dyln = _linear_T(dpre, f1w, D, count=m_count, cap=rows)                                     # d L / d norm2(x1), packed
        g_n2w, g_n2b, xh = ops.rows_ln_bwd(x1, st2, n2w, dyln, gx, rows=m_rows, count=m_count, m_cap=rows, want_xhat=True)   # gx += : now d L / d x1
        g_f1w = _wgrad_T(dpre, xh, None, m_count, rows, vm) * n2w.view(1, -1) + g_f1b.view(-1, 1) * n2b.view(1, -1)

        # ---- attention sub-block: x1 = x0 + proj(mha(qkv(norm1(x0)))) on the rows of the attention list
        g_pb = torch.where(ka, gx, zero).sum(0)
        g_pw = _wgrad_T(att, gx, a_rows, a_count, rows, va).t()
        datt = _linear_T(gx, pw, D, a_rows=a_rows, count=a_count, cap=rows)                        # packed
        mha_bwd = ops.packed_mha_bwd if Lt <= BWD_MAX_TOKENS else ops.packed_mha_bwd_long      # block_train let Lt > 256 in with USE_LONG_BWD only
        dqkv = mha_bwd(qkv, a_rows, prefix, B, ctx.heads, Lt, datt, head_keep=ctx.hk)              # dense rows, zeros off the list
        g_qb = dqkv.sum(0)
        dyln = _linear_T(dqkv, qw, D, a_rows=a_rows, count=a_count, cap=rows)                      # d L / d norm1(x0), packed
        g_n1w, g_n1b, xh = ops.rows_ln_bwd(x0, st1, n1w, dyln, gx, rows=a_rows, count=a_count, m_cap=rows, want_xhat=True)   # gx += : now d L / d x0
        g_qw = _wgrad_T(xh, dqkv, a_rows, a_count, rows, va).t() * n1w.view(1, -1) + g_qb.view(-1, 1) * n1b.view(1, -1)
        return (gx.view(B, Lt, D), g_n1w, g_n1b, g_qw, g_qb, g_pw, g_pb, g_n2w, g_n2b, g_f1w, g_f1b, g_f2w, g_f2b, None, None, None, None, None)


def block_train(block, x, keep, head_keep=None, attn_keep=None, mlp_keep=None):
    """A TokenSkipBlock's forward with a backward: x [B, L, dim], keep [B, L] {0,1} (head_keep [B, heads], attn_keep / mlp_keep [B] as in
    TokenSkipBlock.forward) -> [B, L, dim], differentiable in x and the block's twelve parameter tensors.  The masks are inputs, not
    variables: their straight-through gradients need the sub-blocks' outputs at dropped tokens and heads -- a dense execution."""
    if not isinstance(block, TokenSkipBlock):
        raise LdnError("block_train: expected a TokenSkipBlock")
    if ops.get_math_mode() != "bf16x3":
        raise LdnError("TokenSkipBlock runs in the bf16x3 arithmetic mode (ops.set_math_mode('bf16x3'))")
    for name, m in (("keep", keep), ("head_keep", head_keep), ("attn_keep", attn_keep), ("mlp_keep", mlp_keep)):
        if m is not None and m.requires_grad:
            raise LdnError(f"block_train: the gradient of {name} (a straight-through term of a dense execution) is not built")
    if not block.qkv_kept_only:
        raise LdnError("block_train: q / k / v of unattending tokens (qkv_kept_only = False) are not built for training")
    if x.dim() != 3 or x.shape[2] != block.dim or tuple(keep.shape) != tuple(x.shape[:2]):
        raise LdnError(f"block_train: x must be [B, L, {block.dim}] and keep [B, L], got {tuple(x.shape)} and {tuple(keep.shape)}")
    B, Lt, _ = x.shape
    if Lt > BWD_MAX_TOKENS and not USE_LONG_BWD:
        raise LdnError(f"block_train: the attention backward for more than {BWD_MAX_TOKENS} kept tokens per image is not built (L = {Lt}) unless "
                       "adavit.USE_LONG_BWD is on (env LDN_MHA_BWD_LONG=1)")
    keep = keep.detach()
    lists = block.skip_lists(keep, attn_keep, mlp_keep)
    row_mask = lambda k: (k.reshape(B * Lt, 1) > 0.5)
    ka = row_mask(keep if attn_keep is None else keep * attn_keep.detach().view(B, 1).to(keep.dtype))
    km = row_mask(keep if mlp_keep is None else keep * mlp_keep.detach().view(B, 1).to(keep.dtype))
    return _TokenSkipBlockFn.apply(x, block.norm1.weight, block.norm1.bias, block.qkv.weight, block.qkv.bias, block.proj.weight, block.proj.bias,
                                   block.norm2.weight, block.norm2.bias, block.fc1.weight, block.fc1.bias, block.fc2.weight, block.fc2.bias,
                                   block, lists, head_keep, ka, km)


def train_forward(trunk, x, keeps, head_keeps=None, attn_keeps=None, mlp_keeps=None):
    """TokenSkipViT.forward with a backward: block_train over the trunk's blocks (keeps[i] [B, L]; optional per-block head_keeps[i],
    attn_keeps[i], mlp_keeps[i])."""
    if not isinstance(trunk, TokenSkipViT):
        raise LdnError("train_forward: expected a TokenSkipViT")
    pick = lambda seq, i: None if seq is None else seq[i]
    for i, (blk, keep) in enumerate(zip(trunk.blocks, keeps)):
        x = block_train(blk, x, keep, pick(head_keeps, i), pick(attn_keeps, i), pick(mlp_keeps, i))
    return x
