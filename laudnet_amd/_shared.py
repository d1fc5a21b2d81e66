"""Host-side plumbing shared by laud_resnet, laud_regnet and training: the channel algebra, the dense channel execution, the cached
index lists of all-active batches and of strided shortcuts, the row-count hint and the shape-only constants of the FLOPs bookkeeping.
Private to the package; nothing here is a kernel."""
from __future__ import annotations

import torch

from . import ops


# ------------------------------------------------------------------------------------------------------------------ channel algebra
def channel_constants(w2, w3, s2, t2, t1, s3, t3):
    """The constants of the channel algebra -> (c1, c2, t2_tab, t3c).  A masked channel k of conv1's output is the
    CONSTANT c1[k] = relu(t1[k]) (mask applied before BN, laud_resnet.py:116-118).  Writing h1 = u1 + c1 with u1 = 0 on masked channels
    makes conv2 = W2[A,A] (*) u1 + (W2 (*) c1), whose second term does not depend on the image: t2_tab [16, W] = t2 + s2 * (W2 (*) c1)
    for the 16 border classes cls = 4 * rb + cb (rb bit 0: top row, bit 1: bottom row; cb likewise for the columns -- the taps that
    fall into the padding drop out).  Likewise c2 = relu(t2) and t3c = t3 + s3 * (W3 c2).  w2 [W, W, 3, 3], w3 [cout, W(, 1, 1)]."""
    W = w2.shape[0]
    c1, c2 = torch.relu(t1), torch.relu(t2)
    wc = torch.einsum("okyx,k->oyx", w2, c1)  # [W,3,3]
    tab = torch.empty(16, W, device=wc.device)
    for cls in range(16):
        rb, cb = cls // 4, cls % 4
        ys = [ky for ky in range(3) if not ((ky == 0 and rb & 1) or (ky == 2 and rb & 2))]
        xs = [kx for kx in range(3) if not ((kx == 0 and cb & 1) or (kx == 2 and cb & 2))]
        tab[cls] = t2 + s2 * wc[:, ys][:, :, xs].sum(dim=(1, 2))
    t3c = t3 + s3 * (w3.reshape(w3.shape[0], W) @ c2)
    return c1.contiguous(), c2.contiguous(), tab.contiguous(), t3c.contiguous()


def dense_channel_convs(x2d, B, geom, w1r, w2r, s1, t1, c1, s2, t2_tab, c2, chm2d, ix):
    """conv1 and the 3x3 of channel mode without gathers -> (h1, h2): shared n-major weights over row tiles that span images, the
    outputs u = relu(bn(.)) - c zeroed on the masked channels of each image (chm2d [B, W] {0,1}) -- exactly what the gathered form
    stores / skips.  geom = (Hi, Wi, Ho, Wo, stride); ix = dense_index of the output map."""
    Hi, Wi, Ho, Wo, _ = geom
    W, Cin = w1r.shape[0], x2d.shape[1]
    dev = x2d.device
    fused_mask = ops.dense_kernel_ok() and Cin % 32 == 0 and W % 32 == 0
    h1 = torch.empty(ix.cap1, W, device=dev, dtype=torch.float32)
    if fused_mask:   # k_dense: the per-image channel mask and the post-ReLU constant are epilogue terms (no pass over h1)
        ops.conv_rows(x2d, w1r, s1, t1, h1, taps=1, m_cap=ix.cap1, relu=1, post_sub=c1, chan_mask=chm2d, rows_per_image=Hi * Wi)
    else:
        ops.conv_packed(x2d, w1r, s1, t1, h1, taps=1, m_cap=ix.cap1, post_sub=c1, relu=1)
        h1.view(B, -1, W).mul_(chm2d.view(B, 1, W))
    h2 = torch.empty(ix.cap3, W, device=dev, dtype=torch.float32)
    if fused_mask and 9 in ops.DENSE_TAPS and ops.DENSE_CHANNEL_3X3:
        ops.conv_rows(h1, w2r, s2, t2_tab, h2, a_rows=ix.nbr, taps=9, m_cap=ix.cap3, pix_map=ix.idx3, geom=geom, post_sub=c2, relu=1,
                      chan_mask=chm2d, rows_per_image=Ho * Wo)
    else:
        ops.conv_packed(h1, w2r, s2, t2_tab, h2, a_map=ix.nbr, taps=9, m_cap=ix.cap3, pix_map=ix.idx3, geom=geom, post_sub=c2, relu=1)
        h2.view(B, -1, W).mul_(chm2d.view(B, 1, W))
    return h1, h2


# ------------------------------------------------------------------------------------------------------------------ cached index lists
_INDEX_CACHE = {}   # never evicts: a captured graph (GraphedForward) replays launches that read these tensors


def dense_index(B, Ho, Wo, stride, dev):
    """Index lists of an all-active batch (every pixel of every image), cached per shape: the packed-row machinery then is a dense
    convolution whose M tiles span images."""
    key = ("dense", B, Ho, Wo, stride, str(dev))
    if key not in _INDEX_CACHE:
        _INDEX_CACHE[key] = ops.mask_to_index(torch.ones(B, 1, 1, device=dev), Ho, Wo, stride)
    return _INDEX_CACHE[key]


def image_prefix(B, rows, dev):
    """row_prefix [B + 1] int32 of B images that own `rows` consecutive packed rows each (the dense lists), cached per shape"""
    key = ("prefix", B, rows, str(dev))
    if key not in _INDEX_CACHE:
        _INDEX_CACHE[key] = (torch.arange(B + 1, device=dev, dtype=torch.int32) * rows).contiguous()
    return _INDEX_CACHE[key]


def strided_rows(B, Hi, Wi, Ho, Wo, s, dev):
    """Source row of x (as [B * Hi * Wi, C]) of every output pixel of a stride-s 1x1 convolution (projection shortcuts), cached per shape."""
    key = ("rows", B, Hi, Wi, Ho, Wo, s, str(dev))
    if key not in _INDEX_CACHE:
        b = torch.arange(B, device=dev).view(B, 1, 1)
        y = torch.arange(Ho, device=dev).view(1, Ho, 1) * s
        xx = torch.arange(Wo, device=dev).view(1, 1, Wo) * s
        _INDEX_CACHE[key] = ((b * Hi + y) * Wi + xx).reshape(-1).to(torch.int32).contiguous()
    return _INDEX_CACHE[key]


def rows_hint(owner):
    """Row counts of the previous forward of THIS module (pinned memory, no synchronisation): the tile-width hint of the row kernels."""
    hint = getattr(owner, "_rows_hint", None)
    if hint is None:
        hint = owner._rows_hint = ops.RowsHint(2)
    return hint


def identity_residual(x2d, inplace):
    """(resid, out2d) of a block without a projection shortcut: x >= 0 (post-ReLU) inside the network, so the pixels the branch does not
    touch pass through -- in place where the caller owns x, else into a copy (relu(x) == x)."""
    return (x2d, x2d) if inplace else (x2d, torch.relu(x2d))


# ------------------------------------------------------------------------------------------------------------------ FLOPs bookkeeping
def flops_constants(model, x_shape, dev):
    """(terms [n_blocks, 5 | 6] float64 on dev, static FLOPs) of model.flops_table, cached on the model per (device, input shape)."""
    key = (str(dev), tuple(x_shape[1:]))
    if getattr(model, "_terms_key", None) != key:
        terms, static = model.flops_table(x_shape)
        model._terms_key = key
        model._terms = torch.tensor(terms, dtype=torch.float64, device=dev)
        model._static_flops = float(static)
    return model._terms, model._static_flops


def sparse_flops(model, x_shape, s3, s2, s1, cs):
    """-> (terms, static FLOPs, sparse [n_blocks] float64): the FLOPs every block spends at these sparsities (flat [n_blocks] tensors or
    per-stage lists), laud_resnet.py:112-147 over the first five columns of the terms."""
    flat = lambda v: torch.cat([t.reshape(-1) for t in v]) if isinstance(v, (list, tuple)) else v
    s3, s2, s1, cs = (flat(v).double() for v in (s3, s2, s1, cs))   # fp64 inside: the result does not depend on summation order
    tm, static = flops_constants(model, x_shape, s3.device)
    sparse = tm[:, 0] + tm[:, 1] * cs * s1
    sparse = sparse + tm[:, 2] * cs ** 2 * s2
    sparse = sparse + tm[:, 3] * cs * s3
    sparse = sparse + tm[:, 4]
    return tm, static, sparse


def denoms(model, values, dev):
    """[n] float32 on dev of the channel-mode blocks' B * width, cached on the model."""
    key = (str(dev), tuple(values))
    if getattr(model, "_denoms_key", None) != key:
        model._denoms_key = key
        model._denoms = torch.tensor(key[1], dtype=torch.float32, device=dev)
    return model._denoms
