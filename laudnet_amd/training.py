"""Training under FROZEN BatchNorm on the library's row kernels -- and, behind USE_BATCH_STATS, on batch
statistics.

The reference's ImageNet recipe is dense by construction (BatchNorm in batch-statistics mode, `models/laud_resnet.py:115-133`): nothing
to accelerate (it trains, dense, behind USE_BATCH_STATS: further down).  Its DETECTION fine-tuning freezes the BatchNorm STATISTICS (`norm_eval=True`, `mmdetection-2.21.0/mmdet/models/backbones/
lad_mmdet_resnet.py:753-758`) while the affine parameters keep training (`norm_cfg=dict(type='BN', requires_grad=True)`); the configs it
ships are channel-2222 and layer (`configs/retinanet/scale_backbone_lr/retinanet_ladmmdet_r101_fpn_1x_coco_r101_channel_2222_0x6_lrmult0x2.py:8-17`,
`..._layer_0x5_lrmult0x2.py:8-17`).  Under frozen statistics a block is

    out = relu(identity(x) + m3 * bn3(conv3(relu(bn2(c . conv2(relu(bn1(c . conv1(x)))))))))        (laud_resnet.py:104-147)

with a {0,1} pixel mask m3 (spatial / layer modes) or a {0,1} channel mask c applied BEFORE bn1 / bn2 (channel mode), both sampled with
F.gumbel_softmax(hard=True) in training (`models/utils.py:56-58,124,162`).  This module runs the three convolutions -- forward AND backward --
on the library's kernels:

  pixel masks (spatial, layer; any stride, with or without a projection shortcut): the packed rows of the kept pixels
      forward   x --conv1 (rows of the dilated list)--> h1 --3x3 through the neighbour table--> h2 --conv3, scattered--> branch
      backward  the same kernels with gather and scatter swapped and transposed weights; the 3x3 goes through the TRANSPOSED neighbour
                table (for every h1 row and tap the packed output row whose window reads it; stride-aware).  A skipped image / dropped
                pixel costs nothing in either direction.
  channel masks (any stride): the row kernels over ALL pixels with the channel mask and the constants of the channel algebra as epilogue
      terms (a masked channel is the constant relu(shift); the library's "dense channel execution").  Correct for every
      gradient, but dense in the channels: the masks save no FLOPs here (stated, not hidden).
  pixel x channel masks (dyn_mode 'both', the reference's constructor default; any stride): the pixel mask's packed rows with the channel
      algebra on them -- dense in the channels on those rows: `ops.rows_chanmask` zeroes the masked channels of every packed row (the image
      of a row comes from the lists' per-image prefix, on the device), and the backward's elementwise chain with ALL its reductions (ReLU
      gate, channel mask, d scale / d shift, the per-image sums of the channel mask's straight-through term) is `ops.rows_act_bwd`: two
      launches per layer, no floating-point atomics.  The pixel mask saves its FLOPs in both directions, the channel mask none.
  Weight gradients are the library's own kernel (`ops.wgrad_rows`: dW = sum over the packed rows of dY x A, the nine taps' rows gathered through
  the neighbour table inside the kernel, rows past the device-side count never read, deterministic) wherever `ops.wgrad_rows_ok` holds and
  `USE_WGRAD_KERNEL` is on (the default; env LDN_WGRAD=0 turns it off); otherwise the gather + GEMM path.  BatchNorm's affine gradients come
  out of the folded (scale, shift) pairs, which stay differentiable functions of (weight, bias); the straight-through terms of the hard masks
  need the branch at DROPPED units too -- the library's own dense execution (that term is dense in the reference as well).  The residual add,
  the final ReLU, the projection shortcut, the maskers' tiny heads, the static stem and the classifier are plain autograd ops.

One `autograd.Function` per mask kind; what they share (operand layouts, transposed convolutions, weight / BatchNorm / pixel-mask gradients,
the split of dz^T A into a weight gradient and a BatchNorm scale gradient: `_split_scale` -- no gradient is obtained by dividing by a folded
scale, which may be zero, tiny or negative) is written once above them.  The index lists are built once per block forward (`_branch`) and handed to the Fn.

Entry points: `sparse_block_train(block, x, mask)` (one block, the mask an input), `block_train(block, state, temperature)` (the reference's
block signature in training mode: samples its own masks), `train_forward(model, x, temperature)` (a whole LAUD-ResNet -> the reference's
7-tuple; a `LAD_MMDet_ResNet` -> its (outs, additional, model_configs)), `prepare_for_training(model)` (train mode with BatchNorm statistics
frozen; batch_stats=True: on batch statistics).  Checked against the oracle's autograd -- blocks on the reference-generated block fixtures, whole models on `det_tiny.pt` /
`full_tiny.pt` with identical Gumbel noise (tests/test_hip_training.py, tests/test_hip_training_both.py, plain 1e-3; bf16x3 with a flip
allowance) -- and, element by element to 1e-3 of each gradient's own maximum in both arithmetic modes, against a float64 restatement on inputs
where no ReLU can flip (tests/test_hip_training_f64.py, tests/train_ref.py), the same with zero, +-2^-24 and negative BatchNorm weights
(tests/test_hip_training_bn_scales.py; zero_init_residual's bn3.weight == 0 on a whole detection backbone in tests/test_hip_training.py).

LAD-RegNet (`laud_regnet.ResBottleneckBlock`) trains in its LAYER-SKIP form -- dyn_mode 'spatial' with one keep / skip bit per image, SE present, stride
1 and 2, with and without `proj`: a kept image runs a -> grouped b -> SE -> c on packed rows in both directions (`_RegNetSkipBranchFn`: the grouped
3x3's adjoint is its forward kernel over the transposed neighbour table with per-group transposed weights, its weight gradient `ops.wgrad_grouped_rows`
at group widths 8 / 16 / 24 -- at widths 56 / 112 / 232 `ops.wgrad_grouped_wide_rows` behind USE_WGRAD_GROUPED_WIDE (env LDN_WGRAD_GROUPED_WIDE=1; default OFF:
the gather + bmm path, as before that kernel existed; LDN_WGRAD=0 forces that path everywhere; one chooser, `_weight_grad_conv_b`, for all three
LAD-RegNet branch Fns; tests/test_hip_training_wgrad_grouped_wide.py) --
the squeeze / excite and their backward tensor ops on the [slots, Ho Wo, C] view of the rows); the same three entry points take it and a whole
`LAD_RegNet` (tests/test_hip_training_regnet.py).

LAD-RegNet dyn_mode 'channel' -- the one LAD-RegNet recipe the reference trains (train_scripts.sh:29-40) -- trains behind USE_REGNET_CHANNEL (env
LDN_TRAIN_REGNET_CHANNEL=1; default OFF: with it off a channel block is refused as before).  The mask multiplies the outputs of a and b AFTER
conv + BN + ReLU (laud_regnet.py:182-189), so none of the LAUD-ResNet channel algebra applies: `_RegNetChannelBranchFn` runs the row kernels over all
pixels, DENSE in the channels -- the mask saves no FLOPs in training, for the same reason as above: the straight-through term sum_p d h . relu(zy) needs
relu(zy) and the upstream gradient at the masked channels too -- and its backward's elementwise chain with all its reductions is `ops.rows_postmask_bwd`
(SE prologue, mask, ReLU gate, scale; d shift, d scale, d mask: two launches per layer, deterministic) plus `ops.rows_img_dot` (the SE's d gate)
(tests/test_hip_rows_postmask.py, tests/test_regnet_channel_ref.py, tests/test_hip_training_regnet_channel.py).

BatchNorm on BATCH statistics -- what all three commands of the reference's train_scripts.sh and train/main.py:527-604 train with: plain
model.train() -- trains for LAUD-ResNet blocks behind USE_BATCH_STATS (env LDN_TRAIN_BATCH_STATS=1; default OFF: with it off a block whose
BatchNorm is in training mode is refused as before).  `_BatchStatsBranchFn` serves all four dyn_modes (optional channel mask, optional pixel mask):
    u1 = c . conv1(x)   h1 = relu(BN(u1))     u2 = c . conv2(h1)   h2 = relu(BN(u2))     u3 = conv3(h2)   branch = m3 * BN(u3)
over ALL pixels at any stride.  bn1 / bn2 / bn3 see every pixel and every channel, dropped or not, so this mode is dense by construction: THE
MASKS SAVE NO FLOPs IN IT (stated, not hidden).  The convolutions, their adjoints and weight gradients are the kernels above with scale 1 / shift 0
/ no ReLU (nothing is folded: no _split_scale, bn.weight == 0 is no special case); BatchNorm's forward and its backward through the statistics are
`ops.rows_bn_stats` / `ops.rows_bn_fwd` / `ops.rows_bn_bwd` (csrc/ldn_train_bn.hip: Welford + Chan's merge, never E[u^2] - E[u]^2; the channel
mask in front of the statistics, the pixel mask as a row factor; d gamma, d beta, d u and the channel mask's straight-through sum in three / four
launches per layer; deterministic).  The running statistics are updated once per forward, under no_grad, never in the backward (momentum, the
unbiased variance, num_batches_tracked; momentum=None = the cumulative average).  The stem's, the projection's and the conv_linear masker's
BatchNorms are plain modules.  `prepare_for_training(model, batch_stats=True)` leaves BatchNorm in training mode; block_train and
train_forward(ResNet) are unchanged (tests/test_bn_batch_ref.py, tests/test_hip_rows_bn.py, tests/test_hip_training_batchstats.py).

LAD-RegNet dyn_mode 'channel' on batch statistics -- train_scripts.sh's third command -- trains with BOTH switches on (USE_REGNET_CHANNEL and
USE_BATCH_STATS): a channel block whose BatchNorms (a, b, c and proj's) are all in training mode runs `_RegNetBatchStatsBranchFn`:
    y_a = a(x)   h_a = m . relu(BN(y_a))     y_b = b(h_a)   h_b = m . relu(BN(y_b))     y_c = c(gate . h_b)   branch = BN(y_c)
The mask multiplies AFTER BatchNorm + ReLU, so the statistics see every channel of every image (`ops.rows_bn_stats` without a mask) and THE MASK
SAVES NO FLOPs.  Layers a / b are `ops.rows_bn_postmask_fwd` forward and `ops.rows_bn_postmask_bwd` backward (csrc/ldn_train_bn.hip: SE prologue,
mask, ReLU gate read from the stored masked h, d gamma, d beta, the statistics' terms and the mask's straight-through sum over the RECOMPUTED
unmasked ReLU output, three launches, deterministic); a layer saves the unmasked y and the masked h, one matrix fewer than the frozen path that
keeps relu(zy) for the mask.  Layer c is `ops.rows_bn_fwd` / `ops.rows_bn_bwd` without ReLU; nothing is folded.  The running statistics move once
per forward (`_branch_regnet`); proj, the stem and the maskers stay plain modules.  block_train, train_forward(LAD_RegNet) and
prepare_for_training(model, batch_stats=True) take it unchanged (tests/test_regnet_bn_ref.py, tests/test_hip_rows_bn_postmask.py,
tests/test_hip_training_regnet_batchstats.py).

Not built: mask groups > 1, dilated conv2, grouped conv2 outside the LAD-RegNet blocks, BatchNorm on batch statistics for LAD-RegNet layer skip
and the detection backbone, SyncBatchNorm / cross-rank statistics, a block with some BatchNorms frozen and some not, LAD-RegNet 'both' /
patch-mask (mask_size > 1) training."""
from __future__ import annotations

import functools
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import ops
from ._lib import LdnError
from ._shared import channel_constants, dense_channel_convs, dense_index, image_prefix
from .laud_regnet import LAD_RegNet, ResBottleneckBlock, _conv_b_frag, _conv_b_rows, _conv_b_run, conv_b_choice

# weight gradients on ldn_wgrad_rows / ldn_wgrad_grouped_rows; LDN_WGRAD=0 = the gather + PyTorch GEMM / bmm path.  On by default: the median step is shorter with the kernel for
# all three full-width workloads at batch 32 and 128 (profiles/train_step_wgrad.jsonl), and for LAD-RegNetY-800MF layer skip with the grouped
# kernel (profiles/train_step_regnet.jsonl)
USE_WGRAD_KERNEL = os.environ.get("LDN_WGRAD", "1") != "0"

# conv b's weight gradient at group widths 56 / 112 / 232 (lad_regnet_y_8gf / 16gf / 32gf) on ldn_wgrad_grouped_wide_rows (the matrix cores); env
# LDN_WGRAD_GROUPED_WIDE=1 turns it on, under USE_WGRAD_KERNEL.  Off by default: with it off every dispatch is what it was before the kernel
# existed (the gather + bmm path at these widths).  Independent of laud_regnet.USE_GROUPED_MFMA_WIDE_ROWS (the forward's and the adjoint's switch)
USE_WGRAD_GROUPED_WIDE = os.environ.get("LDN_WGRAD_GROUPED_WIDE", "0") == "1"

# LAD-RegNet channel-mode training (_RegNetChannelBranchFn); env LDN_TRAIN_REGNET_CHANNEL=1 turns it on.  Off by default: with it off every
# LAD-RegNet form but layer skip is refused, as before the path existed
USE_REGNET_CHANNEL = os.environ.get("LDN_TRAIN_REGNET_CHANNEL", "0") == "1"


# BatchNorm on BATCH statistics in LAUD-ResNet blocks (_BatchStatsBranchFn on ops.rows_bn_*): the reference's own ImageNet recipe; env
# LDN_TRAIN_BATCH_STATS=1 turns it on.  Off by default: with it off a block whose BatchNorm is in training mode is refused, as before the path existed
USE_BATCH_STATS = os.environ.get("LDN_TRAIN_BATCH_STATS", "0") == "1"


# ------------------------------------------------------------------------------------------------------------------ index helpers
def transposed_neighbour_table(ix, B, H, W, stride=1, Ho=None, Wo=None):
    """nbrT [cap1, 9]: for every packed h1 row r (an INPUT pixel (iy, ix) of the dilated list) and tap t = (dy, dx), the packed OUTPUT row whose
    3x3 window reads r through tap t: output pixel (oy, ox) with stride * oy + dy - 1 == iy (likewise x), -1 if there is none / it is not active.
    The adjoint of ix.nbr: d h1[r] = sum_t d u2[nbrT[r, t]] . W2[:, t, :].  H, W = the input map; Ho, Wo = the output map (stride 1: the same)."""
    Ho = H if Ho is None else Ho
    Wo = W if Wo is None else Wo
    dev = ix.idx1.device
    cap1 = ix.cap1
    pix = ix.idx1.long().clamp(min=0)                       # flat input pixel b * H * W + iy * W + ix of every list entry (garbage past the count)
    b = pix // (H * W)
    rem = pix - b * (H * W)
    iy, ixx = rem // W, rem - (rem // W) * W
    pos3 = ix.pos3.view(-1).long()
    taps = torch.arange(9, device=dev)
    dy, dx = taps // 3 - 1, taps % 3 - 1                     # all nine taps at once: [cap1, 9] tensors, a dozen launches instead of a hundred
    ny, nx = iy[:, None] - dy[None, :], ixx[:, None] - dx[None, :]      # = stride * oy, stride * ox
    oy, ox = torch.div(ny, stride, rounding_mode="floor"), torch.div(nx, stride, rounding_mode="floor")
    ok = (ny >= 0) & (nx >= 0) & (oy * stride == ny) & (ox * stride == nx) & (oy < Ho) & (ox < Wo)
    q = (b[:, None] * (Ho * Wo) + oy.clamp(0, Ho - 1) * Wo + ox.clamp(0, Wo - 1)).clamp(0, pos3.numel() - 1)
    out = torch.where(ok, pos3[q], torch.full_like(q, -1)).to(torch.int32)
    valid = torch.arange(cap1, device=dev) < ix.cnt[1]
    return torch.where(valid[:, None], out, torch.full_like(out, -1)).contiguous()


def _rows_valid(n_cap, count, dev):
    """[n_cap, 1] float mask of the rows in front of a device-side count (no host read)."""
    return (torch.arange(n_cap, device=dev) < count).to(torch.float32).unsqueeze(1)


def _weight_grad_3x3(du2, h1, nbr, cap1, count3=None):
    """d W2 [n, k, 3, 3] = sum over packed output rows of du2[row, n] * h1[nbr[row, tap], k] (a missing neighbour is a zero row).  Rows past the
    device-side count carry du2 == 0 and are pointed at the zero row (their table entries are uninitialised): no host read is needed."""
    W = du2.shape[1]
    h1z = torch.cat((h1, torch.zeros(1, h1.shape[1], device=h1.device)))
    nb = nbr.view(-1, 9)
    if count3 is not None:
        nb = torch.where((torch.arange(nb.shape[0], device=nb.device) < count3).unsqueeze(1), nb, torch.full_like(nb, -1))
    nb = torch.where(nb < cap1, nb, torch.full_like(nb, -1)).long()
    nb = torch.where(nb >= 0, nb, torch.full_like(nb, cap1))
    cols = h1z[nb.reshape(-1)].view(nb.shape[0], 9 * h1.shape[1])          # [rows, 9 K]: the nine taps' rows side by side -- ONE GEMM
    return (du2.t() @ cols).view(W, 9, h1.shape[1]).permute(0, 2, 1).reshape(W, h1.shape[1], 3, 3)


def _wgrad_kernel(cin, cout, taps):
    """Does this weight gradient run on ldn_wgrad_rows (the module switch and the kernel's shape predicate)?"""
    return USE_WGRAD_KERNEL and ops.wgrad_rows_ok(cin, cout, taps)


def _weight_grad_grouped_3x3(du2, h1, nbr, cap1, gw, count3=None):
    """d W_b [C, gw, 3, 3] of a GROUPED 3x3 (group width gw): the gather of _weight_grad_3x3 reshaped per group, then one bmm -- the path
    without ldn_wgrad_grouped_rows (LDN_WGRAD=0, or a shape outside ops.wgrad_grouped_rows_ok)."""
    C, G = du2.shape[1], du2.shape[1] // gw
    h1z = torch.cat((h1, torch.zeros(1, C, device=h1.device)))
    nb = nbr.view(-1, 9)
    if count3 is not None:
        nb = torch.where((torch.arange(nb.shape[0], device=nb.device) < count3).unsqueeze(1), nb, torch.full_like(nb, -1))
    nb = torch.where(nb < cap1, nb, torch.full_like(nb, -1)).long()
    nb = torch.where(nb >= 0, nb, torch.full_like(nb, cap1))
    R = nb.shape[0]
    cols = h1z[nb.reshape(-1)].view(R, 9, G, gw).permute(2, 0, 1, 3).reshape(G, R, 9 * gw)      # [G, rows, 9 gw]: the group's nine taps side by side
    dw = torch.bmm(du2.view(R, G, gw).permute(1, 2, 0), cols)                                   # [G, gw, 9 gw]
    return dw.view(C, 9, gw).permute(0, 2, 1).reshape(C, gw, 3, 3)


def _wgrad_grouped_kernel(C, gw):
    """Does the grouped weight gradient run on ldn_wgrad_grouped_rows (the same module switch, that kernel's shape predicate)?"""
    return USE_WGRAD_KERNEL and ops.wgrad_grouped_rows_ok(C, gw)


def _wgrad_grouped_wide_kernel(C, gw):
    """Does the grouped weight gradient run on ldn_wgrad_grouped_wide_rows (both switches -- LDN_WGRAD=0 still forces the PyTorch path
    everywhere -- and that kernel's shape predicate: group widths 56 / 112 / 232)?"""
    return USE_WGRAD_KERNEL and USE_WGRAD_GROUPED_WIDE and ops.wgrad_grouped_wide_rows_ok(C, gw)


def _weight_grad_conv_b(dy, h_a, ix, gw, m_count, count3=None):
    """d W_b [C, gw, 3, 3] of LAD-RegNet's conv b from d y_b [cap3, C] and conv b's input h_a [cap1, C]: the one place that chooses between
    ldn_wgrad_grouped_rows (widths 8 / 16 / 24), ldn_wgrad_grouped_wide_rows (widths 56 / 112 / 232, behind USE_WGRAD_GROUPED_WIDE) and the
    gather + bmm path.  m_count = the device-side row count for the kernels; count3 = the same for the fallback (None: rows past the
    count carry d y_b == 0 and valid table entries)."""
    C = dy.shape[1]
    if _wgrad_grouped_kernel(C, gw):
        op = ops.wgrad_grouped_rows
    elif _wgrad_grouped_wide_kernel(C, gw):
        op = ops.wgrad_grouped_wide_rows
    else:
        return _weight_grad_grouped_3x3(dy, h_a, ix.nbr, ix.cap1, gw, count3)
    return op(dy, h_a, ix.nbr, gw, m_count=m_count, m_cap=ix.cap3, a_valid=ix.cap1).permute(0, 2, 1).reshape(C, gw, 3, 3)


def grouped_weight_T(wbr, gw):
    """The adjoint of the grouped 3x3 is the same kernel over the transposed neighbour table with per-group transposed weights
    (ldn_grouped_conv3x3_rows' layout [C, 9, gw]: out channel, tap, in channel of the group):  wT[g gw + j, t, i] = w[g gw + i, t, j]."""
    C = wbr.shape[0]
    return wbr.view(C // gw, gw, 9, gw).permute(0, 3, 2, 1).reshape(C, 9, gw).contiguous()


# ------------------------------------------------------------------------------------------------------------------ shared by the branch Fns
_Prep = namedtuple("_Prep", "x2d w1r w2r w3r w3s bn shape")


def _in_forward_mode(backward):
    """A branch Fn's backward under the arithmetic mode its forward ran in (ctx.math_mode).  ops.set_math_mode is a PER-THREAD default and autograd
    runs the backward of a GPU graph on a thread of its own, where that default is unset: without this the whole backward -- transposed
    convolutions, weight gradients, the dense re-execution of the straight-through terms and the kernel choice of _conv_const -- ran in the
    process default (fp32) whatever mode the caller had selected."""
    @functools.wraps(backward)
    def run(ctx, *grads):
        with ops.math_mode(ctx.math_mode):
            return backward(ctx, *grads)
    return run


def _fold_w3(w3r, s3):
    """conv3's weights with bn3's scale folded in, in conv_rows' layout [cout, 1, W] (recomputed in the backward rather than saved)."""
    return (w3r * s3.view(-1, 1)).reshape(w3r.shape[0], 1, w3r.shape[1]).contiguous()


def _prep(x, w1, w2, w3, bn6, stride):
    """What every branch Fn's forward starts from, detached, fp32, in the row kernels' layouts: x2d [B Hi Wi, Cin] (NHWC rows), w1r [W, 1, Cin],
    w2r [W, 9, W] (tap-major; a grouped conv2: [W, 9, gw]), w3r [cout, W], w3s = _fold_w3, bn = (s1, t1, s2, t2, s3, t3), shape = (B, Cin, Hi, Wi, Ho, Wo, W, cout)."""
    B, Cin, Hi, Wi = x.shape
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    W, cout = w1.shape[0], w3.shape[0]
    x2d = ops.as_nhwc(x.detach()).reshape(B * Hi * Wi, Cin)
    bn = tuple(v.detach().float().contiguous() for v in bn6)
    w1r = w1.detach().reshape(W, 1, Cin).float().contiguous()
    w2r = w2.detach().float().permute(0, 2, 3, 1).reshape(W, 9, w2.shape[1]).contiguous()
    w3r = w3.detach().float().reshape(cout, W)
    return _Prep(x2d, w1r, w2r, w3r, _fold_w3(w3r, bn[4]), bn, (B, Cin, Hi, Wi, Ho, Wo, W, cout))


def _conv_const(a2d, w, scale, shift, out2d, *, a_rows, taps, m_count, m_cap, relu, post_sub=None, pix_map=None, geom=None):
    """A packed-row convolution with the epilogue terms of the channel algebra (post-ReLU constant, border-class shift table): k_dense where the
    arithmetic mode and the widths put conv_rows there, else the same terms on conv_packed (one image = the whole list).  Rows past the
    device-side count are not written."""
    cout, _, cin = w.shape
    if (ops.dense_kernel_ok() and cin % 32 == 0 and cout % 32 == 0 and taps in ops.DENSE_TAPS and (taps == 1 or ops.DENSE_CHANNEL_3X3)):
        return ops.conv_rows(a2d, w, scale, shift, out2d, a_rows=a_rows, taps=taps, m_count=m_count, m_cap=m_cap, relu=relu, post_sub=post_sub,
                             pix_map=pix_map, geom=geom)
    return ops.conv_packed(a2d, w, scale, shift, out2d, a_map=a_rows, taps=taps, m_count=m_count, m_cap=m_cap, relu=relu, post_sub=post_sub,
                           pix_map=pix_map, geom=geom)


def _conv3_T(dy, w3s, zW, m_count, m_cap, alloc):
    """conv3^T: d L / d h2 [m_cap, W] from d L / d (s3 y3 + t3) on the same rows (m_count = None: every row).  alloc = torch.zeros where the rows
    past the count -- never written -- are multiplied later, torch.empty where they are not read."""
    cout, _, W = w3s.shape
    dh2 = alloc(m_cap, W, device=dy.device)
    ops.conv_rows(dy, w3s.view(cout, W).t().reshape(W, 1, cout).contiguous(), None, zW, dh2, taps=1, m_count=m_count, m_cap=m_cap, relu=0)
    return dh2


def _conv2_T(du2, w2r, zW, ix, shape, stride, m_count, alloc):
    """conv2^T: d L / d h1 [cap1, W] on the rows of the dilated list, the 3x3 through the transposed neighbour table (m_count, alloc: as _conv3_T)"""
    B, _, Hi, Wi, Ho, Wo, W, _ = shape
    nbrT = transposed_neighbour_table(ix, B, Hi, Wi, stride, Ho, Wo)
    dh1 = alloc(ix.cap1, W, device=du2.device)
    ops.conv_rows(du2, w2r.permute(2, 1, 0).contiguous(), None, zW, dh1, a_rows=nbrT, taps=9, m_count=m_count, m_cap=ix.cap1, relu=0)
    return dh1


def _grad_x(du1, w1r, ix, m_count, shape):
    """conv1^T scattered into a zeroed input map -> d L / d x [B, Cin, Hi, Wi].  m_count = None: the dense channel case (every row)."""
    (B, Cin, Hi, Wi), W, dev = shape[:4], w1r.shape[0], du1.device
    gx = torch.zeros(B * Hi * Wi, Cin, device=dev)
    ops.conv_rows(du1, w1r.reshape(W, Cin).t().reshape(Cin, 1, W).contiguous(), None, torch.zeros(Cin, device=dev), gx, taps=1, m_count=m_count,
                  m_cap=ix.cap1, relu=0, out_rows=ix.idx1, residual2d=gx)
    return ops.from_nhwc(gx.view(B, Hi, Wi, Cin))


def _weight_grads(want1, want2, want3, dy3, h2, dz2, h1, dz1, x2d, ix, counted, consts=None):
    """(G1, G2, G3), None where not wanted: G = dz^T A in the convolutions' own layouts [cout, cin, kh, kw], from d L / d (s y + t) -- dy3 / dz2 / dz1,
    BEFORE the BatchNorm scale -- and the convs' inputs h2 / h1 / x2d: ldn_wgrad_rows, or the gather + GEMM path for shapes outside its predicate
    and with the switch off.  `_split_scale` makes the weight and the scale gradient of G.  counted: the lists are a pixel mask's -- the kernel
    gets the device-side counts and reads no row past them; the GEMM path relies on dy3 / dz2 / dz1 being zero there (select, then clamp: the
    list entries are uninitialised).  Not counted (the channel Fn's dense lists): every row is live.  consts = (c1, c2) where h1 / h2 are stored
    as u = h - c (the both Fn): conv2 / conv3 see h at every channel, the constants of the masked ones included."""
    W, Cin, cout = h1.shape[1], x2d.shape[1], dy3.shape[1]
    cnt3, cnt1 = (ix.cnt[0:1], ix.cnt[1:2]) if counted else (None, None)
    gw1 = gw2 = gw3 = None
    if want3:
        h2 = h2 if consts is None else h2 + consts[1]
        if _wgrad_kernel(W, cout, 1):
            gw3 = ops.wgrad_rows(dy3, h2, m_count=cnt3, m_cap=ix.cap3).reshape(cout, W, 1, 1)
        else:
            gw3 = (dy3.t() @ h2).reshape(cout, W, 1, 1)
    if want2:       # conv2 sees h1 inside the map, zeros in the padding ring
        h1 = h1 if consts is None else h1 + consts[0]
        if _wgrad_kernel(W, W, 9):
            gw2 = ops.wgrad_rows(dz2, h1, a_rows=ix.nbr, taps=9, m_count=cnt3, m_cap=ix.cap3, a_valid=ix.cap1).permute(0, 2, 1).reshape(W, W, 3, 3)
        else:
            gw2 = _weight_grad_3x3(dz2, h1, ix.nbr, ix.cap1, ix.cnt[0] if counted else None)
    if want1:
        if _wgrad_kernel(Cin, W, 1):
            gw1 = ops.wgrad_rows(dz1, x2d, a_rows=ix.idx1, taps=1, m_count=cnt1, m_cap=ix.cap1).reshape(W, Cin, 1, 1)
        else:
            rows1 = ix.idx1.long() if not counted else torch.where(torch.arange(ix.cap1, device=dz1.device) < ix.cnt[1], ix.idx1.long(),
                                                                   torch.zeros_like(ix.idx1, dtype=torch.long))
            gw1 = (dz1.t() @ x2d[rows1.clamp(0, x2d.shape[0] - 1)]).reshape(W, Cin, 1, 1)
    return gw1, gw2, gw3


def _split_scale(want_w, want_s, G, w, s):
    """(d W, d s) of z = s conv(a; W) + t from G = dz^T A (the weight gradient BEFORE the scale; None: neither is wanted):  d W = s G by rows,
    d s[c] = sum_p dz[p, c] conv(a)[p, c] = sum (G * W)[c] -- a contraction with the weights, never a division by s: exact at s == 0 (where
    relu(z) - t carries nothing of conv(a)) and free of the cancellation in (h - t) / s at a tiny s.  w: the weights in any layout with the
    output channel first and G's number of elements (the row kernels' tap-major one is brought to G's)."""
    if G is None:
        return None, None
    if w.dim() == 3 and G.shape[2] == 3:      # [cout, 9, cin] -> [cout, cin, 3, 3]
        w = w.view(w.shape[0], 3, 3, w.shape[2]).permute(0, 3, 1, 2)
    return G * s.view(-1, 1, 1, 1) if want_w else None, (G * w.reshape(G.shape)).sum((1, 2, 3)) if want_s else None


def _scaled_T(wr, s):
    """the row kernels' weights [cout, taps, cin] with a BatchNorm scale folded into the OUTPUT channels: what a transposed convolution reads
    when it is handed dz = d L / d (s y + t) rather than d L / d y"""
    return wr * s.view(-1, 1, 1)


def _pixel_lists(m3, stride):
    """the packed index lists of a pixel mask m3 [B, 1, Ho, Wo] {0,1} at the block's output size"""
    B, _, Ho, Wo = m3.shape
    return ops.mask_to_index(m3.detach().reshape(B, Ho, Wo).contiguous().float(), Ho, Wo, stride)


def _pixel_mask_grad(go, br, m3d, stride, run_chain):
    """Straight-through term of the hard pixel mask: d L / d m3[p] = sum_c g[p, c] * (s3 conv3(..) + t3)[p, c] needs the branch at the DROPPED
    pixels too (that term is dense in the reference as well).  The kept pixels' branch is `br`; the dropped ones' comes from the Fn's own chain,
    run_chain(cix, full), over the COMPLEMENT's lists into a copy of br -- together one dense execution of the block, of which the forward
    already paid the kept part."""
    B, _, Ho, Wo = m3d.shape
    cix = ops.mask_to_index((1.0 - m3d).reshape(B, Ho, Wo).contiguous(), Ho, Wo, stride)
    full = br.clone()
    run_chain(cix, full)
    return (go * full).sum(dim=1).view(B, 1, Ho, Wo)


# ------------------------------------------------------------------------------------------------------------------ pixel masks
def _pixel_chain(x2d, ix, w1r, w2r, w3s, s1, t1, s2, t2, t3, br):
    """conv1 -> conv2 -> conv3 over the lists of ix, conv3 scattered into br.  -> (h1, h2), ZEROED first: the rows past the counts are never
    written and are multiplied in the backward."""
    W, dev = w1r.shape[0], x2d.device
    h1 = torch.zeros(ix.cap1, W, device=dev)
    ops.conv_rows(x2d, w1r, s1, t1, h1, a_rows=ix.idx1, taps=1, m_count=ix.cnt[1:2], m_cap=ix.cap1)
    h2 = torch.zeros(ix.cap3, W, device=dev)
    ops.conv_rows(h1, w2r, s2, t2, h2, a_rows=ix.nbr, taps=9, m_count=ix.cnt[0:1], m_cap=ix.cap3)
    ops.conv_rows(h2, w3s, None, t3, br, taps=1, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=0, out_rows=ix.idx3)
    return h1, h2


class _PixelBranchFn(torch.autograd.Function):
    """branch = m3 * (s3 * conv3(relu(s2 * conv2(relu(s1 * conv1(x) + t1)) + t2)) + t3)  on the packed rows of the kept pixels (NCHW out, zeros at
    the dropped pixels); ix = _pixel_lists(m3).  Differentiable in x, the three weights, the six folded BatchNorm vectors and the mask."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, m3, s1, t1, s2, t2, s3, t3, stride, ix):
        p = _prep(x, w1, w2, w3, (s1, t1, s2, t2, s3, t3), stride)
        B, _, _, _, Ho, Wo, _, cout = p.shape
        s1, t1, s2, t2, s3, t3 = p.bn
        br = torch.zeros(B * Ho * Wo, cout, device=x.device)
        h1, h2 = _pixel_chain(p.x2d, ix, p.w1r, p.w2r, p.w3s, s1, t1, s2, t2, t3, br)
        ctx.save_for_backward(p.x2d, h1, h2, br, p.w1r, p.w2r, p.w3r, *p.bn, m3.detach().float())
        ctx.ix, ctx.shape, ctx.stride = ix, p.shape, stride
        ctx.math_mode = ops.get_math_mode()
        return ops.from_nhwc(br.view(B, Ho, Wo, cout))

    @staticmethod
    @_in_forward_mode
    def backward(ctx, g):
        x2d, h1, h2, br, w1r, w2r, w3r, s1, t1, s2, t2, s3, t3, m3d = ctx.saved_tensors
        ix, shape, stride, need, dev = ctx.ix, ctx.shape, ctx.stride, ctx.needs_input_grad, g.device
        cnt3, cnt1 = ix.cnt[0:1], ix.cnt[1:2]
        go = ops.as_nhwc(g.contiguous()).reshape(-1, w3r.shape[0])              # [B Ho Wo, cout]
        zW = torch.zeros(w1r.shape[0], device=dev)
        v3, v1 = _rows_valid(ix.cap3, ix.cnt[0], dev), _rows_valid(ix.cap1, ix.cnt[1], dev)
        # d L / d (s3 y3 + t3) at the kept pixels (the gather leaves the rows past the count unwritten -- recycled memory, possibly NaN: select,
        # do not multiply)
        g3 = torch.where(v3 > 0, ops.gather_rows(go, ix.idx3, count=cnt3, cap=ix.cap3), zW[:1])
        w3s = _fold_w3(w3r, s3)
        dh2 = _conv3_T(g3, w3s, zW, cnt3, ix.cap3, torch.zeros)
        dz2 = dh2 * (h2 > 0) * v3                         # through ReLU: d L / d (s2 y2 + t2)
        dh1 = _conv2_T(dz2 * s2, w2r, zW, ix, shape, stride, cnt1, torch.zeros)
        dz1 = dh1 * (h1 > 0) * v1
        grad_x = _grad_x(dz1 * s1, w1r, ix, cnt1, shape) if need[0] else None
        G1, G2, G3 = _weight_grads(need[1] or need[5], need[2] or need[7], need[3] or need[9], g3, h2, dz2, h1, dz1, x2d, ix, counted=True)
        gw1, gs1 = _split_scale(need[1], need[5], G1, w1r, s1)
        gw2, gs2 = _split_scale(need[2], need[7], G2, w2r, s2)
        gw3, gs3 = _split_scale(need[3], need[9], G3, w3r, s3)
        gt1, gt2, gt3 = (d.sum(0) if n else None for d, n in ((dz1, need[6]), (dz2, need[8]), (g3, need[10])))
        chain = lambda cix, full: _pixel_chain(x2d, cix, w1r, w2r, w3s, s1, t1, s2, t2, t3, full)
        gm = _pixel_mask_grad(go, br, m3d, stride, chain) if need[4] else None
        return grad_x, gw1, gw2, gw3, gm, gs1, gt1, gs2, gt2, gs3, gt3, None, None


# ------------------------------------------------------------------------------------------------------------------ channel masks
class _ChannelBranchFn(torch.autograd.Function):
    """branch = s3 * conv3(relu(s2 * (c . conv2(relu(s1 * (c . conv1(x)) + t1))) + t2)) + t3  with a {0,1} channel mask c [B, W] applied before bn1 / bn2
    (laud_resnet.py:116-118,124-126), on the row kernels over all pixels (ix = the cached dense_index): u = relu(bn(.)) - relu(shift) is stored,
    zeroed on the masked channels of each image (the library's dense channel execution, _shared.dense_channel_convs -- what
    Bottleneck._run_channel_dense runs)."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, chm, s1, t1, s2, t2, s3, t3, stride, ix):
        p = _prep(x, w1, w2, w3, (s1, t1, s2, t2, s3, t3), stride)
        B, _, Hi, Wi, Ho, Wo, W, cout = p.shape
        s1, t1, s2, t2, s3, t3 = p.bn
        c1, c2, tab, t3c = channel_constants(w2.detach().float(), p.w3r, s2, t2, t1, s3, t3)
        chm2d = chm.detach().float().reshape(B, W).contiguous()
        h1, h2 = dense_channel_convs(p.x2d, B, (Hi, Wi, Ho, Wo, stride), p.w1r, p.w2r, s1, t1, c1, s2, tab, c2, chm2d, ix)
        br = torch.empty(B * Ho * Wo, cout, device=x.device)
        ops.conv_rows(h2, p.w3s, None, t3c, br, taps=1, m_cap=ix.cap3, relu=0)
        ctx.save_for_backward(p.x2d, h1, h2, br, p.w1r, p.w2r, p.w3r, *p.bn, chm2d, c1, c2, tab)
        ctx.ix, ctx.shape, ctx.stride = ix, p.shape, stride
        ctx.math_mode = ops.get_math_mode()
        return ops.from_nhwc(br.view(B, Ho, Wo, cout))

    @staticmethod
    @_in_forward_mode
    def backward(ctx, g):
        x2d, u1, u2, br, w1r, w2r, w3r, s1, t1, s2, t2, s3, t3, chm2d, c1, c2, tab = ctx.saved_tensors
        ix, shape, stride, need, dev = ctx.ix, ctx.shape, ctx.stride, ctx.needs_input_grad, g.device
        B, _, Hi, Wi, Ho, Wo, W, _ = shape
        go = ops.as_nhwc(g.contiguous()).reshape(-1, w3r.shape[0])              # [B Ho Wo, cout]
        zW = torch.zeros(W, device=dev)
        cm3 = chm2d.view(B, 1, W)
        per_img = lambda t2d: t2d.view(B, -1, W)
        # forward values with the masks applied: h = u + c at every channel (a masked channel is the constant c), z > 0 <=> h > 0
        h1f, h2f = u1 + c1, u2 + c2
        on1 = (per_img(h1f) > 0).float()
        on2 = (per_img(h2f) > 0).float()
        dh2 = _conv3_T(go, _fold_w3(w3r, s3), zW, None, ix.cap3, torch.empty)
        dz2_all = per_img(dh2) * on2                                  # d L / d z2 (z2 = s2 * (c . y2) + t2)
        dz2 = (dz2_all * cm3).reshape(-1, W)
        dh1 = _conv2_T(dz2 * s2, w2r, zW, ix, shape, stride, None, torch.empty)      # (dz2 * s2 = d L / d y2 on the active channels)
        dz1_all = per_img(dh1) * on1
        dz1 = (dz1_all * cm3).reshape(-1, W)
        grad_x = _grad_x(dz1 * s1, w1r, ix, None, shape) if need[0] else None
        # z = s (c . y) + t: d W and d s only see the active channels (dz1 / dz2); d t sums d z over EVERY channel's pixels (a masked channel's
        # z = t still feeds the ReLU)
        G1, G2, G3 = _weight_grads(need[1] or need[5], need[2] or need[7], need[3] or need[9], go, h2f, dz2, h1f, dz1, x2d, ix, counted=False)
        gw1, gs1 = _split_scale(need[1], need[5], G1, w1r, s1)
        gw2, gs2 = _split_scale(need[2], need[7], G2, w2r, s2)
        gw3, gs3 = _split_scale(need[3], need[9], G3, w3r, s3)
        gt1 = dz1_all.reshape(-1, W).sum(0) if need[6] else None
        gt2 = dz2_all.reshape(-1, W).sum(0) if need[8] else None
        gt3 = go.sum(0) if need[10] else None
        gc = None
        if need[4]:
            # straight-through term: d L / d c[b, k] = sum_p d L / d (c . y)[b, k, p] * y[b, k, p] for both masked products, y = the UNMASKED conv
            # output -- needed at the masked channels too: the library's dense execution without the mask (r = s y + t, no ReLU); d z * s * y
            # = d z * (r - t), no division
            r1 = torch.empty(ix.cap1, W, device=dev)
            ops.conv_rows(x2d, w1r, s1, t1, r1, a_rows=ix.idx1, taps=1, m_cap=ix.cap1, relu=0)
            r2 = torch.empty(ix.cap3, W, device=dev)
            # (conv2 of h1 = u1 + c1: the constants' share is the border-class table)
            _conv_const(u1, w2r, s2, tab, r2, a_rows=ix.nbr, taps=9, m_count=None, m_cap=ix.cap3, relu=0, pix_map=ix.idx3, geom=(Hi, Wi, Ho, Wo, stride))
            gc = (dz1_all * per_img(r1 - t1)).sum(1) + (dz2_all * per_img(r2 - t2)).sum(1)          # [B, W]
        return grad_x, gw1, gw2, gw3, gc, gs1, gt1, gs2, gt2, gs3, gt3, None, None


# ------------------------------------------------------------------------------------------------------------------ pixel x channel masks
def _both_chain(x2d, ix, geom, w1r, w2r, w3s, s1, t1, c1, s2, tab, c2, t3c, chm2d, br):
    """conv1 -> conv2 -> conv3 over the lists of ix with the channel mask applied, conv3 scattered into br.  -> (u1, u2)"""
    W, dev = w1r.shape[0], x2d.device
    u1 = torch.empty(ix.cap1, W, device=dev)
    _conv_const(x2d, w1r, s1, t1, u1, a_rows=ix.idx1, taps=1, m_count=ix.cnt[1:2], m_cap=ix.cap1, relu=1, post_sub=c1)
    ops.rows_chanmask(u1, ix.pre1, chm2d, m_count=ix.cnt[1:2], m_cap=ix.cap1)          # (also zeroes the rows past the count)
    u2 = torch.empty(ix.cap3, W, device=dev)
    _conv_const(u1, w2r, s2, tab, u2, a_rows=ix.nbr, taps=9, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1, post_sub=c2, pix_map=ix.idx3, geom=geom)
    ops.rows_chanmask(u2, ix.pre3, chm2d, m_count=ix.cnt[0:1], m_cap=ix.cap3)
    ops.conv_rows(u2, w3s, None, t3c, br, taps=1, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=0, out_rows=ix.idx3)
    return u1, u2


class _BothBranchFn(torch.autograd.Function):
    """branch = m3 * (s3 * conv3(relu(s2 * (c . conv2(relu(s1 * (c . conv1(x)) + t1))) + t2)) + t3)  (dyn_mode 'both', laud_resnet.py:101-147): the pixel
    mask's packed rows (ix = _pixel_lists(m3), any stride) with the channel algebra of _ChannelBranchFn on them.  DENSE in the
    channels: conv_rows over every channel of the packed rows, u = relu(bn(.)) - relu(shift) stored, the masked channels of each row's image
    zeroed by ops.rows_chanmask (the image of a packed row comes from the lists' per-image prefix) -- the pixel mask saves its FLOPs in both
    directions, the channel mask saves none (stated, as for channel mode).  The constants' share of conv2 is the border-class table: every
    in-map neighbour of a kept pixel is in the dilated list, so a missing neighbour is padding and the table's classes are exact.  The
    backward's elementwise chain and its reductions (ReLU gate, channel mask, d scale / d shift, the per-image sums of the channel mask's
    straight-through term) are ops.rows_act_bwd: two launches per layer, deterministic.  Differentiable in x, the three weights, the six
    folded BatchNorm vectors, the pixel mask and the channel mask."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, m3, chm, s1, t1, s2, t2, s3, t3, stride, ix):
        p = _prep(x, w1, w2, w3, (s1, t1, s2, t2, s3, t3), stride)
        B, _, Hi, Wi, Ho, Wo, W, cout = p.shape
        s1, t1, s2, t2, s3, t3 = p.bn
        c1, c2, tab, t3c = channel_constants(w2.detach().float(), p.w3r, s2, t2, t1, s3, t3)
        chm2d = chm.detach().float().reshape(B, W).contiguous()
        br = torch.zeros(B * Ho * Wo, cout, device=x.device)
        u1, u2 = _both_chain(p.x2d, ix, (Hi, Wi, Ho, Wo, stride), p.w1r, p.w2r, p.w3s, s1, t1, c1, s2, tab, c2, t3c, chm2d, br)
        ctx.save_for_backward(p.x2d, u1, u2, br, p.w1r, p.w2r, p.w3r, *p.bn, m3.detach().float(), chm2d, c1, c2, tab, t3c)
        ctx.ix, ctx.shape, ctx.stride = ix, p.shape, stride
        ctx.math_mode = ops.get_math_mode()
        return ops.from_nhwc(br.view(B, Ho, Wo, cout))

    @staticmethod
    @_in_forward_mode
    def backward(ctx, g):
        x2d, u1, u2, br, w1r, w2r, w3r, s1, t1, s2, t2, s3, t3, m3d, chm2d, c1, c2, tab, t3c = ctx.saved_tensors
        ix, shape, stride = ctx.ix, ctx.shape, ctx.stride
        _, _, Hi, Wi, Ho, Wo, W, _ = shape
        dev = g.device
        need = ctx.needs_input_grad          # (x, w1, w2, w3, m3, chm, s1, t1, s2, t2, s3, t3): one further along than the other two Fns from chm on
        geom = (Hi, Wi, Ho, Wo, stride)
        cnt3, cnt1 = ix.cnt[0:1], ix.cnt[1:2]
        go = ops.as_nhwc(g.contiguous()).reshape(-1, w3r.shape[0])              # [B Ho Wo, cout]
        zW = torch.zeros(W, device=dev)
        v3 = _rows_valid(ix.cap3, ix.cnt[0], dev) > 0
        zero = torch.zeros((), device=dev)
        g3 = torch.where(v3, ops.gather_rows(go, ix.idx3, count=cnt3, cap=ix.cap3), zero)     # d L / d (s3 y3 + t3) at the kept pixels (as in _PixelBranchFn)
        w3s = _fold_w3(w3r, s3)
        zy1 = zy2 = None
        if need[5]:
            # the channel mask's straight-through term needs the UNMASKED conv outputs at the masked channels too: two relu=0 launches on the same
            # rows, z = s y + t as stored (rows_act_bwd takes that form); conv2 of h1 = u1 + c1, the constants' share in the border-class table
            zy1 = torch.empty(ix.cap1, W, device=dev)
            _conv_const(x2d, w1r, s1, t1, zy1, a_rows=ix.idx1, taps=1, m_count=cnt1, m_cap=ix.cap1, relu=0)
            zy2 = torch.empty(ix.cap3, W, device=dev)
            _conv_const(u1, w2r, s2, tab, zy2, a_rows=ix.nbr, taps=9, m_count=cnt3, m_cap=ix.cap3, relu=0, pix_map=ix.idx3, geom=geom)
        # conv3^T on the kept rows, then layer 2's elementwise chain + reductions in one kernel; likewise conv2^T and layer 1's.  The kernel is given
        # a scale of ones and so returns dz = d L / d (s y + t): the weight gradient call splits into d W and d s (_split_scale), and the
        # transposed convolutions read the scale out of their weights.  (Its sum dz * (h - t) is not used: dividing that by s is wrong at s == 0.)
        one = torch.ones(W, device=dev)
        dh2 = _conv3_T(g3, w3s, zW, cnt3, ix.cap3, torch.empty)
        dz2, gt2, _, gm2 = ops.rows_act_bwd(dh2, u2, one, t2, post_sub=c2, chan_mask=chm2d, row_prefix=ix.pre3, zy2d=zy2, m_count=cnt3,
                                            m_cap=ix.cap3, out=dh2)
        dh1 = _conv2_T(dz2, _scaled_T(w2r, s2), zW, ix, shape, stride, cnt1, torch.empty)
        dz1, gt1, _, gm1 = ops.rows_act_bwd(dh1, u1, one, t1, post_sub=c1, chan_mask=chm2d, row_prefix=ix.pre1, zy2d=zy1, m_count=cnt1,
                                            m_cap=ix.cap1, out=dh1)
        grad_x = _grad_x(dz1, _scaled_T(w1r, s1), ix, cnt1, shape) if need[0] else None
        G1, G2, G3 = _weight_grads(need[1] or need[6], need[2] or need[8], need[3] or need[10], g3, u2, dz2, u1, dz1, x2d, ix, counted=True,
                                   consts=(c1, c2))
        gw1, gs1 = _split_scale(need[1], need[6], G1, w1r, s1)
        gw2, gs2 = _split_scale(need[2], need[8], G2, w2r, s2)
        gw3, gs3 = _split_scale(need[3], need[10], G3, w3r, s3)        # (conv3 of h2 = u2 + c2: the constants' share is in G3)
        gt3 = g3.sum(0) if need[11] else None
        chain = lambda cix, full: _both_chain(x2d, cix, geom, w1r, w2r, w3s, s1, t1, c1, s2, tab, c2, t3c, chm2d, full)     # WITH the channel mask
        gm = _pixel_mask_grad(go, br, m3d, stride, chain) if need[4] else None
        gc = gm1 + gm2 if need[5] else None
        return grad_x, gw1, gw2, gw3, gm, gc, gs1, gt1 if need[7] else None, gs2, gt2 if need[9] else None, gs3, gt3, None, None


# ------------------------------------------------------------------------------------------------------------------ LAD-RegNet, layer skip
def _se_gate(sq, w1, b1, w2, b2):
    """the excite MLP on the squeezed rows sq [slots, C] -> (u = fc1's output in front of its ReLU, gate = sigmoid(fc2(relu(u))))"""
    u = sq @ w1.t() + b1
    return u, torch.sigmoid(torch.relu(u) @ w2.t() + b2)


def _conv_b_params(wbr, sb, tb, gw):
    """what laud_regnet._conv_b_rows reads of a prepared block, from the live weights (the fragments of the family the chooser names, no other)"""
    pb = {"wb": wbr, "sb": sb, "tb": tb}
    _conv_b_frag(pb, conv_b_choice("rows", wbr.shape[0], gw)[0], gw)
    return pb


def _conv_b_bare(wr, gw, x, nbr, y, m_count, m_cap, families=None):
    """the grouped 3x3 of weights wr [W, 9, gw] alone -- scale 1, shift 0, no ReLU -- over the neighbour table nbr, on laud_regnet.conv_b_choice's
    kernel among `families` (None: all)"""
    W, dev = wr.shape[0], x.device
    pb = {"wb": wr, "sb": torch.ones(W, device=dev), "tb": torch.zeros(W, device=dev)}
    _conv_b_run(conv_b_choice("rows", W, gw, families=families), pb, gw, x, nbr, y, m_count, m_cap, None, relu=0)


def _conv_b_adjoint(dy, nbrT, wbr, gw, dha, m_count, m_cap):
    """b^T: the forward kernel over the transposed neighbour table with per-group transposed weights, into the zeroed dha.  Never the width-16
    matrix-core kernel: the VALU one, or those of widths 8 / 24 and 56 / 112 / 232 behind their switches."""
    _conv_b_bare(grouped_weight_T(wbr, gw), gw, dy, nbrT, dha, m_count, m_cap, families=("gw", "wide"))


def _regnet_chain(x2d, ix, P, f, war, wbr, wcs, sa, ta, sb, tb, tc, se, br):
    """a -> grouped b -> SE -> c over the lists of ix (WHOLE images in list order: the j-th listed image owns rows [j P, (j + 1) P), P = Ho Wo),
    c scattered into br.  -> (h_a, h_b in front of the gate, gate [slots, C]); h_a / h_b ZEROED first, as _pixel_chain's: a slot past the count
    squeezes to zero and its gate multiplies zero rows."""
    W, dev = war.shape[0], x2d.device
    h_a = torch.zeros(ix.cap1, W, device=dev)
    ops.conv_rows(x2d, war, sa, ta, h_a, a_rows=ix.idx1, taps=1, m_count=ix.cnt[1:2], m_cap=ix.cap1)
    h_b = torch.zeros(ix.cap3, W, device=dev)
    _conv_b_rows(_conv_b_params(wbr, sb, tb, f.group_width), f, h_a, ix.nbr, h_b, ix.cnt[0:1], ix.cap3)
    hbv = h_b.view(-1, P, W)
    gate = _se_gate(hbv.mean(1), *se)[1]
    z = (hbv * gate.unsqueeze(1)).view(ix.cap3, W)
    ops.conv_rows(z, wcs, None, tc, br, taps=1, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=0, out_rows=ix.idx3)
    return h_a, h_b, gate


class _RegNetSkipBranchFn(torch.autograd.Function):
    """branch = m3 * (sc * c(gate . h_b) + tc),  h_b = relu(sb * b(relu(sa * a(x) + ta)) + tb),  gate = sigmoid(fc2(relu(fc1(mean_pixels h_b))))
    (laud_regnet.py:179-200 in its layer-skip form: one keep / skip bit per image, m3 constant over an image) on the packed rows of the KEPT
    images: a and c on conv_rows, the grouped 3x3 b on ldn_grouped_conv3x3_rows -- its adjoint the same kernel over the transposed neighbour
    table with per-group transposed weights, its weight gradient ops.wgrad_grouped_rows -- and the squeeze / excite as tensor ops on the
    [slots, Ho Wo, C] view of the rows.  A dropped image costs nothing in either direction.  Differentiable in x, the three weights, the six
    folded BatchNorm vectors, the four SE tensors and the mask."""

    @staticmethod
    def forward(ctx, x, wa, wb, wc, m3, sa, ta, sb, tb, sc, tc, w1, b1, w2, b2, stride, f, ix):
        p = _prep(x, wa, wb, wc, (sa, ta, sb, tb, sc, tc), stride)
        B, _, _, _, Ho, Wo, W, cout = p.shape
        sa, ta, sb, tb, sc, tc = p.bn
        se = (w1.detach().float().reshape(-1, W).contiguous(), b1.detach().float().contiguous(),
              w2.detach().float().reshape(W, -1).contiguous(), b2.detach().float().contiguous())
        br = torch.zeros(B * Ho * Wo, cout, device=x.device)
        h_a, h_b, gate = _regnet_chain(p.x2d, ix, Ho * Wo, f, p.w1r, p.w2r, p.w3s, sa, ta, sb, tb, tc, se, br)
        ctx.save_for_backward(p.x2d, h_a, h_b, gate, br, p.w1r, p.w2r, p.w3r, *p.bn, *se, m3.detach().float())
        ctx.ix, ctx.shape, ctx.stride, ctx.f, ctx.se_shapes = ix, p.shape, stride, f, (w1.shape, w2.shape)
        ctx.math_mode = ops.get_math_mode()
        return ops.from_nhwc(br.view(B, Ho, Wo, cout))

    @staticmethod
    @_in_forward_mode
    def backward(ctx, g):
        x2d, h_a, h_b, gate, br, war, wbr, wcr, sa, ta, sb, tb, sc, tc, w1, b1, w2, b2, m3d = ctx.saved_tensors
        ix, shape, stride, f, need, dev = ctx.ix, ctx.shape, ctx.stride, ctx.f, ctx.needs_input_grad, g.device
        B, _, Hi, Wi, Ho, Wo, W, cout = shape
        P, gw = Ho * Wo, f.group_width
        cnt3, cnt1 = ix.cnt[0:1], ix.cnt[1:2]
        go = ops.as_nhwc(g.contiguous()).reshape(-1, cout)                       # [B Ho Wo, cout]
        zW = torch.zeros(W, device=dev)
        v3, v1 = _rows_valid(ix.cap3, ix.cnt[0], dev), _rows_valid(ix.cap1, ix.cnt[1], dev)
        g3 = torch.where(v3 > 0, ops.gather_rows(go, ix.idx3, count=cnt3, cap=ix.cap3), zW[:1])     # d L / d (sc y_c + tc) at the kept pixels (as in _PixelBranchFn)
        wcs = _fold_w3(wcr, sc)
        dz = _conv3_T(g3, wcs, zW, cnt3, ix.cap3, torch.zeros)                   # d L / d (gate . h_b); zero rows past the count
        # squeeze-excitation: two per-image reductions over the [slots, P, C] view and the excite MLP by hand on [slots, C] tensors.  A slot past
        # the count holds zero rows in dz and h_b alike: d gate is selected to zero there, so nothing of it reaches d fc1 / d fc2
        dzv, hbv = dz.view(-1, P, W), h_b.view(-1, P, W)
        slot_on = (torch.arange(dzv.shape[0], device=dev) * P < ix.cnt[0]).unsqueeze(1)
        sq = hbv.mean(1)
        u = sq @ w1.t() + b1
        r = torch.relu(u)
        dv = torch.where(slot_on, (dzv * hbv).sum(1), zW[:1]) * gate * (1.0 - gate)      # through the sigmoid
        du = (dv @ w2) * (u > 0)
        dsq = du @ w1
        gw1s = (du.t() @ sq).reshape(ctx.se_shapes[0]) if need[11] else None
        gb1s = du.sum(0) if need[12] else None
        gw2s = (dv.t() @ r).reshape(ctx.se_shapes[1]) if need[13] else None
        gb2s = dv.sum(0) if need[14] else None
        dhb = (dzv * gate.unsqueeze(1) + dsq.unsqueeze(1) / P).view(ix.cap3, W)
        dzb = dhb * (h_b > 0) * v3                        # through ReLU: d L / d (sb y_b + tb)
        dub = dzb * sb
        # b^T: the forward kernel over the transposed neighbour table with per-group transposed weights, scale 1, shift 0, no ReLU
        nbrT = transposed_neighbour_table(ix, B, Hi, Wi, stride, Ho, Wo)
        dha = torch.zeros(ix.cap1, W, device=dev)
        _conv_b_adjoint(dub, nbrT, wbr, gw, dha, cnt1, ix.cap1)
        dza = dha * (h_a > 0) * v1
        grad_x = _grad_x(dza * sa, war, ix, cnt1, shape) if need[0] else None
        z = (hbv * gate.unsqueeze(1)).view(ix.cap3, W) if need[3] or need[9] else None       # conv c's input
        Ga, _, Gc = _weight_grads(need[1] or need[5], False, need[3] or need[9], g3, z, None, h_a, dza, x2d, ix, counted=True)
        Gb = None
        if need[2] or need[7]:       # conv b sees h_a inside the map, zeros in the padding ring
            Gb = _weight_grad_conv_b(dzb, h_a, ix, gw, cnt3, ix.cnt[0])
        gwa, gsa = _split_scale(need[1], need[5], Ga, war, sa)
        gwb, gsb = _split_scale(need[2], need[7], Gb, wbr, sb)
        gwc, gsc = _split_scale(need[3], need[9], Gc, wcr, sc)
        gta, gtb, gtc = (d.sum(0) if n else None for d, n in ((dza, need[6]), (dzb, need[8]), (g3, need[10])))
        # the straight-through term needs the branch of the DROPPED images: this Fn's own chain over the complement's lists (their SE squeezes
        # their own rows -- what the dense reference computes)
        se = (w1, b1, w2, b2)
        chain = lambda cix, full: _regnet_chain(x2d, cix, P, f, war, wbr, wcs, sa, ta, sb, tb, tc, se, full)
        gm = _pixel_mask_grad(go, br, m3d, stride, chain) if need[4] else None
        return grad_x, gwa, gwb, gwc, gm, gsa, gta, gsb, gtb, gsc, gtc, gw1s, gb1s, gw2s, gb2s, None, None, None


# ------------------------------------------------------------------------------------------------------------------ LAD-RegNet, channel masks
class _RegNetChannelBranchFn(torch.autograd.Function):
    """branch = sc * c(gate . h_b) + tc,  h_a = m . relu(sa * a(x) + ta),  h_b = m . relu(sb * b(h_a) + tb),  gate = sigmoid(fc2(relu(fc1(mean_pixels h_b))))
    (laud_regnet.py:182-200, dyn_mode 'channel'): the {0,1} channel mask m [B, W] multiplies the outputs of a and b AFTER conv + BN + ReLU, so
    none of the LAUD-ResNet channel algebra applies (no constants, no border classes).  The row kernels run over ALL pixels (ix = the cached
    dense_index) and DENSE in the channels -- the mask saves no FLOPs in training: its straight-through term sum_p d h . relu(zy) needs relu(zy)
    and the upstream gradient at the masked channels too.  a and c on conv_rows, the grouped 3x3 b on ldn_grouped_conv3x3_rows (adjoint and weight
    gradient as in _RegNetSkipBranchFn), the masking ops.rows_chanmask; the backward's elementwise chain with all its reductions is one
    ops.rows_postmask_bwd per layer (layer b's with the squeeze-excitation prologue), d gate ops.rows_img_dot; the excite MLP stays on [B, .]
    tensors.  The UNMASKED relu outputs are kept only when the mask requires grad: a masked unit has a = 0 either way.  Differentiable in x,
    the three weights, the six folded BatchNorm vectors, the four SE tensors and the channel mask."""

    @staticmethod
    def forward(ctx, x, wa, wb, wc, chm, sa, ta, sb, tb, sc, tc, w1, b1, w2, b2, stride, f, ix):
        p = _prep(x, wa, wb, wc, (sa, ta, sb, tb, sc, tc), stride)
        B, _, Hi, Wi, Ho, Wo, W, cout = p.shape
        sa, ta, sb, tb, sc, tc = p.bn
        dev, P = x.device, Ho * Wo
        se = (w1.detach().float().reshape(-1, W).contiguous(), b1.detach().float().contiguous(),
              w2.detach().float().reshape(W, -1).contiguous(), b2.detach().float().contiguous())
        m2d = chm.detach().float().reshape(B, W).contiguous()
        keep_r = ctx.needs_input_grad[4]
        pre1, pre3 = image_prefix(B, Hi * Wi, dev), image_prefix(B, P, dev)
        r_a = torch.empty(ix.cap1, W, device=dev)
        ops.conv_rows(p.x2d, p.w1r, sa, ta, r_a, a_rows=ix.idx1, taps=1, m_cap=ix.cap1)
        h_a = ops.rows_chanmask(r_a.clone() if keep_r else r_a, pre1, m2d, m_cap=ix.cap1)
        r_b = torch.empty(ix.cap3, W, device=dev)
        _conv_b_rows(_conv_b_params(p.w2r, sb, tb, f.group_width), f, h_a, ix.nbr, r_b, ix.cnt[0:1], ix.cap3)
        h_b = ops.rows_chanmask(r_b.clone() if keep_r else r_b, pre3, m2d, m_cap=ix.cap3)
        hbv = h_b.view(B, P, W)
        sq = hbv.mean(1)
        u, gate = _se_gate(sq, *se)
        br = torch.empty(ix.cap3, cout, device=dev)
        ops.conv_rows((hbv * gate.unsqueeze(1)).view(ix.cap3, W), p.w3s, None, tc, br, taps=1, m_cap=ix.cap3, relu=0)
        # r_a / r_b: the unmasked ReLU outputs where the mask wants its gradient, else the masked copies themselves (h_b is r_b . m: not saved)
        ctx.save_for_backward(p.x2d, r_a, h_a, r_b, sq, u, gate, br, p.w1r, p.w2r, p.w3r, *p.bn, *se, m2d)
        ctx.ix, ctx.shape, ctx.stride, ctx.f, ctx.se_shapes, ctx.keep_r = ix, p.shape, stride, f, (w1.shape, w2.shape), keep_r
        ctx.math_mode = ops.get_math_mode()
        return ops.from_nhwc(br.view(B, Ho, Wo, cout))

    @staticmethod
    @_in_forward_mode
    def backward(ctx, g):
        x2d, r_a, h_a, r_b, sq, u, gate, br, war, wbr, wcr, sa, ta, sb, tb, sc, tc, w1, b1, w2, b2, m2d = ctx.saved_tensors
        ix, shape, stride, f, need, dev, keep_r = ctx.ix, ctx.shape, ctx.stride, ctx.f, ctx.needs_input_grad, g.device, ctx.keep_r
        B, _, Hi, Wi, Ho, Wo, W, cout = shape
        P, gw = Ho * Wo, f.group_width
        pre1, pre3 = image_prefix(B, Hi * Wi, dev), image_prefix(B, P, dev)
        go = ops.as_nhwc(g.contiguous()).reshape(-1, cout)                       # [B Ho Wo, cout]
        zW = torch.zeros(W, device=dev)
        dz = _conv3_T(go, _fold_w3(wcr, sc), zW, None, ix.cap3, torch.empty)     # d L / d (gate . h_b)
        # squeeze-excitation: d gate = sum_p dz . h_b in one kernel (h_b = r_b . m), the excite MLP by hand on [B, .] tensors
        dgate = ops.rows_img_dot(dz, r_b, pre3, m_cap=ix.cap3)
        if keep_r:
            dgate = dgate * m2d
        dv = dgate * gate * (1.0 - gate)                                         # through the sigmoid
        du = (dv @ w2) * (u > 0)
        dsq = du @ w1
        gw1s = (du.t() @ sq).reshape(ctx.se_shapes[0]) if need[11] else None
        gb1s = du.sum(0) if need[12] else None
        gw2s = (dv.t() @ torch.relu(u)).reshape(ctx.se_shapes[1]) if need[13] else None
        gb2s = dv.sum(0) if need[14] else None
        gm_gate = gate * m2d if keep_r else gate
        z = (r_b.view(B, P, W) * gm_gate.unsqueeze(1)).view(ix.cap3, W) if need[3] or need[9] else None      # conv c's input
        # layer b: d h_b = dz . gate + dsq / P, the mask, the ReLU and every reduction in one kernel (in place on dz).  The kernel is given a scale
        # of ones and so returns d L / d (sb y_b + tb): the weight gradient call splits into d W and d s (_split_scale), b^T reads sb out of its
        # weights.  (Its sum a * (r - t) is not used: dividing that by s is wrong at s == 0.)
        one = torch.ones(W, device=dev)
        dzb, gtb, _, gmb = ops.rows_postmask_bwd(dz, r_b, one, tb, chan_mask=m2d, row_prefix=pre3, gate=gate, dsq=(dsq / P).contiguous(),
                                                 want_mask=keep_r, m_cap=ix.cap3, out=dz)
        # b^T: the forward kernel over the transposed neighbour table with per-group transposed weights (sb folded in), scale 1, shift 0, no ReLU
        nbrT = transposed_neighbour_table(ix, B, Hi, Wi, stride, Ho, Wo)
        dha = torch.empty(ix.cap1, W, device=dev)
        _conv_b_adjoint(dzb, nbrT, _scaled_T(wbr, sb), gw, dha, ix.cnt[1:2], ix.cap1)
        dza, gta, _, gma = ops.rows_postmask_bwd(dha, r_a, one, ta, chan_mask=m2d, row_prefix=pre1, want_mask=keep_r, m_cap=ix.cap1, out=dha)
        grad_x = _grad_x(dza, _scaled_T(war, sa), ix, None, shape) if need[0] else None
        Ga, _, Gc = _weight_grads(need[1] or need[5], False, need[3] or need[9], go, z, None, h_a, dza, x2d, ix, counted=False)
        Gb = None
        if need[2] or need[7]:       # conv b sees the MASKED h_a inside the map, zeros in the padding ring
            Gb = _weight_grad_conv_b(dzb, h_a, ix, gw, ix.cnt[0:1])
        gwa, gsa = _split_scale(need[1], need[5], Ga, war, sa)
        gwb, gsb = _split_scale(need[2], need[7], Gb, wbr, sb)
        gwc, gsc = _split_scale(need[3], need[9], Gc, wcr, sc)
        gtc = go.sum(0) if need[10] else None
        gc = gma + gmb if keep_r else None
        return (grad_x, gwa, gwb, gwc, gc, gsa, gta if need[6] else None, gsb, gtb if need[8] else None, gsc, gtc, gw1s, gb1s, gw2s, gb2s,
                None, None, None)


# ------------------------------------------------------------------------------------------------------------------ batch statistics
class _BatchStatsBranchFn(torch.autograd.Function):
    """branch = m3 * bn3(conv3(relu(bn2(c . conv2(relu(bn1(c . conv1(x))))))))  with bn1 / bn2 / bn3 on the statistics of THE BATCH (laud_resnet.py:115-133
    in plain model.train(): the reference's ImageNet recipe), for all four dyn_modes: the pixel mask m3 [B, 1, Ho, Wo] and the channel mask c [B, W]
    are both optional.  Dense by construction -- every BatchNorm sees every pixel and every channel, dropped or not, so NEITHER mask saves FLOPs
    here: the convolutions run over all pixels (ix = the cached dense_index, any stride) on ops.conv_rows with scale 1 / shift 0 / no ReLU and
    store the UNMASKED outputs y; nothing is folded, so there is no _split_scale and bn.weight == 0 is no special case.  BatchNorm is
    ops.rows_bn_stats (two launches) + ops.rows_bn_fwd (one) with the channel mask applied in front of both -- a channel dropped in one image
    contributes zeros to the statistics -- and, in the backward, ops.rows_bn_bwd: d gamma, d beta, the gradient through the statistics, the
    channel mask and its straight-through term sum_p d u . y in three (four) launches per layer.  The pixel mask is a per-row factor of layer 3's
    forward and backward; its own gradient sum_k g . bn3(..) re-runs rows_bn_fwd without the factor.
    Inputs: x, the three weights, m3 or None, c or None, (gamma, beta) x 3; eps3 = the three eps.  Returns (branch, mean1, var1, mean2, var2,
    mean3, var3): the batch statistics (biased variances) are non-differentiable outputs -- _branch updates the running statistics from them,
    once per forward and never in the backward."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, m3, chm, g1, b1, g2, b2, g3, b3, eps3, stride, ix):
        one = torch.ones((), device=x.device)
        p = _prep(x, w1, w2, w3, (g1, b1, g2, b2, g3, b3), stride)
        B, _, _, _, Ho, Wo, W, cout = p.shape
        g1, b1, g2, b2, g3, b3 = p.bn
        dev = x.device
        chm2d = None if chm is None else chm.detach().float().reshape(B, W).contiguous()
        m3r = None if m3 is None else m3.detach().float().reshape(B * Ho * Wo).contiguous()
        pre1, pre3 = (ix.pre1, ix.pre3) if chm2d is not None else (None, None)
        zW, zc = torch.zeros(W, device=dev), torch.zeros(cout, device=dev)
        y1 = torch.empty(ix.cap1, W, device=dev)
        ops.conv_rows(p.x2d, p.w1r, None, zW, y1, a_rows=ix.idx1, taps=1, m_cap=ix.cap1, relu=0)
        mean1, var1, inv1 = ops.rows_bn_stats(y1, eps3[0], chan_mask=chm2d, row_prefix=pre1, m_cap=ix.cap1)
        h1 = ops.rows_bn_fwd(y1, mean1, inv1, g1, b1, chan_mask=chm2d, row_prefix=pre1, m_cap=ix.cap1)
        y2 = torch.empty(ix.cap3, W, device=dev)
        ops.conv_rows(h1, p.w2r, None, zW, y2, a_rows=ix.nbr, taps=9, m_cap=ix.cap3, relu=0)
        mean2, var2, inv2 = ops.rows_bn_stats(y2, eps3[1], chan_mask=chm2d, row_prefix=pre3, m_cap=ix.cap3)
        h2 = ops.rows_bn_fwd(y2, mean2, inv2, g2, b2, chan_mask=chm2d, row_prefix=pre3, m_cap=ix.cap3)
        y3 = torch.empty(ix.cap3, cout, device=dev)
        ops.conv_rows(h2, p.w3r.reshape(cout, 1, W), None, zc, y3, taps=1, m_cap=ix.cap3, relu=0)
        mean3, var3, inv3 = ops.rows_bn_stats(y3, eps3[2], m_cap=ix.cap3)
        br = ops.rows_bn_fwd(y3, mean3, inv3, g3, b3, row_scale=m3r, relu=False, m_cap=ix.cap3)
        ctx.save_for_backward(p.x2d, y1, h1, y2, h2, y3, p.w1r, p.w2r, p.w3r, g1, g2, g3, b3, mean1, inv1, mean2, inv2, mean3, inv3,
                              one if chm2d is None else chm2d, one if m3r is None else m3r)
        ctx.ix, ctx.shape, ctx.stride, ctx.masks = ix, p.shape, stride, (m3r is not None, chm2d is not None)
        ctx.math_mode = ops.get_math_mode()
        stats = (mean1, var1, mean2, var2, mean3, var3)
        ctx.mark_non_differentiable(*stats)
        return (ops.from_nhwc(br.view(B, Ho, Wo, cout)),) + stats

    @staticmethod
    @_in_forward_mode
    def backward(ctx, g, *_stats):
        x2d, y1, h1, y2, h2, y3, w1r, w2r, w3r, g1, g2, g3, b3, mean1, inv1, mean2, inv2, mean3, inv3, chm2d, m3r = ctx.saved_tensors
        ix, shape, stride, need, dev = ctx.ix, ctx.shape, ctx.stride, ctx.needs_input_grad, g.device
        B, _, _, _, Ho, Wo, W, cout = shape
        has_m3, has_c = ctx.masks
        m3r, chm2d = m3r if has_m3 else None, chm2d if has_c else None
        pre1, pre3 = (ix.pre1, ix.pre3) if has_c else (None, None)
        want_c = has_c and need[5]
        go = ops.as_nhwc(g.contiguous()).reshape(-1, cout)                       # [B Ho Wo, cout] = d L / d branch
        zW = torch.zeros(W, device=dev)
        gm = None
        if has_m3 and need[4]:      # the pixel mask's straight-through term needs bn3's output at the dropped pixels: the forward's launch without the factor
            z3 = ops.rows_bn_fwd(y3, mean3, inv3, g3, b3, relu=False, m_cap=ix.cap3)
            gm = (go * z3).sum(1).view(B, 1, Ho, Wo)
        # per layer: ONE rows_bn_bwd (pixel / channel mask, ReLU gate read from the stored h, d gamma, d beta, the statistics' terms, d mask) -> d L / d y,
        # then the transposed convolution with the plain weights
        dy3, gg3, gb3, _ = ops.rows_bn_bwd(go, y3, None, mean3, inv3, g3, row_scale=m3r, m_cap=ix.cap3)
        dh2 = _conv3_T(dy3, w3r.reshape(cout, 1, W), zW, None, ix.cap3, torch.empty)
        dy2, gg2, gb2, gc2 = ops.rows_bn_bwd(dh2, y2, h2, mean2, inv2, g2, chan_mask=chm2d, row_prefix=pre3, want_mask=want_c, m_cap=ix.cap3, out=dh2)
        dh1 = _conv2_T(dy2, w2r, zW, ix, shape, stride, None, torch.empty)
        dy1, gg1, gb1, gc1 = ops.rows_bn_bwd(dh1, y1, h1, mean1, inv1, g1, chan_mask=chm2d, row_prefix=pre1, want_mask=want_c, m_cap=ix.cap1, out=dh1)
        grad_x = _grad_x(dy1, w1r, ix, None, shape) if need[0] else None
        gw1, gw2, gw3 = _weight_grads(need[1], need[2], need[3], dy3, h2, dy2, h1, dy1, x2d, ix, counted=False)
        gc = gc1 + gc2 if want_c else None
        keep = lambda v, n: v if n else None
        return (grad_x, gw1, gw2, gw3, gm, gc, keep(gg1, need[6]), keep(gb1, need[7]), keep(gg2, need[8]), keep(gb2, need[9]), keep(gg3, need[10]),
                keep(gb3, need[11]), None, None, None)


def _conv_b_plain(wbr, gw, h_a, nbr, y_b, m_count, m_cap):
    """the grouped 3x3 alone -- scale 1, shift 0, no ReLU -- with laud_regnet._conv_b_rows' choice of kernel: the matrix cores for group width 16
    in bf16x3 mode (widths 8 / 24 and 56 / 112 / 232 behind their switches), else the fp32 VALU kernel"""
    _conv_b_bare(wbr, gw, h_a, nbr, y_b, m_count, m_cap)


class _RegNetBatchStatsBranchFn(torch.autograd.Function):
    """branch = bn_c(c(gate . h_b)),  h_a = m . relu(bn_a(a(x))),  h_b = m . relu(bn_b(b(h_a))),  gate = sigmoid(fc2(relu(fc1(mean_pixels h_b))))
    with bn_a / bn_b / bn_c on the statistics of THE BATCH (laud_regnet.py:182-200, dyn_mode 'channel', in plain model.train(): the third command
    of the reference's train_scripts.sh).  The {0,1} channel mask m [B, W] multiplies AFTER BatchNorm + ReLU, so every channel of every image
    feeds the statistics, dropped or not: dense by construction, THE MASK SAVES NO FLOPs.  a and c on ops.conv_rows, the grouped 3x3 b on the
    grouped kernels, all three with scale 1 / shift 0 / no ReLU over all pixels (ix = the cached dense_index) -- nothing is folded, so there is no
    _split_scale and bn.weight == 0 is no special case.  Layers a / b: ops.rows_bn_stats (no mask) + ops.rows_bn_postmask_fwd forward,
    ops.rows_bn_postmask_bwd backward (layer b's with the squeeze-excitation prologue): the unmasked y and the masked h are all a layer saves.
    Layer c: ops.rows_bn_fwd / ops.rows_bn_bwd without ReLU.  d gate = ops.rows_img_dot(dz, h_b): h_b is masked already.  Adjoints and weight
    gradients as in _RegNetChannelBranchFn, with the plain weights.
    Inputs: x, the three weights, the channel mask, (gamma, beta) x 3, the four SE tensors; eps3 = the three eps.  Returns (branch, mean_a, var_a,
    mean_b, var_b, mean_c, var_c): the batch statistics (biased variances) are non-differentiable outputs -- _branch_regnet updates the running
    statistics from them, once per forward and never in the backward."""

    @staticmethod
    def forward(ctx, x, wa, wb, wc, chm, ga, ba, gb, bb, gc, bc, w1, b1, w2, b2, eps3, stride, f, ix):
        p = _prep(x, wa, wb, wc, (ga, ba, gb, bb, gc, bc), stride)
        B, _, _, _, Ho, Wo, W, cout = p.shape
        ga, ba, gb, bb, gc, bc = p.bn
        dev, P = x.device, Ho * Wo
        se = (w1.detach().float().reshape(-1, W).contiguous(), b1.detach().float().contiguous(),
              w2.detach().float().reshape(W, -1).contiguous(), b2.detach().float().contiguous())
        m2d = chm.detach().float().reshape(B, W).contiguous()
        zW, zc = torch.zeros(W, device=dev), torch.zeros(cout, device=dev)
        y_a = torch.empty(ix.cap1, W, device=dev)
        ops.conv_rows(p.x2d, p.w1r, None, zW, y_a, a_rows=ix.idx1, taps=1, m_cap=ix.cap1, relu=0)
        mean_a, var_a, inv_a = ops.rows_bn_stats(y_a, eps3[0], m_cap=ix.cap1)
        h_a = ops.rows_bn_postmask_fwd(y_a, mean_a, inv_a, ga, ba, chan_mask=m2d, row_prefix=ix.pre1, m_cap=ix.cap1)
        y_b = torch.empty(ix.cap3, W, device=dev)
        _conv_b_plain(p.w2r, f.group_width, h_a, ix.nbr, y_b, ix.cnt[0:1], ix.cap3)
        mean_b, var_b, inv_b = ops.rows_bn_stats(y_b, eps3[1], m_cap=ix.cap3)
        h_b = ops.rows_bn_postmask_fwd(y_b, mean_b, inv_b, gb, bb, chan_mask=m2d, row_prefix=ix.pre3, m_cap=ix.cap3)
        hbv = h_b.view(B, P, W)
        sq = hbv.mean(1)
        u, gate = _se_gate(sq, *se)
        y_c = torch.empty(ix.cap3, cout, device=dev)
        ops.conv_rows((hbv * gate.unsqueeze(1)).view(ix.cap3, W), p.w3r.reshape(cout, 1, W), None, zc, y_c, taps=1, m_cap=ix.cap3, relu=0)
        mean_c, var_c, inv_c = ops.rows_bn_stats(y_c, eps3[2], m_cap=ix.cap3)
        br = ops.rows_bn_fwd(y_c, mean_c, inv_c, gc, bc, relu=False, m_cap=ix.cap3)
        ctx.save_for_backward(p.x2d, y_a, h_a, y_b, h_b, y_c, sq, u, gate, p.w1r, p.w2r, p.w3r, ga, ba, gb, bb, gc, mean_a, inv_a, mean_b, inv_b,
                              mean_c, inv_c, *se, m2d)
        ctx.ix, ctx.shape, ctx.stride, ctx.f, ctx.se_shapes = ix, p.shape, stride, f, (w1.shape, w2.shape)
        ctx.math_mode = ops.get_math_mode()
        stats = (mean_a, var_a, mean_b, var_b, mean_c, var_c)
        ctx.mark_non_differentiable(*stats)
        return (ops.from_nhwc(br.view(B, Ho, Wo, cout)),) + stats

    @staticmethod
    @_in_forward_mode
    def backward(ctx, g, *_stats):
        (x2d, y_a, h_a, y_b, h_b, y_c, sq, u, gate, war, wbr, wcr, ga, ba, gb, bb, gc, mean_a, inv_a, mean_b, inv_b, mean_c, inv_c,
         w1, b1, w2, b2, m2d) = ctx.saved_tensors
        ix, shape, stride, f, need, dev = ctx.ix, ctx.shape, ctx.stride, ctx.f, ctx.needs_input_grad, g.device
        B, _, Hi, Wi, Ho, Wo, W, cout = shape
        P, gw = Ho * Wo, f.group_width
        want_m = need[4]
        go = ops.as_nhwc(g.contiguous()).reshape(-1, cout)                       # [B Ho Wo, cout] = d L / d branch
        zW = torch.zeros(W, device=dev)
        # layer c: through the statistics, no ReLU, then c^T with the plain weights -> d L / d (gate . h_b)
        dyc, ggc, gbc, _ = ops.rows_bn_bwd(go, y_c, None, mean_c, inv_c, gc, m_cap=ix.cap3)
        dz = _conv3_T(dyc, wcr.reshape(cout, 1, W), zW, None, ix.cap3, torch.empty)
        # squeeze-excitation: d gate = sum_p dz . h_b in one kernel (h_b is masked already), the excite MLP by hand on [B, .] tensors
        dgate = ops.rows_img_dot(dz, h_b, ix.pre3, m_cap=ix.cap3)
        dv = dgate * gate * (1.0 - gate)                                         # through the sigmoid
        du = (dv @ w2) * (u > 0)
        dsq = du @ w1
        gw1s = (du.t() @ sq).reshape(ctx.se_shapes[0]) if need[11] else None
        gb1s = du.sum(0) if need[12] else None
        gw2s = (dv.t() @ torch.relu(u)).reshape(ctx.se_shapes[1]) if need[13] else None
        gb2s = dv.sum(0) if need[14] else None
        z = (h_b.view(B, P, W) * gate.unsqueeze(1)).view(ix.cap3, W) if need[3] else None       # conv c's input
        # layer b: d h_b = dz . gate + dsq / P, the mask, the ReLU gate, d gamma, d beta, d mask and the statistics' terms in one op (in place on dz)
        dyb, ggb, gbb, gmb = ops.rows_bn_postmask_bwd(dz, y_b, h_b, mean_b, inv_b, gb, bb, chan_mask=m2d, row_prefix=ix.pre3, gate=gate,
                                                      dsq=(dsq / P).contiguous(), want_mask=want_m, m_cap=ix.cap3, out=dz)
        # b^T: the forward kernel over the transposed neighbour table with the plain per-group transposed weights, scale 1, shift 0, no ReLU
        nbrT = transposed_neighbour_table(ix, B, Hi, Wi, stride, Ho, Wo)
        dha = torch.empty(ix.cap1, W, device=dev)
        _conv_b_adjoint(dyb, nbrT, wbr, gw, dha, ix.cnt[1:2], ix.cap1)
        dya, gga, gba, gma = ops.rows_bn_postmask_bwd(dha, y_a, h_a, mean_a, inv_a, ga, ba, chan_mask=m2d, row_prefix=ix.pre1, want_mask=want_m,
                                                      m_cap=ix.cap1, out=dha)
        grad_x = _grad_x(dya, war, ix, None, shape) if need[0] else None
        gwa, _, gwc = _weight_grads(need[1], False, need[3], dyc, z, None, h_a, dya, x2d, ix, counted=False)
        gwb = None
        if need[2]:                  # conv b sees the MASKED h_a inside the map, zeros in the padding ring
            gwb = _weight_grad_conv_b(dyb, h_a, ix, gw, ix.cnt[0:1])
        gm = gma + gmb if want_m else None
        keep = lambda v, n: v if n else None
        return (grad_x, gwa, gwb, gwc, gm, keep(gga, need[5]), keep(gba, need[6]), keep(ggb, need[7]), keep(gbb, need[8]), keep(ggc, need[9]),
                keep(gbc, need[10]), gw1s, gb1s, gw2s, gb2s, None, None, None, None)


def _update_running_stats(bn, mean, var, n):
    """BatchNorm's own bookkeeping in training mode from the batch statistics of one forward (biased var over n values per channel):
    num_batches_tracked += 1, running = (1 - f) running + f batch with the UNBIASED variance var n / (n - 1), f = momentum or, with
    momentum=None, the cumulative average 1 / num_batches_tracked.  No host read."""
    with torch.no_grad():
        bn.num_batches_tracked += 1
        f = 1.0 / bn.num_batches_tracked.to(torch.float32) if bn.momentum is None else bn.momentum
        bn.running_mean.mul_(1.0 - f).add_(mean * f)
        bn.running_var.mul_(1.0 - f).add_(var * (f * (n / max(n - 1, 1))))


def _batch_stats_branch(block, x, mask):
    """_branch's middle for a LAUD-ResNet block whose BatchNorms are in training mode (USE_BATCH_STATS): -> (branch, ix), running statistics updated"""
    bns = (block.bn1, block.bn2, block.bn3)
    if any(not bn.track_running_stats or bn.running_mean is None for bn in bns):
        raise LdnError("training: batch statistics need track_running_stats=True (running statistics to update)")
    if any(bn.weight is None for bn in bns):
        raise LdnError("training: batch statistics need affine BatchNorm")
    m3 = chm = None
    if block.dyn_mode in ("spatial", "layer"):
        m3 = _spatial_m3(block, x, mask)
    elif block.dyn_mode == "channel":
        chm = _expand_channel_mask(block, x, mask)
    elif block.dyn_mode == "both":
        if not isinstance(mask, (tuple, list)) or len(mask) != 2:
            raise LdnError("training: a dyn_mode 'both' block takes mask = (spatial [B, 1, S, S], channel [B, G]), not a single tensor")
        m3, chm = _spatial_m3(block, x, mask[0]), _expand_channel_mask(block, x, mask[1])
    else:
        raise LdnError(f"training: unknown dyn_mode {block.dyn_mode!r}")
    Ho, Wo = _out_size(block, x)
    # the index lists the block REPORTS are the pixel mask's (block_train reads the dilated masks' means off them); the Fn runs on the dense ones
    ix = _pixel_lists(m3, block.stride) if m3 is not None else None
    dense = dense_index(x.shape[0], Ho, Wo, block.stride, x.device)
    affine = tuple(v for bn in bns for v in (bn.weight, bn.bias))
    branch, *stats = _BatchStatsBranchFn.apply(x, block.conv1.weight, block.conv2.weight, block.conv3.weight, m3, chm, *affine,
                                               tuple(bn.eps for bn in bns), block.stride, dense)
    for bn, mean, var, n in zip(bns, stats[0::2], stats[1::2], (dense.cap1, dense.cap3, dense.cap3)):      # rows = values per channel
        _update_running_stats(bn, mean, var, n)
    return branch, ix if ix is not None else dense


# ------------------------------------------------------------------------------------------------------------------ blocks
def _fold_live(bn):
    """(scale, shift) of a BatchNorm with FROZEN statistics as differentiable functions of its affine parameters."""
    s = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    return s, bn.bias - bn.running_mean * s


def _check_block(block, x):
    """refuses what is not built; -> does the block run on batch statistics (every BatchNorm in training mode, behind USE_BATCH_STATS)?"""
    if block.conv2.groups != 1 or block.conv2.dilation[0] != 1:
        raise LdnError("training: grouped / dilated conv2 is not built")
    if not x.is_cuda:
        raise LdnError("laudnet_amd ops need tensors on a HIP device (cuda:N); there is no CPU path")
    live = [bn.training for bn in (block.bn1, block.bn2, block.bn3)]
    if any(live) and not USE_BATCH_STATS:
        raise LdnError("training: BatchNorm must run on its frozen statistics (norm_eval; call prepare_for_training(model)) -- the "
                       "batch-statistics recipe is dense by construction and trains only behind training.USE_BATCH_STATS (env "
                       "LDN_TRAIN_BATCH_STATS=1, off by default)")
    if not any(live):
        return False
    if block.downsample is not None:      # (the projection shortcut's BatchNorm is a plain module under autograd: it only has to be in the same mode)
        live += [m.training for m in block.downsample.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    if not all(live):
        raise LdnError("training: a block with some BatchNorms in training mode and some frozen is not built (all on batch statistics or all frozen)")
    return True


def _identity(block, x):
    return x if block.downsample is None else block.downsample(x)      # (conv 1x1 stride s + BatchNorm in the block's mode: plain autograd)


def _out_size(block, x):
    return (x.shape[2] - 1) // block.stride + 1, (x.shape[3] - 1) // block.stride + 1


def _spatial_m3(block, x, mask):
    """a block's spatial mask [B, 1, S, S], checked, at the size of the block's output (nearest, laud_resnet.py:106)"""
    if block.masker_spatial.mask_channel_group != 1 or mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[0] != x.shape[0]:
        raise LdnError("training: one spatial mask group ([B, 1, S, S])")
    size = _out_size(block, x)
    return F.interpolate(mask, size=size, mode="nearest") if (mask.shape[2], mask.shape[3]) != size else mask


def _expand_channel_mask(block, x, mask):
    """a block's channel mask [B, G], checked, per channel [B, W]: group j owns channels [j * gran, (j + 1) * gran)"""
    W, gran = block.width, block.channel_dyn_granularity
    if mask.dim() != 2 or mask.shape[0] != x.shape[0] or mask.shape[1] * gran != W:
        raise LdnError("training: channel mask must be [B, G] with G * granularity == width")
    return mask.unsqueeze(2).expand(-1, -1, gran).reshape(mask.shape[0], W)


def _check_regnet_block(block, x):
    """what of LAD-RegNet trains: the layer-skip form run_dynamic executes itself (one keep / skip bit per image, one mask group, SE present) and,
    behind USE_REGNET_CHANNEL, dyn_mode 'channel'; -> does the block run on batch statistics (a channel block with every BatchNorm of the branch
    and of proj in training mode, behind USE_BATCH_STATS as well)?  Some BatchNorms training and some frozen, track_running_stats=False, a
    non-affine BatchNorm and the layer-skip form with a training BatchNorm are refused"""
    f = block.f
    channel = f.dyn_mode == "channel" and USE_REGNET_CHANNEL
    if f.dyn_mode != "spatial" and not channel:
        raise LdnError(f"training: LAD-RegNet dyn_mode {f.dyn_mode!r} is not built (layer skip: dyn_mode 'spatial' with one mask bit per image; "
                       "dyn_mode 'channel' trains behind training.USE_REGNET_CHANNEL, env LDN_TRAIN_REGNET_CHANNEL=1, off by default)")
    if channel:
        if f.w_b % 8 != 0:
            raise LdnError("training: LAD-RegNet channel mode needs a bottleneck width that is a multiple of 8 (as inference does)")
    else:
        if f.mask_size != 1:
            raise LdnError("training: LAD-RegNet patch masks (mask_size > 1) are not built (layer skip only)")
        if f.masker_spatial.mask_channel_group != 1:
            raise LdnError("training: LAD-RegNet spatial mask groups > 1 are not built")
    if not f.has_se:
        raise LdnError("training: LAD-RegNet without squeeze-excitation (RegNet-X) is not built")
    if not x.is_cuda:
        raise LdnError("laudnet_amd ops need tensors on a HIP device (cuda:N); there is no CPU path")
    if x.shape[2] != f.output_size * block.stride or x.shape[3] != f.output_size * block.stride:
        raise LdnError(f"training: input {x.shape[2]}x{x.shape[3]} does not match output_size {f.output_size} * stride {block.stride}")
    bns = (f.a[1], f.b[1], f.c[1])
    live = [bn.training for bn in bns + (() if block.proj is None else (block.proj[1],))]
    if not any(live):
        return False
    if not USE_BATCH_STATS:
        raise LdnError("training: BatchNorm must run on its frozen statistics (norm_eval; call prepare_for_training(model)) -- the "
                       "batch-statistics recipe is dense by construction and not built unless training.USE_BATCH_STATS is on (env "
                       "LDN_TRAIN_BATCH_STATS=1, off by default; LAD-RegNet: dyn_mode 'channel' only)")
    if not channel:
        raise LdnError("training: a LAD-RegNet layer-skip block with a BatchNorm in training mode is not built (batch statistics: dyn_mode "
                       "'channel' only; freeze the statistics with prepare_for_training(model))")
    if not all(live):
        raise LdnError("training: a block with some BatchNorms in training mode and some frozen is not built (all on batch statistics or all frozen)")
    if any(not bn.track_running_stats or bn.running_mean is None for bn in bns):
        raise LdnError("training: batch statistics need track_running_stats=True (running statistics to update)")
    if any(bn.weight is None for bn in bns):
        raise LdnError("training: batch statistics need affine BatchNorm")
    return True


def _branch_regnet(block, x, mask):
    """_branch for a laud_regnet.ResBottleneckBlock: its layer-skip form (mask [B, 1, 1, 1]) or, behind USE_REGNET_CHANNEL, dyn_mode 'channel'
    (mask [B, G], G = w_b // channel_dyn_granularity: the expansion to channels is plain autograd, outside the Fn) -- a channel block on frozen
    statistics, or, with every BatchNorm in training mode and USE_BATCH_STATS on, on batch statistics (the running statistics are updated here)"""
    batch_stats = _check_regnet_block(block, x)
    f = block.f
    w = (f.a[0].weight, f.b[0].weight, f.c[0].weight)
    se = (f.se.fc1.weight, f.se.fc1.bias, f.se.fc2.weight, f.se.fc2.bias)
    if f.dyn_mode == "channel":
        G = f.masker_channel.channel_dyn_group
        if isinstance(mask, (tuple, list)) or mask.dim() != 2 or mask.shape[0] != x.shape[0] or mask.shape[1] != G:
            raise LdnError(f"training: a LAD-RegNet channel block takes one bit per image and channel group (mask [B, {G}])")
        chm = mask.unsqueeze(2).expand(-1, -1, f.w_b // G).reshape(mask.shape[0], f.w_b)      # group j owns channels [j * gran, (j + 1) * gran)
        ix = dense_index(x.shape[0], f.output_size, f.output_size, block.stride, x.device)
        if batch_stats:
            bns = (f.a[1], f.b[1], f.c[1])
            affine = tuple(v for bn in bns for v in (bn.weight, bn.bias))
            branch, *stats = _RegNetBatchStatsBranchFn.apply(x, *w, chm, *affine, *se, tuple(bn.eps for bn in bns), block.stride, f, ix)
            for bn, mean, var, n in zip(bns, stats[0::2], stats[1::2], (ix.cap1, ix.cap3, ix.cap3)):      # rows = values per channel
                _update_running_stats(bn, mean, var, n)
        else:
            bn = _fold_live(f.a[1]) + _fold_live(f.b[1]) + _fold_live(f.c[1])
            branch = _RegNetChannelBranchFn.apply(x, *w, chm, *bn, *se, block.stride, f, ix)
    else:
        bn = _fold_live(f.a[1]) + _fold_live(f.b[1]) + _fold_live(f.c[1])
        if isinstance(mask, (tuple, list)) or mask.dim() != 4 or tuple(mask.shape[1:]) != (1, 1, 1) or mask.shape[0] != x.shape[0]:
            raise LdnError("training: a LAD-RegNet layer-skip block takes one keep / skip bit per image (mask [B, 1, 1, 1])")
        m3 = F.interpolate(mask, size=(f.output_size, f.output_size), mode="nearest")      # laud_regnet.py:173
        ix = _pixel_lists(m3, block.stride)
        branch = _RegNetSkipBranchFn.apply(x, *w, m3, *bn, *se, block.stride, f, ix)
    identity = x if block.proj is None else block.proj(x)      # (conv 1x1 stride s + BatchNorm in the block's mode: plain autograd)
    return F.relu(branch + identity), ix


def _branch(block, x, mask):
    """sparse_block_train -> (out, ix): ix = the index lists the block ran on, built ONCE per forward -- the Fn gets them as an argument and
    block_train reads the dilated masks' means off the same object."""
    if isinstance(block, ResBottleneckBlock):
        return _branch_regnet(block, x, mask)
    if _check_block(block, x):          # every BatchNorm on batch statistics
        branch, ix = _batch_stats_branch(block, x, mask)
        return F.relu(branch + _identity(block, x)), ix
    bn = _fold_live(block.bn1) + _fold_live(block.bn2) + _fold_live(block.bn3)
    w = (block.conv1.weight, block.conv2.weight, block.conv3.weight)
    if block.dyn_mode in ("spatial", "layer"):
        m3 = _spatial_m3(block, x, mask)
        ix = _pixel_lists(m3, block.stride)
        branch = _PixelBranchFn.apply(x, *w, m3, *bn, block.stride, ix)
    elif block.dyn_mode == "channel":
        chm = _expand_channel_mask(block, x, mask)
        ix = dense_index(x.shape[0], *_out_size(block, x), block.stride, x.device)
        branch = _ChannelBranchFn.apply(x, *w, chm, *bn, block.stride, ix)
    elif block.dyn_mode == "both":
        if not isinstance(mask, (tuple, list)) or len(mask) != 2:
            raise LdnError("training: a dyn_mode 'both' block takes mask = (spatial [B, 1, S, S], channel [B, G]), not a single tensor")
        m3, chm = _spatial_m3(block, x, mask[0]), _expand_channel_mask(block, x, mask[1])
        ix = _pixel_lists(m3, block.stride)
        branch = _BothBranchFn.apply(x, *w, m3, chm, *bn, block.stride, ix)
    else:
        raise LdnError(f"training: unknown dyn_mode {block.dyn_mode!r}")
    return F.relu(branch + _identity(block, x)), ix


def sparse_block_train(block, x, mask):
    """Differentiable forward of ONE Bottleneck under frozen BatchNorm statistics with its hard mask as an input.
    dyn_mode 'spatial' / 'layer': mask [B, 1, S, S] {0,1};  dyn_mode 'channel': mask [B, G] {0,1};  dyn_mode 'both': mask = the pair
    (spatial [B, 1, S, S], channel [B, G]).  A mask may require grad (the hard Gumbel sample of the masker's logits): it receives the
    straight-through term.  A `laud_regnet.ResBottleneckBlock` in its layer-skip form (dyn_mode 'spatial', one mask bit per image, SE present):
    mask [B, 1, 1, 1]; with USE_REGNET_CHANNEL on, one in dyn_mode 'channel': mask [B, G] -- on frozen statistics or, with USE_BATCH_STATS on
    too and every BatchNorm of the block in training mode, on the statistics of the batch (the running statistics move once per call); every
    other LAD-RegNet form raises LdnError.  Returns the block's output."""
    return _branch(block, x, mask)[0]


def _gumbel_hard(logits2, temperature):
    """models/utils.py:57,124,162: the hard Gumbel-softmax sample over the (keep, drop) pair, keep component."""
    return F.gumbel_softmax(logits2, dim=1, tau=temperature, hard=True)[:, 0]


def sample_spatial_mask(block, x, temperature):
    """Masker_spatial.forward in training mode (models/utils.py:47-58) as plain autograd ops: -> (mask [B, g, S, S], sparsity, flops)."""
    mk = block.masker_spatial
    ms = mk.mask_size
    pooled = F.adaptive_avg_pool2d(x, ms) if ms < x.shape[2] else x
    flops = pooled.shape[1] * pooled.shape[2] * pooled.shape[3]
    lg = mk.conv(pooled)
    flops += mk.conv_flops_pp * lg.shape[2] * lg.shape[3]
    b, c, h, w = lg.shape
    mask = _gumbel_hard(lg.view(b, 2, c // 2, h, w), temperature)
    return mask, mask.mean(), flops


def sample_channel_mask(block, x, temperature):
    """Masker_channel_MLP / _conv_linear .forward in training mode (models/utils.py:113-127,150-165): -> (mask [B, G], sparsity, flops)."""
    mk = block.masker_channel
    b, c, h, w = x.shape
    if hasattr(mk, "linear"):                       # conv_linear: 1x1 conv + BatchNorm (frozen statistics) + ReLU on the map, GAP, Linear
        y = mk.conv(x)
        flops = y.shape[1] * y.shape[2] * y.shape[3] + mk.masker_flops
        lg = mk.linear(F.adaptive_avg_pool2d(y, (1, 1)).view(b, -1))
    else:
        flops = c * h * w + mk.conv_flops
        lg = mk.conv(F.adaptive_avg_pool2d(x, (1, 1)).view(b, c))
    mask = _gumbel_hard(lg.view(b, 2, lg.shape[1] // 2), temperature)
    return mask, mask.mean(), flops


def _draw_channel(block, x, temperature):
    """the block's channel mask -- forced_channel_mask, else a hard Gumbel sample of its masker -> (mask [B, G], sparsity, flops)"""
    if block.forced_channel_mask is None:
        return sample_channel_mask(block, x, temperature)
    mask = block.forced_channel_mask.to(x.dtype)
    return mask, mask.mean(), block.masker_channel.flops_for(x)


def _draw_spatial(block, x, temperature):
    """the block's spatial mask, likewise -> (mask [B, 1, S, S], sparsity, flops)"""
    if block.forced_spatial_mask is None:
        return sample_spatial_mask(block, x, temperature)
    mask = block.forced_spatial_mask.to(x.dtype)
    return mask, mask.mean(), block.masker_spatial.flops_for(x)


def block_train(block, state, temperature=1.0):
    """Bottleneck.forward of the reference in TRAINING mode (laud_resnet.py:88-165) under frozen BatchNorm statistics: samples the block's hard
    masks from its maskers' logits (forced_*_mask is honoured), runs the convolutions on the row kernels and keeps the reference's bookkeeping
    (sparsity lists, FLOPs ratio, running FLOPs) differentiable where the reference's is (channel sparsity, conv3's spatial sparsity)."""
    if isinstance(block, ResBottleneckBlock):
        return _regnet_block_train(block, state, temperature)
    x, s3l, s2l, s1l, csl, percl, flops = state
    one = lambda: torch.tensor(1.0, device=x.device)
    c_flops = s_flops = 0
    Hi, Wi = x.shape[2], x.shape[3]
    Ho, Wo = _out_size(block, x)
    if block.dyn_mode == "channel":
        cmask, cs, c_flops = _draw_channel(block, x, temperature)
        out, _ = _branch(block, x, cmask)
        s1, s2, s3 = one(), one(), one()
        block.last_channel_mask = cmask.detach()
    elif block.dyn_mode in ("spatial", "layer"):
        m, s3, s_flops = _draw_spatial(block, x, temperature)
        out, ix = _branch(block, x, m)
        # the dilated masks' means (ExpandMask, laud_resnet.py:107-110: thresholded, no gradient) come out of the block's own list build
        s2, s1 = ix.stats[1], ix.stats[2]
        cs = one()
        block.last_spatial_mask = m.detach()
    elif block.dyn_mode == "both":
        # the channel mask is drawn FIRST, then the spatial mask: the reference's order of Gumbel noise (laud_resnet.py:102-103)
        cmask, cs, c_flops = _draw_channel(block, x, temperature)
        m, s3, s_flops = _draw_spatial(block, x, temperature)
        out, ix = _branch(block, x, (m, cmask))
        s2, s1 = ix.stats[1], ix.stats[2]
        block.last_channel_mask, block.last_spatial_mask = cmask.detach(), m.detach()
    else:
        raise LdnError(f"training: unknown dyn_mode {block.dyn_mode!r}")
    W, cin, cout = block.width, block.conv1.in_channels, block.conv3.out_channels
    macs = (cin * W, W * W * 9, W * cout)
    dense = c_flops + s_flops
    sparse = c_flops + s_flops
    dense += macs[0] * Hi * Wi
    sparse = sparse + macs[0] * Hi * Wi * cs * s1
    dense += macs[1] * Ho * Wo
    sparse = sparse + macs[1] * Ho * Wo * cs ** 2 * s2
    dense += macs[2] * Ho * Wo
    sparse = sparse + macs[2] * Ho * Wo * cs * s3
    if block.downsample is not None:
        dsm = cin * cout * Ho * Wo
        dense += dsm
        sparse = sparse + dsm
    flops = flops + sparse
    perc = sparse / dense

    def push(lst, v):
        v = v.reshape(1)
        return v if lst is None else torch.cat((lst, v))
    return out, push(s3l, s3), push(s2l, s2), push(s1l, s1), push(csl, cs), push(percl, perc), flops


def _regnet_block_train(block, state, temperature):
    """ResBottleneckBlock.forward of the reference in TRAINING mode (laud_regnet.py:157-217,272-292).  Layer skip: the keep / skip bits are a hard
    Gumbel sample of the block's masker (forced_spatial_mask is honoured); conv c's sparsity s3 is differentiable, the dilated masks' means come
    out of the list build, channel sparsity 1.  Channel mode (USE_REGNET_CHANNEL): the channel mask likewise (forced_channel_mask is honoured);
    the channel sparsity cs is differentiable, s1 = s2 = s3 = 1 -- on frozen statistics or, behind USE_BATCH_STATS, on the batch's.  The
    bookkeeping is ResBottleneckBlock.forward's."""
    x, s3l, s2l, s1l, csl, percl, flops = state
    f = block.f
    _check_regnet_block(block, x)
    one = lambda: torch.tensor(1.0, device=x.device)
    if f.dyn_mode == "channel":
        cmask, cs, m_flops = _draw_channel(f, x, temperature)
        out, _ = _branch_regnet(block, x, cmask)
        s1, s2, s3 = one(), one(), one()
        f.last_channel_mask = cmask.detach()
    else:
        m, s3, m_flops = _draw_spatial(f, x, temperature)
        out, ix = _branch_regnet(block, x, m)
        s2, s1 = ix.stats[1], ix.stats[2]
        cs = one()
        f.last_spatial_mask = m.detach()
    _, c1, c2, c3, proj, se = block.flops_terms(x.shape)
    dense = m_flops + c1 + c2 + c3 + proj
    sparse = m_flops + c1 * cs * s1
    sparse = sparse + c2 * cs ** 2 * s2
    sparse = sparse + c3 * cs * s3
    sparse = sparse + proj
    flops = flops + se + sparse
    perc = sparse / dense

    def push(lst, v):
        v = v.reshape(1)
        return v if lst is None else torch.cat((lst, v))
    return out, push(s3l, s3), push(s2l, s2), push(s1l, s1), push(csl, cs), push(percl, perc), flops


# ------------------------------------------------------------------------------------------------------------------ models
def prepare_for_training(model, batch_stats=False):
    """Train mode with the BatchNorm STATISTICS frozen (mmdet's norm_eval=True, lad_mmdet_resnet.py:753-758): every BatchNorm runs on its
    running statistics, its affine parameters keep their requires_grad.  batch_stats=True: plain model.train() -- every BatchNorm on the
    statistics of the batch, the reference's ImageNet recipe (behind USE_BATCH_STATS: LAUD-ResNet, and LAD-RegNet in dyn_mode 'channel' with
    USE_REGNET_CHANNEL on as well)."""
    model.train()
    if batch_stats:
        return model
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()
    return model


def _stem(model, x):
    return model.maxpool(model.relu(model.bn1(model.conv1(x))))          # static stem, laud_resnet.py:316-326 (BatchNorm on frozen statistics)


def _regnet_train_forward(model, x, temperature):
    """LAD_RegNet.forward in training mode (laud_regnet.py:573-611): the stem and the head are plain module calls under autograd"""
    cin = x.shape[1]
    h = model.stem(x)
    k = model.stem[0].kernel_size[0]
    flops = torch.tensor(float(cin * h.shape[1] * h.shape[2] * h.shape[3] * k * k), device=x.device)
    percl = None
    stage_stats = []
    for stage in model.trunk_output.children():
        state = (h, None, None, None, None, percl, flops)              # sparsity lists restart per stage, the FLOPs ratios and FLOPs run on
        for blk in stage.children():
            state = block_train(blk, state, temperature)
        h, s3l, s2l, s1l, csl, percl, flops = state
        stage_stats.append((s3l, s2l, s1l, csl))
    h = model.avgpool(h)
    flops = flops + float(h.shape[1] * h.shape[2] * h.shape[3])
    h = h.flatten(start_dim=1)
    flops = flops + float(h.shape[1] * model.fc.out_features)
    s3, s2, s1, cs = ([st[i] for st in stage_stats] for i in range(4))
    return model.fc(h), s3, s2, s1, cs, percl, flops


def train_forward(model, x, temperature=1.0):
    """The reference's forward in training mode on the row kernels.  LAUD-ResNet (`laudnet_amd.ResNet`): -> the 7-tuple (logits, spatial
    sparsity lists of conv3 / conv2 / conv1 per stage, channel sparsity per stage, per-block FLOPs ratios, FLOPs), `laud_resnet.py:312-363`;
    `LAD_MMDet_ResNet`: -> (outs, additional, model_configs), `lad_mmdet_resnet.py:680-751`.  Feed the result to
    `laudnet_amd.sparsity_loss` / the detector's loss as the reference does (`train/main.py:527-604`, `single_stage.py:44-90`)."""
    if not x.is_cuda:
        raise LdnError("laudnet_amd ops need tensors on a HIP device (cuda:N); there is no CPU path")
    if isinstance(model, LAD_RegNet):
        return _regnet_train_forward(model, x, temperature)
    is_det = not hasattr(model, "fc")
    h = _stem(model, x)
    # static terms of the FLOPs count (stem conv + its map; the classifier): the module's own shape-only table
    terms, static = model.flops_table(tuple(x.shape))
    head = float(model._head_flops(model.layer4[-1].conv3.out_channels))
    flops = torch.tensor(float(static) - head, device=x.device)
    percl = None
    stage_stats, outs = [], []
    for s in (1, 2, 3, 4):
        state = (h, None, None, None, None, percl, flops)              # sparsity lists restart per stage, the FLOPs ratios and FLOPs run on (:329-347)
        for blk in getattr(model, f"layer{s}"):
            state = block_train(blk, state, temperature)
        h, s3l, s2l, s1l, csl, percl, flops = state
        stage_stats.append((s3l, s2l, s1l, csl))
        outs.append(h)
    s3, s2, s1, cs = ([st[i] for st in stage_stats] for i in range(4))
    if is_det:
        dense = torch.tensor(float(sum(sum(t) for t in terms)) + float(static), device=x.device)     # shape-only (lad_mmdet_resnet.py:691-695)
        additional = {"spatial_sparsity_conv3": s3, "spatial_sparsity_conv2": s2, "spatial_sparsity_conv1": s1, "channel_sparsity": cs,
                      "flops_perc_list": percl, "flops": flops, "dense_flops": dense}
        return tuple(outs), additional, {"dyn_mode": model.dyn_mode, "sparsity_target": model.sparsity_target}
    y = model.fc(torch.flatten(model.avgpool(h), 1))
    flops = flops + head
    return y, s3, s2, s1, cs, percl, flops
