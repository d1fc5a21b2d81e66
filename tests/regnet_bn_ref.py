"""LAD-RegNet channel-mode blocks on BATCH statistics for the training tests: a float64 restatement of ldn_rows_bn_postmask_fwd /
ldn_rows_bn_postmask_bwd on [rows, C] matrices, and of a whole block step built from them (the equations laudnet_amd/training.py's
_RegNetBatchStatsBranchFn implements), written with plain torch ops so that tests/test_regnet_bn_ref.py can check it against autograd of
oracle/regnet_ref.ResBlockRef in .train().  The block cases and their inputs are those of tests/regnet_channel_ref.py.  Imports nothing of
laudnet_amd.

    h_a = m . relu(bn_a(a(x)))      h_b = m . relu(bn_b(b(h_a)))      gate = sigmoid(fc2(relu(fc1(mean_p h_b))))
    branch = bn_c(c(gate . h_b))    out = relu(branch + identity(x))            every bn on the statistics of the batch

The mask multiplies AFTER BatchNorm + ReLU: every channel of every image feeds the statistics, dropped or not, and the mask's straight-through
term is sum_p d h . relu(bn(y)) at every channel -- the unmasked ReLU output, which the stored masked h does not hold."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from regnet_channel_ref import CASES, block_args, case_inputs, dyn_kw, start_state      # noqa: F401  (re-exported for the tests)
from fill import fill_state_dict

EPS = 1e-5
MOMENTUM = 0.1


# ---- the two ops on [n, C] row matrices (n = the rows below the count); img [n] = the image of every row, cm [B, C] the channel mask
def bn_stats(u, eps=EPS):
    """(mean, biased var, invstd) over the rows; no rows: (0, 0, 1 / sqrt(eps))"""
    if u.shape[0] == 0:
        z = torch.zeros(u.shape[1], dtype=u.dtype)
        return z, z.clone(), torch.rsqrt(z + eps)
    mean = u.mean(0)
    var = ((u - mean) ** 2).mean(0)
    return mean, var, torch.rsqrt(var + eps)


def bn_postmask_fwd(u, mean, inv, gamma, beta, cm=None, img=None):
    r = torch.relu(gamma * ((u - mean) * inv) + beta)
    return r if cm is None else r * cm[img]


def bn_postmask_bwd(dz, u, h, mean, inv, gamma, beta, cm=None, img=None, gate=None, dsq=None, B=None):
    """-> (du, d_gamma, d_beta, g_mask [B, C] or None without B).  h is the STORED masked forward output: the ReLU gate is read from it."""
    dh = dz if gate is None else dz * gate[img] + dsq[img]
    xhat = (u - mean) * inv
    a = torch.where(h > 0, dh if cm is None else dh * cm[img], torch.zeros_like(dh))
    r_ = torch.relu(gamma * xhat + beta)
    d_beta, d_gamma = a.sum(0), (a * xhat).sum(0)
    n = max(u.shape[0], 1)
    du = gamma * inv * (a - d_beta / n - xhat * d_gamma / n)
    g_mask = None
    if B is not None:
        g_mask = torch.zeros(B, u.shape[1], dtype=u.dtype).index_add_(0, img, dh * r_)
    return du, d_gamma, d_beta, g_mask


def bn_plain_bwd(dy, u, mean, inv, gamma):
    """BatchNorm without ReLU or mask, through the statistics (layer c, proj) -> (du, d_gamma, d_beta)"""
    xhat = (u - mean) * inv
    d_beta, d_gamma = dy.sum(0), (dy * xhat).sum(0)
    n = max(u.shape[0], 1)
    return gamma * inv * (dy - d_beta / n - xhat * d_gamma / n), d_gamma, d_beta


# ---- a whole block step
def make_ref_block(name, seed=31, variant=None):
    """the oracle's block in TRAINING mode (every BatchNorm on the statistics of the batch) with the seeded state dict -> (block, state dict).
    variant: a BatchNorm scale edit of tests/train_ref.py ("mixed": zero, negated and +-2^-24 weights by channel index) on that state dict"""
    from oracle import regnet_ref as RR
    ref = RR.ResBlockRef(*block_args(name), **dyn_kw(name))
    sd = fill_state_dict(ref.state_dict(), seed)
    if variant is not None:
        from train_ref import edit_bn_weights
        edit_bn_weights(sd, variant)
    ref.load_state_dict(sd)
    return ref.train(), {k: v.clone() for k, v in sd.items()}


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _maps(r, like):
    B, C, H, W = like.shape
    return r.view(B, H, W, C).permute(0, 3, 1, 2)


def _running(sd, pre, mean, var, n):
    """BatchNorm's bookkeeping of one training forward: momentum 0.1, the UNBIASED variance"""
    return ((1 - MOMENTUM) * sd[pre + ".running_mean"].double() + MOMENTUM * mean,
            (1 - MOMENTUM) * sd[pre + ".running_var"].double() + MOMENTUM * var * (n / (n - 1)))


def block_step_f64(name, sd, x, group_mask, gout):
    """Forward and EVERY gradient of the block on batch statistics, in float64 -> (out, d x, d group mask [B, G], {parameter name: gradient},
    {BatchNorm prefix: (batch mean, biased batch var, running_mean after, running_var after)})"""
    _, wout, gw, stride, _, gran, B, _ = CASES[name]
    d = lambda k: sd[k].double()
    x, gout = x.double(), gout.double()
    W = wout
    groups = W // gw
    m = group_mask.double().repeat_interleave(gran, dim=1)                 # [B, W]
    Wa, Wb, Wc = d("f.a.0.weight"), d("f.b.0.weight"), d("f.c.0.weight")
    w1, b1 = d("f.se.fc1.weight").flatten(1), d("f.se.fc1.bias")
    w2, b2 = d("f.se.fc2.weight").flatten(1), d("f.se.fc2.bias")
    aff = lambda pre: (d(pre + ".weight"), d(pre + ".bias"))
    (ga, ba), (gb, bb), (gc, bc) = aff("f.a.1"), aff("f.b.1"), aff("f.c.1")
    img_of = lambda t: torch.arange(B).repeat_interleave(t.shape[2] * t.shape[3])
    stats = {}

    def note(pre, u, mean, var):
        stats[pre] = (mean, var) + _running(sd, pre, mean, var, u.shape[0])

    # forward
    ya = F.conv2d(x, Wa)
    ua, img1 = _rows(ya), img_of(ya)
    mean_a, var_a, inv_a = bn_stats(ua)
    note("f.a.1", ua, mean_a, var_a)
    ha_r = bn_postmask_fwd(ua, mean_a, inv_a, ga, ba, m, img1)
    h_a = _maps(ha_r, ya)
    yb = F.conv2d(h_a, Wb, stride=stride, padding=1, groups=groups)
    ub, img3 = _rows(yb), img_of(yb)
    mean_b, var_b, inv_b = bn_stats(ub)
    note("f.b.1", ub, mean_b, var_b)
    hb_r = bn_postmask_fwd(ub, mean_b, inv_b, gb, bb, m, img3)
    h_b = _maps(hb_r, yb)
    P = h_b.shape[2] * h_b.shape[3]
    sq = h_b.mean((2, 3))
    u = sq @ w1.t() + b1
    gate = torch.sigmoid(torch.relu(u) @ w2.t() + b2)
    z = gate.view(B, W, 1, 1) * h_b
    yc = F.conv2d(z, Wc)
    uc = _rows(yc)
    mean_c, var_c, inv_c = bn_stats(uc)
    note("f.c.1", uc, mean_c, var_c)
    branch = _maps(gc * ((uc - mean_c) * inv_c) + bc, yc)
    has_proj = "proj.0.weight" in sd
    if has_proj:
        Wp = d("proj.0.weight")
        gp, bp = aff("proj.1")
        yp = F.conv2d(x, Wp, stride=stride)
        up = _rows(yp)
        mean_p, var_p, inv_p = bn_stats(up)
        note("proj.1", up, mean_p, var_p)
        identity = _maps(gp * ((up - mean_p) * inv_p) + bp, yp)
    else:
        identity = x
    pre = branch + identity
    out = torch.relu(pre)
    # backward
    g = gout * (pre > 0)
    grads = {}
    dyc_r, grads["f.c.1.weight"], grads["f.c.1.bias"] = bn_plain_bwd(_rows(g), uc, mean_c, inv_c, gc)
    dyc = _maps(dyc_r, yc)
    dz = conv2d_input(z.shape, Wc, dyc)
    grads["f.c.0.weight"] = conv2d_weight(z, Wc.shape, dyc)
    dgate = (dz * h_b).sum((2, 3))                                     # ops.rows_img_dot(dz, h_b): h_b is masked already
    dv = dgate * gate * (1.0 - gate)
    du = (dv @ w2) * (u > 0)
    dsq = du @ w1
    grads["f.se.fc1.weight"] = (du.t() @ sq).view_as(sd["f.se.fc1.weight"])
    grads["f.se.fc1.bias"] = du.sum(0)
    grads["f.se.fc2.weight"] = (dv.t() @ torch.relu(u)).view_as(sd["f.se.fc2.weight"])
    grads["f.se.fc2.bias"] = dv.sum(0)
    dyb_r, grads["f.b.1.weight"], grads["f.b.1.bias"], gmb = bn_postmask_bwd(_rows(dz), ub, hb_r, mean_b, inv_b, gb, bb, m, img3, gate, dsq / P, B)
    dyb = _maps(dyb_r, yb)
    grads["f.b.0.weight"] = conv2d_weight(h_a, Wb.shape, dyb, stride=stride, padding=1, groups=groups)
    dha = conv2d_input(h_a.shape, Wb, dyb, stride=stride, padding=1, groups=groups)
    dya_r, grads["f.a.1.weight"], grads["f.a.1.bias"], gma = bn_postmask_bwd(_rows(dha), ua, ha_r, mean_a, inv_a, ga, ba, m, img1, B=B)
    dya = _maps(dya_r, ya)
    grads["f.a.0.weight"] = conv2d_weight(x, Wa.shape, dya)
    dx = conv2d_input(x.shape, Wa, dya)
    if has_proj:
        dyp_r, grads["proj.1.weight"], grads["proj.1.bias"] = bn_plain_bwd(_rows(g), up, mean_p, inv_p, gp)
        dyp = _maps(dyp_r, yp)
        dx = dx + conv2d_input(x.shape, Wp, dyp, stride=stride)
        grads["proj.0.weight"] = conv2d_weight(x, Wp.shape, dyp, stride=stride)
    else:
        dx = dx + g
    dmask = (gma + gmb).view(B, W // gran, gran).sum(2)
    return out, dx, dmask, grads, stats
