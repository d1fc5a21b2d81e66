"""LAD-RegNet channel-mode blocks for the training tests: the named block cases, and a float64 restatement of the backward's closed forms
(the equations laudnet_amd/training.py's _RegNetChannelBranchFn and ldn_rows_postmask_bwd / ldn_rows_img_dot implement), written with plain
torch ops so that tests/test_regnet_channel_ref.py can check it against autograd of oracle/regnet_ref.ResBlockRef.  Imports nothing of laudnet_amd.

    h_a = m . relu(s_a a(x) + t_a)      h_b = m . relu(s_b b(h_a) + t_b)      gate = sigmoid(fc2(relu(fc1(mean_p h_b))))
    branch = s_c c(gate . h_b) + t_c    out = relu(branch + identity(x))

The mask multiplies AFTER the ReLU: its straight-through term is sum_p d h . relu(zy), at every channel, and has no shift term."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from fill import fill_state_dict, seeded_bernoulli, seeded_randn

# name -> (width_in, width_out, group width, stride, output size, channel granularity, batch, mask)
CASES = {
    "gw8_s1_g1": (32, 32, 8, 1, 8, 1, 3, "random"),
    "gw16_s2_proj_g2": (32, 64, 16, 2, 4, 2, 3, "random"),
    "gw24_s1_odd_g8": (48, 48, 24, 1, 7, 8, 3, "random"),          # 49 rows per image: the images straddle the row splits
    "gw8_s1_all_on": (32, 32, 8, 1, 8, 1, 3, "ones"),
    "gw8_s1_all_off": (32, 32, 8, 1, 8, 1, 3, "zeros"),
    "gw8_s2_img_off": (32, 32, 8, 2, 4, 1, 3, "img_off"),          # image 0 all zeros, image 1 all ones, image 2 random
}
SE_RATIO = 0.25


def dyn_kw(name):
    S, gran = CASES[name][4], CASES[name][5]
    return dict(spatial_mask_channel_group=1, channel_dyn_granularity=gran, output_size=S, mask_spatial_granularity=S, dyn_mode="channel",
                channel_masker="MLP", channel_masker_layers=2, reduction=16)


def block_args(name):
    win, wout, gw, stride = CASES[name][:4]
    return (win, wout, stride, gw, 1.0, SE_RATIO)


def case_inputs(name, seed=31):
    """-> (x [B, win, S stride, S stride] >= 0, group mask [B, G] {0,1}), fp32 on the CPU"""
    win, wout, _, stride, S, gran, B, kind = CASES[name]
    G = wout // gran
    x = torch.relu(seeded_randn((B, win, S * stride, S * stride), seed + 1))
    m = seeded_bernoulli((B, G), 0.5, seed + 2)
    if kind == "ones":
        m = torch.ones(B, G)
    elif kind == "zeros":
        m = torch.zeros(B, G)
    elif kind == "img_off":
        m[0], m[1] = 0.0, 1.0
    return x, m


def make_ref_block(name, seed=31, variant=None):
    """the oracle's block in eval mode (BatchNorm on its running statistics: frozen) with the seeded state dict -> (block, state dict).
    variant: a BatchNorm scale edit of tests/train_ref.py ("mixed": zero, negated and +-2^-24 weights by channel index) on that state dict"""
    from oracle import regnet_ref as RR
    ref = RR.ResBlockRef(*block_args(name), **dyn_kw(name)).eval()
    sd = fill_state_dict(ref.state_dict(), seed)
    if variant is not None:
        from train_ref import edit_bn_weights
        edit_bn_weights(sd, variant)
    ref.load_state_dict(sd)
    return ref, sd


def start_state(x):
    return (x, None, None, None, None, None, torch.tensor(0.0, device=x.device, dtype=x.dtype))


def _fold(sd, pre):
    inv = torch.rsqrt(sd[pre + ".running_var"].double() + 1e-5)
    s = sd[pre + ".weight"].double() * inv
    return s, sd[pre + ".bias"].double() - sd[pre + ".running_mean"].double() * s, inv, sd[pre + ".running_mean"].double()


def _bn_param_grads(gs, gt, inv, mean):
    """(d weight, d bias) of a BatchNorm on frozen statistics from the gradients of its folded (scale, shift)"""
    return (gs - mean * gt) * inv, gt


def closed_form_f64(name, sd, x, group_mask, gout):
    """Forward and EVERY gradient of the block by the closed forms, in float64 -> (out, d x, d group mask [B, G], {parameter name: gradient})"""
    _, wout, gw, stride, _, gran, B, _ = CASES[name]
    d = lambda k: sd[k].double()
    x, gout = x.double(), gout.double()
    W = wout
    groups = W // gw
    m = group_mask.double().repeat_interleave(gran, dim=1).view(B, W, 1, 1)
    Wa, Wb, Wc = d("f.a.0.weight"), d("f.b.0.weight"), d("f.c.0.weight")
    (sa, ta, ia, ma), (sb, tb, ib, mb), (sc, tc, ic, mc) = _fold(sd, "f.a.1"), _fold(sd, "f.b.1"), _fold(sd, "f.c.1")
    w1, b1 = d("f.se.fc1.weight").flatten(1), d("f.se.fc1.bias")
    w2, b2 = d("f.se.fc2.weight").flatten(1), d("f.se.fc2.bias")
    v = lambda t: t.view(1, -1, 1, 1)
    # forward
    r_a = torch.relu(v(sa) * F.conv2d(x, Wa) + v(ta))
    h_a = m * r_a
    r_b = torch.relu(v(sb) * F.conv2d(h_a, Wb, stride=stride, padding=1, groups=groups) + v(tb))
    h_b = m * r_b
    P = h_b.shape[2] * h_b.shape[3]
    sq = h_b.mean((2, 3))
    u = sq @ w1.t() + b1
    gate = torch.sigmoid(torch.relu(u) @ w2.t() + b2)
    z = gate.view(B, W, 1, 1) * h_b
    yc = F.conv2d(z, Wc)
    has_proj = "proj.0.weight" in sd
    if has_proj:
        Wp = d("proj.0.weight")
        sp, tp, ip, mp = _fold(sd, "proj.1")
        yp = F.conv2d(x, Wp, stride=stride)
        identity = v(sp) * yp + v(tp)
    else:
        identity = x
    pre = v(sc) * yc + v(tc) + identity
    out = torch.relu(pre)
    # backward
    g = gout * (pre > 0)
    grads = {}
    dyc = g * v(sc)
    dz = conv2d_input(z.shape, Wc, dyc)
    grads["f.c.0.weight"] = conv2d_weight(z, Wc.shape, dyc)
    grads["f.c.1.weight"], grads["f.c.1.bias"] = _bn_param_grads((g * yc).sum((0, 2, 3)), g.sum((0, 2, 3)), ic, mc)
    dgate = (dz * r_b).sum((2, 3)) * m.view(B, W)                     # ops.rows_img_dot(dz, r_b) . m
    dv = dgate * gate * (1.0 - gate)
    du = (dv @ w2) * (u > 0)
    dsq = du @ w1
    grads["f.se.fc1.weight"] = (du.t() @ sq).view_as(sd["f.se.fc1.weight"])
    grads["f.se.fc1.bias"] = du.sum(0)
    grads["f.se.fc2.weight"] = (dv.t() @ torch.relu(u)).view_as(sd["f.se.fc2.weight"])
    grads["f.se.fc2.bias"] = dv.sum(0)

    def postmask(dh, r):
        """ldn_rows_postmask_bwd with a scale of ones: -> (a = d L / d (s y + t), g_shift, g_mask [B, W])"""
        a = torch.where(r > 0, dh * m, torch.zeros_like(dh))
        return a, a.sum((0, 2, 3)), (dh * r).sum((2, 3))

    def split_scale(G, Wt, s):
        """training._split_scale: G = a^T A, the weight gradient BEFORE the scale -> (d W = s G, d s = sum G * W): no division by s, which may
        be zero (there relu(s y + t) - t carries nothing of y), tiny or negative"""
        return G * s.view(-1, 1, 1, 1), (G * Wt).sum((1, 2, 3))

    s4 = lambda s: s.view(-1, 1, 1, 1)
    dzb, gtb, gmb = postmask(dz * gate.view(B, W, 1, 1) + dsq.view(B, W, 1, 1) / P, r_b)
    grads["f.b.0.weight"], gsb = split_scale(conv2d_weight(h_a, Wb.shape, dzb, stride=stride, padding=1, groups=groups), Wb, sb)
    grads["f.b.1.weight"], grads["f.b.1.bias"] = _bn_param_grads(gsb, gtb, ib, mb)
    dha = conv2d_input(h_a.shape, Wb * s4(sb), dzb, stride=stride, padding=1, groups=groups)       # b^T reads s_b out of its weights
    dza, gta, gma = postmask(dha, r_a)
    grads["f.a.0.weight"], gsa = split_scale(conv2d_weight(x, Wa.shape, dza), Wa, sa)
    grads["f.a.1.weight"], grads["f.a.1.bias"] = _bn_param_grads(gsa, gta, ia, ma)
    dx = conv2d_input(x.shape, Wa * s4(sa), dza)
    if has_proj:
        dyp = g * v(sp)
        dx = dx + conv2d_input(x.shape, Wp, dyp, stride=stride)
        grads["proj.0.weight"] = conv2d_weight(x, Wp.shape, dyp, stride=stride)
        grads["proj.1.weight"], grads["proj.1.bias"] = _bn_param_grads((g * yp).sum((0, 2, 3)), g.sum((0, 2, 3)), ip, mp)
    else:
        dx = dx + g
    dmask = (gma + gmb).view(B, W // gran, gran).sum(2)
    return out, dx, dmask, grads
