"""Float64 restatement of BatchNorm on BATCH statistics over packed rows with the reference's masks -- the equations ldn_rows_bn_stats,
ldn_rows_bn_fwd and ldn_rows_bn_bwd (csrc/ldn_train_bn.hip) implement and laudnet_amd/training.py's _BatchStatsBranchFn chains -- written with
plain tensor ops, no autograd.  tests/test_bn_batch_ref.py ties it to torch.nn.functional.batch_norm(training=True) autograd and to
oracle.torch_ref.BottleneckRef in .train(); the GPU tests compare the kernels with it.

Rows are [n, C] matrices; `chan_mask` [B, C] with `img` [n] (the image of every row) is the channel mask applied to u BEFORE the statistics and
the normalisation; `row_scale` [n] is the pixel mask on the output."""
import torch
import torch.nn.functional as F


def _x(u, chan_mask, img):
    return u if chan_mask is None else u * chan_mask[img]


def bn_stats(u, eps, chan_mask=None, img=None):
    """-> (mean, biased var, invstd) [C] of x = chan_mask[img] * u over all rows; no rows: (0, 0, 1 / sqrt(eps))"""
    x = _x(u.double(), chan_mask, img)
    if x.shape[0] == 0:
        z = torch.zeros(x.shape[1], dtype=torch.float64)
        return z, z.clone(), torch.full_like(z, eps) ** -0.5
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, (var + eps) ** -0.5


def bn_fwd(u, mean, invstd, gamma, beta, chan_mask=None, img=None, row_scale=None, relu=True):
    z = gamma * ((_x(u.double(), chan_mask, img) - mean) * invstd) + beta
    h = torch.relu(z) if relu else z
    return h if row_scale is None else h * row_scale.double().unsqueeze(1)


def bn_bwd(dh, u, h, mean, invstd, gamma, chan_mask=None, img=None, row_scale=None, B=None):
    """-> (du, d_gamma, d_beta, g_mask [B, C] or None).  h: the stored forward output (the ReLU gate is h > 0), None = no ReLU."""
    u = u.double()
    xhat = (_x(u, chan_mask, img) - mean) * invstd
    dz = dh.double() if h is None else dh.double() * (h > 0)
    if row_scale is not None:
        dz = dz * row_scale.double().unsqueeze(1)
    n = max(u.shape[0], 1)
    d_beta, d_gamma = dz.sum(0), (dz * xhat).sum(0)
    g = gamma * invstd * (dz - d_beta / n - xhat * d_gamma / n)
    g_mask = None
    if B is not None:
        g_mask = torch.zeros(B, u.shape[1], dtype=torch.float64).index_add_(0, img, g * u)
    return (g if chan_mask is None else g * chan_mask[img]), d_gamma, d_beta, g_mask


def _rows(t):
    """NCHW -> ([B H W, C] rows, image of every row)"""
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(-1, C), torch.arange(B).repeat_interleave(H * W)


def _nchw(rows, B, H, W):
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


def block_step(blk, x, gout, m3=None, chm=None):
    """One training step of a LAUD-ResNet bottleneck on batch statistics by hand, float64 (blk: any module with conv1..3 / bn1..3 / downsample /
    stride in .double(); m3 [B, 1, Ho, Wo] or None; chm [B, W] per CHANNEL or None; gout = d L / d out):
        out = relu(identity(x) + m3 * bn3(conv3(relu(bn2(c . conv2(relu(bn1(c . conv1(x)))))))))
    -> (out, {gradients of x, conv1..3.weight, bn1..3.weight / .bias, m3, chm}, [(batch mean, biased var, n)] x 3).  The convolutions and the
    shortcut are torch's; every BatchNorm of the branch is the three functions above."""
    x = x.double()
    w1, w2, w3 = (c.weight.detach().double() for c in (blk.conv1, blk.conv2, blk.conv3))
    s = blk.stride
    B = x.shape[0]
    cm = None if chm is None else chm.double()
    y1 = F.conv2d(x, w1)
    r1, img1 = _rows(y1)
    st1 = bn_stats(r1, blk.bn1.eps, cm, img1)
    h1 = bn_fwd(r1, st1[0], st1[2], blk.bn1.weight.detach().double(), blk.bn1.bias.detach().double(), cm, img1)
    h1n = _nchw(h1, B, *y1.shape[2:])
    y2 = F.conv2d(h1n, w2, stride=s, padding=1)
    Ho, Wo = y2.shape[2:]
    r2, img3 = _rows(y2)
    st2 = bn_stats(r2, blk.bn2.eps, cm, img3)
    h2 = bn_fwd(r2, st2[0], st2[2], blk.bn2.weight.detach().double(), blk.bn2.bias.detach().double(), cm, img3)
    h2n = _nchw(h2, B, Ho, Wo)
    y3 = F.conv2d(h2n, w3)
    r3, _ = _rows(y3)
    st3 = bn_stats(r3, blk.bn3.eps)
    g3 = blk.bn3.weight.detach().double()
    z3 = bn_fwd(r3, st3[0], st3[2], g3, blk.bn3.bias.detach().double(), relu=False)
    rs = None if m3 is None else m3.double().reshape(-1)
    br = z3 if rs is None else z3 * rs.unsqueeze(1)
    xi = x.clone().requires_grad_(True)                      # the shortcut (identity or conv + BatchNorm in its own mode): torch's autograd
    idn = xi if blk.downsample is None else blk.downsample(xi)
    pre = _nchw(br, B, Ho, Wo) + idn
    out = torch.relu(pre).detach()
    gpre = gout.double() * (pre.detach() > 0)
    gx_short, = torch.autograd.grad(idn, xi, gpre, allow_unused=True) if blk.downsample is not None else (gpre,)
    go, _ = _rows(gpre)
    grads = {}
    if m3 is not None:
        grads["m3"] = (go * z3).sum(1).view(B, 1, Ho, Wo)
    dy3, grads["bn3.weight"], grads["bn3.bias"], _ = bn_bwd(go, r3, None, st3[0], st3[2], g3, row_scale=rs)
    dy3n = _nchw(dy3, B, Ho, Wo)
    grads["conv3.weight"] = torch.nn.grad.conv2d_weight(h2n, w3.shape, dy3n)
    dh2, _ = _rows(torch.nn.grad.conv2d_input(h2n.shape, w3, dy3n))
    dy2, grads["bn2.weight"], grads["bn2.bias"], gc2 = bn_bwd(dh2, r2, h2, st2[0], st2[2], blk.bn2.weight.detach().double(), cm, img3,
                                                               B=None if cm is None else B)
    dy2n = _nchw(dy2, B, Ho, Wo)
    grads["conv2.weight"] = torch.nn.grad.conv2d_weight(h1n, w2.shape, dy2n, stride=s, padding=1)
    dh1, _ = _rows(torch.nn.grad.conv2d_input(h1n.shape, w2, dy2n, stride=s, padding=1))
    dy1, grads["bn1.weight"], grads["bn1.bias"], gc1 = bn_bwd(dh1, r1, h1, st1[0], st1[2], blk.bn1.weight.detach().double(), cm, img1,
                                                               B=None if cm is None else B)
    dy1n = _nchw(dy1, B, *y1.shape[2:])
    grads["conv1.weight"] = torch.nn.grad.conv2d_weight(x, w1.shape, dy1n)
    grads["x"] = torch.nn.grad.conv2d_input(x.shape, w1, dy1n) + gx_short
    if cm is not None:
        grads["chm"] = gc1 + gc2
    stats = [(st1[0], st1[1], r1.shape[0]), (st2[0], st2[1], r2.shape[0]), (st3[0], st3[1], r3.shape[0])]
    return out, grads, stats
