"""The channel algebra (`laudnet_amd._shared.channel_constants`) against its DEFINITION: a masked channel of conv1's output is
the constant c1 = relu(t1), so conv2 + BN of a map filled with c1 is, at every pixel, one of 16 image-independent vectors -- one per
border class (which taps fall into the zero padding).  The reference is F.conv2d in float64; all inputs are small integers, so every
product and sum is exact in float32 as well and the comparison is equality."""
import torch
import torch.nn.functional as F

from laudnet_amd._shared import channel_constants

W, COUT = 8, 12


def _int_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    w2, w3 = ri(-3, 3, W, W, 3, 3), ri(-3, 3, COUT, W)
    s2, t2, t1, s3, t3 = ri(-4, 4, W), ri(-4, 4, W), ri(-4, 4, W), ri(-4, 4, COUT), ri(-4, 4, COUT)
    t1[0], t1[1], t2[0], t2[1] = -3.0, 2.0, -2.0, 4.0          # both signs for certain: the ReLU matters
    return w2, w3, s2, t2, t1, s3, t3


def test_channel_constants_match_the_definition():
    w2, w3, s2, t2, t1, s3, t3 = _int_inputs()
    c1, c2, tab, t3c = channel_constants(w2, w3, s2, t2, t1, s3, t3)
    assert tab.shape == (16, W) and tab.dtype == torch.float32
    assert (t1 < 0).any() and (t1 > 0).any() and (t2 < 0).any() and (t2 > 0).any()
    assert torch.equal(c1, torch.relu(t1)) and torch.equal(c2, torch.relu(t2))
    d = lambda t: t.double()
    seen = set()
    for H, Wd in ((1, 1), (1, 4), (4, 1), (4, 4)):
        c1_map = d(torch.relu(t1)).view(1, W, 1, 1).expand(1, W, H, Wd)
        want = d(t2).view(1, W, 1, 1) + d(s2).view(1, W, 1, 1) * F.conv2d(c1_map, d(w2), padding=1, stride=1)
        for y in range(H):
            for x in range(Wd):
                rb = (1 if y == 0 else 0) | (2 if y == H - 1 else 0)
                cb = (1 if x == 0 else 0) | (2 if x == Wd - 1 else 0)
                cls = 4 * rb + cb
                seen.add(cls)
                assert torch.equal(d(tab[cls]), want[0, :, y, x]), (H, Wd, y, x, cls)
    assert seen == set(range(16))
    assert torch.equal(d(t3c), d(t3) + d(s3) * (d(w3) @ d(torch.relu(t2))))


def test_prepare_uses_channel_constants():
    """Bottleneck._prepare folds with plain torch: on the CPU-resident parameters it returns what a direct call gives."""
    from laudnet_amd.laud_resnet import Bottleneck, _fold_bn

    torch.manual_seed(1)
    blk = Bottleneck(16, 4, dyn_mode="channel", channel_masker="MLP", channel_dyn_granularity=2, output_size=8).eval()
    with torch.no_grad():
        for bn in (blk.bn1, blk.bn2, blk.bn3):
            bn.weight.normal_()
            bn.bias.normal_()
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
        p = blk._prepare(torch.device("cpu"))
        (_, t1), (s2, t2), (s3, t3) = (_fold_bn(bn) for bn in (blk.bn1, blk.bn2, blk.bn3))
        want = channel_constants(blk.conv2.weight.float(), blk.conv3.weight.float(), s2, t2, t1, s3, t3)
    assert (t1 < 0).any() and (t2 < 0).any()
    for key, w in zip(("c1", "c2", "t2_tab", "t3c"), want):
        assert torch.equal(p[key], w), key
