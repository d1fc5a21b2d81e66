"""Training of dyn_mode 'both' blocks (pixel x channel masks on packed rows: laudnet_amd.training._BothBranchFn on ops.rows_chanmask /
ops.rows_act_bwd) against the ORACLE's autograd (oracle/torch_ref.py runs 'both' in training mode: channel mask first, then the spatial mask).

Blocks: the reference-generated fixtures `both_s1` / `both_s2` with BOTH injected masks requiring grad -- forward and every gradient (x, the
three conv weights, the six BatchNorm vectors, the projection, d spatial_mask, d channel_mask), both arithmetic modes, the criteria of
tests/test_hip_training.py::_close (imported: plain 1e-3 in fp32, its stated flip allowance in bf16x3).  Full-width blocks (stage-3 identity
block cin 1024 / width 256 / 14 x 14 / B 4; stride-2 projection block cin 512 / width 256 / 28 -> 14 / B 2): fp32 math, seeded masks.  Whole
models `full_tiny.pt::r50_both` / `::r50_mixed` through prepare_for_training / train_forward with the oracle's Gumbel noise: the loss and
the checks of test_classifier_train_step_vs_oracle."""
import pytest
import torch

from fill import fill_state_dict, seeded_bernoulli, seeded_randn
from helpers import block_input, load_golden, make_block
from test_hip_training import BLOCKS, GumbelTape, _close, _compare_param_grads, _err, _freeze_bn_train, _start, oracle_cpu_grads

DEV = "cuda:0"


def _block_case(fx, x0, sm0, cm0, math_mode):
    from laudnet_amd.laud_resnet import Bottleneck
    from laudnet_amd.training import sparse_block_train
    from oracle import torch_ref as TR
    hip = make_block(Bottleneck, fx).to(DEV)
    ref = make_block(TR.BottleneckRef, fx).to(DEV)              # eval mode: BatchNorm uses its running statistics (frozen)
    xr, smr, cmr = (t.clone().requires_grad_(True) for t in (x0, sm0, cm0))
    ref.forced_spatial_mask, ref.forced_channel_mask = smr, cmr
    for p_ in ref.parameters():
        p_.requires_grad_(True)
    out_r = ref(_start(xr), 1.0)[0]
    gout = seeded_randn(tuple(out_r.shape), 77).to(DEV)
    out_r.backward(gout)

    xh, smh, cmh = (t.clone().requires_grad_(True) for t in (x0, sm0, cm0))
    for p_ in hip.parameters():
        p_.requires_grad_(True)
    out_h = sparse_block_train(hip, xh, (smh, cmh))
    out_h.backward(gout)
    torch.cuda.synchronize()

    assert _err(out_h.detach(), out_r.detach()) < 1e-3, "forward"
    _close(xh.grad, xr.grad, math_mode, "d x")
    _close(smh.grad, smr.grad, math_mode, "straight-through term d spatial_mask")
    _close(cmh.grad, cmr.grad, math_mode, "straight-through term d channel_mask")
    ref_grads = dict(ref.named_parameters())
    checked = 0
    for pname, ph in hip.named_parameters():
        if "masker" in pname:
            continue                                             # (the masks are inputs here: the maskers are not part of the graph)
        want = ref_grads[pname].grad
        assert ph.grad is not None and want is not None, pname
        _close(ph.grad, want, math_mode, f"d {pname}")
        checked += 1
    assert checked >= 9 + (2 if fx["has_downsample"] else 0)     # three convs, three BatchNorms (weight + bias) [+ the projection]
    assert (sm0 < 0.5).any() and (cm0 < 0.5).any(), "the case must drop pixels AND channels"
    assert smr.grad.abs().max().item() > 0 and cmr.grad.abs().max().item() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["both_s1", "both_s2"])
def test_both_block_gradients_vs_oracle_autograd(name, math_mode):
    from laudnet_amd import ops
    ops.set_math_mode(math_mode)
    try:
        fx = BLOCKS[name]
        _block_case(fx, block_input(fx).to(DEV), fx["spatial_mask"].float().to(DEV), fx["channel_mask"].float().to(DEV), math_mode)
    finally:
        ops.set_math_mode("fp32")


FULL_WIDTH = {
    "stage3_identity": dict(inplanes=1024, planes=256, stride=1, x_shape=[4, 1024, 14, 14], has_downsample=False),
    "stage3_stride2_projection": dict(inplanes=512, planes=256, stride=2, x_shape=[2, 512, 28, 28], has_downsample=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FULL_WIDTH))
def test_both_full_width_block_vs_oracle(name):
    from laudnet_amd import ops
    ops.set_math_mode("fp32")
    cfg = FULL_WIDTH[name]
    kw = dict(inplanes=cfg["inplanes"], planes=cfg["planes"], stride=cfg["stride"], spatial_mask_channel_group=1, channel_dyn_granularity=2,
              output_size=14, mask_spatial_granularity=2, dyn_mode="both", channel_masker="MLP", channel_masker_layers=2, reduction=16)
    fx = dict(kw=kw, seed=901, x_seed=902, x_shape=cfg["x_shape"], has_downsample=cfg["has_downsample"])
    Bn = cfg["x_shape"][0]
    sm0 = seeded_bernoulli((Bn, 1, 7, 7), 0.5, 903).float().to(DEV)
    cm0 = seeded_bernoulli((Bn, cfg["planes"] // 2), 0.62, 904).float().to(DEV)
    _block_case(fx, block_input(fx).to(DEV), sm0, cm0, "fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["r50_both", "r50_mixed"])
def test_both_classifier_train_step_vs_oracle(case):
    """test_hip_training.py::test_classifier_train_step_vs_oracle on the models with 'both' stages: same loss, same checks."""
    from laudnet_amd import ops, sparsity_loss  # noqa: F401
    import laudnet_amd
    from laudnet_amd.training import prepare_for_training, train_forward
    from oracle import torch_ref as TR
    ops.set_math_mode("fp32")
    fx = load_golden("full_tiny.pt")[case]
    depth = 101 if "101" in fx["factory"] else 50
    ref = (TR.resnet101_ref if depth == 101 else TR.resnet50_ref)(**fx["kw"])
    hip = (laudnet_amd.uni_resnet101 if depth == 101 else laudnet_amd.uni_resnet50)(**fx["kw"])
    assert "both" in fx["kw"]["dyn_mode"]
    sd = fill_state_dict(ref.state_dict(), fx["seed"])
    for k in sd:
        if k.endswith("bn3.weight"):
            sd[k] = sd[k] * 0.3                                   # damped residual branches: O(1) activations through the blocks
    ref.load_state_dict(sd)
    hip.load_state_dict(sd)
    ref, hip = _freeze_bn_train(ref.to(DEV)), prepare_for_training(hip.to(DEV))
    x = seeded_randn((fx["batch"], 3, 224, 224), fx["x_seed"]).to(DEV)
    g = seeded_randn((fx["batch"], fx["kw"].get("num_classes", 1000)), 9).to(DEV)

    def loss_of(out):
        return (out[0] * g.to(out[0].device)).sum() / 10.0 + 10.0 * (out[5].mean() - 0.5) ** 2 + 1e-18 * out[6] ** 2

    tape = GumbelTape()
    torch.manual_seed(77)
    with tape.record():
        out_r = ref(x, 1.0)
    loss_of(out_r).backward()
    torch.manual_seed(77)
    out_h = train_forward(hip, x, 1.0)
    loss_of(out_h).backward()
    torch.cuda.synchronize()
    assert _err(out_h[0].detach(), out_r[0].detach()) < 1e-3, "logits"
    for i in (1, 2, 3, 4):
        for a, b in zip(out_h[i], out_r[i]):
            assert torch.allclose(a.detach().float(), b.detach().float(), atol=1e-6), i
    assert torch.allclose(out_h[5].detach(), out_r[5].detach(), atol=1e-5)
    assert abs(float(out_h[6]) - float(out_r[6])) <= 1e-5 * float(out_r[6])
    cpu_grads = oracle_cpu_grads(ref, tape, lambda m, dev: loss_of(m(x.to(dev), 1.0)).backward())
    n = _compare_param_grads(hip, ref, cpu_grads=cpu_grads, what=f"full_tiny.pt::{case}")
    assert n >= 200, n
    both = [b for s in (1, 2, 3, 4) for b in getattr(hip, f"layer{s}") if b.dyn_mode == "both"]
    assert both and all(getattr(b, "last_channel_mask", None) is not None and getattr(b, "last_spatial_mask", None) is not None for b in both)


@pytest.mark.gpu
def test_both_mask_pair_is_checked():
    from laudnet_amd import LdnError
    from laudnet_amd.laud_resnet import Bottleneck
    from laudnet_amd.training import sparse_block_train
    fx = BLOCKS["both_s1"]
    blk = make_block(Bottleneck, fx).to(DEV)
    x = block_input(fx).to(DEV)
    sm, cm = fx["spatial_mask"].float().to(DEV), fx["channel_mask"].float().to(DEV)
    with pytest.raises(LdnError):                                # a channel mask of the wrong width
        sparse_block_train(blk, x, (sm, cm[:, :-1]))
    with pytest.raises(LdnError):                                # the pair the wrong way round
        sparse_block_train(blk, x, (cm, sm))
    assert sparse_block_train(blk, x, (sm, cm)).shape[0] == x.shape[0]
