"""Training of LAUD-ResNet blocks with BatchNorm on BATCH statistics (laudnet_amd.training._BatchStatsBranchFn on ops.rows_bn_stats / rows_bn_fwd /
rows_bn_bwd, behind training.USE_BATCH_STATS) against the ORACLE's autograd with its BatchNorms in .train() -- the reference's own ImageNet recipe
(train_scripts.sh, train/main.py:527-604).

Blocks: the ten TRAIN_BLOCKS of tests/test_hip_training.py (spatial, layer, channel; stride 1 and stride 2 + projection) and the `both` block
`both_s2` (pixel x channel masks, stride 2 + projection), both arithmetic modes, the injected masks requiring grad.  Compared: the output; the
gradients of x, of the three convolutions, of all six BatchNorm affine vectors (and the projection's), of the masks -- bounds: _close of
tests/test_hip_training.py (fp32: every element within 1e-3; bf16x3: its stated flip allowance); running_mean / running_var /
num_batches_tracked of EVERY BatchNorm after the step at 1e-5.  The `both` block is blocks_s2.pt's: the two of blocks_extra.pt have two spatial
mask groups, which stay refused in this mode as in the others (asserted below).
Running statistics: forward + backward moves them once, a second forward once more; momentum=None is the cumulative average.
bn3.weight == 0: d bn3.weight is non-zero and right.  Classifiers: one step of full_tiny.pt::r101_channel2222 / ::r101_layer in plain
model.train() with the oracle's Gumbel noise, fp32, the harness and bounds of test_classifier_train_step_vs_oracle -- with every bn3.weight
damped by 0.03 instead of 0.3, because at 0.3 the oracle's own float32 step misses those bounds against its float64 step (RESIDUAL_DAMPING
below has the figures; measured on the GPU at 0.03: 446 of 446 and 222 of 227 gradients eligible for the relative check).  Switch off: a
training-mode BatchNorm is refused and the message names LDN_TRAIN_BATCH_STATS."""
import pytest
import torch

from fill import fill_state_dict, seeded_randn
from helpers import apply_math_mode, block_input, load_golden, make_block  # noqa: F401  (apply_math_mode: autouse)
from test_hip_training import BLOCKS, TRAIN_BLOCKS, GumbelTape, _close, _compare_param_grads, _err, _start, oracle_cpu_grads

DEV = "cuda:0"
# The classifier harness damps every bn3.weight so that one step through 33 blocks is well conditioned.  Under frozen statistics 0.3 does that; on
# batch statistics it does not: every BatchNorm's backward multiplies by gamma * invstd, and with the seeded fill the ORACLE'S OWN float32 step then
# disagrees with its float64 step (CPU, the maskers' decisions without noise) by more than 2.5e-4 of a gradient's scale on 106 of 227 tensors
# (r101_layer; gradients down to 9e-19) and 418 of 446 (r101_channel2222; gradients up to 1e31) -- no fp32 implementation can be held to the
# bounds there.  At 0.03 it is 59 of 227 and 4 of 446 (gradients up to 5e13).  Everything else is test_classifier_train_step_vs_oracle's.
RESIDUAL_DAMPING = 0.03
BS_BLOCKS = TRAIN_BLOCKS + ["both_s2"]


def _masks(fx):
    mode = fx["kw"]["dyn_mode"]
    sm = fx["spatial_mask"].float().to(DEV) if mode != "channel" else None
    cm = fx["channel_mask"].float().to(DEV) if mode in ("channel", "both") else None
    return sm, cm


def _pair(fx, edit=None):
    """(hip block, oracle block), both in plain .train() with the same parameters; edit(module) is applied to both"""
    from laudnet_amd.laud_resnet import Bottleneck
    from oracle import torch_ref as TR
    hip, ref = make_block(Bottleneck, fx).to(DEV).train(), make_block(TR.BottleneckRef, fx).to(DEV).train()
    for m in (hip, ref):
        if edit is not None:
            with torch.no_grad():
                edit(m)
        for p_ in m.parameters():
            p_.requires_grad_(True)
    return hip, ref


def _buffers_close(hip, ref, what):
    """running_mean / running_var / num_batches_tracked of every BatchNorm outside the maskers, at 1e-5"""
    want, n = dict(ref.named_buffers()), 0
    for name, b in hip.named_buffers():
        if "masker" in name or name.rsplit(".", 1)[-1] not in ("running_mean", "running_var", "num_batches_tracked"):
            continue
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(want[name]), f"{what}: {name} {int(b)} vs {int(want[name])}"
        else:
            assert torch.allclose(b, want[name], atol=1e-5, rtol=1e-5), f"{what}: {name} differs by {(b - want[name]).abs().max().item():.2e}"
        n += 1
    return n


def _step(hip, ref, fx, math_mode, what):
    """one forward + backward of both with the fixture's masks as differentiable inputs; compares everything; -> (out_h, xh, hip masks)"""
    from laudnet_amd.training import sparse_block_train
    x0 = block_input(fx).to(DEV)
    sm0, cm0 = _masks(fx)
    xr = x0.clone().requires_grad_(True)
    smr, cmr = (None if t is None else t.clone().requires_grad_(True) for t in (sm0, cm0))
    ref.forced_spatial_mask, ref.forced_channel_mask = smr, cmr
    out_r = ref(_start(xr), 1.0)[0]
    gout = seeded_randn(tuple(out_r.shape), 77).to(DEV)
    out_r.backward(gout)

    xh = x0.clone().requires_grad_(True)
    smh, cmh = (None if t is None else t.clone().requires_grad_(True) for t in (sm0, cm0))
    mask = (smh, cmh) if fx["kw"]["dyn_mode"] == "both" else (smh if smh is not None else cmh)
    out_h = sparse_block_train(hip, xh, mask)
    out_h.backward(gout)
    torch.cuda.synchronize()

    print(f"{what}: forward err {_err(out_h.detach(), out_r.detach()):.2e}, d x err {_err(xh.grad, xr.grad):.2e}")
    assert _err(out_h.detach(), out_r.detach()) < 1e-3, f"{what}: forward"
    _close(xh.grad, xr.grad, math_mode, f"{what}: d x")
    for gh, gr, name in ((smh, smr, "spatial"), (cmh, cmr, "channel")):
        if gh is not None:
            assert (gr.detach() < 0.5).any() and gr.grad.abs().max().item() > 0, f"{what}: the {name} mask must drop units and receive a gradient"
            _close(gh.grad, gr.grad, math_mode, f"{what}: straight-through term d {name}_mask")
    want = dict(ref.named_parameters())
    checked = 0
    for pname, ph in hip.named_parameters():
        if "masker" in pname:
            continue                                             # (the masks are inputs here: the maskers are not part of the graph)
        assert ph.grad is not None and want[pname].grad is not None, pname
        _close(ph.grad, want[pname].grad, math_mode, f"{what}: d {pname}")
        checked += 1
    assert checked >= 9 + (2 if fx["has_downsample"] else 0)     # three convs, three BatchNorms (weight + bias) [+ the projection]
    assert _buffers_close(hip, ref, what) >= 9 + (3 if fx["has_downsample"] else 0)
    return out_h, hip, ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", BS_BLOCKS)
def test_block_step_vs_oracle_on_batch_statistics(name, math_mode, monkeypatch):
    from laudnet_amd import training
    monkeypatch.setattr(training, "USE_BATCH_STATS", True)
    fx = BLOCKS[name]
    hip, ref = _pair(fx)
    _step(hip, ref, fx, math_mode, f"{name}[{math_mode}]")
    assert int(hip.bn1.num_batches_tracked) == 1


@pytest.mark.gpu
def test_running_statistics_move_once_per_forward(monkeypatch):
    """forward + backward: once (the backward re-runs nothing that updates them); a second forward: once more; momentum=None: the cumulative
    average 1 / num_batches_tracked -- all against the oracle's own modules"""
    from laudnet_amd import training
    monkeypatch.setattr(training, "USE_BATCH_STATS", True)
    fx = BLOCKS["channel_g2_s2"]

    def cumulative(m):
        m.bn2.momentum = None
    hip, ref = _pair(fx, cumulative)
    before = {n: b.clone() for n, b in hip.named_buffers()}
    _step(hip, ref, fx, "fp32", "first step")
    for bn in (hip.bn1, hip.bn2, hip.bn3):
        assert int(bn.num_batches_tracked) == 1
    assert not torch.equal(hip.bn1.running_mean, before["bn1.running_mean"]) and not torch.equal(hip.bn3.running_var, before["bn3.running_var"])
    for p_ in list(hip.parameters()) + list(ref.parameters()):
        p_.grad = None
    _step(hip, ref, fx, "fp32", "second step")                 # (compares the buffers with the oracle's after ITS second step)
    for bn in (hip.bn1, hip.bn2, hip.bn3):
        assert int(bn.num_batches_tracked) == 2


@pytest.mark.gpu
def test_zero_bn3_weight_on_batch_statistics(monkeypatch):
    """zero_init_residual: bn3.weight == 0 -> the branch is the constant bn3.bias, d u3 == 0, and d bn3.weight = sum dz . xhat is non-zero and right"""
    from laudnet_amd import training
    monkeypatch.setattr(training, "USE_BATCH_STATS", True)
    fx = BLOCKS["spatial_g1_s1"]

    def zero(m):
        m.bn3.weight.zero_()
    hip, ref = _pair(fx, zero)
    _step(hip, ref, fx, "fp32", "bn3.weight == 0")
    g, w = hip.bn3.weight.grad, ref.bn3.weight.grad
    assert float(hip.bn3.weight.detach().abs().max()) == 0 and w.abs().max().item() > 0 and g.abs().max().item() > 0
    assert bool(torch.isfinite(g).all())
    _close(g, w, "fp32", "d bn3.weight at bn3.weight == 0")


@pytest.mark.gpu
def test_batch_statistics_scope_is_enforced(monkeypatch):
    from laudnet_amd import LdnError, training
    from laudnet_amd.laud_resnet import Bottleneck
    fx = BLOCKS["channel_g2_s1"]
    x, cm = block_input(fx).to(DEV), fx["channel_mask"].float().to(DEV)
    blk = make_block(Bottleneck, fx).to(DEV).train()
    monkeypatch.setattr(training, "USE_BATCH_STATS", False)
    with pytest.raises(LdnError, match="LDN_TRAIN_BATCH_STATS"):                 # switch off: refused as before, the message names the switch
        training.sparse_block_train(blk, x, cm)
    monkeypatch.setattr(training, "USE_BATCH_STATS", True)
    training.sparse_block_train(blk, x, cm)
    blk.bn2.eval()
    with pytest.raises(LdnError, match="some"):                                  # some BatchNorms training, some frozen
        training.sparse_block_train(blk, x, cm)
    blk.bn2.train()
    blk.bn1.track_running_stats, keep = False, (blk.bn1.running_mean, blk.bn1.running_var)
    with pytest.raises(LdnError, match="track_running_stats"):
        training.sparse_block_train(blk, x, cm)
    blk.bn1.track_running_stats = True
    assert blk.bn1.running_mean is keep[0]
    fx2 = load_golden("blocks_extra.pt")["both_grp2_s1"]                         # two spatial mask groups: refused in this mode as in the others
    blk2 = make_block(Bottleneck, fx2).to(DEV).train()
    with pytest.raises(LdnError, match="mask group"):
        training.sparse_block_train(blk2, block_input(fx2).to(DEV), (fx2["spatial_mask"].float().to(DEV), fx2["channel_mask"].float().to(DEV)))
    model = training.prepare_for_training(torch.nn.Sequential(torch.nn.BatchNorm2d(4)), batch_stats=True)
    assert model[0].training and not training.prepare_for_training(model)[0].training


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["r101_channel2222", "r101_layer"])
def test_classifier_train_step_on_batch_statistics(case, monkeypatch):
    """test_classifier_train_step_vs_oracle in plain model.train(): every BatchNorm -- the stem's, the blocks', the projections' -- on batch statistics"""
    from laudnet_amd import ops, training
    import laudnet_amd
    from oracle import torch_ref as TR
    monkeypatch.setattr(training, "USE_BATCH_STATS", True)
    ops.set_math_mode("fp32")
    fx = load_golden("full_tiny.pt")[case]
    ref, hip = TR.resnet101_ref(**fx["kw"]), laudnet_amd.uni_resnet101(**fx["kw"])
    sd = fill_state_dict(ref.state_dict(), fx["seed"])
    for k in sd:
        if k.endswith("bn3.weight"):
            sd[k] = sd[k] * RESIDUAL_DAMPING
    ref.load_state_dict(sd)
    hip.load_state_dict(sd)
    ref, hip = ref.to(DEV).train(), training.prepare_for_training(hip.to(DEV), batch_stats=True)
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
    out_h = training.train_forward(hip, x, 1.0)
    loss_of(out_h).backward()
    torch.cuda.synchronize()
    assert _err(out_h[0].detach(), out_r[0].detach()) < 1e-3, "logits"
    for i in (1, 2, 3, 4):
        for a, b in zip(out_h[i], out_r[i]):
            assert torch.allclose(a.detach().float(), b.detach().float(), atol=1e-6), i
    assert torch.allclose(out_h[5].detach(), out_r[5].detach(), atol=1e-5)
    assert abs(float(out_h[6]) - float(out_r[6])) <= 1e-5 * float(out_r[6])
    cpu_grads = oracle_cpu_grads(ref, tape, lambda m, dev: loss_of(m(x.to(dev), 1.0)).backward())
    n = _compare_param_grads(hip, ref, cpu_grads=cpu_grads, what=f"batch statistics full_tiny.pt::{case}")
    assert n >= 200, n
    assert _buffers_close(hip, ref, case) >= 3 * 33 * 3
