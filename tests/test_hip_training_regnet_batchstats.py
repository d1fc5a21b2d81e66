"""Training of LAD-RegNet CHANNEL-mode blocks with every BatchNorm on the statistics of the BATCH (laudnet_amd/training.py:
_RegNetBatchStatsBranchFn on ops.rows_bn_stats / ops.rows_bn_postmask_fwd / ops.rows_bn_postmask_bwd, behind training.USE_REGNET_CHANNEL and
training.USE_BATCH_STATS) against the ORACLE's autograd in plain .train() (oracle/regnet_ref.py; the same hard channel mask as a leaf that
requires grad) -- the third command of the reference's train_scripts.sh.

Blocks (tests/regnet_channel_ref.py's six cases, tests/regnet_bn_ref.py's training-mode oracle): the forward value, ALL gradients -- x, the
mask's straight-through term, the a / b / c weights and their BatchNorm affine parameters, se.fc1 / se.fc2 weight and bias, proj and its
BatchNorm -- and every BatchNorm's running_mean / running_var / num_batches_tracked after the forward, in both arithmetic modes.  Whole model:
regnet_tiny.pt::channel_g2 through train_forward against RegNetRef.train() with identical Gumbel noise, fp32 arithmetic.

Tolerances: _close of tests/test_hip_training_regnet_channel.py (fp32: every element within 1e-3 of max(1, scale); bf16x3: that file's flip
allowance); buffers: _buffers_close of tests/test_hip_training_batchstats.py (1e-5)."""
import pytest
import torch
import torch.nn as nn

import regnet_bn_ref as R
from fill import fill_state_dict, seeded_randn
from helpers import load_golden
from test_hip_training import GumbelTape, _relative_param_grads, oracle_cpu_grads
from test_hip_training_batchstats import _buffers_close
from test_hip_training_regnet_channel import _close, _compare, _err, _run_hip, _run_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REGNET = load_golden("regnet_tiny.pt")


@pytest.fixture
def both_on(monkeypatch):
    from laudnet_amd import training
    monkeypatch.setattr(training, "USE_REGNET_CHANNEL", True)
    monkeypatch.setattr(training, "USE_BATCH_STATS", True)
    return training


def _make(name, variant=None, edit=None):
    """(hip block, oracle block), both in .train() with the same state dict, and the case's inputs on the device"""
    from laudnet_amd.laud_regnet import ResBottleneckBlock
    ref, sd = R.make_ref_block(name, variant=variant)
    hip = ResBottleneckBlock(*R.block_args(name)[:3], nn.BatchNorm2d, nn.ReLU, *R.block_args(name)[3:], **R.dyn_kw(name))
    hip.load_state_dict(sd)
    if edit is not None:
        edit(hip)
        edit(ref)
    x, m = R.case_inputs(name)
    return hip.to(DEV).train(), ref.to(DEV).train(), x.to(DEV), m.to(DEV)


def _n_bn(hip):
    return 3 * (3 + (1 if hip.proj is not None else 0))


@pytest.mark.parametrize("name", list(R.CASES))
def test_regnet_batchstats_block_step_vs_oracle(name, math_mode, both_on):
    from laudnet_amd import ops
    ops.set_math_mode(math_mode)
    try:
        hip, ref, x0, mask0 = _make(name)
        want = _run_ref(ref, x0, mask0)
        got = _run_hip(hip, x0, mask0, want[4])
        _compare(got, want[:4], math_mode, hip.proj is not None)
        assert want[2].abs().max().item() > 0, "the straight-through term must not vanish"
        assert _buffers_close(hip, ref, name) == _n_bn(hip)
        assert int(hip.f.b[1].num_batches_tracked) == int(ref.f.b[1].num_batches_tracked)
        if name.endswith("all_off"):
            # every unit masked: conv c sees zeros and bn_c's output is its bias -- f.c.1.bias and the mask alone keep a gradient on the branch
            for pname, gh in got[3].items():
                if pname.startswith("f.") and "masker" not in pname and pname != "f.c.1.bias":
                    assert gh.abs().max().item() == 0, f"{pname}: an all-zero mask must leave no gradient on the branch"
            assert got[3]["f.c.1.bias"].abs().max().item() > 0 and got[2].abs().max().item() > 0
    finally:
        ops.set_math_mode("fp32")


def test_regnet_batchstats_block_with_zero_tiny_and_negative_bn_weights(both_on):
    """gw16_s2_proj_g2 with train_ref's `mixed` edit (BatchNorm weight 0 / negated / +2^-24 / -2^-24 by channel index, every BatchNorm of the
    block): nothing is folded or divided, so the zero-weight channels' weight gradients are right and non-zero"""
    from laudnet_amd import ops
    from train_ref import mixed_classes
    ops.set_math_mode("fp32")
    hip, ref, x0, mask0 = _make("gw16_s2_proj_g2", "mixed")
    assert bool((hip.f.c[1].weight[mixed_classes(64)["zero"]] == 0).all())
    want = _run_ref(ref, x0, mask0)
    got = _run_hip(hip, x0, mask0, want[4])
    _compare(got, want[:4], "fp32", True)
    for pname, gh in got[3].items():
        assert gh is None or bool(torch.isfinite(gh).all()), f"d {pname} holds NaN or Inf"
    for k in ("f.a.1.weight", "f.b.1.weight", "f.c.1.weight"):
        zero = mixed_classes(got[3][k].numel())["zero"].to(DEV)
        gh, gr = got[3][k][zero], want[3][k][zero]
        print(f"d {k} on the zero-weight channels: err {(gh - gr).abs().max().item():.2e}, max |want| {gr.abs().max().item():.2e}")
        assert gr.abs().max().item() > 0 and gh.abs().max().item() > 0, f"d {k} vanishes on the zero-weight channels"
        assert (gh - gr).abs().max().item() < 1e-3 * max(1.0, want[3][k].abs().max().item()), f"d {k} on the zero-weight channels"
    assert _buffers_close(hip, ref, "mixed") == _n_bn(hip)


def test_regnet_batchstats_block_without_mask_gradient(both_on):
    from laudnet_amd import ops
    ops.set_math_mode("fp32")
    hip, ref, x0, mask0 = _make("gw16_s2_proj_g2")
    want = _run_ref(ref, x0, mask0)
    got = _run_hip(hip, x0, mask0, want[4], mask_grad=False)
    assert got[2] is None
    _compare(got, want[:4], "fp32", True, mask_grad=False)


def test_regnet_batchstats_running_statistics_move_once_per_forward(both_on):
    """forward + backward: once; a second forward: once more; momentum=None on bn_b: the cumulative average -- all against the oracle's modules"""
    from laudnet_amd import ops
    ops.set_math_mode("fp32")

    def cumulative(blk):
        blk.f.b[1].momentum = None
    hip, ref, x0, mask0 = _make("gw8_s2_img_off", edit=cumulative)
    assert hip.f.b[1].momentum is None and ref.f.b[1].momentum is None
    before = {n: b.clone() for n, b in hip.named_buffers()}
    start = int(hip.f.a[1].num_batches_tracked)
    for step in (1, 2):
        want = _run_ref(ref, x0, mask0)
        got = _run_hip(hip, x0, mask0, want[4])
        _compare(got, want[:4], "fp32", hip.proj is not None)
        assert _buffers_close(hip, ref, f"step {step}") == _n_bn(hip)
        for bn in (hip.f.a[1], hip.f.b[1], hip.f.c[1], hip.proj[1]):
            assert int(bn.num_batches_tracked) == start + step
        if step == 1:
            after1 = {n: b.clone() for n, b in hip.named_buffers()}
            assert not torch.equal(after1["f.a.1.running_mean"], before["f.a.1.running_mean"])
            assert not torch.equal(after1["f.c.1.running_var"], before["f.c.1.running_var"])
    # (bn_a: momentum 0.1.  bn_b's cumulative average of the same batch twice stays where the first step put it -- the oracle's does too)
    assert not torch.equal(hip.f.a[1].running_mean, after1["f.a.1.running_mean"])


def test_regnet_batchstats_wgrad_switch_off_agrees_with_the_kernel_path(monkeypatch, both_on):
    from laudnet_amd import ops
    training = both_on
    ops.set_math_mode("fp32")
    hip, ref, x0, mask0 = _make("gw16_s2_proj_g2")
    want = _run_ref(ref, x0, mask0)
    assert training.USE_WGRAD_KERNEL and training._wgrad_grouped_kernel(64, 16)
    on = _run_hip(hip, x0, mask0, want[4])
    monkeypatch.setattr(training, "USE_WGRAD_KERNEL", False)
    assert not training._wgrad_grouped_kernel(64, 16)
    off = _run_hip(hip, x0, mask0, want[4])
    _compare(off, want[:4], "fp32", True)
    _close(off[0], on[0], "fp32", "forward: switch off vs kernel")
    _close(off[1], on[1], "fp32", "d x: switch off vs kernel")
    for pname, g_on in on[3].items():
        if "masker" not in pname:
            _close(off[3][pname], g_on, "fp32", f"d {pname}: switch off vs kernel")


def _dyn(S, dyn_mode):
    return dict(spatial_mask_channel_group=1, channel_dyn_granularity=1, output_size=S, mask_spatial_granularity=S, dyn_mode=dyn_mode)


def test_regnet_batchstats_scope_is_enforced(monkeypatch):
    from laudnet_amd import LdnError, training
    from laudnet_amd.laud_regnet import ResBottleneckBlock
    from laudnet_amd.training import sparse_block_train
    x = torch.relu(seeded_randn((2, 32, 8, 8), 5)).to(DEV)
    bit = torch.ones(2, 1, 1, 1, device=DEV)
    ones = torch.ones(2, 32, device=DEV)
    mk = lambda **dyn: ResBottleneckBlock(32, 32, 1, nn.BatchNorm2d, nn.ReLU, 8, 1.0, 0.25, **dyn).to(DEV).train()
    chan = mk(**_dyn(8, "channel"))
    assert training.USE_REGNET_CHANNEL is False and training.USE_BATCH_STATS is False, "both switches are off by default"
    with pytest.raises(LdnError, match="not built"):                             # both off
        sparse_block_train(chan, x, ones)
    monkeypatch.setattr(training, "USE_BATCH_STATS", True)
    with pytest.raises(LdnError, match="not built.*LDN_TRAIN_REGNET_CHANNEL"):   # the channel switch off
        sparse_block_train(chan, x, ones)
    monkeypatch.setattr(training, "USE_BATCH_STATS", False)
    monkeypatch.setattr(training, "USE_REGNET_CHANNEL", True)
    with pytest.raises(LdnError, match="not built.*LDN_TRAIN_BATCH_STATS"):      # the batch-statistics switch off: the message names it
        sparse_block_train(chan, x, ones)
    monkeypatch.setattr(training, "USE_BATCH_STATS", True)
    assert tuple(sparse_block_train(chan, x, ones).shape) == (2, 32, 8, 8)
    assert int(chan.f.a[1].num_batches_tracked) == 1
    chan.f.b[1].eval()
    with pytest.raises(LdnError, match="some.*not built"):                       # some BatchNorms training, some frozen
        sparse_block_train(chan, x, ones)
    chan.f.b[1].train()
    chan.f.a[1].track_running_stats = False
    with pytest.raises(LdnError, match="track_running_stats"):
        sparse_block_train(chan, x, ones)
    chan.f.a[1].track_running_stats = True
    plain = ResBottleneckBlock(32, 32, 1, lambda c: nn.BatchNorm2d(c, affine=False), nn.ReLU, 8, 1.0, 0.25, **_dyn(8, "channel")).to(DEV).train()
    with pytest.raises(LdnError, match="affine"):
        sparse_block_train(plain, x, ones)
    with pytest.raises(LdnError, match="layer-skip.*not built"):                 # layer skip with a training BatchNorm stays refused
        sparse_block_train(mk(**_dyn(8, "spatial")), x, bit)
    assert tuple(sparse_block_train(mk(**_dyn(8, "spatial")).eval(), x, bit).shape) == (2, 32, 8, 8)       # ... and trains frozen, as before
    assert int(chan.f.a[1].num_batches_tracked) == 1, "a refused call must not move the statistics"


def test_regnet_batchstats_train_step_vs_oracle(both_on):
    """regnet_tiny.pt::channel_g2 in plain .train(): one training forward + backward of the whole model, every BatchNorm -- the stem's, the
    blocks', the projections' -- on batch statistics, the channel masks sampled from its own MLP maskers with the oracle's Gumbel noise: the
    7-tuple, the gradient of EVERY one of the 102 parameters, and every BatchNorm buffer."""
    import laudnet_amd
    from laudnet_amd import ops
    from laudnet_amd.training import prepare_for_training, train_forward
    from oracle import regnet_ref as RR
    ops.set_math_mode("fp32")     # (true-fp32 arithmetic: the Gumbel samples and every ReLU decision must coincide with the oracle's)
    fx = REGNET["cases"]["channel_g2"]
    ref = RR.RegNetRef(REGNET["tiny_params"] | {}, se_ratio=REGNET["tiny_params"]["se_ratio"], **fx["kw"])
    hip = laudnet_amd.LAD_RegNet(laudnet_amd.BlockParams(**REGNET["tiny_params"]), **fx["kw"])
    sd = fill_state_dict(ref.state_dict(), fx["seed"])
    ref.load_state_dict(sd)
    hip.load_state_dict(sd)
    ref, hip = ref.to(DEV).train(), prepare_for_training(hip.to(DEV), batch_stats=True)
    assert all(m_.training for m_ in hip.modules() if isinstance(m_, torch.nn.modules.batchnorm._BatchNorm))
    size = fx["kw"]["input_size"]
    B = fx["batch"]
    x = seeded_randn((B, 3, size, size), fx["x_seed"]).to(DEV)
    g = seeded_randn((B, fx["kw"]["num_classes"]), 9).to(DEV)

    def loss_of(out):
        return (out[0] * g.to(out[0].device)).sum() / 10.0 + 10.0 * (out[5].mean() - 0.5) ** 2 + 1e-14 * out[6] ** 2

    tape = GumbelTape()
    torch.manual_seed(77)
    with tape.record():
        out_r = ref(x, 1.0)
    loss_of(out_r).backward()
    torch.manual_seed(77)
    out_h = train_forward(hip, x, 1.0)
    loss_of(out_h).backward()
    torch.cuda.synchronize()
    print(f"logits: err {_err(out_h[0].detach(), out_r[0].detach()):.2e}")
    assert _err(out_h[0].detach(), out_r[0].detach()) < 1e-3, "logits"
    for i in (1, 2, 3, 4):
        assert len(out_h[i]) == len(out_r[i]) == 4
        for a, b in zip(out_h[i], out_r[i]):
            assert a.shape == b.shape and torch.allclose(a.detach().float(), b.detach().float(), atol=1e-6), i     # identical Gumbel samples
    assert torch.allclose(out_h[5].detach(), out_r[5].detach(), atol=1e-5)
    assert abs(float(out_h[6].detach()) - float(out_r[6].detach())) <= 1e-5 * float(out_r[6].detach())
    cs = torch.cat([v.detach() for v in out_r[4]])
    assert 0 < float(cs.min()) and float(cs.max()) < 1, "the sampled masks must keep some channels and drop some in every block"
    n_buf = _buffers_close(hip, ref, "regnet_tiny.pt::channel_g2")
    assert n_buf == 3 * sum(isinstance(m_, torch.nn.modules.batchnorm._BatchNorm) for n_, m_ in hip.named_modules() if "masker" not in n_) > 3
    want = dict(ref.named_parameters())
    n = 0
    for name, p_ in hip.named_parameters():
        w = want[name].grad
        assert (w is None) == (p_.grad is None), f"{name}: gradient present on one side only"
        assert w is not None, f"{name}: every parameter gets a gradient in channel mode"
        _close(p_.grad, w, "fp32", f"d {name}")
        n += 1
    assert n == len(want) == 102, (n, len(want))
    # the scale-relative statement for the tensors on which the oracle's CPU and GPU steps agree (tests/test_hip_training.py)
    cpu_grads = oracle_cpu_grads(ref, tape, lambda m, dev: loss_of(m(x.to(dev), 1.0)).backward())
    _relative_param_grads(hip, ref, cpu_grads, "batch statistics regnet_tiny.pt::channel_g2")
