"""No cached, folded weight may outlive an edit of its source: whole models on the GPU, run, edited, run again.

Every eval forward runs on derived weights that are built once and kept until their source changes: the per-module _prep of _PrepCache
(keyed on (data_ptr, version) of the sub-tree's parameters and buffers), the entries added to it later (Bottleneck.tail_weights, w2_nk,
laud_regnet._conv_b_frag), ResNet._chain_cache (raw device pointers into the prepared tensors of a chained run), the stems, TokenSkipBlock._w
and the global ops._SPLIT_CACHE.  A stale hit faults nothing: it returns yesterday's weights in today's logits.

ONE pattern for every case: run the model (out0; the caches are built, asserted), make one edit, run again (out1), then build the reference --
ops._SPLIT_CACHE.clear(), a NEW model of the same configuration, a clone of the edited model's state_dict() loaded into it, one forward on the
same input: it has never run, so it cannot be stale.  out1 must equal it bit for bit (logits, every sparsity and FLOPs tensor, every block's
masks and channel counts), and the reference must differ from out0 (the edit mattered; both sides of that come from never-edited models).
There are no tolerances in this module: the reference is the same code.  The host mechanics are tests/test_prep_cache.py (no GPU).
Out of scope: GraphedForward (a captured graph holds raw pointers; its owner rebuilds it after an edit)."""
import copy
import gc
import os
import sys

import pytest
import torch

from fill import fill_state_dict, seeded_bernoulli, seeded_randn
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGNET = load_golden("regnet_tiny.pt")
REGNET_SWITCHES = ("USE_GROUPED_MFMA", "USE_GROUPED_IMAGES", "USE_GROUPED_MFMA_WIDTHS", "USE_GROUPED_MFMA_WIDTHS_IMAGES", "USE_GROUPED_MFMA_CHANNEL",
                   "USE_GROUPED_MFMA_WIDE", "USE_GROUPED_MFMA_WIDE_ROWS", "USE_SE_FUSED", "USE_CHANNEL_SE_FUSED", "USE_CHANNEL_SE_FUSED_WIDE",
                   "USE_BOTH_SE_FUSED")


@pytest.fixture(autouse=True)
def _restore():
    from laudnet_amd import laud_regnet, ops
    from laudnet_amd.laud_resnet import ResNet
    saved = {n: getattr(laud_regnet, n) for n in REGNET_SWITCHES}
    assert len(saved) == len([n for n in vars(laud_regnet) if n.startswith("USE_")]), "a new conv b / SE switch: add it to REGNET_SWITCHES"
    ops._SPLIT_CACHE.clear()
    ops.set_math_mode("bf16x3")
    yield
    ops.set_math_mode("fp32")
    ResNet.use_chain = True
    for n, v in saved.items():
        setattr(laud_regnet, n, v)
    ops._SPLIT_CACHE.clear()


def _all_switches_on():
    """every conv b / SE switch of laud_regnet on: the matrix-core and SE-fused forms wherever their fit queries take the shape"""
    from laudnet_amd import laud_regnet
    for n in REGNET_SWITCHES:
        setattr(laud_regnet, n, True)


# ------------------------------------------------------------------------------------------------ the three model families
def _flat(v):
    if torch.is_tensor(v):
        return [v]
    return [t for u in v for t in _flat(u)]


def _run_model(m, x, ctx=torch.no_grad):
    """one forward -> [(name, tensor)]: the 7-tuple flattened, then every block's masks / channel counts where the block leaves them"""
    with ctx():
        out = m(x, 1.0)
    torch.cuda.synchronize()
    items = [(f"output {i}", t) for i, t in enumerate(_flat(out))]
    blocks = m.blocks() if hasattr(m, "trunk_output") else [b for s in (1, 2, 3, 4) for b in getattr(m, f"layer{s}")]
    for i, blk in enumerate(blocks):
        holder = blk.f if hasattr(blk, "f") else blk
        for name in ("last_channel_mask", "last_channel_cnt", "last_spatial_mask"):
            t = getattr(holder, name, None)
            if torch.is_tensor(t):
                items.append((f"block {i} {name}", t))
    return [(n, t.detach().clone()) for n, t in items]


def _same(a, b, what):
    assert [n for n, _ in a] == [n for n, _ in b], what
    for (n, ta), (_, tb) in zip(a, b):
        assert ta.shape == tb.shape and ta.dtype == tb.dtype, f"{what}: {n}"
        assert torch.equal(ta, tb), f"{what}: {n} differs" + (f" (max |diff| {float((ta.double() - tb.double()).abs().max()):.3e})" if ta.numel() else "")


def _differs(a, b):
    return not torch.equal(a[0][1], b[0][1])


class Family:
    """A model configuration: fresh() -> a new, never-run model on the device holding `state` (default: the configuration's base
    weights, calibrated so that every masker makes real decisions); run(model) -> [(name, tensor)]."""

    def __init__(self, name, make, x, base, run=_run_model, built=None):
        self.name, self._make, self.x, self.base, self._run, self.built = name, make, x, base, run, built

    def fresh(self, state=None):
        m = self._make().eval()
        m.load_state_dict({k: v.detach().clone() for k, v in (state if state is not None else self.base).items()})
        return m.to(DEV).eval()

    def run(self, m, **kw):
        return self._run(m, self.x, **kw)

    def reference(self, m, **kw):
        """the model that cannot be stale: a new one, holding a clone of m's state, run once on the same input"""
        from laudnet_amd import ops
        ops._SPLIT_CACHE.clear()
        return self.run(self.fresh(m.state_dict()), **kw)


_FAMILIES = {}


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


RESNET_KW = {
    # the configuration of tests/test_hip_chain.py::_model: the chain (stage 3), k_smallmap (stage 4) and the fused tail all run
    "channel": dict(dyn_mode=["channel"] * 4, channel_dyn_granularity=[2, 2, 2, 2], channel_masker=["MLP"] * 4, channel_masker_layers=[2, 2, 2, 2],
                    reduction_ratio=[16] * 4),
    "spatial": dict(dyn_mode=["spatial"] * 4, mask_spatial_granularity=[4, 4, 2, 1]),
    "layer": dict(dyn_mode=["layer"] * 4),
}


def _resnet(mode, width_mult=0.25):
    """uni_resnet50 at a quarter of the width (half: the one-launch stem and its packed weights run), batch 2, masks calibrated (channel:
    62 % kept; spatial / layer: half)"""
    key = ("resnet", mode, width_mult)
    if key not in _FAMILIES:
        import laudnet_amd
        from laudnet_amd import ops
        make = lambda: laudnet_amd.uni_resnet50(width_mult=width_mult, input_size=224, num_classes=1000, **RESNET_KW[mode])
        m = make().eval()
        sd = fill_state_dict(m.state_dict(), 3)
        m.load_state_dict({k: (v * 0.3 if k.endswith("bn3.weight") else v) for k, v in sd.items()})
        m = m.to(DEV)
        x = seeded_randn((2, 3, 224, 224), 77).to(DEV).contiguous(memory_format=torch.channels_last)
        with ops.math_mode("bf16x3"):
            _bench().calibrate_maskers(m, x, 0.62 if mode == "channel" else None, None if mode == "channel" else 0.5)
        base = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

        def built(m):
            assert m.layer3[1]._cache_valid() and m.layer2[0]._cache_valid() and getattr(m, "_stem_key", None) is not None
            if width_mult == 0.5:
                assert m._stem_frag_key == m._stem_key, "a 32-channel stem must run as the one launch, on packed weights"
            if mode == "channel":
                assert m.layer3[1].masker_channel._cache_valid() and len(m._chain_cache) == 1, "stage 3 must run as a chain"
            else:
                assert m.layer3[1].masker_spatial._cache_valid()
        _FAMILIES[key] = Family(f"resnet-{mode}-x{width_mult}", make, x, base, built=built)
    return _FAMILIES[key]


REGNET_CASE = {"spatial": "spatial_g2", "channel": "channel_g2", "both": "both"}


def _calibrate_regnet(model, x):
    """bench.calibrate_maskers for LAD-RegNet blocks (whose granularity is w_b / groups): one sequential pass that shifts each masker's
    keep-logit bias so that 62 % of the channel groups / half of the patches are kept on this batch"""
    with torch.no_grad():
        h = model.stem(x.contiguous(memory_format=torch.channels_last))
        for blk in model.blocks():
            f = blk.f
            mk, ms = f.masker_channel, f.masker_spatial
            if mk is not None:
                G = mk.channel_dyn_group
                logits = mk.lists(h, f.w_b // G, want_logits=True)[3]
                diff = (logits[:, :G] - logits[:, G:]).flatten().float().cpu()
                last = mk.conv[-1] if mk.layers == 2 else mk.conv
                last.bias[:G] -= torch.quantile(diff, 1.0 - 0.62).item()
            if ms is not None:
                g = ms.mask_channel_group
                logits = ms(h, 1.0, want_logits=True)[3]
                diff = (logits[:, :g] - logits[:, g:]).flatten().float().cpu()
                ms.conv.bias[:g] -= torch.quantile(diff, 0.5).item()
            h = blk.run_dynamic(h)[0]


def _regnet(mode):
    """the tiny LAD-RegNet of tests/golden/regnet_tiny.pt (group width 8, 64 px input, batch 2)"""
    key = ("regnet", mode)
    if key not in _FAMILIES:
        import laudnet_amd
        from laudnet_amd import ops
        fx = REGNET["cases"][REGNET_CASE[mode]]
        make = lambda: laudnet_amd.LAD_RegNet(laudnet_amd.BlockParams(**REGNET["tiny_params"]), **fx["kw"])
        m = make().eval()
        m.load_state_dict(fill_state_dict(m.state_dict(), fx["seed"]))
        m = m.to(DEV)
        size = fx["kw"]["input_size"]
        x = seeded_randn((fx["batch"], 3, size, size), fx["x_seed"]).to(DEV).contiguous(memory_format=torch.channels_last)
        with ops.math_mode("bf16x3"):
            _calibrate_regnet(m, x)
        base = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

        def built(m):
            blk = m.blocks()[3]
            assert blk.f._cache_valid() and m.blocks()[2]._cache_valid()
            for mk in (blk.f.masker_channel, blk.f.masker_spatial):
                assert mk is None or mk._cache_valid()
        _FAMILIES[key] = Family(f"regnet-{mode}", make, x, base, built=built)
    return _FAMILIES[key]


ADAVIT_B, ADAVIT_L, ADAVIT_DIM = 2, 17, 128


def _adavit():
    """one TokenSkipBlock(dim 128, 2 heads) through run_packed: 2 images of 17 tokens, about half of them kept"""
    key = ("adavit",)
    if key not in _FAMILIES:
        from laudnet_amd import ops
        from laudnet_amd.adavit import TokenSkipBlock
        make = lambda: TokenSkipBlock(dim=ADAVIT_DIM, heads=2)
        base = {}
        for i, (k, v) in enumerate(make().state_dict().items()):
            r = seeded_randn(tuple(v.shape), 900 + i)
            base[k] = r * 0.05 if v.dim() > 1 else (1.0 + 0.1 * r if k.startswith("norm") and k.endswith("weight") else 0.1 * r)
        keep = seeded_bernoulli((ADAVIT_B, ADAVIT_L), 0.5, 931)
        keep[:, 0] = 1.0
        assert 0.3 < float(keep.mean()) < 0.7
        lists = ops.token_lists(keep.to(DEV))
        x = seeded_randn((ADAVIT_B * ADAVIT_L, ADAVIT_DIM), 932).to(DEV)

        def run(blk, x, ctx=torch.no_grad):
            x2d = x.clone()
            with ctx():
                blk.run_packed(x2d, lists[0], lists[1], lists[2], ADAVIT_B, ADAVIT_L)
            torch.cuda.synchronize()
            return [("x2d", x2d.detach().clone())]

        def built(blk):
            assert blk._w is not None
        _FAMILIES[key] = Family("adavit", make, x, base, run=run, built=built)
    return _FAMILIES[key]


# ------------------------------------------------------------------------------------------------ edits
def _scale(ts):
    for t in ts:
        t.mul_(1.5)


def _var(ts):
    for t in ts:
        t.mul_(4.0)


def _shift(ts):
    for t in ts:
        t.add_(0.5)


def _negate(ts):      # a masker's last layer, weight and bias: every decision flips
    for t in ts:
        t.neg_()


def _edit_site(m, site):
    get, how = site
    with torch.no_grad():
        how(get(m))


def _mlp_last(mk):
    last = mk.conv[-1] if mk.layers == 2 else mk.conv
    return [last.weight, last.bias]


RESNET_SITES = {
    "stem_conv": (lambda m: [m.conv1.weight], _scale),
    "stem_bn_var": (lambda m: [m.bn1.running_var], _var),
    "s3_b1_conv1": (lambda m: [m.layer3[1].conv1.weight], _scale),          # the first identity block of stage 3 (channel mode: run[0] of the chain)
    "s3_b1_conv2": (lambda m: [m.layer3[1].conv2.weight], _scale),
    "s3_b1_conv3": (lambda m: [m.layer3[1].conv3.weight], _scale),
    "s3_b1_bn2_mean": (lambda m: [m.layer3[1].bn2.running_mean], _shift),
    "s2_b0_downsample": (lambda m: [m.layer2[0].downsample[0].weight], _scale),
    "s3_b1_spatial_masker": (lambda m: [m.layer3[1].masker_spatial.conv.weight, m.layer3[1].masker_spatial.conv.bias], _negate),
    "chain_mid_masker": (lambda m: _mlp_last(m.layer3[3].masker_channel), _negate),      # the MIDDLE of the chained run layer3[1:6]
    "chain_mid_conv2": (lambda m: [m.layer3[3].conv2.weight], _scale),
    "chain_mid_bn3_var": (lambda m: [m.layer3[3].bn3.running_var], _var),
    "s4_b1_conv2": (lambda m: [m.layer4[1].conv2.weight], _scale),          # channel mode: a k_smallmap block (tail_weights' w1s / w2p / w3p)
    "s4_b0_conv1": (lambda m: [m.layer4[0].conv1.weight], _scale),          # channel mode: the dense execution (w2_nk / w3_nk added to _prep later)
    "s4_b0_conv2": (lambda m: [m.layer4[0].conv2.weight], _scale),
    "fc": (lambda m: [m.fc.weight], _scale),
}
_COMMON = ["stem_conv", "stem_bn_var", "s3_b1_conv1", "s3_b1_conv2", "s3_b1_conv3", "s3_b1_bn2_mean", "s2_b0_downsample", "fc"]
RESNET_CASES = ([("channel", "bf16x3", s) for s in _COMMON + ["chain_mid_masker", "chain_mid_conv2", "chain_mid_bn3_var", "s4_b1_conv2", "s4_b0_conv1",
                                                              "s4_b0_conv2"]]
                + [("channel", "fp32", s) for s in ["s3_b1_conv1", "chain_mid_masker", "chain_mid_conv2", "chain_mid_bn3_var", "s2_b0_downsample"]]
                + [("spatial", "bf16x3", s) for s in _COMMON + ["s3_b1_spatial_masker"]]
                + [("layer", "bf16x3", s) for s in _COMMON + ["s3_b1_spatial_masker"]])

_RB, _RP = 3, 2        # LAD-RegNet tiny: blocks()[3] is the identity block of stage 3, blocks()[2] the projection block in front of it
REGNET_SITES = {
    "stem_conv": (lambda m: [m.stem[0].weight], _scale),
    "a_conv": (lambda m: [m.blocks()[_RB].f.a[0].weight], _scale),
    "b_conv": (lambda m: [m.blocks()[_RB].f.b[0].weight], _scale),
    "c_conv": (lambda m: [m.blocks()[_RB].f.c[0].weight], _scale),
    "b_bn_var": (lambda m: [m.blocks()[_RB].f.b[1].running_var], _var),
    "se_fc1_bias": (lambda m: [m.blocks()[_RB].f.se.fc1.bias], _shift),
    "proj_conv": (lambda m: [m.blocks()[_RP].proj[0].weight], _scale),
    "spatial_masker": (lambda m: [m.blocks()[_RB].f.masker_spatial.conv.weight, m.blocks()[_RB].f.masker_spatial.conv.bias], _negate),
    "channel_masker": (lambda m: _mlp_last(m.blocks()[_RB].f.masker_channel), _negate),
}
_RCOMMON = ["stem_conv", "a_conv", "b_conv", "c_conv", "b_bn_var", "se_fc1_bias", "proj_conv"]
REGNET_CASES = [(mode, s) for mode, extra in (("spatial", ["spatial_masker"]), ("channel", ["channel_masker"]), ("both", ["spatial_masker", "channel_masker"]))
                for s in _RCOMMON + extra]

ADAVIT_SITES = {
    "norm1_weight": (lambda b: [b.norm1.weight], _scale),         # LayerNorm is folded into qkv
    "qkv_weight": (lambda b: [b.qkv.weight], _scale),
    "fc2_bias": (lambda b: [b.fc2.bias], _shift),
}


def _edit_then_compare(fam, edit, what):
    """the pattern of this module (see the header) for an edit of the model in place"""
    m = fam.fresh()
    out0 = fam.run(m)
    fam.built(m)
    edit(m)
    out1 = fam.run(m)
    ref = fam.reference(m)
    _same(out1, ref, f"{fam.name}, {what}: the forward after the edit against a model that never ran")
    assert _differs(ref, out0), f"{fam.name}, {what}: the edit does not change the output -- the case proves nothing"
    return m, out0, out1


# ------------------------------------------------------------------------------------------------ one source tensor at a time
@pytest.mark.parametrize("mode,math,site", RESNET_CASES)
def test_resnet_one_source_tensor(mode, math, site):
    from laudnet_amd import ops
    fam = _resnet(mode)
    ops.set_math_mode(math)
    _edit_then_compare(fam, lambda m: _edit_site(m, RESNET_SITES[site]), site)


@pytest.mark.parametrize("site", ["stem_conv", "stem_bn_var"])
def test_resnet_fused_stem_source_tensor(site):
    """half width: the stem is ldn_stem_conv_pool on fragments packed from the folded weights (_stem_frag / _stem_frag_key), and it leaves
    the first channel masker's GAP partials"""
    _edit_then_compare(_resnet("channel", 0.5), lambda m: _edit_site(m, RESNET_SITES[site]), site)


@pytest.mark.parametrize("switches", ["default", "all_on"])
@pytest.mark.parametrize("mode,site", REGNET_CASES)
def test_regnet_one_source_tensor(mode, site, switches):
    fam = _regnet(mode)
    if switches == "all_on":
        _all_switches_on()
    _edit_then_compare(fam, lambda m: _edit_site(m, REGNET_SITES[site]), f"{site}, switches {switches}")


@pytest.mark.parametrize("site", sorted(ADAVIT_SITES))
def test_adavit_one_source_tensor(site):
    _edit_then_compare(_adavit(), lambda b: _edit_site(b, ADAVIT_SITES[site]), site)


# ------------------------------------------------------------------------------------------------ every way an edit arrives
def _family(name):
    return {"resnet": lambda: _resnet("channel"), "regnet": lambda: _regnet("both"), "adavit": _adavit}[name]()


SITE_OF = {"resnet": RESNET_SITES["chain_mid_conv2"], "regnet": REGNET_SITES["b_conv"], "adavit": ADAVIT_SITES["qkv_weight"]}


def _set_grads(m, seed):
    for i, p in enumerate(m.parameters()):
        p.grad = seeded_randn(tuple(p.shape), seed + i).to(p.device)


def _way_sgd(m, site):
    _set_grads(m, 4000)
    torch.optim.SGD(m.parameters(), lr=0.01).step()


def _way_adamw_fused(m, site):
    _set_grads(m, 5000)
    torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True).step()


def _scaled_state(m):
    return {k: (v.detach().clone() * 1.25 if v.is_floating_point() else v.detach().clone()) for k, v in m.state_dict().items()}


def _way_load(m, site):
    m.load_state_dict(_scaled_state(m))


def _way_load_assign(m, site):
    m.load_state_dict(_scaled_state(m), assign=True)


def _way_cpu_round_trip(m, site):
    m.cpu()
    _edit_site(m, site)
    m.to(DEV)


WAYS = {"sgd_step": _way_sgd, "adamw_fused_step": _way_adamw_fused, "load_state_dict": _way_load, "load_state_dict_assign": _way_load_assign,
        "cpu_round_trip": _way_cpu_round_trip}


@pytest.mark.parametrize("way", sorted(WAYS))
@pytest.mark.parametrize("family", ["resnet", "regnet", "adavit"])
def test_every_way_an_edit_arrives(family, way):
    fam = _family(family)
    _edit_then_compare(fam, lambda m: WAYS[way](m, SITE_OF[family]), way)


@pytest.mark.parametrize("family", ["resnet", "regnet", "adavit"])
def test_deepcopy_after_a_forward(family):
    """the copy carries the original's caches: edited, it must match its own fresh reference, and the original must not move"""
    fam = _family(family)
    m = fam.fresh()
    out0 = fam.run(m)
    fam.built(m)
    c = copy.deepcopy(m)
    _same(fam.run(c), out0, f"{fam.name}: the unedited copy")
    _edit_site(c, SITE_OF[family])
    out_c = fam.run(c)
    _same(fam.run(m), out0, f"{fam.name}: the original after its copy was edited")
    ref = fam.reference(c)
    _same(out_c, ref, f"{fam.name}: the edited copy against a model that never ran")
    assert _differs(ref, out0)
    _same(fam.run(m), out0, f"{fam.name}: the original, once more")


def test_resnet_math_mode_flip_around_an_edit():
    """tail_weights keeps the bf16x3 layouts and their fp32 twins under separate keys of ONE _prep, the chain table is keyed on the mode:
    forward in bf16x3, in fp32, edit, forward in bf16x3, in fp32 -- each against a fresh model in that mode."""
    from laudnet_amd import ops
    fam = _resnet("channel")
    m = fam.fresh()
    first = {}
    for step in ("before", "after"):
        if step == "after":
            _edit_site(m, RESNET_SITES["chain_mid_conv2"])
        for math in ("bf16x3", "fp32"):
            ops.set_math_mode(math)
            got = fam.run(m)
            fam.built(m)
            ref = fam.reference(m)
            _same(got, ref, f"{step} the edit, {math}")
            if step == "before":
                first[math] = ref
            else:
                assert _differs(ref, first[math])
    assert _differs(first["bf16x3"], first["fp32"]), "the two modes must be two arithmetics"
    assert len(m._chain_cache) == 1


@pytest.mark.parametrize("mode", ["channel", "both"])
def test_regnet_switch_flip_around_an_edit(mode):
    """_conv_b_frag packs wb_frag* into an EXISTING _prep when a switch is turned on after the weights were prepared; after an edit the
    rebuilt _prep must not keep those fragments.  Forward with the switches off, on, edit f.b[0].weight, forward: each against a fresh
    model under the same switches."""
    from laudnet_amd import laud_regnet
    fam = _regnet(mode)
    for n in REGNET_SWITCHES:
        if n not in ("USE_GROUPED_MFMA", "USE_GROUPED_IMAGES", "USE_SE_FUSED"):      # (the three that are on by default stay on)
            setattr(laud_regnet, n, False)
    m = fam.fresh()
    off = fam.run(m)
    _same(off, fam.reference(m), "switches off")
    p = m.blocks()[_RB].f._prep
    assert "wb_frag_gw" not in p, "group width 8 with its switches off: the VALU kernel, no fragments yet"
    _all_switches_on()
    on = fam.run(m)
    assert m.blocks()[_RB].f._prep is p and "wb_frag_gw" in p, "the fragments are packed into the existing _prep"
    _same(on, fam.reference(m), "switches on")
    _edit_site(m, REGNET_SITES["b_conv"])
    after = fam.run(m)
    assert m.blocks()[_RB].f._prep is not p
    ref = fam.reference(m)
    _same(after, ref, "switches on, after the edit")
    assert _differs(ref, on)


@pytest.mark.parametrize("family", ["resnet", "regnet", "adavit"])
def test_control_an_edit_through_data_is_served_stale(family):
    """The documented blind spot, at model level -- the negative control of this module: an edit through `p.data` (of a weight whose
    folded form is a real copy) leaves the output where it was; invalidate() on the owning module brings the new weights in."""
    fam = _family(family)
    m = fam.fresh()
    out0 = fam.run(m)
    fam.built(m)
    owner = {"resnet": lambda: m.layer3[3], "regnet": lambda: m.blocks()[_RB].f, "adavit": lambda: m}[family]()
    for t in SITE_OF[family][0](m):
        t.data.mul_(1.5)
    _same(fam.run(m), out0, f"{fam.name}: the documented blind spot has closed -- update _PrepCache's docstring")
    owner.invalidate()
    out1 = fam.run(m)
    ref = fam.reference(m)
    _same(out1, ref, f"{fam.name}: after invalidate()")
    assert _differs(ref, out0)


def test_chain_table_follows_a_masker_that_is_rebuilt_alone():
    """The chain table holds raw pointers into the maskers' folded weights too, and a masker can be rebuilt without its block: after an edit
    through `.data`, invalidate() on the MASKER is the documented remedy.  (Every tracked edit of a masker's parameter also rebuilds the
    block that owns it -- the block's key covers its sub-tree -- so only this case needs the maskers' _prep_gen in the chain key.  A float64
    masker: its float32 folded weights are real copies; those of a float32 masker alias the parameters and could not go stale.)"""
    fam = _resnet("channel")
    m = fam.fresh()
    blk = m.layer3[3]                                  # the middle of the chained run layer3[1:6]
    blk.masker_channel.double()
    out0 = fam.run(m)
    fam.built(m)
    gen = blk._prep_gen
    for t in _mlp_last(blk.masker_channel):
        t.data.neg_()
    _same(fam.run(m), out0, "the documented blind spot has closed -- update _PrepCache's docstring")
    blk.masker_channel.invalidate()
    out1 = fam.run(m)
    assert blk._prep_gen == gen and len(m._chain_cache) == 1, "only the masker was rebuilt"
    ref = fam.reference(m)
    _same(out1, ref, "after invalidate() on the masker alone")
    assert _differs(ref, out0)


# ------------------------------------------------------------------------------------------------ torch.inference_mode()
@pytest.mark.parametrize("family", ["resnet", "regnet", "adavit"])
def test_first_forward_under_inference_mode(family):
    """The folded weights of a first forward under torch.inference_mode() are inference tensors, which have no version counter
    (ops.tensor_version counts them as -1): the forward must succeed, equal the no_grad forward of a fresh twin, follow an edit made
    outside the context, and leave a model that still runs under no_grad.  (Parameters that are inference tensors are out of scope.)"""
    from laudnet_amd import ops
    fam = _family(family)
    m = fam.fresh()
    out0 = fam.run(m, ctx=torch.inference_mode)
    fam.built(m)
    prep = {"resnet": lambda: m.layer3[3]._prep["w3"], "regnet": lambda: m.blocks()[_RB].f._prep["wb"], "adavit": lambda: m._w[1][0]}[family]()
    assert prep.is_inference() and ops.tensor_version(prep) == -1 and ops.version_key([prep])[0] == (prep.data_ptr(), -1)
    _same(out0, fam.reference(m), f"{fam.name}: first forward under inference_mode against the no_grad forward of a fresh twin")
    _edit_site(m, SITE_OF[family])
    out1 = fam.run(m, ctx=torch.inference_mode)
    ref = fam.reference(m)
    _same(out1, ref, f"{fam.name}: second forward under inference_mode, after an edit outside it")
    assert _differs(ref, out0)
    _same(fam.run(m), ref, f"{fam.name}: the same model under no_grad, on the caches built under inference_mode")
    _edit_site(m, SITE_OF[family])
    _same(fam.run(m), fam.reference(m), f"{fam.name}: no_grad after another edit")


# ------------------------------------------------------------------------------------------------ bounded memory
def test_caches_stay_bounded_over_edit_forward_rounds_and_die_with_the_model():
    from laudnet_amd import ops
    fam = _resnet("channel")
    gc.collect()
    ops._SPLIT_CACHE.clear()
    n_before = len(ops._SPLIT_CACHE)
    m = fam.fresh()
    fam.run(m)
    fam.built(m)
    n_split, n_chain = len(ops._SPLIT_CACHE), len(m._chain_cache)
    assert n_split > 0, "the projections and stage 4's dense execution run on pre-split weights: the model must have entries"
    sites = ["chain_mid_conv2", "s2_b0_downsample", "s4_b0_conv1", "s3_b1_conv3", "s4_b0_conv2"]
    for r in range(10):
        _edit_site(m, (RESNET_SITES[sites[r % len(sites)]][0], lambda ts: [t.mul_(1.01) for t in ts]))
        fam.run(m)
        assert len(ops._SPLIT_CACHE) <= n_split, f"round {r}: ops._SPLIT_CACHE grew from {n_split} to {len(ops._SPLIT_CACHE)} entries"
        assert len(m._chain_cache) <= n_chain, f"round {r}: the chain cache grew to {len(m._chain_cache)} entries"
    _same(fam.run(m), fam.reference(m), "after the rounds")       # (reference() empties the split cache: the model's next forward refills it)
    fam.run(m)
    assert 0 < len(ops._SPLIT_CACHE) <= n_split
    del m
    gc.collect()
    assert len(ops._SPLIT_CACHE) == n_before, "split copies outlived the model that owned their sources"
