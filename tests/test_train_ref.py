"""tests/train_ref.py on the CPU: the float64 restatement is tied to the oracle, every case of tests/test_hip_training_f64.py can be made
tie-free, and plain float32 torch meets the bound the HIP path is held to.

1. `block_f64` equals the oracle's autograd (oracle.torch_ref.BottleneckRef / oracle.regnet_ref.ResBlockRef in .double(), forced masks that
   require grad) on the committed fixtures -- one block of every mode and stride, one LAD-RegNet layer-skip block with a projection: the
   forward and every gradient to 1e-9 of the tensor's scale.
2. Every case of train_ref.CASES: `make_tie_free` succeeds with no bias moved by more than 0.25, the achieved clearance |z| / E(bf16x3) is at
   least 4 at every ReLU, every mask keeps and drops units, and the case's map is the LARGEST of its ladder at which that holds.
3. On those inputs the same restatement in float32 has EXACTLY the float64 gates at every ReLU, and every gradient is within 1e-3 of its
   tensor's own maximum, every element, no floor on the scale (measured: the worst tensor of any case sits at 9e-7, profiles/train_parity_f64.json).
4. The error bound's refinement (the previous layer's bound is propagated from the ON units only -- train_ref's module docstring): every unit that is
   off in float64 is exactly 0 in the float32 run, and the refined bound never exceeds the unrefined formula's.
5. BatchNorm scale variants (train_ref.VARIANT_CASES: zero, +-2^-24 and negated weights; the last BatchNorm's weight all zero): points 1 - 3 again
   on them, the default (no variant) bit for bit what it was, `mixed` is not vacuous (the zero-weight channels of the last BatchNorm carry a
   weight gradient of at least 0.1 of the tensor's maximum -- a hundred times the bound the HIP path is held to) and `zero_last` zeroes
   exactly the gradients in front of the last BatchNorm."""
import pytest
import torch

import train_ref as R
from fill import fill_state_dict, seeded_randn
from helpers import assert_close, block_input, load_golden, make_block, start_state

BLOCKS = dict(load_golden("blocks_s1.pt"))
BLOCKS.update(load_golden("blocks_s2.pt"))
ORACLE_BLOCKS = ["spatial_g4_s1", "spatial_g1_s2", "layer_s1", "layer_s2", "channel_g2_s1", "channel_g1_s2", "both_s1", "both_s2"]


def _against(ref, params, x, masks, forced, allow_zero=False):
    """oracle autograd in double against train_ref.gradients: forward and every gradient to 1e-9 of the tensor's scale.  allow_zero: a gradient
    may vanish in the oracle where the restatement's is identically zero too (edited BatchNorm scales); otherwise every one is non-zero."""
    ref = ref.double()
    xr = x.double().clone().requires_grad_(True)
    mr = {k: v.double().clone().requires_grad_(True) for k, v in masks.items()}
    forced(ref, mr)
    for p_ in ref.parameters():
        p_.requires_grad_(True)
    out_r = ref(start_state(xr), 1.0)[0]
    gout = seeded_randn(tuple(out_r.shape), 77)
    out_r.backward(gout.double())
    out, grads, _ = R.gradients(params, x, masks, gout)
    assert_close(out, out_r, 1e-9 * out_r.abs().max().item(), 0, "forward")
    want = {"x": xr.grad, **{f"mask.{k}": v.grad for k, v in mr.items()}}
    want.update({k: p_.grad for k, p_ in ref.named_parameters() if "masker" not in k})
    assert set(want) == set(grads), set(want) ^ set(grads)
    for k, w in want.items():
        assert w is not None, k
        if allow_zero and w.abs().max().item() == 0:
            assert grads[k].abs().max().item() == 0, f"d {k}: zero in the oracle, not in the restatement"
            continue
        assert w.abs().max().item() > 0, k
        assert_close(grads[k], w, 1e-9 * w.abs().max().item(), 0, f"d {k}")


def _oracle_resnet(name, variant=None):
    from oracle import torch_ref as TR
    fx = BLOCKS[name]
    ref = make_block(TR.BottleneckRef, fx)
    if variant is not None:
        ref.load_state_dict(R.edit_bn_weights(ref.state_dict(), variant))
    params = R.params_from_state_dict(ref.state_dict(), kind="resnet", mode=fx["kw"]["dyn_mode"], stride=fx["kw"]["stride"])
    masks = {k: fx[k + "_mask"].float() for k in ("spatial", "channel") if fx.get(k + "_mask") is not None}

    def forced(blk, m):
        blk.forced_spatial_mask, blk.forced_channel_mask = m.get("spatial"), m.get("channel")

    _against(ref, params, block_input(fx), masks, forced, allow_zero=variant is not None)


@pytest.mark.parametrize("name", ORACLE_BLOCKS)
def test_restatement_equals_oracle_resnet(name):
    _oracle_resnet(name)


@pytest.mark.parametrize("name", ["both_s2", "channel_g2_s1"])
def test_restatement_equals_oracle_resnet_mixed_scales(name):
    """the same identity with zero, +-2^-24 and negated BatchNorm weights in the fixture's state dict (the projection's included)"""
    _oracle_resnet(name, "mixed")


def _oracle_regnet(variant=None):
    from oracle import regnet_ref as RR
    win, wout, gw, stride, S = 32, 64, 16, 2, 8
    dyn = dict(spatial_mask_channel_group=1, channel_dyn_granularity=1, output_size=S, mask_spatial_granularity=S, dyn_mode="spatial")
    ref = RR.ResBlockRef(win, wout, stride, gw, 1.0, 0.25, **dyn).eval()
    ref.load_state_dict(fill_state_dict(ref.state_dict(), 31))
    if variant is not None:
        ref.load_state_dict(R.edit_bn_weights(ref.state_dict(), variant))
    params = R.params_from_state_dict(ref.state_dict(), kind="regnet", mode="layer", stride=stride, gw=gw)
    x = torch.relu(seeded_randn((3, win, S * stride, S * stride), 32))
    masks = {"spatial": torch.tensor(R.LAYER_MASK).view(3, 1, 1, 1)}

    def forced(blk, m):
        blk.f.forced_spatial_mask = m["spatial"]

    _against(ref, params, x, masks, forced, allow_zero=variant is not None)


def test_restatement_equals_oracle_regnet():
    _oracle_regnet()


def test_restatement_equals_oracle_regnet_mixed_scales():
    _oracle_regnet("mixed")


def test_case_parameters_are_the_seeded_fill_of_the_modules():
    """train_ref fills its own template of a block's state dict: the values must be those a module of the same seed is filled with (what the
    GPU test loads into the HIP block before it overrides the moved biases)"""
    from oracle import regnet_ref as RR
    from oracle import torch_ref as TR
    for name in ("narrow_s2_both", "wide_s1_layer", "regnet_gw16_s2_proj", "regnet_gw24_s1"):
        fx = R.case_fixture(name)
        if fx["kind"] == "resnet":
            sd = make_block(TR.BottleneckRef, fx).state_dict()
        else:
            dyn = dict(spatial_mask_channel_group=1, channel_dyn_granularity=1, output_size=fx["output_size"],
                       mask_spatial_granularity=fx["output_size"], dyn_mode="spatial")
            blk = RR.ResBlockRef(*fx["widths"], fx["stride"], fx["gw"], 1.0, 0.25, **dyn)
            sd = fill_state_dict(blk.state_dict(), fx["seed"])
        mine = R.case_params(fx)["sd"]
        theirs = {k: v for k, v in sd.items() if "masker" not in k and not k.endswith("num_batches_tracked")}
        assert set(mine) == set(theirs), set(mine) ^ set(theirs)
        for k, v in theirs.items():
            assert torch.equal(mine[k], v.double()), k


@pytest.mark.parametrize("name", R.CASES)
def test_every_gpu_case_can_be_made_tie_free(name):
    case = R.tie_free_case(name)                    # (raises where a channel has no gap within the cap)
    assert case.moved <= R.MAX_MOVE, case.moved
    assert case.clearance >= R.CLEARANCE, case.clearance
    assert R.clearance(case.params, case.x, case.masks) == case.clearance
    assert R.clearance(case.params0, case.x, case.masks) < 1.0, "the seeded block already had no near-tie: the construction is not exercised"
    assert R.masks_keep_and_drop(case.masks), "every mask must keep and drop units"
    for k, v in case.params["sd"].items():          # only biases moved, and they stay float32 values
        if not torch.equal(v, case.params0["sd"][k]):
            assert k.endswith(".bias") and torch.equal(v, v.float().double()) and (v - case.params0["sd"][k]).abs().max().item() <= R.MAX_MOVE, k
    # the table's map is the largest of the ladder that can be made tie-free (never a smaller one than necessary, never a reduced factor)
    assert R.find_map(name) == R._MAPS[name], (R.find_map(name), R._MAPS[name])
    assert R.CLEARANCE == 4.0 and R.MAX_MOVE == 0.25 and R.EPS == {"fp32": 2.0 ** -23, "bf16x3": 2.0 ** -15}


def test_the_table_keeps_the_intended_seams():
    """every narrow case and at least one mid case per stride runs on the intended map: more than 256 rows (a second, ragged row tile)"""
    rows = {n: R.BATCH * R._MAPS[n][0] ** 2 for n in R.CASES}
    assert all(rows[n] > 256 for n in R.CASES if n.startswith("narrow")), rows
    for stride in ("s1", "s2"):
        assert any(rows[n] > 256 for n in R.CASES if n.startswith(f"mid_{stride}")), rows
    assert {R._REGNET[n][2] for n in R._REGNET} == {8, 16, 24}
    assert [R._REGNET[n][3] for n in R._REGNET].count(2) >= 1 and [R._REGNET[n][3] for n in R._REGNET].count(1) >= 1


@pytest.mark.parametrize("name", R.CASES)
def test_float32_reference_alone_meets_the_gpu_bound(name):
    out64, want, gates64 = R.reference(name)
    out32, got, gates32 = R.reference(name, torch.float32)
    for site, g in gates64.items():
        assert torch.equal(g, gates32[site]), f"{site}: float32 flipped {int((g != gates32[site]).sum())} gates on tie-free inputs"
    assert_close(out32, out64, 1e-3 * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out32 > 0, out64 > 0)
    assert set(got) == set(want)
    for k, w in want.items():
        scale = w.abs().max().item()
        assert scale > 0, f"d {k}: the reference gradient vanishes"
        err = assert_close(got[k], w, 1e-3 * scale, 0, f"d {k}")
        print(f"train_ref float32 {name}: d {k} ratio {err / scale:.3e}")


@pytest.mark.parametrize("name", R.CASES)
def test_off_units_are_exactly_zero_in_float32(name):
    """What the refinement of train_ref.forward_error_bound rests on (E_prev is propagated from the ON units only): on the tie-free inputs a
    unit that is off in float64 is EXACTLY 0 in the float32 run, at every tensor a later layer reads -- so it carries no error forward."""
    case = R.tie_free_case(name)
    with torch.no_grad():
        _, r64 = R._forward(case.params, case.x, case.masks, torch.float64)
        _, r32 = R._forward(case.params, case.x, case.masks, torch.float32)
    pairs = [("relu1", "relu2"), ("relu2", "branch")] if case.fx["kind"] == "resnet" else [("relu_a", "relu_b"), ("relu_b", "branch")]
    for site, reader in pairs:                      # r[reader].a is what the next convolution reads: relu(z) (times SE's gate for conv c)
        off = r64[site].z <= 0
        assert bool(off.any()) and bool((~off).any()), site
        assert bool((r32[reader].a[off] == 0).all()) and bool((r64[reader].a[off] == 0).all()), f"{site}: an off unit is not exactly zero"
        assert bool((r32[reader].a[~off] > 0).all()), f"{site}: an on unit of float64 is off in float32"
    if case.fx["kind"] == "regnet":
        assert torch.equal(r32["se"].u > 0, r64["se"].u > 0)


@pytest.mark.parametrize("name", R.CASES)
def test_refined_bound_against_the_unrefined_formula(name):
    """The refinement only ever removes the off units' share: the unrefined bound (gated=False) is never smaller at any unit, and equal at the
    first layer, whose input is exact.  Prints the committed case's clearance under both (the unrefined one is below 4 for most cases: the
    module docstring of train_ref states that, and that four wide cases admit no tie-free map under it)."""
    case = R.tie_free_case(name)
    refined = R.forward_error_bound(case.params, case.x, case.masks, "bf16x3")
    plain = R.forward_error_bound(case.params, case.x, case.masks, "bf16x3", gated=False)
    assert [s[:2] for s in refined] == [s[:2] for s in plain]
    assert torch.equal(refined[0][3], plain[0][3])
    for (site, _, _, E, sel), (_, _, _, E0, _) in zip(refined, plain):
        assert bool((E <= E0).all()) and bool((E[sel] > 0).all()), site
    print(f"train_ref {name}: clearance {case.clearance:.2f}, under the unrefined formula {R.clearance(case.params, case.x, case.masks, gated=False):.2f}")


# ------------------------------------------------------------------------------------------------------------------ BatchNorm scale variants
VARIANT_IDS = [f"{n}-{v}" for n, v in R.VARIANT_CASES]


def test_variant_table():
    assert len(R.VARIANT_CASES) == 22 and set(R.VARIANT_BASES) <= set(R.CASES) and R.VARIANTS == ("mixed", "zero_last") and R.TINY == 2.0 ** -24


@pytest.mark.parametrize("name", ["narrow_s1_spatial", "narrow_s1_layer", "narrow_s2_channel", "mid_s1_both", "regnet_gw16_s2_proj"])
def test_no_variant_is_bit_for_bit_the_old_construction(name):
    """one case per kind: tie_free_case(name) -- variant None -- against the construction spelled out without the variant code path"""
    fx = R.case_fixture(name)
    params0 = R.case_params(fx)
    params, got, moved = R.make_tie_free(params0, R.case_input(fx), fx["masks"])
    case = R.tie_free_case(name)
    assert case.variant is None and (case.clearance, case.moved) == (got, moved)
    for mine, theirs in ((case.params0, params0), (case.params, params)):
        assert set(mine["sd"]) == set(theirs["sd"]) and mine["cfg"] == theirs["cfg"]
        for k, v in theirs["sd"].items():
            assert torch.equal(mine["sd"][k], v), k
    assert torch.equal(R.case_gout(case), R.case_gout(case, None))
    for a, b in zip(R.reference(name)[1].values(), R.gradients(params, R.case_input(fx), fx["masks"], R.case_gout(case))[1].values()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,variant", R.VARIANT_CASES, ids=VARIANT_IDS)
def test_every_variant_case_can_be_made_tie_free(name, variant):
    case = R.tie_free_case(name, variant)           # (raises where a channel has no gap within the cap)
    assert case.moved <= R.MAX_MOVE, case.moved
    assert case.clearance >= R.CLEARANCE, case.clearance
    assert R.clearance(case.params, case.x, case.masks) == case.clearance
    assert R.masks_keep_and_drop(case.masks), "every mask must keep and drop units"
    # params0 is the EDITED seeded fill: exactly the variant's edit of the base case's, weights of BatchNorms only
    base0 = R.tie_free_case(name).params0["sd"]
    edited = R.edit_bn_weights({k: v.clone() for k, v in base0.items()}, variant)
    lb = R.last_bn(base0)
    for k, v in case.params0["sd"].items():
        assert torch.equal(v, edited[k]), k
        if not torch.equal(v, base0[k]):
            assert k.endswith(".weight") and k[:-6] + "running_var" in base0, k
    if variant == "zero_last":
        assert [k for k in base0 if not torch.equal(base0[k], case.params0["sd"][k])] == [lb + ".weight"]
        assert bool((case.params0["sd"][lb + ".weight"] == 0).all())
    else:
        for k in (k for k in base0 if k.endswith("running_var")):
            w, w0, cls = case.params0["sd"][k[:-11] + "weight"], base0[k[:-11] + "weight"], R.mixed_classes(base0[k].numel())
            assert bool((w[cls["zero"]] == 0).all()) and torch.equal(w[cls["negated"]], -w0[cls["negated"]])
            assert bool((w[cls["tiny"]] == R.TINY).all()) and bool((w[cls["neg_tiny"]] == -R.TINY).all())
            rest = ~(cls["zero"] | cls["negated"] | cls["tiny"] | cls["neg_tiny"])
            assert torch.equal(w[rest], w0[rest]) and all(bool(m.any()) for m in cls.values()) and bool(rest.any())
    for k, v in case.params["sd"].items():          # relative to the edited fill only biases moved, and they stay float32 values
        if not torch.equal(v, case.params0["sd"][k]):
            assert k.endswith(".bias") and torch.equal(v, v.float().double()) and (v - case.params0["sd"][k]).abs().max().item() <= R.MAX_MOVE, k
        assert torch.equal(v, v.float().double()), f"{k} is not a float32 value"
    # the folded scale of a zero weight is exactly 0
    s = R._fold(case.params["sd"], lb)[0]
    assert bool((s[case.params["sd"][lb + ".weight"] == 0] == 0).all())


@pytest.mark.parametrize("name,variant", R.VARIANT_CASES, ids=VARIANT_IDS)
def test_float32_reference_alone_meets_the_gpu_bound_on_variants(name, variant):
    out64, want, gates64 = R.reference(name, variant=variant)
    out32, got, gates32 = R.reference(name, torch.float32, variant)
    for site, g in gates64.items():
        assert torch.equal(g, gates32[site]), f"{site}: float32 flipped {int((g != gates32[site]).sum())} gates on tie-free inputs"
    assert_close(out32, out64, 1e-3 * out64.abs().max().item(), 0, "forward")
    assert torch.equal(out32 > 0, out64 > 0)
    assert set(got) == set(want)
    for k, w in want.items():
        scale = w.abs().max().item()
        if scale == 0:
            assert got[k].abs().max().item() == 0, f"d {k}: identically zero in float64, not in float32"
            continue
        err = assert_close(got[k], w, 1e-3 * scale, 0, f"d {k}")
        print(f"train_ref float32 {name}/{variant}: d {k} ratio {err / scale:.3e}")


@pytest.mark.parametrize("name", R.VARIANT_BASES)
def test_mixed_is_not_vacuous(name):
    """the last BatchNorm's weight gradient over its ZERO-weight channels is at least 0.1 of the tensor's maximum (measured: 0.14 at the least,
    regnet_gw16_s2_proj) -- what (h - t) / s returns 0 for -- and does not vanish over the 2^-24 channels; no gradient of the case vanishes"""
    case = R.tie_free_case(name, "mixed")
    _, want, _ = R.reference(name, variant="mixed")
    g = want[R.last_bn(case.params["sd"]) + ".weight"]
    cls, top = R.mixed_classes(g.numel()), g.abs().max().item()
    assert g[cls["zero"]].abs().max().item() >= 0.1 * top, g[cls["zero"]].abs().max().item() / top
    assert g[cls["tiny"]].abs().max().item() > 0 and g[cls["neg_tiny"]].abs().max().item() > 0
    for k, w in want.items():
        assert w.abs().max().item() > 0, k


@pytest.mark.parametrize("name", R.VARIANT_BASES)
def test_zero_last_zeroes_exactly_what_lies_in_front_of_the_last_batchnorm(name):
    case = R.tie_free_case(name, "zero_last")
    _, want, _ = R.reference(name, variant="zero_last")
    if case.fx["kind"] == "resnet":
        expect = {"conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias"}
        if "channel" in case.masks:
            expect.add("mask.channel")
    else:
        expect = {"f.a.0.weight", "f.b.0.weight", "f.c.0.weight", "f.a.1.weight", "f.a.1.bias", "f.b.1.weight", "f.b.1.bias",
                  "f.se.fc1.weight", "f.se.fc1.bias", "f.se.fc2.weight", "f.se.fc2.bias"}
    assert {k for k, w in want.items() if w.abs().max().item() == 0} == expect
