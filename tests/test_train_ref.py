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
   off in float64 is exactly 0 in the float32 run, and the refined bound never exceeds the unrefined formula's."""
import pytest
import torch

import train_ref as R
from fill import fill_state_dict, seeded_randn
from helpers import assert_close, block_input, load_golden, make_block, start_state

BLOCKS = dict(load_golden("blocks_s1.pt"))
BLOCKS.update(load_golden("blocks_s2.pt"))
ORACLE_BLOCKS = ["spatial_g4_s1", "spatial_g1_s2", "layer_s1", "layer_s2", "channel_g2_s1", "channel_g1_s2", "both_s1", "both_s2"]


def _against(ref, params, x, masks, forced):
    """oracle autograd in double against train_ref.gradients: forward and every gradient to 1e-9 of the tensor's scale"""
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
        assert w is not None and w.abs().max().item() > 0, k
        assert_close(grads[k], w, 1e-9 * w.abs().max().item(), 0, f"d {k}")


@pytest.mark.parametrize("name", ORACLE_BLOCKS)
def test_restatement_equals_oracle_resnet(name):
    from oracle import torch_ref as TR
    fx = BLOCKS[name]
    ref = make_block(TR.BottleneckRef, fx)
    params = R.params_from_state_dict(ref.state_dict(), kind="resnet", mode=fx["kw"]["dyn_mode"], stride=fx["kw"]["stride"])
    masks = {k: fx[k + "_mask"].float() for k in ("spatial", "channel") if fx.get(k + "_mask") is not None}

    def forced(blk, m):
        blk.forced_spatial_mask, blk.forced_channel_mask = m.get("spatial"), m.get("channel")

    _against(ref, params, block_input(fx), masks, forced)


def test_restatement_equals_oracle_regnet():
    from oracle import regnet_ref as RR
    win, wout, gw, stride, S = 32, 64, 16, 2, 8
    dyn = dict(spatial_mask_channel_group=1, channel_dyn_granularity=1, output_size=S, mask_spatial_granularity=S, dyn_mode="spatial")
    ref = RR.ResBlockRef(win, wout, stride, gw, 1.0, 0.25, **dyn).eval()
    ref.load_state_dict(fill_state_dict(ref.state_dict(), 31))
    params = R.params_from_state_dict(ref.state_dict(), kind="regnet", mode="layer", stride=stride, gw=gw)
    x = torch.relu(seeded_randn((3, win, S * stride, S * stride), 32))
    masks = {"spatial": torch.tensor(R.LAYER_MASK).view(3, 1, 1, 1)}

    def forced(blk, m):
        blk.f.forced_spatial_mask = m["spatial"]

    _against(ref, params, x, masks, forced)


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
