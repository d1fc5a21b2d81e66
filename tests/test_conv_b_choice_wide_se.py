"""The 'image_gap_wide' form of LAD-RegNet's conv b chooser (channel mode with the SE block folded in at group widths 56, 112 and 232:
laud_regnet.USE_CHANNEL_SE_FUSED_WIDE on top of USE_CHANNEL_SE_FUSED): its truth table, and that nothing else moved.  No GPU: stubbed ops as in
tests/test_conv_b_choice_channel_se.py (tools/record_conv_b_choice.py), the library's host-arithmetic fit queries."""
import itertools
import json
import os

import pytest

import test_conv_b_choice_channel_se as S

SHAPES = [(56, 112), (112, 224), (232, 464)]                  # (group width, channels): the three widths of k_grouped_wide, two groups each
NARROW = [(8, 24), (16, 32), (24, 48)]                       # ... and of k_grouped_chan, which keep the form 'image_gap'
SITES = S.SITES
NEW_OPS = S.NEW_OPS + ["grouped_wide_conv3x3_image_gap"]
rec = S.rec                                                    # (the module-scoped fixture that loads tools/record_conv_b_choice.py)


def _recorded(want, site, gw, w_b, mode, setting):
    """the parent's calls at the site.  The record holds widths 56 and 112 of the wide family; width 232 joined the family after it was made
    and is compared with the record of width 112: a record names tagged tensors, ops and packers, never a width, and
    tests/test_grouped_wide_232_abi.py pins that the chooser treats the three widths alike."""
    return want[(site, 112, 224, mode, setting) if gw == 232 else (site, gw, w_b, mode, setting)]


def test_truth_table_of_the_image_gap_wide_form(rec, golden_dir, monkeypatch):
    """('wide', 'image_gap_wide') iff the plain 'image' form of the wide family would be chosen (USE_GROUPED_MFMA, USE_GROUPED_MFMA_WIDE,
    bf16x3, a fitting map), USE_CHANNEL_SE_FUSED and USE_CHANNEL_SE_FUSED_WIDE are both on, ops.conv_image_gated_ok takes the block's conv c
    and the sums fit; then the site has called the gap op and se_gate_image and returns the gate.  Otherwise: exactly the calls of
    _conv_b_image, which are those of the record made in front of the chooser, whatever the new switches say -- and with either of them off
    conv_image_gated_ok is not even asked."""
    from laudnet_amd import laud_regnet as R, ops
    with open(os.path.join(golden_dir, "conv_b_choice.json")) as fh:
        want = rec.ungrouped(json.load(fh))
    asked = []
    n_fused = 0
    with rec.stubbed():
        for n in NEW_OPS:
            monkeypatch.setattr(ops, n, rec._stub(n))
        for (gw, w_b), mode, (site, (Hi, Ho, stride)) in itertools.product(SHAPES, rec.MODES, SITES.items()):
            ops.set_math_mode(mode)
            images = (4, Hi, Hi, Ho, Ho, stride)
            assert ops.grouped_wide_ok(w_b, gw, Hi, Hi, stride) and ops.grouped_wide_gap_ok(w_b, gw, Hi, Hi, stride)
            for setting, se_on, wide_on, gated in itertools.product(range(128), (False, True), (False, True), (False, True)):
                rec.set_switches(setting)
                monkeypatch.setattr(R, "USE_CHANNEL_SE_FUSED", se_on)
                monkeypatch.setattr(R, "USE_CHANNEL_SE_FUSED_WIDE", wide_on)
                monkeypatch.setattr(ops, "conv_image_gated_ok", lambda *a, _g=gated: (asked.append(a), _g)[1])
                case = (gw, mode, site, setting, se_on, wide_on, gated)
                plain_choice = R.conv_b_choice("image", w_b, gw, images=images)
                assert plain_choice[1] == "image" and R.conv_b_choice("image", w_b, gw, images=images, conv_c=w_b * 2) == plain_choice, case
                _, plain_calls = S._drive(rec, R, R._conv_b_image, gw, w_b, Hi, Ho, stride)
                assert " ".join(plain_calls) == _recorded(want, site, gw, w_b, mode, setting), case         # string for string the parent's
                del asked[:]
                choice = R.conv_b_choice("image", w_b, gw, images=images, se_fused=True, conv_c=2 * w_b)
                gate, calls = S._drive(rec, R, R._conv_b_image_se, gw, w_b, Hi, Ho, stride, 2 * w_b)
                fused = bool(mode == "bf16x3" and R.USE_GROUPED_MFMA and R.USE_GROUPED_MFMA_WIDE and se_on and wide_on and gated)
                assert all(a == (4, Ho * Ho, w_b, 2 * w_b, True, True) for a in asked), (case, asked)
                if fused:
                    n_fused += 1
                    op = "grouped_wide_conv3x3_image_gap"
                    assert choice == ("wide", "image_gap_wide") and gate is not None, case
                    assert calls[-2:] == [f"{op}(pack_grouped_wide_weights,sb,tb)[relu=1]",
                                          f"se_gate_image({op},se_w1,se_b1,se_w2,se_b2)[relu=None]"], (case, calls)
                    assert calls[:-2] == plain_calls[:-1] == ["pack_grouped_wide_weights(wb)"], case       # the same lazy pack of the fragments
                else:
                    assert choice == plain_choice and gate is None and calls == plain_calls, (case, calls)
                    if not (se_on and wide_on):
                        assert asked == [], case                                                        # a switch off: not even a question
                # without se_fused, and for a caller that names no conv c, nothing changes
                assert R.conv_b_choice("image", w_b, gw, images=images, se_fused=True) == plain_choice, case
    assert n_fused == 3 * 2 * 32           # three widths x two sites x the settings with the two old switches on


def test_the_narrow_widths_never_take_the_wide_form(rec, monkeypatch):
    """widths 8 / 16 / 24 answer 'image_gap' or 'image' whatever USE_CHANNEL_SE_FUSED_WIDE says, and the wide form's switch alone folds nothing"""
    from laudnet_amd import laud_regnet as R, ops
    with rec.stubbed():
        for n in NEW_OPS:
            monkeypatch.setattr(ops, n, rec._stub(n))
        monkeypatch.setattr(ops, "conv_image_gated_ok", lambda *a: True)
        ops.set_math_mode("bf16x3")
        for (gw, w_b), (site, (Hi, Ho, stride)), setting, se_on in itertools.product(NARROW + SHAPES, SITES.items(), range(128), (False, True)):
            rec.set_switches(setting)
            monkeypatch.setattr(R, "USE_CHANNEL_SE_FUSED", se_on)
            images = (4, Hi, Hi, Ho, Ho, stride)
            monkeypatch.setattr(R, "USE_CHANNEL_SE_FUSED_WIDE", False)
            off = R.conv_b_choice("image", w_b, gw, images=images, se_fused=True, conv_c=2 * w_b)
            monkeypatch.setattr(R, "USE_CHANNEL_SE_FUSED_WIDE", True)
            on = R.conv_b_choice("image", w_b, gw, images=images, se_fused=True, conv_c=2 * w_b)
            if (gw, w_b) in NARROW:
                assert on == off and on[1] in ("image", "image_gap") and on[0] != "wide", (gw, site, setting, se_on)
            else:
                assert off[1] == "image" and (se_on or on == off), (gw, site, setting, se_on)


def test_the_switch_is_off_by_default_and_the_form_has_its_own_key():
    import inspect
    from laudnet_amd import laud_regnet as R
    assert R.USE_CHANNEL_SE_FUSED_WIDE is False and R.USE_CHANNEL_SE_FUSED is False, "off by default"
    assert "LDN_CHANNEL_SE_FUSED_WIDE" in inspect.getsource(R)
    f = R.CONV_B["wide"].forms["image_gap_wide"]
    assert (f.op, f.switch, f.fit) == ("grouped_wide_conv3x3_image_gap", "USE_CHANNEL_SE_FUSED_WIDE", "grouped_wide_gap_ok")
    assert "image_gap" not in R.CONV_B["wide"].forms
    assert all("image_gap_wide" not in R.CONV_B[k].forms for k in ("valu", "g16", "gw"))
