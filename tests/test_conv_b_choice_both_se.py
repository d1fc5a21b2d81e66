"""The conv_c_rows='packed' question of LAD-RegNet's conv b chooser ('both' mode with the SE block folded in: laud_regnet.USE_BOTH_SE_FUSED on
top of the channel-mode fold's switches of the width): its truth table, and that nothing else moved.  No GPU: stubbed ops as in
tests/test_conv_b_choice_channel_se.py (tools/record_conv_b_choice.py), the library's host-arithmetic fit queries."""
import inspect
import itertools
import json
import os

import test_conv_b_choice_channel_se as S

SHAPES = [(8, 24), (16, 32), (24, 48), (56, 112)]            # (group width, channels): the three widths of k_grouped_chan and one of k_grouped_wide
SITES = S.SITES
NEW_OPS = S.NEW_OPS + ["grouped_wide_conv3x3_image_gap"]
rec = S.rec                                                    # (the module-scoped fixture that loads tools/record_conv_b_choice.py)


def _gap(gw):
    """(family, form, op, fragments) of the width's gap form"""
    if gw == 56:
        return "wide", "image_gap_wide", "grouped_wide_conv3x3_image_gap", "pack_grouped_wide_weights"
    return ("g16" if gw == 16 else "gw"), "image_gap", "grouped_chan_mfma_conv3x3_image_gap", ("wb_frag" if gw == 16 else "pack_grouped_mfma_weights")


def test_truth_table_of_the_packed_conv_c_question(rec, golden_dir, monkeypatch):
    """With conv_c_rows='packed' the answer is the width's gap form iff the channel-mode fold would be taken there (the plain 'image' form on
    the matrix cores, USE_CHANNEL_SE_FUSED, at width 56 USE_CHANNEL_SE_FUSED_WIDE, the sums fit), USE_BOTH_SE_FUSED is on and
    ops.conv_packed_gated_ok takes one mask group's conv c; ops.conv_image_gated_ok is never asked.  Otherwise: exactly the calls of
    _conv_b_image, those of the record made in front of the chooser.  With a switch off the query is not even asked."""
    from laudnet_amd import laud_regnet as R, ops
    with open(os.path.join(golden_dir, "conv_b_choice.json")) as fh:
        want = rec.ungrouped(json.load(fh))
    asked, asked_image = [], []
    n_fused = 0
    with rec.stubbed():
        for n in NEW_OPS:
            monkeypatch.setattr(ops, n, rec._stub(n))
        monkeypatch.setattr(ops, "conv_image_gated_ok", lambda *a: (asked_image.append(a), True)[1])
        for (gw, w_b), mode, (site, (Hi, Ho, stride)) in itertools.product(SHAPES, rec.MODES, SITES.items()):
            ops.set_math_mode(mode)
            images = (4, Hi, Hi, Ho, Ho, stride)
            conv_c = w_b                                # two mask groups over 2 * w_b output channels
            family, form, op, frag = _gap(gw)
            for setting, both_on, se_on, wide_on, gated in itertools.product(range(128), *[(False, True)] * 4):
                rec.set_switches(setting)
                monkeypatch.setattr(R, "USE_BOTH_SE_FUSED", both_on)
                monkeypatch.setattr(R, "USE_CHANNEL_SE_FUSED", se_on)
                monkeypatch.setattr(R, "USE_CHANNEL_SE_FUSED_WIDE", wide_on)
                monkeypatch.setattr(ops, "conv_packed_gated_ok", lambda *a, _g=gated: (asked.append(a), _g)[1])
                case = (gw, mode, site, setting, both_on, se_on, wide_on, gated)
                plain_choice = R.conv_b_choice("image", w_b, gw, images=images)
                _, plain_calls = S._drive(rec, R, R._conv_b_image, gw, w_b, Hi, Ho, stride)
                assert " ".join(plain_calls) == want[site, gw, w_b, mode, setting], case         # string for string the parent's
                # without the new keyword every answer is today's: the channel-mode question, whatever USE_BOTH_SE_FUSED says
                del asked[:], asked_image[:]
                channel_choice = R.conv_b_choice("image", w_b, gw, images=images, se_fused=True, conv_c=2 * w_b)
                mfma = bool(mode == "bf16x3" and R.USE_GROUPED_MFMA and (R.USE_GROUPED_MFMA_WIDE if gw == 56 else R.USE_GROUPED_MFMA_CHANNEL))
                channel_fold = mfma and se_on and (wide_on or gw != 56)
                assert channel_choice == ((family, form) if channel_fold else plain_choice) and asked == [], case
                assert asked_image == ([(4, Ho * Ho, w_b, 2 * w_b, True, True)] if channel_fold else []), case
                assert R.conv_b_choice("image", w_b, gw, images=images, se_fused=True, conv_c=2 * w_b, conv_c_rows=None) == channel_choice, case
                # with it
                del asked[:], asked_image[:]
                choice = R.conv_b_choice("image", w_b, gw, images=images, se_fused=True, conv_c=conv_c, conv_c_rows="packed")
                gate, calls = S._drive(rec, R, R._conv_b_image_se, gw, w_b, Hi, Ho, stride, conv_c, "packed")
                assert asked_image == [], case
                assert all(a == (4, Ho * Ho, w_b, conv_c, True, True) for a in asked), (case, asked)
                if channel_fold and both_on:
                    assert len(asked) == 2, case                                                       # the chooser and the site, once each
                else:
                    assert asked == [], case                                                           # a switch off: not even a question
                if channel_fold and both_on and gated:
                    n_fused += 1
                    assert choice == (family, form) and gate is not None, case
                    assert calls[-2:] == [f"{op}({frag},sb,tb)[relu=1]", f"se_gate_image({op},se_w1,se_b1,se_w2,se_b2)[relu=None]"], (case, calls)
                    assert calls[:-2] == plain_calls[:-1], case                                      # the same lazy pack of the fragments, if any
                else:
                    assert choice == plain_choice and gate is None and calls == plain_calls, (case, calls)
                # for a caller that names no conv c, nothing changes
                assert R.conv_b_choice("image", w_b, gw, images=images, se_fused=True, conv_c_rows="packed") == plain_choice, case
                assert R.conv_b_choice("image", w_b, gw, images=images, conv_c=conv_c, conv_c_rows="packed") == plain_choice, case
    # two sites x the 32 settings with the width's two old switches on x (three narrow widths, whatever the wide fold's switch says, + width
    # 56 with it on)
    assert n_fused == 2 * 32 * (3 * 2 + 1)


def test_the_both_branch_asks_the_chooser_only_behind_the_switch():
    """_run_spatial_general reaches _conv_b_image_se only with USE_BOTH_SE_FUSED on: off, the module runs the code path it ran before; the
    patch-mask 'spatial' branch is left alone"""
    from laudnet_amd import laud_regnet as R
    assert R.USE_BOTH_SE_FUSED is False, "off by default"
    assert 'os.environ.get("LDN_BOTH_SE_FUSED", "0") == "1"' in inspect.getsource(R)
    src = inspect.getsource(R.ResBottleneckBlock._run_spatial_general)
    assert '_conv_b_image_se(p, f, h_a, idx, cnt, h_b, s, cout // G, "packed") if USE_BOTH_SE_FUSED else _conv_b_image(p, f, h_a, idx, cnt, h_b, s)' in src
    assert src.count("ops.conv_packed_gated(") == 1 and src.count("ops.conv_packed(") == 1 and src.count("ops.se_packed(") == 2
    assert "conv_c_rows" not in inspect.getsource(R.ResBottleneckBlock._run_channel)
    assert inspect.signature(R.conv_b_choice).parameters["conv_c_rows"].default is None
