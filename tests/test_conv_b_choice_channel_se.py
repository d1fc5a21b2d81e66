"""The 'image_gap' form of LAD-RegNet's conv b chooser (channel mode with the SE block folded in, laud_regnet.USE_CHANNEL_SE_FUSED): its truth
table, and that nothing else moved.  No GPU: stubbed ops as in tests/test_conv_b_choice.py (tools/record_conv_b_choice.py), the library's
host-arithmetic fit queries."""
import importlib.util
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 24), (16, 32), (24, 48), (56, 112)]            # (group width, channels): the three widths of k_grouped_chan and one of k_grouped_wide
SITES = {"image": (7, 7, 1), "image:s2": (14, 7, 2)}         # the conv b sites of _run_channel in the record: Hi, Ho, stride
NEW_OPS = ["grouped_chan_mfma_conv3x3_image_gap", "se_gate_image"]


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("record_conv_b_choice", os.path.join(ROOT, "tools", "record_conv_b_choice.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def _drive(rec, R, fn, gw, w_b, Hi, Ho, stride, *extra):
    class F:
        group_width = gw
    p = {k: rec.tagged(k) for k in ("wb", "sb", "tb", "se_w1", "se_b1", "se_w2", "se_b2")}
    if gw == 16:
        p["wb_frag"] = rec.tagged("wb_frag")
    del rec.calls[:]
    out = fn(p, F, _Shape(4, Hi, Hi, w_b), None, None, _Shape(4, Ho, Ho, w_b), stride, *extra)      # (as the record drives the site)
    return out, list(rec.calls)


def test_truth_table_of_the_image_gap_form(rec, golden_dir, monkeypatch):
    """(family, 'image_gap') iff the plain 'image' form would be chosen on the matrix cores (USE_GROUPED_MFMA, USE_GROUPED_MFMA_CHANNEL, bf16x3,
    width 8 / 16 / 24 and a fitting map), USE_CHANNEL_SE_FUSED is on, ops.conv_image_gated_ok takes the block's conv c and the sums fit; then the
    site has called the gap op and se_gate_image and returns the gate.  Otherwise: exactly the calls of _conv_b_image, which are those of the
    record made in front of the chooser, whatever the new switch says."""
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
            fits = gw in (8, 16, 24) and ops.grouped_chan_mfma_ok(w_b, gw, Hi, Hi, stride) and ops.grouped_chan_mfma_gap_ok(w_b, gw, Hi, Hi, stride)
            assert fits == (gw != 56)
            for setting, new_on, gated in itertools.product(range(128), (False, True), (False, True)):
                rec.set_switches(setting)
                monkeypatch.setattr(R, "USE_CHANNEL_SE_FUSED", new_on)
                monkeypatch.setattr(ops, "conv_image_gated_ok", lambda *a, _g=gated: (asked.append(a), _g)[1])
                case = (gw, mode, site, setting, new_on, gated)
                plain_choice = R.conv_b_choice("image", w_b, gw, images=images)
                assert plain_choice[1] == "image" and R.conv_b_choice("image", w_b, gw, images=images, conv_c=w_b * 2) == plain_choice, case
                _, plain_calls = _drive(rec, R, R._conv_b_image, gw, w_b, Hi, Ho, stride)
                assert " ".join(plain_calls) == want[site, gw, w_b, mode, setting], case         # string for string the parent's
                del asked[:]
                choice = R.conv_b_choice("image", w_b, gw, images=images, se_fused=True, conv_c=2 * w_b)
                gate, calls = _drive(rec, R, R._conv_b_image_se, gw, w_b, Hi, Ho, stride, 2 * w_b)
                fused = bool(mode == "bf16x3" and R.USE_GROUPED_MFMA and R.USE_GROUPED_MFMA_CHANNEL and fits and new_on and gated)
                assert all(a == (4, Ho * Ho, w_b, 2 * w_b, True, True) for a in asked), (case, asked)
                if fused:
                    n_fused += 1
                    family = "g16" if gw == 16 else "gw"
                    frag = "wb_frag" if gw == 16 else "pack_grouped_mfma_weights"
                    op = "grouped_chan_mfma_conv3x3_image_gap"
                    assert choice == (family, "image_gap") and gate is not None, case
                    assert calls[-2:] == [f"{op}({frag},sb,tb)[relu=1]", f"se_gate_image({op},se_w1,se_b1,se_w2,se_b2)[relu=None]"], (case, calls)
                    assert calls[:-2] == plain_calls[:-1], case                                      # the same lazy pack of the fragments, if any
                else:
                    assert choice == plain_choice and gate is None and calls == plain_calls, (case, calls)
                    if not new_on:
                        assert asked == [], case                                                        # switch off: not even a question
                # without se_fused, and for a caller that names no conv c, nothing changes
                assert R.conv_b_choice("image", w_b, gw, images=images, se_fused=True) == plain_choice, case
    assert n_fused == 3 * 2 * 32           # three widths x two sites x the settings with the two old switches on


def test_run_channel_asks_the_chooser_only_behind_the_switch():
    """_run_channel reaches _conv_b_image_se only with USE_CHANNEL_SE_FUSED on: off, the module runs the code path it ran before"""
    import inspect
    from laudnet_amd import laud_regnet as R
    assert R.USE_CHANNEL_SE_FUSED is False, "off by default"
    src = inspect.getsource(R.ResBottleneckBlock._run_channel)
    assert "_conv_b_image_se(p, f, h_a, idx, cnt, h_b, s, cout) if USE_CHANNEL_SE_FUSED else _conv_b_image(p, f, h_a, idx, cnt, h_b, s)" in src
    for family in ("g16", "gw"):
        f = R.CONV_B[family].forms["image_gap"]
        assert (f.op, f.switch, f.fit) == ("grouped_chan_mfma_conv3x3_image_gap", "USE_CHANNEL_SE_FUSED", "grouped_chan_mfma_gap_ok")
    assert "image_gap" not in R.CONV_B["wide"].forms and "image_gap" not in R.CONV_B["valu"].forms
