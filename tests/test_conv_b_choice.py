"""The one chooser of LAD-RegNet's conv b makes the choices the five hand-written dispatch ladders made.  No GPU: stubbed ops, the library's
host-arithmetic fit queries.

tests/golden/conv_b_choice.json is the output of tools/record_conv_b_choice.py on the commit in front of the chooser (every call site x 128
switch settings x 2 math modes x 6 shapes).  The record of the working tree must equal it except for the ONE correction the chooser makes:
training._conv_b_plain said it follows _conv_b_rows but ran the width-16 matrix-core kernel with USE_GROUPED_MFMA off (bf16x3 mode), because
training._conv_b_params packed wb_frag without looking at the switch.  Both now follow the switch: the exception set below, spelled out.
The SE-fused site was inline before and is checked against its rule written out as a truth table."""
import importlib.util
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("record_conv_b_choice", os.path.join(ROOT, "tools", "record_conv_b_choice.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_site_makes_the_parents_choice(rec, golden_dir):
    with open(os.path.join(golden_dir, "conv_b_choice.json")) as fh:
        want = rec.ungrouped(json.load(fh))
    got = rec.record()
    assert got.keys() == want.keys() and len(got) == 11 * 128 * 2 * 6
    corrected = {"plain": ("pack_grouped16_weights(wbr) grouped16_conv3x3_rows(pack_grouped16_weights)[relu=0]", "grouped_conv3x3_rows(wbr)[relu=0]"),
                 "params": ("sb,tb,wb,wb_frag", "sb,tb,wb")}
    n_corrected = 0
    for case, outcome in got.items():
        site, gw, w_b, mode, setting = case
        if site in corrected and gw == 16 and mode == "bf16x3" and not setting >> rec.SWITCHES.index("USE_GROUPED_MFMA") & 1:
            assert (want[case], outcome) == corrected[site], case           # g16 at the parent -> valu now, and nothing packed for it
            n_corrected += 1
        else:
            assert outcome == want[case], case
    assert n_corrected == 2 * 64


IMAGES = [(4, 7, 7, 7, 7, 1), (4, 14, 14, 7, 7, 2), (1, 8, 1 << 20, 8, 1 << 20, 1), (4, 9, 9, 3, 3, 3)]


def test_se_fused_site_follows_its_rule(rec, monkeypatch):
    """_conv_b_rows_se returns a gate iff USE_SE_FUSED, ops.conv_rows_gated_fits and the whole-image rule of the width hold (all matrix-core
    families need USE_GROUPED_MFMA and bf16x3 mode; width 16: USE_GROUPED_IMAGES and a fitting map; widths 8 / 24: USE_GROUPED_MFMA_WIDTHS,
    USE_GROUPED_MFMA_WIDTHS_IMAGES, stride 1 or 2 and a fitting map; widths 56 / 112 and the VALU kernel: never).  Then it has called the
    family's *_images_gap and se_gate_slots; otherwise exactly what _conv_b_rows calls.  At most one fit query either way."""
    from laudnet_amd import laud_regnet as R, ops
    queries = []
    for name in ("grouped16_images_fit", "grouped_mfma_images_fit", "grouped_mfma_ok", "grouped_wide_rows_ok"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _n=name: (queries.append(_n), _real(*a))[1])
    with rec.stubbed():
        for (gw, w_b), mode, images in itertools.product(rec.SHAPES, rec.MODES, IMAGES):
            ops.set_math_mode(mode)
            _, Hi, Wi, Ho, Wo, stride = images
            fit16 = gw == 16 and ops.grouped16_images_fit(Hi, Wi, w_b) > 0
            fitgw = gw in (8, 24) and ops.grouped_mfma_images_fit(Hi, Wi, w_b, gw) > 0

            class F:
                group_width = gw
            for setting, se_on, gated in itertools.product(range(128), (False, True), (False, True)):
                rec.set_switches(setting)
                monkeypatch.setattr(R, "USE_SE_FUSED", se_on)
                monkeypatch.setattr(ops, "conv_rows_gated_fits", lambda C, rows, _g=gated: _g)
                mfma = R.USE_GROUPED_MFMA and mode == "bf16x3"
                whole = mfma and ((R.USE_GROUPED_IMAGES and fit16) or
                                  (R.USE_GROUPED_MFMA_WIDTHS and R.USE_GROUPED_MFMA_WIDTHS_IMAGES and stride in (1, 2) and fitgw))
                p = {k: rec.tagged(k) for k in ("wb", "sb", "tb", "se_w1", "se_b1", "se_w2", "se_b2")}
                if gw == 16:
                    p["wb_frag"] = rec.tagged("wb_frag")
                args = (F, rec.tagged("h_a"), None, type("H", (), {"shape": (Ho * Wo * 4, w_b)}), rec.tagged("cnt"), 196)
                del rec.calls[:], queries[:]
                gate = R._conv_b_rows_se(dict(p), *args, images)
                fused, n_queries = list(rec.calls), len(queries)
                del rec.calls[:]
                R._conv_b_rows(dict(p), *args, images=images)
                case = (gw, mode, images, setting, se_on, gated)
                assert n_queries <= 1, (case, queries)
                if se_on and gated and whole:
                    op, frag = ("grouped16_conv3x3_images_gap", "wb_frag") if gw == 16 else ("grouped_mfma_conv3x3_images_gap", "pack_grouped_mfma_weights")
                    assert gate is not None and fused[-2:] == [f"{op}(h_a,{frag},sb,tb)[relu=1]", f"se_gate_slots({op},cnt,se_w1,se_b1,se_w2,se_b2)[relu=None]"], case
                else:
                    assert gate is None and fused == rec.calls, case


def test_predicates_are_views_of_the_chooser(rec):
    from laudnet_amd import laud_regnet as R, ops
    with rec.stubbed():
        for (gw, C), mode, setting in itertools.product(rec.SHAPES, rec.MODES, range(128)):
            ops.set_math_mode(mode)
            rec.set_switches(setting)
            mfma = R.USE_GROUPED_MFMA and mode == "bf16x3"
            rows = R.conv_b_choice("rows", C, gw)
            assert rows[1] == "rows" and (rows[0] != "valu") <= mfma
            assert R.grouped_mfma_widths_on(C, gw) == (rows[0] == "gw") == bool(mfma and R.USE_GROUPED_MFMA_WIDTHS and gw in (8, 24))
            assert R.grouped_wide_rows_on(C, gw) == (rows[0] == "wide") == bool(mfma and R.USE_GROUPED_MFMA_WIDE_ROWS and gw in (56, 112))
            assert (rows[0] == "g16") == bool(mfma and gw == 16)
            assert R.conv_b_choice("rows", C, gw, families=("gw", "wide"))[0] == (rows[0] if rows[0] != "g16" else "valu")
            for Hi, stride in ((7, 1), (14, 2), (9, 3)):
                images = (4, Hi, Hi, (Hi - 1) // stride + 1, (Hi - 1) // stride + 1, stride)
                whole = R.conv_b_choice("rows", C, gw, images=images)
                assert whole[0] == rows[0] and R.conv_b_choice("rows", C, gw, images=images, have_count=False) == rows
                assert R.grouped_mfma_images_on(C, gw, Hi, Hi, stride) == (whole == ("gw", "images"))
                img = R.conv_b_choice("image", C, gw, images=images)
                assert img[1] == "image"
                assert R.grouped_chan_mfma_on(C, gw, Hi, Hi, stride) == (img[0] in ("g16", "gw")) == bool(
                    mfma and R.USE_GROUPED_MFMA_CHANNEL and ops.grouped_chan_mfma_ok(C, gw, Hi, Hi, stride))
                assert R.grouped_wide_on(C, gw, Hi, Hi, stride) == (img[0] == "wide") == bool(
                    mfma and R.USE_GROUPED_MFMA_WIDE and ops.grouped_wide_ok(C, gw, Hi, Hi, stride))


def test_the_tables_widths_are_the_librarys():
    """the chooser answers from the table's widths (C a positive multiple) what the library's shape queries answer; every name of the table exists"""
    from laudnet_amd import laud_regnet as R, ops
    for gw, C in itertools.product((0, 8, 16, 24, 40, 56, 112), (-56, 0, 24, 32, 48, 100, 112, 168, 224, 336)):
        built = R._WIDTH_FAMILY.get(gw) if gw and C > 0 and C % gw == 0 else None
        assert (built == "gw") == ops.grouped_mfma_ok(C, gw), (C, gw)
        assert (built == "wide") == ops.grouped_wide_rows_ok(C, gw), (C, gw)
    for family in R.CONV_B.values():
        names = [n for f in family.forms.values() for n in (f.op, f.fit)] + [family.packer]
        assert all(callable(getattr(ops, n)) for n in names if n is not None)
        assert all(isinstance(getattr(R, f.switch), bool) for f in family.forms.values() if f.switch is not None)
