"""GPU tests of the wiring behind laud_regnet.conv_b_choice: _conv_b_rows, _conv_b_rows_se and _conv_b_image hand the kernel they choose the
right arguments in the right order.  The stubs of tests/test_conv_b_choice.py cannot see a swapped scale / shift or Ho / Wo, so here each site
runs on the device and must equal, BIT FOR BIT, a direct call of the public ops wrapper that tests/golden/conv_b_choice.json names for the
case (the same kernel on the same inputs: no tolerance), with the wrapper's arguments written out here, not taken from the package.

Two groups per width; B = 2 kept images; a 7x7 map at stride 1, 14x14 -> 7x7 at stride 2 and a non-square 6x10 map; random scale and shift
that differ; every switch on (the family's own forms) and the switches as shipped.  The forms of a family are bit-identical by design, so each
site's calls of the ops entry points are also counted: exactly the named one, once (the 6x10 map is held to the form the record names at 7x7)."""
import functools
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [(8, 16), (16, 32), (24, 48), (56, 112), (112, 224)]
GOLDEN_C = {8: 24, 16: 32, 24: 48, 56: 112, 112: 224}          # the channel count the golden file records each width at
MAPS = [(7, 7, 1), (7, 7, 2), (6, 10, 1)]                      # Ho, Wo, stride
B, S = 2, 8


@functools.lru_cache(maxsize=None)
def _golden():
    spec = importlib.util.spec_from_file_location("record_conv_b_choice", os.path.join(ROOT, "tools", "record_conv_b_choice.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(ROOT, "tests", "golden", "conv_b_choice.json")) as fh:
        return rec, rec.ungrouped(json.load(fh))


def _named(site, gw, setting):
    """(ops entry point, tag of its weight argument) that the golden file names for the site at this width, bf16x3 mode"""
    rec, table = _golden()
    last = table[site, gw, GOLDEN_C[gw], "bf16x3", setting].split()[-1]          # (a lazy pack in front of it is not a launch)
    name, args = last[:last.index("(")], last[last.index("(") + 1:last.index(")")].split(",")
    return name, args[1 if site.startswith("rows") else 0]


def _weights(ops, tag, wb, gw):
    if tag == "wb":
        return wb
    packer = "pack_grouped16_weights" if tag == "wb_frag" else tag
    return getattr(ops, packer)(wb, *(() if packer == "pack_grouped16_weights" else (gw,)))


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()
    return _ops


@pytest.fixture(params=["all-on", "as-shipped"])
def setting(request, monkeypatch):
    from laudnet_amd import laud_regnet, ops
    rec, _ = _golden()
    n = 127 if request.param == "all-on" else rec.setting_of(USE_GROUPED_MFMA=True, USE_GROUPED_IMAGES=True)
    for k, name in enumerate(rec.SWITCHES):
        monkeypatch.setattr(laud_regnet, name, bool(n >> k & 1))
    monkeypatch.setattr(laud_regnet, "USE_SE_FUSED", True)
    ops.set_math_mode("bf16x3")
    yield n
    ops.set_math_mode("fp32")


@functools.lru_cache(maxsize=None)
def _problem(gw, C, Ho, Wo, stride):
    """a prepared dict of random weights (no fragments: the sites pack them), the lists of B kept images, h_a as rows and as images, the channel
    lists with image 1 cut to C - 3 channels; shared by the tests, never modified"""
    from laudnet_amd import ops
    g = torch.Generator().manual_seed(1000 * gw + 10 * Ho + stride)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    Hi, Wi = Ho * stride, Wo * stride
    p = {"wb": rnd(C, 9, gw) * 0.1, "sb": 0.5 + torch.rand(C, generator=g), "tb": rnd(C), "se_w1": rnd(S, C) * 0.1, "se_b1": rnd(S), "se_w2": rnd(C, S) * 0.1,
         "se_b2": rnd(C)}
    assert not torch.equal(p["sb"], p["tb"])
    p = {k: v.to(DEV) for k, v in p.items()}
    ix = ops.mask_to_index(torch.ones(B, 1, 1, device=DEV), Ho, Wo, stride)
    assert ix.cap1 == B * Hi * Wi and ix.cap3 == B * Ho * Wo
    h_a = rnd(B, Hi, Wi, C).to(DEV)
    keep = torch.ones(B, C)
    keep[1, 5:8] = 0.0
    _, idx, cnt, _ = ops.channel_masker(None, None, None, None, None, C, 1, mask_in=keep.to(DEV))
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [C, C - 3] and (C - 3) % 4
    return p, ix, h_a, idx, cnt


def _case(gw, C, m):
    Ho, Wo, stride = m
    return _problem(gw, C, Ho, Wo, stride), (B, Ho * stride, Wo * stride, Ho, Wo, stride)


class _F:
    def __init__(self, gw):
        self.group_width = gw


def _launched(ops, monkeypatch, site):
    """runs the site -> (its result, the names of the ops entry points it called, in order): the forms of a family are bit-identical by design,
    so the outputs alone would not tell which one ran"""
    rec, _ = _golden()
    names = []
    with monkeypatch.context() as m:
        for name in rec.ENTRY_POINTS:
            m.setattr(ops, name, lambda *a, _real=getattr(ops, name), _name=name, **k: (names.append(_name), _real(*a, **k))[1])
        result = site()
    return result, names


@pytest.mark.parametrize("m", MAPS, ids=lambda m: "%dx%d-s%d" % m)
@pytest.mark.parametrize("gw,C", WIDTHS)
@pytest.mark.parametrize("with_images", [False, True])
def test_conv_b_rows(ops, setting, gw, C, m, with_images, monkeypatch):
    from laudnet_amd import laud_regnet
    (p, ix, h_a, _, _), images = _case(gw, C, m)
    a2d = h_a.view(ix.cap1, C)
    got = torch.full((ix.cap3, C), -7.0, device=DEV)
    _, launched = _launched(ops, monkeypatch, lambda: laud_regnet._conv_b_rows(dict(p), _F(gw), a2d, ix.nbr, got, ix.cnt[0:1], ix.cap3,
                                                                               images=images if with_images else None))
    site = "rows" if not with_images else "rows:s2" if m[2] == 2 else "rows:fit"
    name, tag = _named(site, gw, setting)
    assert launched == [name]
    assert name.endswith("_images") == (with_images and setting == 127 and gw in (8, 16, 24) or with_images and gw == 16)
    want = torch.full((ix.cap3, C), -7.0, device=DEV)
    w = (_weights(ops, tag, p["wb"], gw),) + (() if name.startswith("grouped16_") else (gw,))
    if name.endswith("_images"):
        getattr(ops, name)(a2d, *w, p["sb"], p["tb"], want, m_count=ix.cnt[0:1], images=images, relu=1)
    else:
        getattr(ops, name)(a2d, ix.nbr, *w, p["sb"], p["tb"], want, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)
    torch.cuda.synchronize()
    assert bool((want != -7.0).any()) and torch.equal(got, want), (name, tag)


@pytest.mark.parametrize("m", MAPS, ids=lambda m: "%dx%d-s%d" % m)
@pytest.mark.parametrize("gw,C", WIDTHS)
def test_conv_b_rows_se(ops, setting, gw, C, m, monkeypatch):
    """the fused site: the family's *_images_gap + se_gate_slots where the rule of tests/test_conv_b_choice.py takes the fold (width 16; widths
    8 / 24 with their switches on), else no gate and the op of the 'rows with images' site"""
    from laudnet_amd import laud_regnet
    (p, ix, h_a, _, _), images = _case(gw, C, m)
    Ho, Wo = m[0], m[1]
    assert ops.conv_rows_gated_fits(C, Ho * Wo)
    a2d = h_a.view(ix.cap1, C)
    got = torch.full((ix.cap3, C), -7.0, device=DEV)
    gate, launched = _launched(ops, monkeypatch, lambda: laud_regnet._conv_b_rows_se(dict(p), _F(gw), a2d, ix.nbr, got, ix.cnt[0:1], ix.cap3, images))
    name, tag = _named("rows:s2" if m[2] == 2 else "rows:fit", gw, setting)
    assert launched == ([name + "_gap", "se_gate_slots"] if name.endswith("_images") else [name])
    want = torch.full((ix.cap3, C), -7.0, device=DEV)
    w = (_weights(ops, tag, p["wb"], gw),) + (() if name.startswith("grouped16_") else (gw,))
    if name.endswith("_images"):
        gap = getattr(ops, name + "_gap")(a2d, *w, p["sb"], p["tb"], want, m_count=ix.cnt[0:1], images=images, relu=1)
        want_gate = ops.se_gate_slots(gap, ix.cnt[0:1], Ho * Wo, p["se_w1"], p["se_b1"], p["se_w2"], p["se_b2"])
        torch.cuda.synchronize()
        assert gate is not None and gate.shape == (B, C) and torch.equal(gate, want_gate)
    else:
        getattr(ops, name)(a2d, ix.nbr, *w, p["sb"], p["tb"], want, m_count=ix.cnt[0:1], m_cap=ix.cap3, relu=1)
        torch.cuda.synchronize()
        assert gate is None
    assert bool((want != -7.0).any()) and torch.equal(got, want), (name, tag)


@pytest.mark.parametrize("m", MAPS, ids=lambda m: "%dx%d-s%d" % m)
@pytest.mark.parametrize("gw,C", WIDTHS)
def test_conv_b_image(ops, setting, gw, C, m, monkeypatch):
    from laudnet_amd import laud_regnet
    (p, ix, h_a, idx, cnt), images = _case(gw, C, m)
    Ho, Wo, stride = m
    got = torch.full((B, Ho, Wo, C), -7.0, device=DEV)
    _, launched = _launched(ops, monkeypatch, lambda: laud_regnet._conv_b_image(dict(p), _F(gw), h_a, idx, cnt, got, stride))
    name, tag = _named("image:s2" if stride == 2 else "image", gw, setting)
    assert launched == [name]
    assert (name != "grouped_conv3x3_image") == (setting == 127)
    want = torch.full((B, Ho, Wo, C), -7.0, device=DEV)
    getattr(ops, name)(h_a, _weights(ops, tag, p["wb"], gw), gw, idx, cnt, p["sb"], p["tb"], want, stride=stride, relu=1)
    torch.cuda.synchronize()
    assert bool((want != -7.0).any()) and torch.equal(got, want), (name, tag)
