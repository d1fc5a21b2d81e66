#!/usr/bin/env python3
"""Which op does each call site of LAD-RegNet's conv b reach, under every setting of its switches?  No GPU needed.

    tools/record_conv_b_choice.py [OUT.json]          (PYTHONPATH=<an export of another commit> records that tree instead)

The entry points and packers of laudnet_amd.ops are replaced by stubs BY NAME (the library's host-arithmetic fit queries stay real), then for
every setting of the seven USE_GROUPED_* switches of laud_regnet (128), both math modes and six (group width, channels) the sites are driven:

    rows         laud_regnet._conv_b_rows without images            rows:fit     ... with images (4, 7, 7, 7, 7, 1)
    rows:s2      ... with images (4, 14, 14, 7, 7, 2)               rows:nofit   ... with images (1, 8, 1 << 20, 8, 1 << 20, 1)
    rows:nocount ... with the fitting images and no device-side count
    image        laud_regnet._conv_b_image, 7x7 at stride 1         image:s2     ... 14x14 at stride 2
    adjoint      training._conv_b_adjoint                           plain        training._conv_b_plain
    params       the keys of training._conv_b_params                prepared     the keys of BottleneckTransform.prepared("cpu")

The prepared dict handed to the laud_regnet sites holds what prepared() always packs (wb_frag at width 16) and none of the switched fragments, so
the lazy packs show up in the record.  An outcome is the sequence of stubbed calls, each "name(tagged tensor arguments)[relu]", or the sorted keys.

The file is grouped by outcome to stay small: {"switches": [...], "table": {outcome: {"site gw w_b mode": hex}}} where bit s of the hex number is
set iff switch setting s has that outcome, and setting s has switch k (in the order of "switches") on iff bit k of s is set.
Only names that exist before and after the dispatch refactor are used, so the same file records either tree.
"""
import contextlib
import itertools
import json
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from laudnet_amd import laud_regnet, ops, training  # noqa: E402

SWITCHES = ["USE_GROUPED_MFMA", "USE_GROUPED_IMAGES", "USE_GROUPED_MFMA_WIDTHS", "USE_GROUPED_MFMA_WIDTHS_IMAGES", "USE_GROUPED_MFMA_CHANNEL",
            "USE_GROUPED_MFMA_WIDE", "USE_GROUPED_MFMA_WIDE_ROWS"]
SHAPES = [(8, 24), (16, 32), (24, 48), (56, 112), (112, 224), (40, 80)]
MODES = ["bf16x3", "fp32"]
ENTRY_POINTS = ["grouped_conv3x3_rows", "grouped16_conv3x3_rows", "grouped_mfma_conv3x3_rows", "grouped_wide_conv3x3_rows", "grouped16_conv3x3_images",
                "grouped_mfma_conv3x3_images", "grouped16_conv3x3_images_gap", "grouped_mfma_conv3x3_images_gap", "grouped_conv3x3_image",
                "grouped_chan_mfma_conv3x3_image", "grouped_wide_conv3x3_image", "se_gate_slots"]
PACKERS = ["pack_grouped16_weights", "pack_grouped_mfma_weights", "pack_grouped_wide_weights"]
ROWS_SITES = {"rows": (None, True), "rows:fit": ((4, 7, 7, 7, 7, 1), True), "rows:s2": ((4, 14, 14, 7, 7, 2), True),
              "rows:nofit": ((1, 8, 1 << 20, 8, 1 << 20, 1), True), "rows:nocount": ((4, 7, 7, 7, 7, 1), False)}
IMAGE_SITES = {"image": (7, 7, 1), "image:s2": (14, 7, 2)}

_tags, _keep, calls = {}, [], []


def tagged(name):
    """a tensor the stubs recognise among their arguments"""
    t = torch.zeros(1)
    _tags[id(t)] = name
    _keep.append(t)
    return t


def _stub(name):
    def entry_point(*args, **kw):
        calls.append(f"{name}({','.join(_tags[id(a)] for a in args if id(a) in _tags)})[relu={kw.get('relu')}]")
        return tagged(name)

    def packer(*args):
        calls.append(f"{name}({','.join(_tags[id(a)] for a in args if id(a) in _tags)})")
        return tagged(name)
    return packer if name in PACKERS else entry_point


class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def _sites(gw, w_b, block):
    """site -> a function that drives it and returns its outcome"""
    class F:
        group_width = gw

    def prepared_dict():
        p = {k: tagged(k) for k in ("wb", "sb", "tb")}
        if gw == 16:
            p["wb_frag"] = tagged("wb_frag")
        return p

    def seq(fn):
        del calls[:]
        fn()
        return " ".join(calls)

    def rows(images, count):
        return lambda: seq(lambda: laud_regnet._conv_b_rows(prepared_dict(), F, tagged("h_a"), None, _Shape(196, w_b), object() if count else None,
                                                            196, images=images))

    def image(Hi, Ho, stride):
        return lambda: seq(lambda: laud_regnet._conv_b_image(prepared_dict(), F, _Shape(4, Hi, Hi, w_b), None, None, _Shape(4, Ho, Ho, w_b), stride))
    wbr, x, nbr = torch.zeros(w_b, 9, gw), torch.zeros(4, w_b), None
    _tags[id(wbr)] = "wbr"
    _keep.extend((wbr, x))      # (a tag is an id: no tagged tensor may die, or a later untagged one takes its id and its tag)

    def prepared():
        block.invalidate()
        return ",".join(sorted(k for k in block.prepared("cpu") if k.startswith("wb")))
    sites = {name: rows(*a) for name, a in ROWS_SITES.items()}
    sites.update({name: image(*a) for name, a in IMAGE_SITES.items()})
    sites["adjoint"] = lambda: seq(lambda: training._conv_b_adjoint(x, nbr, wbr, gw, x, None, 4))
    sites["plain"] = lambda: seq(lambda: training._conv_b_plain(wbr, gw, x, nbr, x, None, 4))
    sites["params"] = lambda: ",".join(sorted(training._conv_b_params(wbr, x, x, gw)))
    sites["prepared"] = prepared
    return sites


@contextlib.contextmanager
def stubbed():
    """ops' entry points and packers replaced by the recording stubs; switches, math mode and ops restored on the way out"""
    saved = {n: getattr(ops, n) for n in ENTRY_POINTS + PACKERS}
    saved_sw = {n: getattr(laud_regnet, n) for n in SWITCHES}
    before = ops.get_math_mode()
    try:
        for n in ENTRY_POINTS + PACKERS:
            setattr(ops, n, _stub(n))
        yield
    finally:
        for n, v in saved.items():
            setattr(ops, n, v)
        for n, v in saved_sw.items():
            setattr(laud_regnet, n, v)
        ops.set_math_mode(before if before != ops.get_math_mode() else None)
        ops.set_math_mode(None)
        del _keep[:]
        _tags.clear()


def set_switches(setting):
    for k, n in enumerate(SWITCHES):
        setattr(laud_regnet, n, bool(setting >> k & 1))


def record():
    """{(site, gw, w_b, mode, setting): outcome} of the tree that laudnet_amd was imported from"""
    out = {}
    with stubbed():
        for gw, w_b in SHAPES:
            torch.manual_seed(0)
            block = laud_regnet.BottleneckTransform(w_b, w_b, 1, nn.BatchNorm2d, nn.ReLU, gw, 1.0, 0.25, output_size=8, dyn_mode="spatial").eval()
            sites = _sites(gw, w_b, block)
            for mode, setting in itertools.product(MODES, range(1 << len(SWITCHES))):
                ops.set_math_mode(mode)
                set_switches(setting)
                for site, run in sites.items():
                    out[site, gw, w_b, mode, setting] = run()
    return out


def grouped(rec):
    """the record in the file's form"""
    table = {}
    for (site, gw, w_b, mode, setting), outcome in rec.items():
        cell = table.setdefault(outcome, {})
        key = f"{site} {gw} {w_b} {mode}"
        cell[key] = cell.get(key, 0) | 1 << setting
    return {"switches": SWITCHES,
            "table": {o: {k: f"{v:x}" for k, v in sorted(cell.items())} for o, cell in sorted(table.items())}}


def ungrouped(doc):
    """the inverse of grouped()"""
    assert doc["switches"] == SWITCHES
    rec = {}
    for outcome, cell in doc["table"].items():
        for key, bits in cell.items():
            site, gw, w_b, mode = key.split()
            for setting in range(1 << len(SWITCHES)):
                if int(bits, 16) >> setting & 1:
                    rec[site, int(gw), int(w_b), mode, setting] = outcome
    return rec


def setting_of(**on):
    """the number of the switch setting with exactly the named switches on, e.g. setting_of(USE_GROUPED_MFMA=True)"""
    return sum(1 << SWITCHES.index(n) for n, v in on.items() if v)


if __name__ == "__main__":
    doc = json.dumps(grouped(record()), indent=1) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(doc)
    else:
        sys.stdout.write(doc)
