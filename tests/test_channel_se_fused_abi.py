"""CPU checks of the channel-mode SE fold's four entry points (ldn_grouped_chan_mfma_conv3x3_image_gap, ldn_se_gate_image,
ldn_conv_image_gated, ldn_conv_image_gated_ok; + ldn_grouped_chan_mfma_gap_ok): declared in the header, exported by the library and bound in
_lib.SIGNATURES with the header's argument lists; the fit queries are host arithmetic and answer without a GPU; the entry points refuse bad
arguments before any launch."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ldn_grouped_chan_mfma_conv3x3_image_gap", "ldn_se_gate_image", "ldn_conv_image_gated", "ldn_conv_image_gated_ok"]


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


def _header_args(name):
    """the argument types of a prototype of include/ldn_hip.h as ctypes: every pointer a c_void_p, int an c_int"""
    text = open(os.path.join(ROOT, "include", "ldn_hip.h")).read()
    m = re.search(r"^int " + name + r"\(([^;]*?)\);", text, re.M | re.S)
    assert m, f"{name} is not declared in include/ldn_hip.h"
    out = []
    for arg in m.group(1).replace("\n", " ").split(","):
        arg = arg.strip()
        if "*" in arg:
            out.append(ctypes.c_void_p)
        else:
            assert re.fullmatch(r"int \w+", arg), arg
            out.append(ctypes.c_int)
    return out


@pytest.mark.parametrize("name", NEW + ["ldn_grouped_chan_mfma_gap_ok"])
def test_header_library_and_signatures_agree(lib, name):
    from laudnet_amd import _lib
    argtypes, restype = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and list(argtypes) == _header_args(name), name
    so = os.path.join(ROOT, "laudnet_amd", "libldn_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    assert name in exported
    assert callable(getattr(lib, name))


def test_the_new_argument_lists_extend_the_plain_ones():
    """_gap = the plain conv b + gap_partial in front of stream; _gated = ldn_conv_image + gate in front of math_mode"""
    from laudnet_amd._lib import SIGNATURES as S
    plain, gap = S["ldn_grouped_chan_mfma_conv3x3_image"][0], S["ldn_grouped_chan_mfma_conv3x3_image_gap"][0]
    assert list(gap) == list(plain[:-1]) + [ctypes.c_void_p, plain[-1]]
    conv, gated = S["ldn_conv_image"][0], S["ldn_conv_image_gated"][0]
    assert list(gated) == list(conv[:-2]) + [ctypes.c_void_p] + list(conv[-2:])


# RegNetY at 224 px: (widths of the four stages, bottleneck multiplier 1) -- conv c is w_b = width -> width over the stage's output map
REGNETY = {"400mf": (48, 104, 208, 440), "800mf": (64, 144, 320, 784), "1.6gf": (48, 120, 336, 888), "3.2gf": (72, 216, 576, 1512)}


def test_gated_ok_takes_every_conv_c_of_the_small_regnets(lib):
    for name, widths in REGNETY.items():
        for stage, w in enumerate(widths):
            rows = (56 >> stage) ** 2
            for B in (1, 64):
                for residual in (0, 1):          # (conv c always adds the identity or the projection; the launch without is admitted too)
                    for scale in (0, 1):
                        assert lib.ldn_conv_image_gated_ok(B, rows, w, w, residual, scale) == 1, (name, stage, B, residual, scale)


def test_gated_ok_refuses_what_does_not_fit(lib):
    assert lib.ldn_conv_image_gated_ok(64, 49, 100, 320, 1, 1) == 0          # cin % 8 != 0
    assert lib.ldn_conv_image_gated_ok(64, 49, 12, 320, 1, 1) == 0
    assert lib.ldn_conv_image_gated_ok(64, 49, 104, 320, 1, 1) == 1
    assert lib.ldn_conv_image_gated_ok(64, 49, 104, 322, 1, 1) == 0          # cout % 4 != 0
    assert lib.ldn_conv_image_gated_ok(0, 49, 104, 320, 1, 1) == 0
    assert lib.ldn_conv_image_gated_ok(64, 0, 104, 320, 1, 1) == 0
    # the plan's LDS: the 2 x 10 tile holds 12 x 8 KiB of staging + tables + (list + gate) of 2 x 4 bytes a channel
    assert lib.ldn_conv_image_gated_ok(64, 49, 4096, 320, 1, 1) == 1
    assert lib.ldn_conv_image_gated_ok(64, 49, 8192, 320, 1, 1) == 0          # 98 304 + tables + 65 536 > 160 KiB
    assert lib.ldn_conv_image_gated_ok(64, 3136, 16384, 64, 1, 1) == 0


def test_gap_ok_follows_the_plain_fit(lib):
    for C, gw, Hi, s in [(48, 8, 56, 1), (104, 8, 28, 1), (440, 8, 7, 1), (64, 16, 56, 1), (320, 16, 14, 1), (784, 16, 14, 2), (48, 24, 112, 2),
                         (120, 24, 56, 2), (336, 24, 14, 1), (888, 24, 7, 1)]:
        assert lib.ldn_grouped_chan_mfma_ok(C, gw, Hi, Hi, s) == 1 and lib.ldn_grouped_chan_mfma_gap_ok(C, gw, Hi, Hi, s) == 1, (C, gw, Hi, s)
    assert lib.ldn_grouped_chan_mfma_gap_ok(448, 56, 14, 14, 1) == 0
    assert lib.ldn_grouped_chan_mfma_gap_ok(100, 8, 7, 7, 1) == 0
    assert lib.ldn_grouped_chan_mfma_gap_ok(24, 24, 8, 1 << 20, 1) == 0


def test_refusals_before_any_launch(lib):
    d = ctypes.c_void_p(256)              # never dereferenced: every call below is refused by its arguments
    odd = ctypes.c_void_p(260)
    gap = lib.ldn_grouped_chan_mfma_conv3x3_image_gap
    assert gap(d, 64, 1, 7, 7, 1, 7, 7, d, 64, 16, d, d, d, d, 1, d, 64, None, None) == -1         # null gap_partial
    assert gap(d, 64, 1, 7, 7, 1, 7, 7, d, 64, 16, d, d, d, d, 1, d, 64, odd, None) == -1          # misaligned gap_partial
    assert gap(d, 64, 1, 7, 7, 1, 6, 7, d, 64, 16, d, d, d, d, 1, d, 64, d, None) == -1            # the plain entry point's checks
    assert gap(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, d, 112, d, None) == -1
    assert gap(d, 64, 1, 7, 7, 1, 7, 7, d, 64, 16, d, None, d, d, 1, d, 64, d, None) == -1
    se = lib.ldn_se_gate_image
    assert se(None, 1, 4, 49, 64, 16, d, d, d, d, d, d, d, None) == -1
    assert se(d, 1, 4, 49, 64, 16, d, d, d, d, None, d, d, None) == -1                               # the channel lists are required
    assert se(d, 0, 4, 49, 64, 16, d, d, d, d, d, d, d, None) == -1
    assert se(d, 1, 0, 49, 64, 16, d, d, d, d, d, d, d, None) == -1
    g = lib.ldn_conv_image_gated

    def call(**kw):
        a = dict(a=d, lda=64, B=2, Hi=7, Wi=7, ksize=1, stride=1, Ho=7, Wo=7, w=d, cin=64, cout=64, k_idx=d, k_cnt=d, kgran=1, n_idx=None, n_cnt=None,
                 scale=d, shift=d, shift_classes=1, post_sub=None, relu=1, residual=d, ldr=64, out=d, ldo=64, colsum=None, out_format=0, gate=d,
                 math_mode=1, stream=None)
        a.update(kw)
        return g(*a.values())
    for bad in (dict(gate=None), dict(gate=odd), dict(math_mode=0), dict(n_idx=d, n_cnt=d), dict(ksize=3), dict(colsum=d), dict(out_format=1),
                dict(shift_classes=16), dict(stride=2, Ho=4, Wo=4), dict(post_sub=d), dict(k_idx=None, k_cnt=None), dict(cin=60, lda=60), dict(lda=32),
                dict(cin=8192, lda=8192, cout=320, ldo=320, ldr=320), dict(relu=2)):
        assert call(**bad) == -1, bad
