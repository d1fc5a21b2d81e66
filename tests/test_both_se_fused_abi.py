"""CPU checks of the 'both'-mode SE fold's two entry points (ldn_conv_packed_gated, ldn_conv_packed_gated_ok): declared in the header, exported
by the library and bound in _lib.SIGNATURES with the header's argument lists; the fit query is host arithmetic and answers without a GPU; the
entry point refuses bad arguments before any launch."""
import ctypes
import os
import subprocess

import pytest

import test_channel_se_fused_abi as A
import test_conv_packed_gated_plan as PP

ROOT = A.ROOT
NEW = ["ldn_conv_packed_gated", "ldn_conv_packed_gated_ok"]
lib = A.lib                                   # (the module-scoped fixture that loads the library)


@pytest.mark.parametrize("name", NEW)
def test_header_library_and_signatures_agree(lib, name):
    from laudnet_amd import _lib
    argtypes, restype = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and list(argtypes) == A._header_args(name), name
    so = os.path.join(ROOT, "laudnet_amd", "libldn_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    assert name in exported
    assert callable(getattr(lib, name))


def test_the_new_argument_list_extends_the_plain_one():
    """_gated = ldn_conv_packed + gate in front of math_mode; the query has the image form's six integers"""
    from laudnet_amd._lib import SIGNATURES as S
    conv, gated = S["ldn_conv_packed"][0], S["ldn_conv_packed_gated"][0]
    assert list(gated) == list(conv[:-2]) + [ctypes.c_void_p] + list(conv[-2:])
    assert S["ldn_conv_packed_gated_ok"] == S["ldn_conv_image_gated_ok"]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert f"_lib.{name}.argtypes" in text, f"{name} is missing from the INTEGRATION.md stub"


def test_ok_takes_every_conv_c_of_the_small_regnets(lib):
    """conv c of a 'both' block: w_b = width -> width (one mask group) or width / 2 (two), at most the stage's map of rows per image"""
    for name, widths in A.REGNETY.items():
        for stage, w in enumerate(widths):
            rows = (56 >> stage) ** 2
            for B, G, residual, scale in [(b, g, r, s) for b in (1, 64) for g in (1, 2) for r in (0, 1) for s in (0, 1)]:
                assert lib.ldn_conv_packed_gated_ok(B, rows, w, w // G, residual, scale) == 1, (name, stage, B, G, residual, scale)


def test_ok_answers_what_the_plan_says(lib):
    """the library's query against the plan header compiled on the host (tests/conv_packed_gated_plan_cli.cpp), over the whole sweep"""
    swept = PP._swept()
    for s, p in swept:
        assert lib.ldn_conv_packed_gated_ok(*s) == p["ok"], (s, p)
    assert any(not p["ok"] for _, p in swept)


def test_ok_refuses_what_does_not_fit(lib):
    ok = lib.ldn_conv_packed_gated_ok
    assert ok(64, 49, 100, 320, 1, 1) == 0          # cin % 8 != 0
    assert ok(64, 49, 12, 320, 1, 1) == 0
    assert ok(64, 49, 104, 320, 1, 1) == 1
    assert ok(64, 49, 104, 322, 1, 1) == 0          # cout % 4 != 0
    assert ok(0, 49, 104, 320, 1, 1) == 0
    assert ok(64, 0, 104, 320, 1, 1) == 0
    assert ok(64, 49, 3712, 320, 1, 1) == 1
    assert ok(64, 49, 8192, 320, 1, 1) == 0         # 98 304 + tables + 65 536 > 160 KiB
    assert ok(64, 3136, 16384, 64, 1, 1) == 0


def test_refusals_before_any_launch(lib):
    d = ctypes.c_void_p(256)              # never dereferenced: every call below is refused by its arguments
    odd = ctypes.c_void_p(260)
    g = lib.ldn_conv_packed_gated

    def call(**kw):
        a = dict(a=d, lda=64, B=2, row_prefix=d, m_count=None, m_cap=49, a_map=d, taps=1, out_map=d, pix_map=None, Hi=0, Wi=0, Ho=0, Wo=0, stride=1,
                 w=d, cin=64, cout=64, k_idx=d, k_cnt=d, kgran=1, n_idx=None, n_cnt=None, scale=d, shift=d, shift_classes=1, post_sub=None, relu=1,
                 relu_if_neg=None, residual=d, ldr=64, out=d, ldo=64, gate=d, math_mode=1, stream=None)
        a.update(kw)
        return g(*a.values())
    for bad in (dict(gate=None), dict(gate=odd), dict(math_mode=0), dict(n_idx=d, n_cnt=d), dict(taps=9), dict(row_prefix=None), dict(row_prefix=None, B=1),
                dict(shift_classes=16, pix_map=d, Hi=7, Wi=7, Ho=7, Wo=7), dict(pix_map=d), dict(post_sub=d), dict(k_idx=None, k_cnt=None),
                dict(cin=60, lda=60), dict(lda=32), dict(relu=2, relu_if_neg=d), dict(relu=2), dict(relu_if_neg=d), dict(kgran=0), dict(ldo=60),
                dict(ldr=32), dict(out=odd), dict(residual=odd), dict(cin=8192, lda=8192, cout=320, ldo=320, ldr=320), dict(B=0), dict(m_cap=-1)):
        assert call(**bad) == -1, bad
    assert call(m_cap=0) == 0             # nothing to do, after the checks
