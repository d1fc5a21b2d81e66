"""CPU checks of the SE-squeeze form of the matrix-core channel-mode grouped 3x3 at group widths 56, 112 and 232
(ldn_grouped_wide_conv3x3_image_gap, k_grouped_wide<GW, true>; + ldn_grouped_wide_gap_ok): declared in the header, exported by the library and
bound in _lib.SIGNATURES with the header's argument lists; the fit query is host arithmetic, answers without a GPU and equals the plain
form's; the entry point refuses bad arguments before any launch."""
import ctypes
import itertools
import os
import subprocess

import pytest

import test_channel_se_fused_abi as A
import test_grouped_wide_232_abi as W232
import test_grouped_wide_abi as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# conv b of every stage of RegNetY-8GF (56), 16GF (112) and 32GF (232) at 224 px: the stride-2 first block and the stride-1 blocks
STAGE_SHAPES = W.MODEL_SHAPES + [(C, W232.GW, H, H, s) for C, H, s in W232.MODEL_MAPS]


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", ["ldn_grouped_wide_conv3x3_image_gap", "ldn_grouped_wide_gap_ok"])
def test_header_library_and_signatures_agree(lib, name):
    from laudnet_amd import _lib
    argtypes, restype = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and list(argtypes) == A._header_args(name), name
    so = os.path.join(ROOT, "laudnet_amd", "libldn_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    assert name in exported
    assert callable(getattr(lib, name))


def test_the_argument_list_extends_the_plain_one():
    """_gap = the plain conv b + gap_partial in front of stream: the argument list of ldn_grouped_chan_mfma_conv3x3_image_gap"""
    from laudnet_amd._lib import SIGNATURES as S
    plain, gap = S["ldn_grouped_wide_conv3x3_image"][0], S["ldn_grouped_wide_conv3x3_image_gap"][0]
    assert list(gap) == list(plain[:-1]) + [ctypes.c_void_p, plain[-1]]
    assert list(gap) == list(S["ldn_grouped_chan_mfma_conv3x3_image_gap"][0])
    assert list(S["ldn_grouped_wide_gap_ok"][0]) == list(S["ldn_grouped_wide_ok"][0])


def test_the_python_face_exists():
    import inspect
    from laudnet_amd import ops
    assert list(inspect.signature(ops.grouped_wide_gap_ok).parameters) == ["C", "group_width", "Hi", "Wi", "stride"]
    assert (str(inspect.signature(ops.grouped_wide_conv3x3_image_gap)) ==
            str(inspect.signature(ops.grouped_chan_mfma_conv3x3_image_gap)))
    assert ops.grouped_wide_gap_ok(2016, 56, 7, 7, 1) is True and ops.grouped_wide_gap_ok(96, 24, 7, 7, 1) is False


def test_gap_ok_takes_every_stage_shape_of_the_three_models(lib):
    assert len(STAGE_SHAPES) == 24
    for C, gw, Hi, Wi, s in STAGE_SHAPES:
        assert lib.ldn_grouped_wide_gap_ok(C, gw, Hi, Wi, s) == 1, (C, gw, Hi, Wi, s)


def test_gap_ok_takes_nothing_else(lib):
    assert lib.ldn_grouped_wide_gap_ok(96, 24, 14, 14, 1) == 0                  # width 24
    assert lib.ldn_grouped_wide_gap_ok(100, 56, 7, 7, 1) == 0                   # C % gw != 0
    assert lib.ldn_grouped_wide_gap_ok(168, 112, 7, 7, 1) == 0
    assert lib.ldn_grouped_wide_gap_ok(240, 232, 7, 7, 1) == 0
    assert lib.ldn_grouped_wide_gap_ok(112, 56, 14, 14, 3) == 0                 # stride 3
    assert lib.ldn_grouped_wide_gap_ok(0, 56, 7, 7, 1) == 0 and lib.ldn_grouped_wide_gap_ok(112, 56, 0, 7, 1) == 0
    assert lib.ldn_grouped_wide_gap_ok(56, 56, 8, 1 << 20, 1) == 0              # where the plain plan finds no rectangle


def test_gap_ok_equals_the_plain_fit(lib):
    """the tile sums' scratch (pixel tiles of the workgroup x 64 / 128 / 256 floats) fits the 10 KB between the plain plan's 150 KB and the
    160 KB of a CU wherever the plain plan fits: on the shapes tests/test_grouped_wide_abi.py and tests/test_grouped_wide_232_abi.py ask
    ldn_grouped_wide_ok about, and on every map from 1 x 1 to 72 x 72 plus the long thin ones, at every width and both strides"""
    grid = list(STAGE_SHAPES)
    grid += [(gw * 4, gw, 14, 14, 1) for gw in (8, 16, 24, 40)]
    grid += [(100, 56, 7, 7, 1), (168, 112, 7, 7, 1), (0, 56, 7, 7, 1), (112, 56, 0, 7, 1), (112, 56, 14, 14, 3), (56, 56, 8, 1 << 20, 1),
             (112, 112, 8, 1 << 20, 2), (96, 24, 14, 14, 1), (464, 116, 7, 7, 1), (240, 232, 7, 7, 1), (528, 264, 7, 7, 1), (0, 232, 7, 7, 1),
             (-232, 232, 7, 7, 1), (232, 232, 7, 7, 3), (232, 232, 8, 1 << 20, 1)]
    sides = list(range(1, 73)) + [100, 112, 113, 224, 225, 500, 1000, 4000]
    grid += [(gw, gw, H, Wd, s) for gw, H, Wd, s in itertools.product((56, 112, 232), sides, sides, (1, 2))]
    yes = 0
    for C, gw, Hi, Wi, s in grid:
        ok = lib.ldn_grouped_wide_ok(C, gw, Hi, Wi, s)
        assert lib.ldn_grouped_wide_gap_ok(C, gw, Hi, Wi, s) == ok, (C, gw, Hi, Wi, s)
        yes += ok
    assert 0 < yes < len(grid)


def test_entry_point_refuses_before_any_launch(lib):
    f = lib.ldn_grouped_wide_conv3x3_image_gap
    d = ctypes.c_void_p(256)              # never dereferenced: every call below is refused by its arguments
    odd = ctypes.c_void_p(260)
    assert f(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, d, 112, None, None) == -1         # null gap_partial
    assert b"null" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, d, 112, odd, None) == -1          # misaligned gap_partial
    assert b"aligned" in lib.ldn_last_error()
    # ... and what tests/test_grouped_wide_abi.py sees the plain entry point refuse
    assert f(None, 112, 1, 7, 7, 1, 7, 7, None, 112, 56, None, None, None, None, 1, None, 112, d, None) == -1
    assert b"null" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, None, d, d, 1, d, 112, d, None) == -1         # a channel list without its counts
    assert b"null" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 1, 6, 7, d, 112, 56, d, d, d, d, 1, d, 112, d, None) == -1            # Ho of another geometry
    assert b"geometry" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 3, 3, 3, d, 112, 56, d, d, d, d, 1, d, 112, d, None) == -1            # stride 3
    assert b"not built" in lib.ldn_last_error()
    for gw, C in ((24, 96), (16, 64), (8, 64), (40, 80)):                                           # the other widths
        assert f(d, C, 1, 7, 7, 1, 7, 7, d, C, gw, d, d, d, d, 1, d, C, d, None) == -1
        assert b"not built" in lib.ldn_last_error()
    assert f(d, 114, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, d, 112, d, None) == -1            # lda % 4
    assert b"strides" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, d, 114, d, None) == -1            # ldo % 4
    assert f(d, 224, 1, 7, 7, 1, 7, 7, d, 224, 112, d, d, d, d, 1, d, 220, d, None) == -1           # ldo < C
    assert b"strides" in lib.ldn_last_error()
    assert f(d, 112, 1, 7, 7, 1, 7, 7, d, 112, 56, d, d, d, d, 1, odd, 112, d, None) == -1
    assert b"aligned" in lib.ldn_last_error()
    assert b"ldn_grouped_wide_conv3x3_image_gap" in lib.ldn_last_error()
    # the plain entry point still names itself
    assert lib.ldn_grouped_wide_conv3x3_image(d, 112, 1, 7, 7, 1, 6, 7, d, 112, 56, d, d, d, d, 1, d, 112, None) == -1
    assert b"ldn_grouped_wide_conv3x3_image:" in lib.ldn_last_error()
