"""CPU: the yardstick and the host side of ldn_wgrad_grouped_wide_rows (the matrix-core weight gradient of the grouped 3x3 at group widths 56
and 112; csrc/ldn_wgrad_grouped_wide.hip).
  * tests/wgrad_grouped_ref.py's float64 formula at the new widths against torch.autograd.grad of F.conv2d(groups=C / gw), stride 1 and 2, on
    the case builder of tests/test_wgrad_grouped_ref.py (B = 2, a 5 x 4 map, C = 2 gw) with that file's tolerance;
  * the shape predicate and the workspace plan, which are host arithmetic and answer without a GPU; the entry point refuses null pointers
    before any launch."""
import pytest

from test_wgrad_grouped_ref import _case
from wgrad_grouped_ref import wgrad_grouped_ref_f64


@pytest.fixture(scope="module")
def lib():
    from laudnet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("gw", [56, 112])
def test_wgrad_grouped_ref_is_the_autograd_weight_gradient_at_the_wide_widths(gw, stride):
    c = _case(gw, stride, 100 + gw + stride)
    got, bound = wgrad_grouped_ref_f64(c.dy, c.a, c.nbr, gw)
    assert tuple(got.shape) == (c.C, 9, gw)
    assert (got - c.gw_auto).abs().max().item() < 1e-12 * max(1.0, c.gw_auto.abs().max().item())
    assert bool((bound >= got.abs() - 1e-12).all())


def test_predicate(lib):
    from laudnet_amd import ops
    for C, gw in ((56, 56), (2016, 56), (112, 112), (3024, 112)):
        assert lib.ldn_wgrad_grouped_wide_rows_ok(C, gw) == 1, (C, gw)
        assert ops.wgrad_grouped_wide_rows_ok(C, gw) is True
    for C, gw in ((64, 8), (64, 16), (48, 24), (100, 56), (0, 56), (4144, 56), (112, 0)):
        assert lib.ldn_wgrad_grouped_wide_rows_ok(C, gw) == 0, (C, gw)
        assert ops.wgrad_grouped_wide_rows_ok(C, gw) is False


def test_workspace_plan(lib):
    f = lib.ldn_wgrad_grouped_wide_rows_workspace_bytes
    for C, gw in ((64, 8), (100, 56), (0, 56), (4144, 56), (112, 0)):
        assert f(1568, C, gw) == 0, (C, gw)
    assert f(-1, 112, 56) == 0 and f(-100352, 224, 112) == 0
    for C, gw in ((56, 56), (168, 56), (2016, 56), (112, 112), (3024, 112)):
        got = [f(m_cap, C, gw) for m_cap in (0, 31, 32, 255, 256, 1568, 100352)]
        assert all(b % (C * 9 * gw * 4) == 0 for b in got), (C, gw, got)
        assert got == sorted(got), (C, gw, got)
        assert got[0] == 0                                   # no rows, no split
        assert got == [f(m_cap, C, gw) for m_cap in (0, 31, 32, 255, 256, 1568, 100352)]      # a function of its arguments only
    assert f(100352, 56, 56) >= 2 * 56 * 9 * 56 * 4          # one group, many rows: the rows are split


def test_entry_point_refuses_null_pointers_before_any_launch(lib):
    # (dy, lddy, a, lda, a_valid, nbr, m_count, m_cap, C, gw, dw, work, math_mode, stream)
    assert lib.ldn_wgrad_grouped_wide_rows(None, 112, None, 112, 32, None, None, 32, 112, 56, None, None, -1, None) == -1
    assert b"null" in lib.ldn_last_error()
