"""ops.wgrad_grouped_wide_rows (ldn_wgrad_grouped_wide_rows: the matrix-core weight gradient of the grouped 3x3 over packed rows at group
widths 56 and 112) against the float64 reference of tests/wgrad_grouped_ref.py (pinned against autograd at these widths by
tests/test_wgrad_grouped_wide_ref.py), both arithmetic modes.

Tables and operands: those of tests/test_hip_wgrad_grouped.py (its _tables and _operands) -- real ops.mask_to_index lists of Bernoulli pixel
masks with a corner, an edge and its neighbour forced on; dY [cap3, C + 12] and h_a [cap1, C + 8] with NaN in the padding columns, in dY's rows
past the count and in h_a's rows past the dilated list's count; an output pre-filled with NaN.

Error statement: that of tests/test_hip_wgrad.py.  e = max |got - ref| / max(sum_r |dY| |A|) (wgrad_ref.wgrad_error); the yardstick is the
computation this kernel replaces, training._weight_grad_grouped_3x3 (the gather and one torch.bmm in fp32 on the GPU) on the first `count` rows
of dY and of the table, measured by every test on ITS OWN case as e_parent:
    fp32 mode:    e <= 4 * e_parent
    bf16x3 mode:  e <= 4 * e_parent + 2^-15        (the dropped lo * lo term and the rounding of lo, per product, relative to |dy| |a|)
No floor; at count == 0 both sides are exactly zero.  e_parent, e and the bound are printed per case; LDN_WGRAD_GROUPED_WIDE_PARITY_OUT=<file>
dumps them as JSON (profiles/wgrad_grouped_wide_parity.json)."""
import json
import os

import pytest
import torch

from fill import seeded_randn
from helpers import apply_math_mode  # noqa: F401  (autouse: sets the thread's math mode from the `math_mode` parameter)
from test_hip_wgrad_grouped import _operands, _tables
from wgrad_grouped_ref import wgrad_grouped_ref_f64
from wgrad_ref import wgrad_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF16X3_TERM = 2.0 ** -15
_MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measurements():
    yield
    path = os.environ.get("LDN_WGRAD_GROUPED_WIDE_PARITY_OUT")
    if path and _MEASURED:
        with open(path, "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


def _splits(m_cap, C, gw):
    """the row splits of the launch, read off the workspace plan (0 bytes = one split)"""
    from laudnet_amd import _lib
    nbytes = _lib.load().ldn_wgrad_grouped_wide_rows_workspace_bytes(m_cap, C, gw)
    assert nbytes % (C * 9 * gw * 4) == 0
    return max(1, nbytes // (C * 9 * gw * 4))


def _parent_fp32(dy, a, nbr, cap1, gw, count):
    """What training.py runs without the kernel: the gather + one fp32 bmm on the GPU, on the first `count` rows of dY and of the table (sliced
    first: the fallback multiplies, so NaN past the count must not reach it) -> [C, 9, gw]"""
    from laudnet_amd import training
    C = dy.shape[1]
    if count == 0:
        return torch.zeros(C, 9, gw, device=dy.device)
    dw = training._weight_grad_grouped_3x3(dy[:count].contiguous(), a, nbr.view(-1, 9)[:count].contiguous(), cap1, gw)
    return dw.reshape(C, gw, 9).permute(0, 2, 1).contiguous()


def _check(name, math_mode, ix, n1, gw, C, seed, count, m_count):
    from laudnet_amd import ops
    dy_dev, a_dev = _operands(ix, n1, C, seed, count)
    dy, a = dy_dev[:, :C], a_dev[:, :C]
    ref, bound = wgrad_grouped_ref_f64(dy, a, ix.nbr, gw, count, ix.cap1)
    out = torch.full((C, 9, gw), NAN, device=DEV)
    got = ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, gw, m_count=m_count, m_cap=ix.cap3, a_valid=ix.cap1, out=out)
    again = ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, gw, m_count=m_count, m_cap=ix.cap3, a_valid=ix.cap1)
    parent = _parent_fp32(dy, a, ix.nbr, ix.cap1, gw, count)
    torch.cuda.synchronize()
    assert got is out and tuple(again.shape) == (C, 9, gw) and again.dtype == torch.float32
    assert not bool(torch.isnan(got).any()), f"{name}: NaN in the result (a row past the count was read, or the output is not fully overwritten)"
    assert torch.equal(got, again), f"{name}: two launches on the same inputs differ"
    e, e_parent = wgrad_error(got, ref, bound), wgrad_error(parent, ref, bound)
    limit = 4 * e_parent + (BF16X3_TERM if math_mode == "bf16x3" else 0.0)
    _MEASURED[f"{name}[{math_mode}]"] = {"rows": count, "m_cap": ix.cap3, "C": C, "gw": gw, "splits": _splits(ix.cap3, C, gw),
                                         "e_parent_fp32_bmm": e_parent, "e_kernel": e, "bound": limit}
    print(f"wgrad_grouped_wide parity {name}[{math_mode}]: rows {count}  e_parent {e_parent:.3e}  e_kernel {e:.3e}  bound {limit:.3e}")
    if count == 0:
        assert got.abs().max().item() == 0, f"{name}: count == 0 must give zeros"
        assert parent.abs().max().item() == 0
    assert e <= limit, f"{name}: e {e:.3e} > {limit:.3e} (parent fp32 bmm {e_parent:.3e})"
    dy_dev.zero_(), a_dev.zero_()          # no NaN block goes back to the caching allocator (a later torch.empty would hand it out)


# gw, C, B, Ho, Wo, stride, keep
CASES = [
    (56, 56, 3, 9, 14, 1, 0.5),            # one group, a ragged last chunk
    (56, 112, 3, 14, 10, 2, 0.5),          # the group offset, stride 2
    (56, 168, 8, 14, 14, 1, 0.6),          # several row splits live
    (112, 112, 3, 9, 14, 2, 0.6),
    (112, 224, 3, 14, 14, 1, 0.5),
]


@pytest.mark.parametrize("gw,C,B,Ho,Wo,stride,keep", CASES)
def test_wgrad_grouped_wide_rows_vs_fp64(gw, C, B, Ho, Wo, stride, keep, math_mode):
    ix, n3, n1, seed = _tables(gw, C, B, Ho, Wo, stride, keep)
    assert 0 < n3 < ix.cap3 and 0 < n1 <= ix.cap1, "the device-side count of the kept rows must be below the capacity"      # (stride 1: the dilated list may hold every pixel)
    if B == 8:
        # the plan splits the rows at least two ways, each split at most m_cap / 2 rounded up to a chunk of 32 rows: more kept rows than that
        # means at least two splits hold rows
        assert _splits(ix.cap3, C, gw) >= 2 and n3 > ix.cap3 // 2 + 32, (_splits(ix.cap3, C, gw), n3, ix.cap3)
    _check(f"gw{gw}_C{C}_B{B}_{Ho}x{Wo}_s{stride}", math_mode, ix, n1, gw, C, seed, n3, ix.cnt[0:1])


@pytest.mark.parametrize("count_kind", ["zero", "one", "m_cap"])
@pytest.mark.parametrize("gw,C", [(56, 112), (112, 112)])
def test_wgrad_grouped_wide_rows_counts_0_1_and_m_cap(gw, C, count_kind, math_mode):
    """count 0 (zeros), 1, and m_cap (every pixel kept: the table is full); the count is read on the device"""
    keep = 1.0 if count_kind == "m_cap" else 0.5
    ix, n3, n1, seed = _tables(gw, C, 3, 9, 14, 1, keep)
    count = {"zero": 0, "one": 1, "m_cap": ix.cap3}[count_kind]
    assert count <= n3 and (count_kind != "m_cap" or n3 == ix.cap3)
    m_count = torch.tensor([count], dtype=torch.int32, device=DEV)
    _check(f"count_{count_kind}_gw{gw}_C{C}", math_mode, ix, n1, gw, C, seed, count, m_count)


def test_wgrad_grouped_wide_rows_without_a_device_count_reads_every_row(math_mode):
    """m_count = None: the count is m_cap"""
    ix, n3, n1, seed = _tables(56, 56, 2, 7, 7, 1, 1.0)
    assert n3 == ix.cap3
    _check("no_device_count_gw56_C56", math_mode, ix, n1, 56, 56, seed, ix.cap3, None)


def test_wgrad_grouped_wide_rows_predicate_and_argument_errors():
    from laudnet_amd import LdnError, ops
    assert ops.wgrad_grouped_wide_rows_ok(112, 56) and ops.wgrad_grouped_wide_rows_ok(112, 112) and ops.wgrad_grouped_wide_rows_ok(3024, 112)
    assert not ops.wgrad_grouped_wide_rows_ok(64, 8) and not ops.wgrad_grouped_wide_rows_ok(100, 56)
    assert not ops.wgrad_grouped_rows_ok(112, 56), "the VALU kernel's predicate is what it was"
    ix, n3, n1, seed = _tables(56, 112, 2, 7, 7, 1, 0.5)
    dy, a = seeded_randn((ix.cap3, 112), 1).to(DEV), seeded_randn((ix.cap1, 112), 2).to(DEV)
    with pytest.raises(LdnError):                     # group width 8 belongs to wgrad_grouped_rows -- an error, never a fallback
        ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, 8, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # 56 channels are no multiple of 112 ...
        ops.wgrad_grouped_wide_rows(dy[:, :56], a[:, :56], ix.nbr, 112, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # ... nor 112 of 48
        ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, 48, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # m_cap beyond dy
        ops.wgrad_grouped_wide_rows(dy[:10], a, ix.nbr, 56, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # a_valid beyond a
        ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, 56, m_count=ix.cnt[0:1], a_valid=ix.cap1 + 1)
    with pytest.raises(LdnError):                     # the wrong output shape
        ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, 56, m_count=ix.cnt[0:1], out=torch.empty(112, 56, 9, device=DEV))
    got = ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, 56, m_count=ix.cnt[0:1], a_valid=ix.cap1, math="fp32")
    assert tuple(got.shape) == (112, 9, 56) and bool(torch.isfinite(got).all())
