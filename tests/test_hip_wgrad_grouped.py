"""ops.wgrad_grouped_rows (ldn_wgrad_grouped_rows: the weight gradient of the grouped 3x3 over packed rows) against the float64 reference of
tests/wgrad_grouped_ref.py (pinned against autograd by tests/test_wgrad_grouped_ref.py), both arithmetic modes.

Tables: real ops.mask_to_index lists of Bernoulli pixel masks with a corner, an edge and its neighbour forced on (the cases of
test_hip_regnet_ops.py::ROWS_CASES that the kernel's three group widths take, plus one whose rows are split over several workgroups).  Every case
has lddy > C and lda > C (column slices of wider matrices, NaN in the padding columns), NaN in every row of dY past the count and in the h_a
rows past the dilated list's count, and an output pre-filled with NaN.

Bound, derived: the kernel forms fp32 products and adds them in fp32, n = count terms per element in a fixed order of at most n + 4 rounded
operations on any term (the FMAs of a row slice, then the slices, then the row splits), so elementwise
    |got - exact| <= (n + 4) * 2^-24 * sum_r |dY| |A|
Both arithmetic modes run this fp32 form (there is no three-product form), so bf16x3 gets no further allowance.  The measured maximum of
|got - exact| / ((n + 4) 2^-24 sum |dY| |A|) per case is printed; LDN_WGRAD_GROUPED_PARITY_OUT=<file> dumps the figures as JSON
(profiles/wgrad_grouped_parity.json)."""
import json
import os

import pytest
import torch

from fill import seeded_bernoulli, seeded_randn
from helpers import apply_math_mode  # noqa: F401  (autouse: sets the thread's math mode from the `math_mode` parameter)
from wgrad_grouped_ref import wgrad_grouped_ref_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U = 2.0 ** -24
_MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measurements():
    yield
    path = os.environ.get("LDN_WGRAD_GROUPED_PARITY_OUT")
    if path and _MEASURED:
        with open(path, "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


def _splits(ops, m_cap, C, gw):
    """the row splits of the launch, read off the workspace plan (0 bytes = one split)"""
    from laudnet_amd import _lib
    nbytes = _lib.load().ldn_wgrad_grouped_rows_workspace_bytes(m_cap, C, gw)
    assert nbytes % (C * 9 * gw * 4) == 0
    return max(1, nbytes // (C * 9 * gw * 4))


def _tables(gw, C, B, Ho, Wo, stride, keep):
    from laudnet_amd import ops
    seed = 3000 + 7 * gw + C + stride
    mask = seeded_bernoulli((B, Ho, Wo), keep, seed)
    mask[0, 0, 0] = 1.0                     # a corner, an edge and its neighbour: every border class of the neighbour table
    mask[0, 0, 1] = 1.0
    mask[0, -1, -1] = 1.0
    ix = ops.mask_to_index(mask.to(DEV), Ho, Wo, stride)
    torch.cuda.synchronize()
    return ix, int(ix.cnt[0]), int(ix.cnt[1]), seed


def _operands(ix, n1, C, seed, count):
    """dY [cap3, C + 12] and h_a [cap1, C + 8] on the device: NaN in the padding columns, in dY's rows past `count`, in h_a's rows past n1"""
    dy_wide, a_wide = seeded_randn((ix.cap3, C + 12), seed + 1), seeded_randn((ix.cap1, C + 8), seed + 2)
    dy_wide[count:] = NAN
    dy_wide[:, C:] = NAN
    a_wide[n1:] = NAN
    a_wide[:, C:] = NAN
    return dy_wide.to(DEV), a_wide.to(DEV)


def _check(name, math_mode, ix, n1, gw, C, seed, count, m_count):
    from laudnet_amd import ops
    dy_dev, a_dev = _operands(ix, n1, C, seed, count)
    dy, a = dy_dev[:, :C], a_dev[:, :C]
    ref, bound = wgrad_grouped_ref_f64(dy, a, ix.nbr, gw, count, ix.cap1)
    out = torch.full((C, 9, gw), NAN, device=DEV)
    got = ops.wgrad_grouped_rows(dy, a, ix.nbr, gw, m_count=m_count, m_cap=ix.cap3, a_valid=ix.cap1, out=out)
    again = ops.wgrad_grouped_rows(dy, a, ix.nbr, gw, m_count=m_count, m_cap=ix.cap3, a_valid=ix.cap1)
    torch.cuda.synchronize()
    assert got is out and tuple(again.shape) == (C, 9, gw) and again.dtype == torch.float32
    assert not bool(torch.isnan(got).any()), f"{name}: NaN in the result (a row past the count was read, or the output is not fully overwritten)"
    assert torch.equal(got, again), f"{name}: two launches on the same inputs differ"
    err = (got.double().cpu() - ref).abs()
    limit = (count + 4) * U * bound
    ratio = torch.where(limit > 0, err / limit.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = ratio.max().item()
    _MEASURED[f"{name}[{math_mode}]"] = {"rows": count, "m_cap": ix.cap3, "C": C, "gw": gw, "splits": _splits(ops, ix.cap3, C, gw),
                                         "max_abs_err": err.max().item(), "max_err_over_bound": worst,
                                         "bound": "(rows + 4) * 2^-24 * sum_r |dY| |A|, elementwise"}
    print(f"wgrad_grouped parity {name}[{math_mode}]: rows {count}  max |err| {err.max().item():.3e}  max err / bound {worst:.3e}")
    if count == 0:
        assert got.abs().max().item() == 0, f"{name}: count == 0 must give zeros"
    assert bool((err <= limit).all()), f"{name}: |got - exact| exceeds (n + 4) 2^-24 sum |dY| |A| by a factor of {worst:.3e}"
    dy_dev.zero_(), a_dev.zero_()          # no NaN block goes back to the caching allocator (a later torch.empty would hand it out)


# gw, C, B, Ho, Wo, stride, keep
CASES = [
    (8, 8, 3, 14, 14, 1, 0.5),             # one group
    (8, 64, 3, 14, 10, 2, 0.5),
    (16, 16, 3, 14, 14, 2, 0.5),
    (16, 64, 8, 14, 14, 1, 0.6),           # several row splits live
    (24, 48, 3, 9, 14, 2, 0.6),
]


@pytest.mark.parametrize("gw,C,B,Ho,Wo,stride,keep", CASES)
def test_wgrad_grouped_rows_vs_fp64(gw, C, B, Ho, Wo, stride, keep, math_mode):
    from laudnet_amd import ops
    ix, n3, n1, seed = _tables(gw, C, B, Ho, Wo, stride, keep)
    assert 0 < n3 < ix.cap3 and 0 < n1 <= ix.cap1, "the device-side count of the kept rows must be below the capacity"      # (stride 1: the dilated list may hold every pixel)
    if B == 8:
        # the plan splits the rows at least two ways, each split at most m_cap / 2 rounded up to a chunk of 32 rows: more kept rows than that
        # means at least two splits hold rows
        assert _splits(ops, ix.cap3, C, gw) >= 2 and n3 > ix.cap3 // 2 + 32, (_splits(ops, ix.cap3, C, gw), n3, ix.cap3)
    _check(f"gw{gw}_C{C}_B{B}_{Ho}x{Wo}_s{stride}", math_mode, ix, n1, gw, C, seed, n3, ix.cnt[0:1])


@pytest.mark.parametrize("count_kind", ["zero", "one", "m_cap"])
@pytest.mark.parametrize("gw,C", [(8, 16), (16, 32), (24, 48)])
def test_wgrad_grouped_rows_counts_0_1_and_m_cap(gw, C, count_kind, math_mode):
    """count 0 (zeros), 1, and m_cap (every pixel kept: the table is full); the count is read on the device"""
    keep = 1.0 if count_kind == "m_cap" else 0.5
    ix, n3, n1, seed = _tables(gw, C, 3, 9, 14, 1, keep)
    count = {"zero": 0, "one": 1, "m_cap": ix.cap3}[count_kind]
    assert count <= n3 and (count_kind != "m_cap" or n3 == ix.cap3)
    m_count = torch.tensor([count], dtype=torch.int32, device=DEV)
    _check(f"count_{count_kind}_gw{gw}_C{C}", math_mode, ix, n1, gw, C, seed, count, m_count)


def test_wgrad_grouped_rows_without_a_device_count_reads_every_row():
    """m_count = None: the count is m_cap"""
    ix, n3, n1, seed = _tables(16, 32, 2, 7, 7, 1, 1.0)
    assert n3 == ix.cap3
    _check("no_device_count_gw16_C32", "fp32", ix, n1, 16, 32, seed, ix.cap3, None)


def test_wgrad_grouped_rows_predicate_and_argument_errors():
    from laudnet_amd import LdnError, ops
    for gw in (8, 16, 24):
        assert ops.wgrad_grouped_rows_ok(gw, gw) and ops.wgrad_grouped_rows_ok(2 * gw, gw) and ops.wgrad_grouped_rows_ok(2048 // gw * gw, gw)
    assert not ops.wgrad_grouped_rows_ok(12, 6) and not ops.wgrad_grouped_rows_ok(20, 8) and not ops.wgrad_grouped_rows_ok(4096, 16)
    assert not ops.wgrad_grouped_rows_ok(112, 56) and not ops.wgrad_grouped_rows_ok(0, 8)
    ix, n3, n1, seed = _tables(8, 24, 2, 7, 7, 1, 0.5)
    dy, a = seeded_randn((ix.cap3, 24), 1).to(DEV), seeded_randn((ix.cap1, 24), 2).to(DEV)
    with pytest.raises(LdnError):                     # group width 6: outside the predicate -- an error, never a fallback
        ops.wgrad_grouped_rows(dy, a, ix.nbr, 6, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # 24 channels are no multiple of 16
        ops.wgrad_grouped_rows(dy, a, ix.nbr, 16, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # m_cap beyond dy
        ops.wgrad_grouped_rows(dy[:10], a, ix.nbr, 8, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # a_valid beyond a
        ops.wgrad_grouped_rows(dy, a, ix.nbr, 8, m_count=ix.cnt[0:1], a_valid=ix.cap1 + 1)
    with pytest.raises(LdnError):                     # the wrong output shape
        ops.wgrad_grouped_rows(dy, a, ix.nbr, 8, m_count=ix.cnt[0:1], out=torch.empty(24, 8, 9, device=DEV))
    got = ops.wgrad_grouped_rows(dy, a, ix.nbr, 8, m_count=ix.cnt[0:1], a_valid=ix.cap1, math="bf16x3")
    assert torch.equal(got, ops.wgrad_grouped_rows(dy, a, ix.nbr, 8, m_count=ix.cnt[0:1], a_valid=ix.cap1, math="fp32")), "both modes run the fp32 form"
