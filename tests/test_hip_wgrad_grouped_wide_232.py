"""ops.wgrad_grouped_wide_rows at group width 232, the width of lad_regnet_y_32gf (ldn_wgrad_grouped_wide_rows: two dY tiles of 128 out
channels per group -- the second with 104 live -- and 17 column tiles over F = 2088, the last with 40 live) against the float64 reference of
tests/wgrad_grouped_ref.py, both arithmetic modes.

Tables, operands and the error statement are those of tests/test_hip_wgrad_grouped_wide.py: real ops.mask_to_index lists; dY [cap3, C + 12]
and h_a [cap1, C + 8] with NaN in the padding columns, in dY's rows past the count and in h_a's rows past the dilated list's count; an output
pre-filled with NaN.  e = max |got - ref| / max(sum_r |dY| |A|); the yardstick is the gather + bmm path this kernel replaces
(training._weight_grad_grouped_3x3), measured by every test on ITS OWN case as e_parent:
    fp32 mode:    e <= 4 * e_parent
    bf16x3 mode:  e <= 4 * e_parent + 2^-15
The rule is applied to the whole dW and, with the yardstick and the scale taken on the same slice, to each n-tile on its own: out channels
0-127 and 128-231 of every group.  e_parent, e and the bound are printed per case; LDN_WGRAD_GROUPED_WIDE_232_PARITY_OUT=<file> dumps them as
JSON (profiles/wgrad_grouped_wide_232_parity.json)."""
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
GW = 232
BF16X3_TERM = 2.0 ** -15
_MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measurements():
    yield
    path = os.environ.get("LDN_WGRAD_GROUPED_WIDE_232_PARITY_OUT")
    if path and _MEASURED:
        with open(path, "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


def _splits(m_cap, C):
    """the row splits of the launch, read off the workspace plan (0 bytes = one split)"""
    from laudnet_amd import _lib
    nbytes = _lib.load().ldn_wgrad_grouped_wide_rows_workspace_bytes(m_cap, C, GW)
    assert nbytes % (C * 9 * GW * 4) == 0
    return max(1, nbytes // (C * 9 * GW * 4))


def _parent_fp32(dy, a, nbr, cap1, count):
    """the gather + one fp32 bmm on the GPU, on the first `count` rows of dY and of the table -> [C, 9, gw]"""
    from laudnet_amd import training
    C = dy.shape[1]
    if count == 0:
        return torch.zeros(C, 9, GW, device=dy.device)
    dw = training._weight_grad_grouped_3x3(dy[:count].contiguous(), a, nbr.view(-1, 9)[:count].contiguous(), cap1, GW)
    return dw.reshape(C, GW, 9).permute(0, 2, 1).contiguous()


def _check(name, math_mode, ix, n1, C, seed, count, m_count):
    from laudnet_amd import ops
    dy_dev, a_dev = _operands(ix, n1, C, seed, count)
    dy, a = dy_dev[:, :C], a_dev[:, :C]
    assert dy.stride(0) == C + 12 and a.stride(0) == C + 8
    ref, bound = wgrad_grouped_ref_f64(dy, a, ix.nbr, GW, count, ix.cap1)
    out = torch.full((C, 9, GW), NAN, device=DEV)
    got = ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, GW, m_count=m_count, m_cap=ix.cap3, a_valid=ix.cap1, out=out)
    again = ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, GW, m_count=m_count, m_cap=ix.cap3, a_valid=ix.cap1)
    parent = _parent_fp32(dy, a, ix.nbr, ix.cap1, count)
    torch.cuda.synchronize()
    assert got is out and tuple(again.shape) == (C, 9, GW) and again.dtype == torch.float32
    assert not bool(torch.isnan(got).any()), f"{name}: NaN in the result (a row past the count was read, or the output is not fully overwritten)"
    assert torch.equal(got, again), f"{name}: two launches on the same inputs differ"
    G = C // GW
    rec = {"rows": count, "m_cap": ix.cap3, "C": C, "gw": GW, "splits": _splits(ix.cap3, C)}
    for part, rows in (("all", slice(0, GW)), ("n_tile_0", slice(0, 128)), ("n_tile_1", slice(128, GW))):
        def cut(t):
            return t.reshape(G, GW, 9, GW)[:, rows]
        e, e_parent = wgrad_error(cut(got), cut(ref), cut(bound)), wgrad_error(cut(parent), cut(ref), cut(bound))
        limit = 4 * e_parent + (BF16X3_TERM if math_mode == "bf16x3" else 0.0)
        rec[part] = {"e_parent_fp32_bmm": e_parent, "e_kernel": e, "bound": limit}
        print(f"wgrad_grouped_wide_232 parity {name}[{math_mode}] {part}: rows {count}  e_parent {e_parent:.3e}  e_kernel {e:.3e}  bound {limit:.3e}")
    _MEASURED[f"{name}[{math_mode}]"] = rec
    if count == 0:
        assert got.abs().max().item() == 0, f"{name}: count == 0 must give zeros"
        assert parent.abs().max().item() == 0
    for part in ("all", "n_tile_0", "n_tile_1"):
        r = rec[part]
        assert r["e_kernel"] <= r["bound"], f"{name} {part}: e {r['e_kernel']:.3e} > {r['bound']:.3e} (parent fp32 bmm {r['e_parent_fp32_bmm']:.3e})"
    dy_dev.zero_(), a_dev.zero_()          # no NaN block goes back to the caching allocator (a later torch.empty would hand it out)


# C, B, Ho = Wo, stride, keep
CASES = [
    (232, 3, 5, 1, 1.0),            # one group, every pixel kept: 75 rows, a ragged last chunk
    (232, 3, 5, 1, 0.6),
    (232, 3, 7, 2, 0.6),            # stride 2
    (464, 3, 5, 1, 0.6),            # the group offset into dY, A and dW
    (464, 3, 7, 2, 1.0),
    (464, 3, 7, 2, 0.6),
    (464, 8, 7, 1, 0.6),            # 392 rows of capacity: the plan splits them and more than one split holds rows
]


@pytest.mark.parametrize("C,B,Ho,stride,keep", CASES)
def test_wgrad_grouped_wide_rows_232_vs_fp64(C, B, Ho, stride, keep, math_mode):
    ix, n3, n1, seed = _tables(GW, C + B + int(10 * keep), B, Ho, Ho, stride, keep)      # (the second argument only seeds the mask)
    if keep < 1:
        assert 0 < n3 < ix.cap3 and 0 < n1 <= ix.cap1
    else:
        assert n3 == ix.cap3
    if B == 8:
        # each split holds at most m_cap / 2 rounded up to a chunk of 32 rows: more kept rows than that means at least two splits hold rows
        assert _splits(ix.cap3, C) >= 2 and n3 > ix.cap3 // 2 + 32, (_splits(ix.cap3, C), n3, ix.cap3)
    else:
        assert _splits(ix.cap3, C) == 1
    _check(f"gw{GW}_C{C}_B{B}_{Ho}x{Ho}_s{stride}_keep{keep}", math_mode, ix, n1, C, seed, n3, ix.cnt[0:1])


@pytest.mark.parametrize("count_kind", ["zero", "one", "m_cap"])
@pytest.mark.parametrize("C", [232, 464])
def test_wgrad_grouped_wide_rows_232_counts_0_1_and_m_cap(C, count_kind, math_mode):
    """count 0 (zeros), 1, and m_cap (every pixel kept: the table is full); the count is read on the device.  8 images of 7 x 7: the rows are
    split, so count 0 and 1 run the reduce launch with no or one live split"""
    keep = 1.0 if count_kind == "m_cap" else 0.5
    ix, n3, n1, seed = _tables(GW, C, 8, 7, 7, 1, keep)
    assert _splits(ix.cap3, C) >= 2
    count = {"zero": 0, "one": 1, "m_cap": ix.cap3}[count_kind]
    assert count <= n3 and (count_kind != "m_cap" or n3 == ix.cap3)
    m_count = torch.tensor([count], dtype=torch.int32, device=DEV)
    _check(f"count_{count_kind}_gw{GW}_C{C}", math_mode, ix, n1, C, seed, count, m_count)


def test_wgrad_grouped_wide_rows_232_without_a_device_count_reads_every_row(math_mode):
    """m_count = None: the count is m_cap"""
    ix, n3, n1, seed = _tables(GW, 464, 2, 5, 5, 1, 1.0)
    assert n3 == ix.cap3
    _check(f"no_device_count_gw{GW}_C464", math_mode, ix, n1, 464, seed, ix.cap3, None)


def test_wgrad_grouped_wide_rows_232_predicate_and_argument_errors():
    from laudnet_amd import LdnError, ops
    for C in (232, 696, 1392, 3712):
        assert ops.wgrad_grouped_wide_rows_ok(C, GW)
    assert not ops.wgrad_grouped_wide_rows_ok(464, 116) and not ops.wgrad_grouped_wide_rows_ok(240, GW)
    assert not ops.wgrad_grouped_wide_rows_ok(4176, GW) and not ops.wgrad_grouped_wide_rows_ok(528, 264)
    assert not ops.wgrad_grouped_rows_ok(464, GW), "the VALU kernel's predicate is what it was"
    ix, n3, n1, seed = _tables(GW, 464, 2, 5, 5, 1, 0.5)
    dy, a = seeded_randn((ix.cap3, 464), 1).to(DEV), seeded_randn((ix.cap1, 464), 2).to(DEV)
    with pytest.raises(LdnError):                     # half the width: an error, never a fallback
        ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, 116, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # 240 channels are no multiple of 232
        ops.wgrad_grouped_wide_rows(dy[:, :240], a[:, :240], ix.nbr, GW, m_count=ix.cnt[0:1])
    with pytest.raises(LdnError):                     # the wrong output shape
        ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, GW, m_count=ix.cnt[0:1], out=torch.empty(464, GW, 9, device=DEV))
    got = ops.wgrad_grouped_wide_rows(dy, a, ix.nbr, GW, m_count=ix.cnt[0:1], a_valid=ix.cap1, math="fp32")
    assert tuple(got.shape) == (464, 9, GW) and bool(torch.isfinite(got).all())
