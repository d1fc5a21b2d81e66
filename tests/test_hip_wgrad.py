"""ops.wgrad_rows (ldn_wgrad_rows: the weight gradient of a packed-row convolution) against a float64 CPU reference, both arithmetic modes.

Reference: tests/wgrad_ref.py -- an explicit gather plus einsum in float64, itself pinned against torch.autograd.grad of F.conv2d by
tests/test_wgrad_ref.py.  Error metric: e = max |got - ref| / max(sum_r |dY| |A|) (the float64 componentwise bound matrix).

Tolerance.  The yardstick is the computation this kernel replaces in laudnet_amd/training.py: the gathered columns and `du.t() @ cols` in fp32
on the GPU (PyTorch's GEMM), measured by every test on ITS OWN case as e_parent:
    fp32 mode:    e <= 4 * e_parent                (the margin covers a different summation order over up to 1e5 rows)
    bf16x3 mode:  e <= 4 * e_parent + 2^-15        (the dropped lo * lo term and the rounding of lo, per product, relative to |dy| |a|)
profiles/wgrad_parity.json holds e_parent, e and the bound of every case as measured on an MI355X (count == 0: exactly zero on both sides,
asserted as such).

Cases: taps 1 and 9 with and without a_rows; the count equal to m_cap, strictly inside it and 0; rows past the count poisoned (NaN in dY,
out-of-range garbage in a_rows); -1 and >= a_valid neighbours; lddy > cout and lda > cin; row counts that are no multiple of any tile or
split size; the ResNet shapes; neighbour tables from ops.mask_to_index of a seeded mask at stride 1 and 2; bit-identical repeats; a shape
outside ops.wgrad_rows_ok raises LdnError.  Set LDN_WGRAD_PARITY_OUT=<file> to dump the measured figures as JSON."""
import json
import os

import pytest
import torch

from fill import seeded_bernoulli
from helpers import apply_math_mode  # noqa: F401  (autouse: sets the thread's math mode from the `math_mode` parameter)
from wgrad_ref import wgrad_error, wgrad_ref_f64

DEV = "cuda:0"
BF16X3_TERM = 2.0 ** -15
_MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measurements():
    yield
    path = os.environ.get("LDN_WGRAD_PARITY_OUT")
    if path and _MEASURED:
        with open(path, "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _parent_fp32(dy, a, a_rows, taps, count, a_valid):
    """What training.py computed before the kernel: the [rows, taps * cin] gather (zero row for a missing neighbour) and ONE fp32 GEMM on
    the GPU -- on the first `count` rows."""
    cout, cin = dy.shape[1], a.shape[1]
    if count == 0:
        return torch.zeros(cout, taps, cin, device=dy.device)
    d = dy[:count].contiguous()
    if a_rows is None:
        cols = a[:count].unsqueeze(1).expand(count, taps, cin).reshape(count, taps * cin)
    else:
        nb = a_rows.view(-1, taps)[:count].long()
        az = torch.cat((a[:, :cin], torch.zeros(1, cin, device=a.device)))
        nb = torch.where((nb >= 0) & (nb < a_valid), nb, torch.full_like(nb, a.shape[0]))
        cols = az[nb.reshape(-1)].view(count, taps * cin)
    return (d.t() @ cols).view(cout, taps, cin)


def _check(name, math_mode, dy, a, *, a_rows=None, taps=1, count=None, m_count=None, m_cap=None, a_valid=None):
    """dy / a / a_rows on the device; `count` = the host's knowledge of *m_count (reference only)."""
    from laudnet_amd import ops
    m_cap = (dy.shape[0] if a_rows is None else a_rows.numel() // taps) if m_cap is None else m_cap
    count = m_cap if count is None else count
    av = a.shape[0] if a_valid is None else a_valid
    ref, bound = wgrad_ref_f64(dy, a, a_rows, taps, count, av)
    got = ops.wgrad_rows(dy, a, a_rows=a_rows, taps=taps, m_count=m_count, m_cap=m_cap, a_valid=a_valid)
    again = ops.wgrad_rows(dy, a, a_rows=a_rows, taps=taps, m_count=m_count, m_cap=m_cap, a_valid=a_valid)
    parent = _parent_fp32(dy, a, a_rows, taps, count, av)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (dy.shape[1], taps, a.shape[1]) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    assert torch.equal(got, again), f"{name}: two calls on the same inputs differ"
    e, e_parent = wgrad_error(got, ref, bound), wgrad_error(parent, ref, bound)
    limit = 4 * e_parent + (BF16X3_TERM if math_mode == "bf16x3" else 0.0)
    _MEASURED[f"{name}[{math_mode}]"] = {"rows": count, "m_cap": m_cap, "cin": a.shape[1], "cout": dy.shape[1], "taps": taps,
                                         "e_parent_fp32_gemm": e_parent, "e_kernel": e, "bound": limit}
    print(f"wgrad parity {name}[{math_mode}]: e_parent {e_parent:.3e}  e_kernel {e:.3e}  bound {limit:.3e}")
    if count == 0:
        assert got.abs().max().item() == 0, f"{name}: count == 0 must give zeros"
    assert e <= limit, f"{name}: e {e:.3e} > {limit:.3e} (parent fp32 GEMM {e_parent:.3e})"
    return got


def _random_table(rows, a_n, taps, seed, missing=0.2, beyond=None):
    """[rows, taps] int32: rows of A, a share of -1 entries and (beyond = (a_valid, a_n)) some entries in [a_valid, a_n) -- zero rows too"""
    g = torch.Generator().manual_seed(seed)
    hi = a_n if beyond is None else beyond[0]
    t = torch.randint(0, hi, (rows, taps), generator=g)
    u = torch.rand((rows, taps), generator=g)
    t = torch.where(u < missing, torch.full_like(t, -1), t)
    if beyond is not None:
        t = torch.where(u > 0.9, torch.randint(beyond[0], beyond[1], (rows, taps), generator=g), t)
    return t.to(torch.int32)


# (name, rows, cin, cout, taps, use a_rows): ResNet shapes first
SHAPES = [
    ("r50_s1_conv2_64x64_t9_2x56x56", 2 * 56 * 56, 64, 64, 9, True),
    ("r50_s1_conv1_256to64_t1", 2 * 28 * 28, 256, 64, 1, True),
    ("r50_s1_conv3_64to256_t1", 2 * 28 * 28, 64, 256, 1, False),
    ("r50_s4_conv2_512x512_t9_14x14", 2 * 14 * 14, 512, 512, 9, True),
    ("r50_s4_conv1_2048to512_t1_7x7", 4 * 7 * 7, 2048, 512, 1, True),
    ("odd_rows_20011_64x64_t1", 20011, 64, 64, 1, False),
    ("odd_rows_1237_72x36_t9", 1237, 72, 36, 9, True),
    ("ragged_tiles_200x132_t1", 777, 200, 132, 1, True),
    ("t9_without_a_rows_40x8", 333, 40, 8, 9, False),
    ("tiny_5_rows_8x4_t1", 5, 8, 4, 1, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_wgrad_rows_vs_fp64(shape, math_mode):
    """count == m_cap, no device-side count: every row is read"""
    name, rows, cin, cout, taps, use_rows = shape
    a_n = rows + 37 if use_rows else rows
    dy, a = _randn((rows, cout), 1).to(DEV), _randn((a_n, cin), 2).to(DEV)
    a_rows = _random_table(rows, a_n, taps, 3).to(DEV) if use_rows else None
    _check(name, math_mode, dy, a, a_rows=a_rows, taps=taps)


@pytest.mark.gpu
@pytest.mark.parametrize("taps,use_rows", [(1, False), (1, True), (9, True), (9, False)])
@pytest.mark.parametrize("count_kind", ["full", "inside", "zero"])
def test_wgrad_rows_device_count_and_poisoned_tail(taps, use_rows, count_kind, math_mode):
    """The count is read on the device; rows past it hold NaN in dY and out-of-range garbage in a_rows and must not be read: the result is
    finite and equals the reference.  Also: lddy > cout, lda > cin (column slices of wider matrices), -1 and >= a_valid neighbours."""
    rows, cin, cout = 3001, 64, 72
    count = {"full": rows, "inside": 1789, "zero": 0}[count_kind]
    a_n, a_valid = rows + 100, rows + 50
    dy_wide, a_wide = _randn((rows, cout + 12), 11), _randn((a_n, cin + 8), 12)
    dy_wide[count:] = float("nan")
    dy_wide[:, cout:] = float("nan")                        # the padding columns are not the op's to read either
    a_wide[:, cin:] = float("nan")
    a_wide[a_valid:] = float("nan")                         # rows >= a_valid are zero rows by contract: never loaded
    dy_dev, a_dev = dy_wide.to(DEV), a_wide.to(DEV)
    dy, a = dy_dev[:, :cout], a_dev[:, :cin]
    a_rows = None
    if use_rows:
        t = _random_table(rows, a_n, taps, 13, beyond=(a_valid, a_n))
        t[count:] = torch.randint(1 << 28, 1 << 30, t[count:].shape, generator=torch.Generator().manual_seed(14), dtype=torch.int32)
        a_rows = t.to(DEV)
    m_count = torch.tensor([count], dtype=torch.int32, device=DEV)
    _check(f"count_{count_kind}_t{taps}_{'list' if use_rows else 'nolist'}", math_mode, dy, a, a_rows=a_rows, taps=taps, count=count,
           m_count=m_count, m_cap=rows, a_valid=a_valid if use_rows else None)
    dy_dev.zero_(), a_dev.zero_()          # no NaN block goes back to the caching allocator (a later torch.empty would hand it out)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
def test_wgrad_rows_on_real_index_lists(stride, math_mode):
    """The neighbour table (taps 9) and the pixel list (taps 1) of ops.mask_to_index of a seeded mask, with its device-side counts; the
    tables' rows past the counts are whatever the list build left there."""
    from laudnet_amd import ops
    B, S, Ho, Wo, W, Cin = 3, 7, 28, 28, 64, 256
    Hi, Wi = Ho * stride, Wo * stride
    mask = seeded_bernoulli((B, S, S), 0.5, 21 + stride).float().to(DEV)
    ix = ops.mask_to_index(mask, Ho, Wo, stride)
    n3, n1 = (int(v) for v in ix.cnt.tolist())
    assert 0 < n3 < ix.cap3 and 0 < n1 < ix.cap1
    h1, du2 = _randn((ix.cap1, W), 31).to(DEV), _randn((ix.cap3, W), 32).to(DEV)
    du2[n3:] = float("nan")
    _check(f"mask_to_index_s{stride}_conv2", math_mode, du2, h1, a_rows=ix.nbr, taps=9, count=n3, m_count=ix.cnt[0:1], m_cap=ix.cap3,
           a_valid=ix.cap1)
    x2d, du1 = _randn((B * Hi * Wi, Cin), 33).to(DEV), _randn((ix.cap1, W), 34).to(DEV)
    du1[n1:] = float("nan")
    _check(f"mask_to_index_s{stride}_conv1", math_mode, du1, x2d, a_rows=ix.idx1, taps=1, count=n1, m_count=ix.cnt[1:2], m_cap=ix.cap1)
    du2.zero_(), du1.zero_()               # (as above: no NaN block goes back to the allocator)


@pytest.mark.gpu
def test_wgrad_rows_out_argument_and_predicate():
    from laudnet_amd import LdnError, ops
    assert ops.wgrad_rows_ok(64, 64, 9) and ops.wgrad_rows_ok(2048, 512, 1) and ops.wgrad_rows_ok(72, 36, 9)
    assert not ops.wgrad_rows_ok(64, 64, 3) and not ops.wgrad_rows_ok(12, 64, 1) and not ops.wgrad_rows_ok(64, 6, 1)
    assert not ops.wgrad_rows_ok(1024, 64, 9) and not ops.wgrad_rows_ok(64, 4096, 1)
    dy, a = _randn((100, 64), 1).to(DEV), _randn((100, 12), 2).to(DEV)
    with pytest.raises(LdnError):                     # cin % 8 != 0: an error, never a fallback
        ops.wgrad_rows(dy, a)
    with pytest.raises(LdnError):                     # taps outside {1, 9}
        ops.wgrad_rows(dy, _randn((100, 64), 2).to(DEV), taps=3)
    with pytest.raises(LdnError):                     # m_cap beyond dy
        ops.wgrad_rows(dy, _randn((100, 64), 2).to(DEV), m_cap=101)
    a = _randn((100, 64), 2).to(DEV)
    out = torch.full((64, 1, 64), float("nan"), device=DEV)
    got = ops.wgrad_rows(dy, a, out=out, math="fp32")
    assert got is out and bool(torch.isfinite(out).all())            # fully overwritten
    assert torch.equal(out, ops.wgrad_rows(dy, a, math="fp32"))
    with pytest.raises(LdnError):
        ops.wgrad_rows(dy, a, out=torch.empty(64, 64, device=DEV))
