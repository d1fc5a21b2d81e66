"""ops.rows_chanmask / ops.rows_act_bwd (csrc/ldn_train_rows.hip: the elementwise backward chain of training on packed rows) against a float64
CPU reference written here.  The kernels are plain fp32 VALU code: there is one arithmetic, no math_mode.

Inputs: u is built as m * (relu(z) - c) in fp32 with |z| >= 0.05, so no ReLU decision sits at a rounding boundary (h = u + c is either 0 or
>= 0.05 up to one rounding of a value of size <= a few).  B = 3 images, the middle one holds ZERO rows; counts 0, 1, 197 and m_cap; every
matrix has a leading dimension larger than C; rows >= count of dh, u and zy are NaN (they must not be read).

Bounds (derived, not measured; eps = 2^-24, the unit roundoff of fp32; `exact` = the float64 evaluation of the documented formula on the
fp32 inputs):
  elementwise (du, the masked u):  |got - exact| <= 4 eps |exact|   -- du = (dh * m) * s is two roundings, u * m is one.
  reduced (g_shift, g_scale_num, g_mask):  |got - exact| <= (n + 4) eps sum|terms|, n = the number of rows summed -- a term carries at most
      three roundings (zy - t or h - t: one each, h - t being formed in double from u, c, t; a * m; the product), a sum of n terms in ANY
      order at most n - 1 more, and (1 + eps)^(n + 2) - 1 < (n + 4) eps for every n here.  n == 0: exactly 0.
Determinism: every case runs twice, all outputs bit-identical -- with m_cap = 300 the rows are split four ways (75 rows per workgroup, pinned
by the CPU test below), so for counts 197 and 300 both non-empty images straddle the split and their g_mask is the sum of partials."""
import pytest
import torch

DEV = "cuda:0"
EPS = 2.0 ** -24
M_CAP = 300
B = 3


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _prefix(count):
    n0 = (3 * count) // 5
    return [0, n0, n0, count]                       # image 1 owns no rows


def _wide(t2d, poison_from=None):
    """the same values inside a matrix with a larger leading dimension (C + 8 columns), rows >= poison_from NaN"""
    rows, C = t2d.shape
    big = torch.full((rows, C + 8), float("nan"))
    big[:, :C] = t2d
    if poison_from is not None:
        big[poison_from:] = float("nan")
    return big.to(DEV)[:, :C]


def _inputs(C, count, with_mask, with_c, seed):
    pre = _prefix(count)
    img = torch.zeros(M_CAP, dtype=torch.long)
    img[pre[2]:] = 2
    z = _randn((M_CAP, C), seed)
    z = torch.sign(z) * (0.05 + z.abs())
    z[z == 0] = 0.05
    s = (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 1))) * torch.sign(_randn((C,), seed + 2))
    s[s == 0] = 1.0
    t = 0.5 * _randn((C,), seed + 3)
    c = torch.relu(t) if with_c else torch.zeros(C)
    m = (torch.rand(B, C, generator=torch.Generator().manual_seed(seed + 4)) < 0.6).float() if with_mask else torch.ones(B, C)
    u = (torch.relu(z) - c) * m[img]                # fp32, as the forward stores it
    dh = _randn((M_CAP, C), seed + 5)
    return dict(pre=pre, img=img, z=z, s=s, t=t, c=c, m=m, u=u, dh=dh)


def _reference(d, count, with_zy):
    """float64 evaluation of include/ldn_hip.h's formulas on the fp32 inputs -> values and the sum|terms| of every reduced output"""
    f = lambda x: x[:count].double() if x.dim() == 2 and x.shape[0] == M_CAP else x.double()
    u, dh, zy = f(d["u"]), f(d["dh"]), f(d["z"])
    s, t, c, m = d["s"].double(), d["t"].double(), d["c"].double(), d["m"].double()
    img = d["img"][:count]
    h = u + c
    a = torch.where(h > 0, dh, torch.zeros_like(dh))
    dz = a * m[img]
    out = dict(du=dz * s, g_shift=a.sum(0), g_shift_abs=a.abs().sum(0), g_scale=(dz * (h - t)).sum(0), g_scale_abs=(dz * (h - t)).abs().sum(0))
    if with_zy:
        term = a * (zy - t)
        out["g_mask"] = torch.stack([term[img == b].sum(0) for b in range(B)])
        out["g_mask_abs"] = torch.stack([term[img == b].abs().sum(0) for b in range(B)])
        out["g_mask_n"] = [int((img == b).sum()) for b in range(B)]
    return out


def _assert_reduced(got, exact, abs_sum, n, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    bound = (n + 4) * EPS * abs_sum
    bad = (got - exact).abs() > bound
    if n == 0:
        assert (got == 0).all(), f"{what}: no rows summed, must be exactly 0"
    worst = ((got - exact).abs() / bound.clamp(min=1e-300)).max().item() if n else 0.0
    print(f"{what}: n {n}, worst |err| / bound = {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside (n + 4) eps sum|terms| (n {n}, worst ratio {worst:.3f})"


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 197, M_CAP])
@pytest.mark.parametrize("C", [16, 40, 256, 264])
def test_rows_act_bwd_vs_float64(C, count):
    from laudnet_amd import ops
    # chan_mask / zy / post_sub each absent and present
    for vi, (with_mask, with_zy, with_c) in enumerate([(True, True, True), (False, False, False), (True, False, True), (False, True, False), (True, True, False)]):
        what = f"C {C} count {count} mask {with_mask} zy {with_zy} post_sub {with_c}"
        d = _inputs(C, count, with_mask, with_c, 100 * C + 7 * count + vi)
        ref = _reference(d, count, with_zy)
        dh, u = _wide(d["dh"], count), _wide(d["u"], count)
        zy = _wide(d["z"], count) if with_zy else None
        pre = torch.tensor(d["pre"], dtype=torch.int32, device=DEV)
        cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
        kw = dict(post_sub=d["c"].to(DEV) if with_c else None, chan_mask=d["m"].to(DEV) if with_mask else None,
                  row_prefix=pre if (with_mask or with_zy) else None, zy2d=zy, m_count=cnt, m_cap=M_CAP)
        runs = []
        for _ in range(2):
            out = torch.full((M_CAP, C + 8), float("nan"), device=DEV)[:, :C]
            du, g_shift, g_scale, g_mask = ops.rows_act_bwd(dh, u, d["s"].to(DEV), d["t"].to(DEV), out=out, **kw)
            torch.cuda.synchronize()
            runs.append((du.clone(), g_shift, g_scale, g_mask))
        for x, y in zip(*runs):
            assert (x is None and y is None) or torch.equal(x, y), f"{what}: two runs differ"
        du, g_shift, g_scale, g_mask = runs[0]
        assert torch.isfinite(du).all() and (du[count:] == 0).all(), f"{what}: du must be exactly 0 on the rows past the count"
        dud = du[:count].double().cpu()
        assert ((dud - ref["du"]).abs() <= 4 * EPS * ref["du"].abs()).all(), f"{what}: du outside 4 eps |exact|"
        _assert_reduced(g_shift, ref["g_shift"], ref["g_shift_abs"], count, what + " g_shift")
        _assert_reduced(g_scale, ref["g_scale"], ref["g_scale_abs"], count, what + " g_scale_num")
        assert (g_mask is not None) == with_zy
        if with_zy:
            assert tuple(g_mask.shape) == (B, C)
            for b in range(B):
                _assert_reduced(g_mask[b], ref["g_mask"][b], ref["g_mask_abs"][b], ref["g_mask_n"][b], what + f" g_mask[{b}]")


@pytest.mark.gpu
def test_rows_act_bwd_in_place_and_without_count():
    """du may be dh itself (training.py does that); without m_count every row of m_cap counts"""
    from laudnet_amd import ops
    C = 40
    d = _inputs(C, M_CAP, True, True, 5)
    ref = _reference(d, M_CAP, True)
    dh, u, zy = _wide(d["dh"]), _wide(d["u"]), _wide(d["z"])
    pre = torch.tensor(d["pre"], dtype=torch.int32, device=DEV)
    du, g_shift, _, g_mask = ops.rows_act_bwd(dh, u, d["s"].to(DEV), d["t"].to(DEV), post_sub=d["c"].to(DEV), chan_mask=d["m"].to(DEV),
                                              row_prefix=pre, zy2d=zy, out=dh)
    torch.cuda.synchronize()
    assert du.data_ptr() == dh.data_ptr()
    assert ((du.double().cpu() - ref["du"]).abs() <= 4 * EPS * ref["du"].abs()).all()
    _assert_reduced(g_shift, ref["g_shift"], ref["g_shift_abs"], M_CAP, "in place g_shift")
    _assert_reduced(g_mask[2], ref["g_mask"][2], ref["g_mask_abs"][2], ref["g_mask_n"][2], "in place g_mask[2]")


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 197, M_CAP])
@pytest.mark.parametrize("C", [16, 40, 256, 264])
def test_rows_chanmask_vs_float64(C, count):
    from laudnet_amd import ops
    d = _inputs(C, count, True, False, 3 * C + count)
    src = _randn((M_CAP, C), 11 * C + count)
    u = _wide(src, count)
    pre = torch.tensor(d["pre"], dtype=torch.int32, device=DEV)
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    got = ops.rows_chanmask(u, pre, d["m"].to(DEV), m_count=cnt, m_cap=M_CAP)
    torch.cuda.synchronize()
    assert got.data_ptr() == u.data_ptr()
    exact = src[:count].double() * d["m"].double()[d["img"][:count]]
    g = got.double().cpu()
    assert torch.isfinite(g).all() and (g[count:] == 0).all(), "rows past the count must be exactly 0"
    assert ((g[:count] - exact).abs() <= 4 * EPS * exact.abs()).all()
    assert (g[:count][exact == 0] == 0).all(), "u must be exactly 0 on the masked channels"


@pytest.mark.gpu
def test_train_rows_argument_errors():
    from laudnet_amd import LdnError, ops
    u = torch.zeros(8, 16, device=DEV)
    v = torch.zeros(16, device=DEV)
    pre = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    with pytest.raises(LdnError):                                # chan_mask without the row prefix
        ops.rows_act_bwd(u, u, v, v, chan_mask=torch.ones(1, 16, device=DEV))
    with pytest.raises(LdnError):                                # C % 4
        ops.rows_act_bwd(u[:, :6], u[:, :6], v[:6], v[:6])
    with pytest.raises(LdnError):                                # m_cap past the matrix
        ops.rows_chanmask(u, pre, torch.ones(1, 16, device=DEV), m_cap=9)
    with pytest.raises(LdnError):                                # prefix / mask disagree
        ops.rows_chanmask(u, pre, torch.ones(2, 16, device=DEV))


def test_rows_act_bwd_split_plan_is_shape_only_cpu():
    """The workspace pins the plan the determinism cases rely on: m_cap = 300 splits four ways (>= 64 rows per workgroup), so 2 * 4 partial
    vectors for g_shift / g_scale_num plus 4 + B slots for g_mask; no B, no g_mask slots; one workgroup below 128 rows."""
    from laudnet_amd import _lib
    lib = _lib.load()
    assert lib.ldn_rows_act_bwd_workspace_bytes(M_CAP, 256, B) == (2 * 4 + 4 + B) * 256 * 4
    assert lib.ldn_rows_act_bwd_workspace_bytes(M_CAP, 256, 0) == 2 * 4 * 256 * 4
    assert lib.ldn_rows_act_bwd_workspace_bytes(100, 16, 0) == 2 * 16 * 4
    assert lib.ldn_rows_act_bwd_workspace_bytes(0, 16, 2) == (2 + 1 + 2) * 16 * 4
    assert lib.ldn_rows_act_bwd_workspace_bytes(300, 6, 0) == 0          # C % 4: no such launch
