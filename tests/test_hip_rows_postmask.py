"""ops.rows_postmask_bwd / ops.rows_img_dot (csrc/ldn_train_rows.hip: the backward of a channel mask applied AFTER the ReLU, and the per-image
dot product of the squeeze-excitation backward) against a float64 CPU reference written here.  Plain fp32 VALU code: one arithmetic, no math_mode.

Inputs: r = relu(z) in fp32 with |z| >= 0.05 -- the UNMASKED activation, as the forward stores it.  B = 3 images, the middle one holds ZERO rows;
counts 0, 1, 197 and m_cap; C = 8, 48 and 264 (two column tiles, the last of 2 quads); every matrix has a leading dimension C + 8; rows >= count of
dz and r are NaN (they must not be read).

Bounds (derived, not measured; eps = 2^-24; `exact` = the float64 evaluation of include/ldn_hip.h's formulas on the fp32 inputs):
  elementwise du:  |got - exact| <= 4 eps |exact| -- du = (dh * m) * s is two roundings; with the SE prologue 6 eps (dh = dz * gate + dsq adds
      two more; the kernel forms it as ONE fused multiply-add, which is inside that).
  reduced (g_shift, g_scale_num, g_mask, rows_img_dot):  |got - exact| <= (n + 4) eps sum|terms|, n = the number of rows summed -- a term carries
      at most four roundings (dh; dh * m; r - t; the product), a sum of n terms in ANY order at most n - 1 more.  n == 0: exactly 0.
Determinism: every case runs twice, all outputs bit-identical -- with m_cap = 300 the rows are split four ways (75 rows per workgroup, pinned by
the CPU test below), so for counts 197 and 300 both non-empty images straddle a split and their per-image sums are sums of partials."""
import pytest
import torch

DEV = "cuda:0"
EPS = 2.0 ** -24
M_CAP = 300
B = 3
COUNTS = [0, 1, 197, M_CAP]
WIDTHS = [8, 48, 264]


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


def _inputs(C, count, seed):
    pre = _prefix(count)
    img = torch.zeros(M_CAP, dtype=torch.long)
    img[pre[2]:] = 2
    z = _randn((M_CAP, C), seed)
    z = torch.sign(z) * (0.05 + z.abs())
    z[z == 0] = 0.05
    s = (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 1))) * torch.sign(_randn((C,), seed + 2))
    s[s == 0] = 1.0
    t = 0.5 * _randn((C,), seed + 3)
    m = (torch.rand(B, C, generator=torch.Generator().manual_seed(seed + 4)) < 0.6).float()
    gate = torch.sigmoid(_randn((B, C), seed + 6))
    dsq = 0.1 * _randn((B, C), seed + 7)
    return dict(pre=pre, img=img, r=torch.relu(z), s=s, t=t, m=m, gate=gate, dsq=dsq, dz=_randn((M_CAP, C), seed + 5))


def _reference(d, count, with_mask, with_se):
    """float64 evaluation of include/ldn_hip.h's formulas on the fp32 inputs -> values and the sum|terms| of every reduced output"""
    r, dz = d["r"][:count].double(), d["dz"][:count].double()
    s, t = d["s"].double(), d["t"].double()
    img = d["img"][:count]
    m = d["m"].double()[img] if with_mask else torch.ones_like(r)
    dh = dz * d["gate"].double()[img] + d["dsq"].double()[img] if with_se else dz
    a = torch.where(r > 0, dh * m, torch.zeros_like(dh))
    term = dh * r
    per = lambda x: torch.stack([x[img == b].sum(0) for b in range(B)])
    return dict(du=a * s, g_shift=a.sum(0), g_shift_abs=a.abs().sum(0), g_scale=(a * (r - t)).sum(0), g_scale_abs=(a * (r - t)).abs().sum(0),
                g_mask=per(term), g_mask_abs=per(term.abs()), n=[int((img == b).sum()) for b in range(B)])


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


# (chan_mask, SE prologue, g_mask) each absent and present
VARIANTS = [(True, True, True), (False, False, False), (True, False, True), (False, True, False), (True, True, False), (False, False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("C", WIDTHS)
def test_rows_postmask_bwd_vs_float64(C, count):
    from laudnet_amd import ops
    for vi, (with_mask, with_se, with_gm) in enumerate(VARIANTS):
        what = f"C {C} count {count} mask {with_mask} prologue {with_se} g_mask {with_gm}"
        d = _inputs(C, count, 100 * C + 7 * count + vi)
        ref = _reference(d, count, with_mask, with_se)
        dz, r = _wide(d["dz"], count), _wide(d["r"], count)
        pre = torch.tensor(d["pre"], dtype=torch.int32, device=DEV)
        cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
        kw = dict(chan_mask=d["m"].to(DEV) if with_mask else None, row_prefix=pre if (with_mask or with_se or with_gm) else None,
                  gate=d["gate"].to(DEV) if with_se else None, dsq=d["dsq"].to(DEV) if with_se else None, want_mask=with_gm, m_count=cnt, m_cap=M_CAP)
        runs = []
        for _ in range(2):
            out = torch.full((M_CAP, C + 8), float("nan"), device=DEV)[:, :C]
            du, g_shift, g_scale, g_mask = ops.rows_postmask_bwd(dz, r, d["s"].to(DEV), d["t"].to(DEV), out=out, **kw)
            torch.cuda.synchronize()
            runs.append((du.clone(), g_shift, g_scale, g_mask))
        for x, y in zip(*runs):
            assert (x is None and y is None) or torch.equal(x, y), f"{what}: two runs differ"
        du, g_shift, g_scale, g_mask = runs[0]
        assert torch.isfinite(du).all() and (du[count:] == 0).all(), f"{what}: du must be exactly 0 on the rows past the count"
        dud = du[:count].double().cpu()
        k = 6 if with_se else 4
        worst = ((dud - ref["du"]).abs() / (EPS * ref["du"].abs()).clamp(min=1e-300)).max().item() if count else 0.0
        print(f"{what}: du worst |err| / (eps |exact|) = {worst:.3f} (bound {k})")
        assert ((dud - ref["du"]).abs() <= k * EPS * ref["du"].abs()).all(), f"{what}: du outside {k} eps |exact|"
        _assert_reduced(g_shift, ref["g_shift"], ref["g_shift_abs"], count, what + " g_shift")
        _assert_reduced(g_scale, ref["g_scale"], ref["g_scale_abs"], count, what + " g_scale_num")
        assert (g_mask is not None) == with_gm
        if with_gm:
            assert tuple(g_mask.shape) == (B, C)
            for b in range(B):
                _assert_reduced(g_mask[b], ref["g_mask"][b], ref["g_mask_abs"][b], ref["n"][b], what + f" g_mask[{b}]")


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("C", WIDTHS)
def test_rows_img_dot_vs_float64(C, count):
    from laudnet_amd import ops
    d = _inputs(C, count, 13 * C + count)
    a, b = _wide(d["dz"], count), _wide(d["r"], count)
    pre = torch.tensor(d["pre"], dtype=torch.int32, device=DEV)
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    runs = []
    for _ in range(2):
        runs.append(ops.rows_img_dot(a, b, pre, m_count=cnt, m_cap=M_CAP))
        torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]), "two runs differ"
    assert tuple(runs[0].shape) == (B, C)
    term = d["dz"][:count].double() * d["r"][:count].double()
    img = d["img"][:count]
    for i in range(B):
        sel = term[img == i]
        _assert_reduced(runs[0][i], sel.sum(0), sel.abs().sum(0), sel.shape[0], f"C {C} count {count} rows_img_dot[{i}]")


@pytest.mark.gpu
def test_rows_postmask_bwd_in_place_and_without_count():
    """du may be dz itself (training.py does that); without m_count every row of m_cap counts"""
    from laudnet_amd import ops
    C = 48
    d = _inputs(C, M_CAP, 5)
    ref = _reference(d, M_CAP, True, True)
    dz, r = _wide(d["dz"]), _wide(d["r"])
    pre = torch.tensor(d["pre"], dtype=torch.int32, device=DEV)
    du, g_shift, g_scale, g_mask = ops.rows_postmask_bwd(dz, r, d["s"].to(DEV), d["t"].to(DEV), chan_mask=d["m"].to(DEV), row_prefix=pre,
                                                         gate=d["gate"].to(DEV), dsq=d["dsq"].to(DEV), want_mask=True, out=dz)
    torch.cuda.synchronize()
    assert du.data_ptr() == dz.data_ptr()
    assert ((du.double().cpu() - ref["du"]).abs() <= 6 * EPS * ref["du"].abs()).all()
    _assert_reduced(g_shift, ref["g_shift"], ref["g_shift_abs"], M_CAP, "in place g_shift")
    _assert_reduced(g_scale, ref["g_scale"], ref["g_scale_abs"], M_CAP, "in place g_scale_num")
    for b in range(B):
        _assert_reduced(g_mask[b], ref["g_mask"][b], ref["g_mask_abs"][b], ref["n"][b], f"in place g_mask[{b}]")
    # the masked channels carry the straight-through term and nothing else
    off = d["m"][2] == 0
    assert (du.cpu()[d["pre"][2]:][:, off] == 0).all() and g_mask.cpu()[2][off].abs().max().item() > 0


@pytest.mark.gpu
def test_rows_postmask_argument_errors():
    from laudnet_amd import LdnError, ops
    u = torch.zeros(8, 16, device=DEV)
    v = torch.zeros(16, device=DEV)
    pre = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    one = torch.ones(1, 16, device=DEV)
    with pytest.raises(LdnError):                                # chan_mask without the row prefix
        ops.rows_postmask_bwd(u, u, v, v, chan_mask=one)
    with pytest.raises(LdnError):                                # g_mask without the row prefix
        ops.rows_postmask_bwd(u, u, v, v, want_mask=True)
    with pytest.raises(LdnError):                                # half a prologue
        ops.rows_postmask_bwd(u, u, v, v, row_prefix=pre, gate=one)
    with pytest.raises(LdnError):                                # C % 4
        ops.rows_postmask_bwd(u[:, :6], u[:, :6], v[:6], v[:6])
    with pytest.raises(LdnError):                                # prefix / mask disagree
        ops.rows_postmask_bwd(u, u, v, v, chan_mask=torch.ones(2, 16, device=DEV), row_prefix=pre)
    with pytest.raises(LdnError):                                # m_cap past the matrix
        ops.rows_img_dot(u, u, pre, m_cap=9)
    with pytest.raises(LdnError):                                # widths disagree
        ops.rows_img_dot(u, u[:, :8], pre)


def test_rows_postmask_split_plan_is_shape_only_cpu():
    """The workspaces pin the plan the determinism cases rely on (that of ldn_rows_act_bwd): m_cap = 300 splits four ways (>= 64 rows per
    workgroup) at every width, so 2 * 4 partial vectors for g_shift / g_scale_num plus 4 + B slots for g_mask, and 4 + B slots for rows_img_dot."""
    from laudnet_amd import _lib
    lib = _lib.load()
    for C in WIDTHS:
        assert lib.ldn_rows_postmask_bwd_workspace_bytes(M_CAP, C, B) == (2 * 4 + 4 + B) * C * 4
        assert lib.ldn_rows_postmask_bwd_workspace_bytes(M_CAP, C, 0) == 2 * 4 * C * 4
        assert lib.ldn_rows_img_dot_workspace_bytes(M_CAP, C, B) == (4 + B) * C * 4
        assert lib.ldn_rows_postmask_bwd_workspace_bytes(M_CAP, C, B) == lib.ldn_rows_act_bwd_workspace_bytes(M_CAP, C, B)
    assert lib.ldn_rows_postmask_bwd_workspace_bytes(100, 16, 0) == 2 * 16 * 4       # one workgroup below 128 rows
    assert lib.ldn_rows_img_dot_workspace_bytes(0, 16, 2) == (1 + 2) * 16 * 4
    assert lib.ldn_rows_postmask_bwd_workspace_bytes(300, 6, 0) == 0                 # C % 4: no such launch
    assert lib.ldn_rows_img_dot_workspace_bytes(300, 6, 1) == 0
