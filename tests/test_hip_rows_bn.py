"""ops.rows_bn_stats / ops.rows_bn_fwd / ops.rows_bn_bwd (csrc/ldn_train_bn.hip: BatchNorm on batch statistics over packed rows, forward and
backward through the statistics, with the channel mask in front and the pixel-mask row factor behind) against the float64 restatement of
tests/bn_batch_ref.py.

Shapes (m_cap, count, C, B, ld): one workgroup; a count below the cap under one split; several row splits with a second 256-channel column tile
and a ragged last split (588 rows -> 9 splits of 66, the last of 60; C 320); zero rows; an odd row count at the narrowest tile (C 8: 128 row
lanes); a leading dimension larger than C.  Inputs: channel 0 constant (var == 0), channel 1 dropped by the channel mask in every image, channel 2
in image 0 only, channel 3 with |mean| = 1000 std; gamma[4] = 0, gamma[5] = 2^-24, gamma[6] = -1.  Rows past the count hold NaN (never read).

Bounds: every element of every output within 1e-3 of the tensor's own maximum (the project's bar, tests/test_hip_training_f64.py); mean, var and
invstd additionally within 1e-4 RELATIVE, element by element -- what the |mean| = 1000 std channel is for: test_bounds_tell_two_pass_from_naive_cpu
shows on these very inputs that a float32 two-pass restatement stays inside both and float32 E[u^2] - E[u]^2 does not.  Rows past the count are
exact zeros; two runs are torch.equal.  The ReLU gate of the backward is read from the stored forward output, so the reference gets the same h."""
import functools

import pytest
import torch

import bn_batch_ref as R

DEV = "cuda:0"
EPS = 1e-5
BOUND, REL = 1e-3, 1e-4
CASES = [(98, 98, 64, 2, 64), (98, 61, 64, 2, 64), (588, 588, 320, 3, 320), (588, 0, 64, 3, 64), (130, 129, 8, 2, 8), (98, 61, 64, 2, 72)]
IDS = [f"m{m}_n{n}_C{C}_B{B}_ld{ld}" for m, n, C, B, ld in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(m_cap, count, C, B, ld):
    g = torch.Generator().manual_seed(1000 * m_cap + 10 * count + C)
    u = torch.full((m_cap, ld), float("nan"))
    offs = 0.5 + 1.5 * torch.rand(C, generator=g)                     # per-channel means clear of zero: the relative bound on mean says something
    u[:count, :C] = torch.randn(count, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + offs
    u[:count, 0] = 3.25                                               # var == 0
    u[:count, 3] = 1000.0 + torch.randn(count, generator=g)          # |mean| = 1000 std
    cuts = torch.linspace(0, count, B + 1).long()
    cuts[1:-1] = (cuts[1:-1] * 0.8).long()                            # uneven images
    img = torch.bucketize(torch.arange(count), cuts[1:], right=True).clamp(max=B - 1)
    cm = (torch.rand(B, C, generator=g) < 0.7).float()
    cm[:, 0], cm[:, 1], cm[:, 2], cm[:, 3] = 1.0, 0.0, 1.0, 1.0
    cm[0, 2] = 0.0                                                    # dropped in one image only
    gamma = torch.randn(C, generator=g)
    gamma[4], gamma[5], gamma[6] = 0.0, 2.0 ** -24, -1.0
    beta = torch.randn(C, generator=g)
    rs = torch.full((m_cap,), float("nan"))
    rs[:count] = (torch.rand(count, generator=g) < 0.6).float()
    dh = torch.full((m_cap, ld), float("nan"))
    dh[:count, :C] = torch.randn(count, C, generator=g)
    return dict(u=u, prefix=cuts.int(), img=img, cm=cm, gamma=gamma, beta=beta, rs=rs, dh=dh)


def _within(got, want, what, rel=None):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got - want).abs()
    print(f"{what}: max |err| {err.max().item() if err.numel() else 0.0:.3e}, max |want| {want.abs().max().item() if want.numel() else 0.0:.3e}")
    if err.numel():
        assert err.max().item() <= BOUND * want.abs().max().item(), f"{what}: {err.max().item():.3e} exceeds 1e-3 of max |want| {want.abs().max().item():.3e}"
        if rel is not None:
            bad = err > rel * want.abs()
            assert not bool(bad.any()), f"{what}: relative error {(err / want.abs().clamp(min=1e-300))[bad].max().item():.3e} at channels {bad.nonzero().flatten().tolist()}"


def test_bounds_tell_two_pass_from_naive_cpu():
    """On the inputs of the GPU cases: a float32 two-pass variance (mean, then the mean of squared differences) is inside both bounds, and
    float32 E[u^2] - E[u]^2 is outside the relative one at the |mean| = 1000 std channel -- so the bounds can tell the two."""
    told = 0
    for m_cap, count, C, B, ld in CASES:
        if count == 0:
            continue
        d = _inputs(m_cap, count, C, B, ld)
        u, cmr = d["u"][:count, :C], d["cm"][d["img"]]
        for x in (u, u * cmr):
            want = x.double().var(0, unbiased=False)
            mean32 = x.mean(0)
            two_pass = ((x - mean32) ** 2).mean(0)
            naive = (x * x).mean(0) - mean32 * mean32
            e2, en = (two_pass.double() - want).abs(), (naive.double() - want).abs()
            assert bool((e2 <= REL * want).all()) and e2.max() <= BOUND * want.max(), (m_cap, count, C)
            assert bool((mean32.double() - x.double().mean(0)).abs().le(REL * x.double().mean(0).abs()).all())
            assert en[3] > REL * want[3], f"E[u^2] - E[u]^2 in float32 passes at the large-mean channel: {en[3].item():.3e} vs var {want[3].item():.3e}"
            told += 1
    assert told >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "chanmask"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_bn_vs_float64(case, masked):
    from laudnet_amd import ops
    m_cap, count, C, B, ld = case
    d = _inputs(*case)
    u = d["u"].to(DEV)[:, :C]
    dh = d["dh"].to(DEV)[:, :C]
    assert u.stride(0) == ld
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    cm, pre = (d["cm"].to(DEV), d["prefix"].to(DEV)) if masked else (None, None)
    gamma, beta, rs = d["gamma"].to(DEV), d["beta"].to(DEV), d["rs"].to(DEV)
    u64, dh64 = d["u"][:count, :C].double(), d["dh"][:count, :C].double()
    cm64, img = (d["cm"].double(), d["img"]) if masked else (None, None)
    g64, b64 = d["gamma"].double(), d["beta"].double()

    runs = []
    for _ in range(2):
        mean, var, inv = ops.rows_bn_stats(u, EPS, chan_mask=cm, row_prefix=pre, m_count=cnt, m_cap=m_cap)
        h = ops.rows_bn_fwd(u, mean, inv, gamma, beta, chan_mask=cm, row_prefix=pre, m_count=cnt, m_cap=m_cap)                     # layers 1 / 2
        z = ops.rows_bn_fwd(u, mean, inv, gamma, beta, chan_mask=cm, row_prefix=pre, row_scale=rs, relu=False, m_count=cnt, m_cap=m_cap)     # layer 3
        out = torch.full((m_cap, ld), float("nan"), device=DEV)[:, :C]
        du, dg, db, gm = ops.rows_bn_bwd(dh, u, h, mean, inv, gamma, chan_mask=cm, row_prefix=pre, want_mask=masked, m_count=cnt, m_cap=m_cap, out=out)
        du3, dg3, db3, _ = ops.rows_bn_bwd(dh, u, None, mean, inv, gamma, chan_mask=cm, row_prefix=pre, row_scale=rs, m_count=cnt, m_cap=m_cap)
        torch.cuda.synchronize()
        runs.append((mean, var, inv, h, z, du, dg, db, du3, dg3, db3) + ((gm,) if masked else ()))
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), f"output {i} differs between two runs"
    for t, name in ((h, "h"), (z, "z"), (du, "du"), (du3, "du3")):
        assert t.shape == (m_cap, C) and bool((t[count:] == 0).all()), f"{name}: rows past the count must be exact zeros"

    tag = f"{IDS[CASES.index(case)]} {'chanmask' if masked else 'plain'}"
    wmean, wvar, winv = R.bn_stats(u64, EPS, cm64, img)
    _within(mean, wmean, f"{tag} mean", REL)
    _within(var, wvar, f"{tag} var", REL)
    _within(inv, winv, f"{tag} invstd", REL)
    rs64 = d["rs"][:count].double()
    _within(h[:count], R.bn_fwd(u64, wmean, winv, g64, b64, cm64, img), f"{tag} h")
    _within(z[:count], R.bn_fwd(u64, wmean, winv, g64, b64, cm64, img, rs64, relu=False), f"{tag} z")
    h_stored = h[:count].double().cpu()                       # the gate is the stored forward output's
    wdu, wdg, wdb, wgm = R.bn_bwd(dh64, u64, h_stored, wmean, winv, g64, cm64, img, B=B if masked else None)
    _within(du[:count], wdu, f"{tag} du")
    _within(dg, wdg, f"{tag} d_gamma")
    _within(db, wdb, f"{tag} d_beta")
    if masked:
        _within(gm, wgm, f"{tag} g_mask")
    wdu3, wdg3, wdb3, _ = R.bn_bwd(dh64, u64, None, wmean, winv, g64, cm64, img, rs64)
    _within(du3[:count], wdu3, f"{tag} du (row factor, no ReLU)")
    _within(dg3, wdg3, f"{tag} d_gamma (row factor, no ReLU)")
    _within(db3, wdb3, f"{tag} d_beta (row factor, no ReLU)")
    if count:
        assert wdg3[4].abs() > 0 and (du[:count, 4] == 0).all() and (du3[:count, 4] == 0).all(), "gamma == 0: du vanishes, d_gamma does not"
        assert wvar[0] == 0 and var[0] == 0, "the constant channel's variance is exactly 0"


@pytest.mark.gpu
def test_rows_bn_in_place_and_without_count():
    """du written over dh; no count tensor = every row"""
    from laudnet_amd import ops
    case = CASES[2]
    m_cap, _, C, B, _ = case
    d = _inputs(*case)
    u, dh = d["u"].to(DEV), d["dh"].to(DEV)
    cm, pre = d["cm"].to(DEV), d["prefix"].to(DEV)
    gamma, beta = d["gamma"].to(DEV), d["beta"].to(DEV)
    mean, var, inv = ops.rows_bn_stats(u, EPS, chan_mask=cm, row_prefix=pre)
    h = ops.rows_bn_fwd(u, mean, inv, gamma, beta, chan_mask=cm, row_prefix=pre)
    want = ops.rows_bn_bwd(dh, u, h, mean, inv, gamma, chan_mask=cm, row_prefix=pre, want_mask=True)
    buf = dh.clone()
    got = ops.rows_bn_bwd(buf, u, h, mean, inv, gamma, chan_mask=cm, row_prefix=pre, want_mask=True, out=buf)
    assert got[0].data_ptr() == buf.data_ptr()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_rows_bn_argument_errors():
    from laudnet_amd import LdnError, ops
    u = torch.zeros(8, 16, device=DEV)
    v = torch.ones(16, device=DEV)
    pre = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    one = torch.ones(1, 16, device=DEV)
    with pytest.raises(LdnError):
        ops.rows_bn_stats(u, EPS, chan_mask=one)                           # a channel mask without the prefix
    with pytest.raises(LdnError):
        ops.rows_bn_stats(u[:, :6], EPS)                                   # C % 4
    with pytest.raises(LdnError):
        ops.rows_bn_fwd(u, v, v, v, v, chan_mask=torch.ones(2, 16, device=DEV), row_prefix=pre)
    with pytest.raises(LdnError):
        ops.rows_bn_fwd(u, v, v, v, v, m_cap=9)
    with pytest.raises(LdnError):
        ops.rows_bn_bwd(u, u, None, v, v, v, want_mask=True)               # g_mask without the prefix
    with pytest.raises(LdnError):
        ops.rows_bn_bwd(u, u, u[:, :8], v, v, v)


def test_rows_bn_split_plan_is_shape_only_cpu():
    """the workspace sizes are functions of (m_cap, C, B): 588 rows split nine ways at every width"""
    from laudnet_amd import _lib
    lib = _lib.load()
    for C in (8, 64, 320):
        assert lib.ldn_rows_bn_stats_workspace_bytes(588, C) == 2 * 9 * C * 4
        assert lib.ldn_rows_bn_bwd_workspace_bytes(588, C, 3) == (2 * 9 + 9 + 3) * C * 4
        assert lib.ldn_rows_bn_bwd_workspace_bytes(588, C, 0) == 2 * 9 * C * 4
        assert lib.ldn_rows_bn_bwd_workspace_bytes(588, C, 3) == lib.ldn_rows_act_bwd_workspace_bytes(588, C, 3)
    assert lib.ldn_rows_bn_stats_workspace_bytes(98, 64) == 2 * 64 * 4          # one workgroup below 128 rows
    assert lib.ldn_rows_bn_stats_workspace_bytes(300, 6) == 0 and lib.ldn_rows_bn_bwd_workspace_bytes(300, 6, 0) == 0      # C % 4: no such launch
