"""ops.rows_bn_postmask_fwd / ops.rows_bn_postmask_bwd (csrc/ldn_train_bn.hip: BatchNorm on batch statistics over packed rows with the channel
mask AFTER the ReLU -- LAD-RegNet channel mode -- forward, and backward through the statistics with the optional squeeze-excitation prologue)
against the float64 restatement of tests/regnet_bn_ref.py.  The statistics come from ops.rows_bn_stats without a mask: in this form every channel
of every image feeds them.

Shapes and inputs: the six (m_cap, count, C, B, ld) and the input scheme of tests/test_hip_rows_bn.py -- one workgroup; a count below the cap;
588 rows -> 9 ragged splits with a second column tile at C 320; zero rows; 129 rows at C 8; ld 72 > C 64.  Channel 0 constant (var == 0), channel 1
dropped in every image, channel 2 in image 0 only, channel 3 with |mean| = 1000 std; gamma[4] = 0, gamma[5] = 2^-24, gamma[6] = -1; NaN past the
count; beta[1] = 0.75 and beta[4] = 0.5, so that the ReLUs of the dropped channel and of the gamma == 0 channel are on and g_mask / d_gamma have
something to show there (_beta).  Variants: no mask; a mask without and with g_mask; with the SE prologue (gate, dsq [B, C]) behind a mask and without one.

Bounds: every element of every output within 1e-3 of the tensor's own maximum (the project's bar).  Rows past the count are exact zeros; two
runs are torch.equal.  The ReLU gate of the backward is read from the stored forward output, so the reference gets the GPU's h."""
import ctypes
import functools

import pytest
import torch

import regnet_bn_ref as R
from test_hip_rows_bn import CASES, IDS, _inputs

DEV = "cuda:0"
EPS = 1e-5
BOUND = 1e-3
# name -> (channel mask, g_mask, SE prologue)
VARIANTS = {"plain": (False, False, False), "mask": (True, False, False), "mask_gmask": (True, True, False), "mask_gmask_se": (True, True, True),
            "gmask_se": (False, True, True)}


@functools.lru_cache(maxsize=None)
def _prologue(B, C):
    g = torch.Generator().manual_seed(77 + 10 * B + C)
    return torch.rand(B, C, generator=g), 0.1 * torch.randn(B, C, generator=g)


def _beta(d):
    """that scheme's beta with the ReLU of channel 1 -- the one the mask drops in every image -- switched on (beta[1] is -1.73 against gamma[1] 0.26
    in the first case: a dead ReLU, and g_mask = sum dh . relu(..) would be zero there whatever the kernel does) -- and that of channel 4 likewise:
    at gamma[4] == 0 the pre-activation IS beta[4], and d_gamma[4] != 0 can only be seen where it is positive"""
    beta = d["beta"].clone()
    beta[1], beta[4] = 0.75, 0.5
    return beta


def _within(got, want, what):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got - want).abs()
    print(f"{what}: max |err| {err.max().item() if err.numel() else 0.0:.3e}, max |want| {want.abs().max().item() if want.numel() else 0.0:.3e}")
    if err.numel():
        assert err.max().item() <= BOUND * want.abs().max().item(), f"{what}: {err.max().item():.3e} exceeds 1e-3 of max |want| {want.abs().max().item():.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_bn_postmask_vs_float64(case, variant):
    from laudnet_amd import ops
    m_cap, count, C, B, ld = case
    masked, want_mask, se = VARIANTS[variant]
    d = _inputs(*case)
    u = d["u"].to(DEV)[:, :C]
    dz = d["dh"].to(DEV)[:, :C]
    assert u.stride(0) == ld
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    pre = d["prefix"].to(DEV) if (masked or want_mask or se) else None
    cm = d["cm"].to(DEV) if masked else None
    gate, dsq = (t.to(DEV) for t in _prologue(B, C)) if se else (None, None)
    gamma, beta = d["gamma"].to(DEV), _beta(d).to(DEV)
    u64, dz64 = d["u"][:count, :C].double(), d["dh"][:count, :C].double()
    img = d["img"]
    cm64 = d["cm"].double() if masked else None
    gate64, dsq64 = (t.double() for t in _prologue(B, C)) if se else (None, None)
    g64, b64 = d["gamma"].double(), _beta(d).double()

    runs = []
    for _ in range(2):
        mean, var, inv = ops.rows_bn_stats(u, EPS, m_count=cnt, m_cap=m_cap)
        h = ops.rows_bn_postmask_fwd(u, mean, inv, gamma, beta, chan_mask=cm, row_prefix=pre, m_count=cnt, m_cap=m_cap)
        out = torch.full((m_cap, ld), float("nan"), device=DEV)[:, :C]
        du, dg, db, gm = ops.rows_bn_postmask_bwd(dz, u, h, mean, inv, gamma, beta, chan_mask=cm, row_prefix=pre, gate=gate, dsq=dsq,
                                                  want_mask=want_mask, m_count=cnt, m_cap=m_cap, out=out)
        torch.cuda.synchronize()
        assert (gm is not None) == want_mask
        runs.append((mean, var, inv, h, du, dg, db) + ((gm,) if want_mask else ()))
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), f"output {i} differs between two runs"
    for t, name in ((h, "h"), (du, "du")):
        assert t.shape == (m_cap, C) and bool((t[count:] == 0).all()), f"{name}: rows past the count must be exact zeros"

    tag = f"{IDS[CASES.index(case)]} {variant}"
    wmean, wvar, winv = R.bn_stats(u64, EPS)
    _within(mean, wmean, f"{tag} mean")
    _within(var, wvar, f"{tag} var")
    _within(h[:count], R.bn_postmask_fwd(u64, wmean, winv, g64, b64, cm64, img), f"{tag} h")
    h_stored = h[:count].double().cpu()                       # the gate is the stored forward output's
    wdu, wdg, wdb, wgm = R.bn_postmask_bwd(dz64, u64, h_stored, wmean, winv, g64, b64, cm64, img, gate64, dsq64, B=B if want_mask else None)
    _within(du[:count], wdu, f"{tag} du")
    _within(dg, wdg, f"{tag} d_gamma")
    _within(db, wdb, f"{tag} d_beta")
    if want_mask:
        _within(gm, wgm, f"{tag} g_mask")
    if count:
        assert wdg[4].abs() > 0 and dg[4].abs() > 0 and bool((du[:count, 4] == 0).all()), "gamma == 0: du vanishes, d_gamma does not"
        if masked:
            assert bool((h[:count, 1] == 0).all()) and dg[1] == 0 and db[1] == 0, "a channel dropped in every image: h, d_gamma and d_beta are zero"
            if want_mask:
                assert bool((gm[:, 1] != 0).all()) and bool((wgm[:, 1] != 0).all()), "g_mask lives on the channel dropped in every image"


@pytest.mark.gpu
def test_rows_bn_postmask_in_place_and_without_count():
    """du written over dz, h over u; no count tensor = every row"""
    from laudnet_amd import ops
    case = CASES[2]
    m_cap, _, C, B, _ = case
    d = _inputs(*case)
    u, dz = d["u"].to(DEV), d["dh"].to(DEV)
    cm, pre = d["cm"].to(DEV), d["prefix"].to(DEV)
    gate, dsq = (t.to(DEV) for t in _prologue(B, C))
    gamma, beta = d["gamma"].to(DEV), _beta(d).to(DEV)
    mean, var, inv = ops.rows_bn_stats(u, EPS)
    h = ops.rows_bn_postmask_fwd(u, mean, inv, gamma, beta, chan_mask=cm, row_prefix=pre)
    ubuf = u.clone()
    h2 = ops.rows_bn_postmask_fwd(ubuf, mean, inv, gamma, beta, chan_mask=cm, row_prefix=pre, out=ubuf)
    assert h2.data_ptr() == ubuf.data_ptr() and torch.equal(h2, h)
    kw = dict(chan_mask=cm, row_prefix=pre, gate=gate, dsq=dsq, want_mask=True)
    want = ops.rows_bn_postmask_bwd(dz, u, h, mean, inv, gamma, beta, **kw)
    buf = dz.clone()
    got = ops.rows_bn_postmask_bwd(buf, u, h, mean, inv, gamma, beta, out=buf, **kw)
    assert got[0].data_ptr() == buf.data_ptr()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # the same numbers against float64 with every row live
    u64, dz64, img = d["u"].double(), d["dh"].double(), d["img"]
    wmean, _, winv = R.bn_stats(u64, EPS)
    wdu, wdg, wdb, wgm = R.bn_postmask_bwd(dz64, u64, h.double().cpu(), wmean, winv, d["gamma"].double(), _beta(d).double(), d["cm"].double(), img,
                                           *(t.double() for t in _prologue(B, C)), B=B)
    for a, b, name in zip(want, (wdu, wdg, wdb, wgm), ("du", "d_gamma", "d_beta", "g_mask")):
        _within(a, b, f"no count tensor: {name}")


@pytest.mark.gpu
def test_rows_bn_postmask_wrapper_argument_errors():
    from laudnet_amd import LdnError, ops
    u = torch.zeros(8, 16, device=DEV)
    v = torch.ones(16, device=DEV)
    pre = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    one = torch.ones(1, 16, device=DEV)
    with pytest.raises(LdnError):
        ops.rows_bn_postmask_fwd(u, v, v, v, v, chan_mask=one)                                  # a channel mask without the prefix
    with pytest.raises(LdnError):
        ops.rows_bn_postmask_fwd(u, v, v, v, v, chan_mask=torch.ones(2, 16, device=DEV), row_prefix=pre)
    with pytest.raises(LdnError):
        ops.rows_bn_postmask_fwd(u, v, v, v, v, m_cap=9)
    with pytest.raises(LdnError):
        ops.rows_bn_postmask_bwd(u, u, u, v, v, v, v, want_mask=True)                           # g_mask without the prefix
    with pytest.raises(LdnError):
        ops.rows_bn_postmask_bwd(u, u, u, v, v, v, v, gate=one, row_prefix=pre)                 # gate without dsq
    with pytest.raises(LdnError):
        ops.rows_bn_postmask_bwd(u, u, None, v, v, v, v)                                        # the stored h is required
    with pytest.raises(LdnError):
        ops.rows_bn_postmask_bwd(u, u, u[:, :8], v, v, v, v)


def test_rows_bn_postmask_library_argument_errors_cpu():
    """NULL pointers, a bad leading dimension, a mask without the prefix and gate without dsq are LDN_EINVAL before any launch (no device needed)"""
    from laudnet_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)        # non-NULL, 16-byte aligned, never followed: every call below is refused first
    fwd = lambda **k: lib.ldn_rows_bn_postmask_fwd(k.get("u", p), k.get("ldu", 16), p, p, p, p, k.get("cm"), k.get("pre"), k.get("B", 0), None, 8,
                                                   k.get("C", 16), k.get("h", p), k.get("ldh", 16), None)
    assert fwd(u=None) == -1 and b"null" in lib.ldn_last_error()
    assert fwd(h=None) == -1
    assert fwd(ldu=12) == -1 and fwd(ldh=18) == -1 and fwd(C=6) == -1
    assert fwd(cm=p) == -1 and b"row_prefix" in lib.ldn_last_error()
    assert fwd(cm=p, pre=p, B=0) == -1
    assert fwd(u=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.ldn_last_error()

    def bwd(**k):
        return lib.ldn_rows_bn_postmask_bwd(k.get("dz", p), k.get("lddz", 16), p, k.get("ldu", 16), k.get("h", p), k.get("ldh", 16), p, p, p,
                                            k.get("beta", p), k.get("cm"), k.get("pre"), k.get("B", 0), k.get("gate"), k.get("dsq"), None, 8,
                                            k.get("C", 16), p, k.get("lddu", 16), p, p, k.get("gm"), k.get("work", p), None)
    assert bwd(dz=None) == -1 and b"null" in lib.ldn_last_error()
    assert bwd(h=None) == -1 and bwd(beta=None) == -1 and bwd(work=None) == -1
    assert bwd(lddz=12) == -1 and bwd(ldu=18) == -1 and bwd(ldh=8) == -1 and bwd(lddu=17) == -1 and bwd(C=10) == -1
    assert bwd(cm=p) == -1 and b"row_prefix" in lib.ldn_last_error()
    assert bwd(gm=p) == -1 and bwd(gm=p, pre=p, B=0) == -1
    assert bwd(gate=p, pre=p, B=1) == -1 and b"both or neither" in lib.ldn_last_error()
    assert bwd(dsq=p, pre=p, B=1) == -1
    assert bwd(gate=p, dsq=p) == -1 and b"row_prefix" in lib.ldn_last_error()


def test_rows_bn_postmask_split_plan_is_shape_only_cpu():
    """the workspace is the layout of rows_act_bwd: two column vectors per split, and splits + B image slots where g_mask is wanted"""
    from laudnet_amd import _lib
    lib = _lib.load()
    for C in (8, 64, 320):
        assert lib.ldn_rows_bn_postmask_bwd_workspace_bytes(588, C, 3) == (2 * 9 + 9 + 3) * C * 4
        assert lib.ldn_rows_bn_postmask_bwd_workspace_bytes(588, C, 0) == 2 * 9 * C * 4
        assert lib.ldn_rows_bn_postmask_bwd_workspace_bytes(588, C, 3) == lib.ldn_rows_postmask_bwd_workspace_bytes(588, C, 3)
    assert lib.ldn_rows_bn_postmask_bwd_workspace_bytes(98, 64, 0) == 2 * 64 * 4
    assert lib.ldn_rows_bn_postmask_bwd_workspace_bytes(300, 6, 0) == 0
