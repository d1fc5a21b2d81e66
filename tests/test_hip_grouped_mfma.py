"""GPU tests of the matrix-core grouped 3x3 for group widths 8 and 24 (ops.grouped_mfma_conv3x3_rows -> ldn_grouped_mfma_conv3x3_rows,
bf16x3) against F.conv2d(groups = C / gw) in float64 at the kept pixels, bound 1e-4 max(1, |want|max): the bound of the width-16 matrix-core
kernel (tests/test_hip_ops.py::test_grouped16_conv3x3_rows_mfma_vs_torch).  Odd group counts (13, 55, 5, 37), more groups than one
workgroup's chunk, ragged last row tiles, one row, a device-side count of zero; row strides wider than C with sentinels in the pads; NaN in
the input rows past the dilated list; zero and negative scales; with and without ReLU; twice, bit for bit.  Then the dispatch: with
laud_regnet.USE_GROUPED_MFMA_WIDTHS on, the layer-skip and spatial cases of regnet_tiny.pt (group width 8) pass the comparison of
tests/test_hip_blocks.py on the new kernel; with it off the kernel is never called."""
import functools

import pytest
import torch
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn
from helpers import assert_tuple_close, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0

# (gw, B, Ho, stride, C, keep)
CASES = [(8, 1, 5, 1, 8, 1.0),        # one group, 25 rows
         (8, 2, 7, 2, 24, 0.6),       # 3 groups
         (8, 3, 14, 1, 104, 0.5),     # 13 groups
         (8, 2, 9, 2, 440, 0.4),      # 55 groups, past one chunk
         (24, 1, 5, 1, 24, 1.0),
         (24, 2, 7, 2, 48, 0.6),
         (24, 3, 14, 1, 120, 0.5),    # 5 groups
         (24, 2, 9, 2, 888, 0.4),     # 37 groups, past one chunk
         # With few row tiles the launch gives every workgroup ONE group (csrc/ldn_grouped_gw.hip: launch_grouped_gw).  A wave walks SEVERAL
         # groups, its loads running across the group boundary, only once the row tiles alone fill the device: 1250 / 1563 tiles here
         # -> 2 groups per workgroup on 256 CUs, the last chunk of the 13 a lone group.
         (8, 2, 100, 1, 104, 0.9),
         (24, 5, 100, 1, 120, 0.9)]


@pytest.fixture(autouse=True)
def _bf16x3():
    from laudnet_amd import ops
    ops.set_math_mode("bf16x3")
    yield
    ops.set_math_mode("fp32")


@pytest.fixture(scope="module")
def ops():
    from laudnet_amd import ops as _ops, load_library
    load_library()
    return _ops


@functools.lru_cache(maxsize=None)
def _problem(gw, B, Ho, stride, C, keep, single=False):
    """-> (ix, n3, a [cap1, C + 8] on the device, w [C, 9, gw], scale, shift, y64 [n3, C] = scale conv + shift in float64 at the kept pixels);
    built once per case and shared by the ReLU / no-ReLU runs, never modified"""
    from laudnet_amd import ops
    Hi = Ho * stride
    if single:
        patch = torch.zeros(B, Ho, Ho)
        patch[B - 1, Ho // 2, 1] = 1.0
    else:
        patch = seeded_bernoulli((B, Ho, Ho), keep, 191 + C)
    ix = ops.mask_to_index(patch.to(DEV), Ho, Ho, stride)
    n3, n1 = int(ix.cnt[0].item()), int(ix.cnt[1].item())
    x = seeded_randn((B, C, Hi, Hi), 192 + C)
    w = seeded_randn((C, gw, 3, 3), 193 + C) * 0.1
    scale = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(194))
    scale[0::5] = 0.0
    scale[1::5] = -scale[1::5]
    shift = 0.1 * seeded_randn((C,), 195)
    idx1, idx3 = ix.idx1[:n1].long().cpu(), ix.idx3[:n3].long().cpu()
    m1 = torch.zeros(B * Hi * Hi, dtype=torch.bool)
    m1[idx1] = True
    xm = (x * m1.view(B, 1, Hi, Hi)).double()            # the packed input holds the dilated-list pixels only; the others read as zero
    y = F.conv2d(xm, w.double(), None, stride, 1, 1, C // gw) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    y64 = y.permute(0, 2, 3, 1).reshape(B * Ho * Ho, C)[idx3]
    a = torch.full((ix.cap1, C + 8), float("nan"))        # rows outside the dilated list: NaN
    a[:n1] = SENTINEL * 1e6                               # the pad columns of the listed rows
    a[:n1, :C] = x.permute(0, 2, 3, 1).reshape(B * Hi * Hi, C)[idx1]
    return ix, n3, a.to(DEV), w.permute(0, 2, 3, 1).reshape(C, 9, gw).contiguous(), scale, shift, y64


def _run(ops, prob, gw, relu, m_count="list"):
    ix, n3, a, w, scale, shift, _ = prob
    C = w.shape[0]
    frag = ops.pack_grouped_mfma_weights(w.to(DEV), gw)
    out = torch.full((ix.cap3, C + 4), SENTINEL, device=DEV)
    cnt = ix.cnt[0:1] if m_count == "list" else m_count
    ops.grouped_mfma_conv3x3_rows(a[:, :C], ix.nbr, frag, gw, scale.to(DEV), shift.to(DEV), out[:, :C], m_count=cnt, m_cap=ix.cap3, relu=relu)
    torch.cuda.synchronize()
    return out


def _check(ops, prob, gw, relu):
    ix, n3, a, w, scale, shift, y64 = prob
    C = w.shape[0]
    assert a.stride(0) == C + 8
    out = _run(ops, prob, gw, relu)
    want = torch.relu(y64) if relu else y64
    got = out[:n3, :C].cpu()
    assert torch.isfinite(got).all()
    err, bound = (got.double() - want).abs().max().item(), 1e-4 * max(1.0, want.abs().max().item())
    print(f"grouped_mfma gw {gw} C {C} rows {n3} relu {relu}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err < bound
    assert bool((out[n3:] == SENTINEL).all()), "rows at or past the device-side count must not be written"
    assert bool((out[:, C:] == SENTINEL).all()), "columns past C must not be written"
    if not relu:
        assert bool((got < 0).any())
        zero = scale == 0
        assert torch.equal(got[:, zero], shift[zero].expand(n3, -1)), "a zero scale leaves the shift"
    assert torch.equal(_run(ops, prob, gw, relu), out), "two runs differ"


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gw,B,Ho,stride,C,keep", CASES)
def test_grouped_mfma_conv3x3_rows_vs_float64(ops, gw, B, Ho, stride, C, keep, relu):
    assert ops.grouped_mfma_ok(C, gw)
    prob = _problem(gw, B, Ho, stride, C, keep)
    ix, n3 = prob[0], prob[1]
    if keep < 1:
        assert 0 < n3 < ix.cap3
    else:
        assert n3 == ix.cap3
    _check(ops, prob, gw, relu)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("gw,C", [(8, 24), (24, 48)])
def test_one_kept_pixel(ops, gw, C, relu):
    prob = _problem(gw, 2, 5, 1, C, 0.0, single=True)
    assert prob[1] == 1
    _check(ops, prob, gw, relu)


@pytest.mark.parametrize("gw,B,Ho,stride,C,keep", [CASES[1], CASES[5]])
def test_a_device_side_count_of_zero_writes_nothing(ops, gw, B, Ho, stride, C, keep):
    prob = _problem(gw, B, Ho, stride, C, keep)
    out = _run(ops, prob, gw, 1, m_count=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert bool((out == SENTINEL).all())
    # ... and no count at all means m_cap rows: the rows past the list read whatever their table entries name, so only the listed rows are compared
    ix, n3, a, w, scale, shift, y64 = prob
    nbr = ix.nbr.view(-1, 9).clone()
    nbr[n3:] = -1                                         # rows past the list: zero rows -> relu(shift)
    frag = ops.pack_grouped_mfma_weights(w.to(DEV), gw)
    out = torch.full((ix.cap3, C), SENTINEL, device=DEV)
    ops.grouped_mfma_conv3x3_rows(a[:, :C], nbr.reshape(-1).contiguous(), frag, gw, scale.to(DEV), shift.to(DEV), out, relu=1)
    assert (out[:n3].cpu().double() - torch.relu(y64)).abs().max().item() < 1e-4 * max(1.0, y64.abs().max().item())
    assert torch.equal(out[n3:].cpu(), torch.relu(shift).expand(ix.cap3 - n3, -1))


def test_refusals(ops):
    from laudnet_amd._lib import LdnError
    prob = _problem(*CASES[1])
    ix, n3, a, w, scale, shift, _ = prob
    C = w.shape[0]
    frag = ops.pack_grouped_mfma_weights(w.to(DEV), 8)
    out = torch.full((ix.cap3, C), SENTINEL, device=DEV)
    args = (scale.to(DEV), shift.to(DEV), out)
    with pytest.raises(LdnError):
        ops.grouped_mfma_conv3x3_rows(a[:, :C], ix.nbr, frag.reshape(-1)[:-16], 8, *args, m_count=ix.cnt[0:1], m_cap=ix.cap3)
    with pytest.raises(LdnError):
        ops.grouped_mfma_conv3x3_rows(a[:, :C], ix.nbr, frag, 24, *args, m_count=ix.cnt[0:1], m_cap=ix.cap3)     # fragments of another width
    with pytest.raises(LdnError):
        ops.grouped_mfma_conv3x3_rows(a[:, :C], ix.nbr, frag.float(), 8, *args, m_count=ix.cnt[0:1], m_cap=ix.cap3)
    w16 = torch.zeros(32, 9, 16, device=DEV)
    with pytest.raises(LdnError):
        ops.grouped_mfma_conv3x3_rows(a[:, :C], ix.nbr, ops.pack_grouped16_weights(w16), 16, *args, m_count=ix.cnt[0:1], m_cap=ix.cap3)
    with pytest.raises(LdnError):
        ops.pack_grouped_mfma_weights(w16, 16)
    with pytest.raises(LdnError):        # a row stride that is no multiple of 4: refused by the entry point itself
        wide = torch.zeros(ix.cap3, C + 2, device=DEV)
        ops.grouped_mfma_conv3x3_rows(a[:, :C], ix.nbr, frag, 8, scale.to(DEV), shift.to(DEV), wide[:, :C], m_count=ix.cnt[0:1], m_cap=ix.cap3)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ the dispatch switch on regnet_tiny.pt (group width 8)
REGNET = load_golden("regnet_tiny.pt")
TOL = 1e-3                     # tests/test_hip_blocks.py: TOL, LOGIT_SCALE_TOL / LOGIT_RTOL of bf16x3
LOGIT_SCALE_TOL, LOGIT_RTOL = 1e-5, 0.0


def _logit_atol(want):
    return TOL + LOGIT_SCALE_TOL * float(torch.as_tensor(want[0]).abs().max())


def _hip_regnet(fx):
    import laudnet_amd
    model = laudnet_amd.LAD_RegNet(laudnet_amd.BlockParams(**REGNET["tiny_params"]), **fx["kw"]).eval()
    assert list(model.state_dict().keys()) == fx["keys"]
    model.load_state_dict(fill_state_dict(model.state_dict(), fx["seed"]))
    size = fx["kw"]["input_size"]
    return model.to(DEV), seeded_randn((fx["batch"], 3, size, size), fx["x_seed"]).to(DEV)


def _counted(ops, monkeypatch):
    calls, real = [], ops.grouped_mfma_conv3x3_rows

    def counted(a2d, nbr, w_frag, group_width, *args, **kwargs):
        calls.append(group_width)
        return real(a2d, nbr, w_frag, group_width, *args, **kwargs)
    monkeypatch.setattr(ops, "grouped_mfma_conv3x3_rows", counted)
    return calls


def _regnet_run(case, run, injected):
    fx = REGNET["cases"][case]
    model, x = _hip_regnet(fx)
    assert {blk.f.group_width for blk in model.blocks()} == {8}
    if injected:
        for i, blk in enumerate(model.blocks()):
            ms = blk.f.masker_spatial.mask_size if case != "layerskip" else 1
            blk.f.forced_spatial_mask = seeded_bernoulli((fx["batch"], 1, ms, ms), 0.5, fx["mask_seed"] + 2 * i)
    with torch.no_grad():
        got = model(x, 1.0)
    want = fx[run]
    assert_tuple_close(got[1:6], want[1:6], atol=1e-6, what=f"regnet {case} stats")
    assert_tuple_close(got[:1], want[:1], atol=_logit_atol(want), rtol=LOGIT_RTOL, what=f"regnet {case} logits")
    if injected:
        assert_tuple_close(got[6:], want[6:], atol=0.0, rtol=1e-5, what=f"regnet {case} flops")


@pytest.mark.parametrize("case,run", [("layerskip", "injected_run"), ("layerskip", "masker_run"), ("spatial_g2", "injected_run")])
def test_regnet_tiny_on_the_new_kernel(ops, monkeypatch, case, run):
    from laudnet_amd import laud_regnet
    monkeypatch.setattr(laud_regnet, "USE_GROUPED_MFMA_WIDTHS", True)
    calls = _counted(ops, monkeypatch)
    _regnet_run(case, run, run == "injected_run")
    assert calls and set(calls) == {8}, calls


def test_switch_off_never_calls_the_new_kernel(ops, monkeypatch):
    from laudnet_amd import laud_regnet
    assert laud_regnet.USE_GROUPED_MFMA_WIDTHS is False
    calls = _counted(ops, monkeypatch)
    _regnet_run("layerskip", "injected_run", True)
    assert calls == []
