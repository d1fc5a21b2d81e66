"""k_stem's persistent tile loop and its GAP partials, and k_stem3, against float64 on buffers the test owns.

No case of tests/test_hip_stem.py gives a workgroup of k_stem a second tile: launch_stem starts min(ntiles, cus * per_cu) workgroups
(per_cu = 2 at 32 channels, 1 at 64) and the largest case there has 112 tiles.  The fetch of the next tile's patch inside the MFMA loop,
the pooled values stored during the next tile's MFMA loop, and the two-slot LDS buffer of the per-wave channel sums (flushed behind the
next tile's barrier) therefore ran only inside the full-size model tests.  Here the batch is sized from the device's CU count so that
every workgroup makes at least three passes with a ragged end, and the partials are checked tile by tile.

Reference: float64 on the CPU, relu(max_pool2d(conv2d(x, w_scaled, stride 2, pad 3), 3, 2, 1) + shift), from the float32 tensors the
kernel receives cast to double (no float32 rounding of its own).  Tolerances:
  output       |got - ref| <= 1e-4 + 1e-5 |ref|            (the project's bound for this kernel; a CPU emulation of the three-product
               bf16 arithmetic reaches about a third of it at these shapes)
  GAP partial  of a tile <= sum over its pixels of (1e-4 + 1e-5 |ref|)  +  64 * 2^-24 * sum |ref|   (the per-pixel bound summed, plus
               the slack of a float32 sum of at most 56 terms)
  output of the launch with gap == output of the launch without it, bit for bit.
Measured on an MI355X (256 CUs) when these tests were written: worst error / bound 0.51 for the output of k_stem, 0.14 for its GAP
partials, 0.54 for k_stem3, 0.06 for the masker's logits; no masker decision of the float64 reference inside the tie margin.
The kernels are called through laudnet_amd._lib: `out` and `gap` sit inside larger flat tensors between guards of 4096 floats filled
with a sentinel, the payload is NaN before each launch; afterwards the guards must be bit-identical and the payload free of NaN (every
element was written by THIS launch -- torch.empty from the caching allocator proves nothing)."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fill import seeded_randn
from oracle import index_ref as IR
from oracle import torch_ref as TR
from test_hip_stem import _params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                     # floats in front of and behind every payload (16 KiB: payload offsets stay 16-byte aligned)
SENTINEL = -7.25e5               # finite, exactly representable, far from every value of the tests
S_PH, S_PW = 8, 7                # k_stem's pooled pixels per tile (ldn_stem.hip)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _lib():
    import laudnet_amd._lib as L
    from laudnet_amd import load_library
    load_library()
    return L, L.load()


@functools.lru_cache(maxsize=None)
def _cus():
    _, lib = _lib()
    c = ctypes.c_int(0)
    assert lib.ldn_device_cus(ctypes.byref(c)) == 0 and c.value > 0
    return c.value


class _Banded:
    """n floats on the device between two guards: payload NaN, guards SENTINEL."""

    def __init__(self, n):
        self.n = n
        self.flat = torch.full((GUARD + n + GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
        self.flat[GUARD:GUARD + n] = float("nan")
        assert self.flat.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def ptr(self, byte_offset=0):
        return ctypes.c_void_p(self.flat.data_ptr() + 4 * GUARD + byte_offset)

    def fetch(self):
        """-> (payload on the CPU, guards bit-identical to the sentinel?)"""
        torch.cuda.synchronize()
        h = self.flat.cpu()
        want = torch.full((GUARD,), SENTINEL, dtype=torch.float32).view(torch.int32)
        ok = torch.equal(h[:GUARD].view(torch.int32), want) and torch.equal(h[GUARD + self.n:].view(torch.int32), want)
        return h[GUARD:GUARD + self.n].clone(), ok


def _pooled(n):
    return ((n - 1) // 2 + 1 - 1) // 2 + 1


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _stem_ref64(x, w_scaled, shift):
    """x [B,3,H,W], w_scaled [C,3,7,7], shift [C] float32 -> float64 [B,C,Hp,Wp]."""
    y = F.max_pool2d(F.conv2d(x.double(), w_scaled.double(), None, 2, 3), 3, 2, 1)
    return F.relu(y + shift.double().view(1, -1, 1, 1))


def _tile_sums(v):
    """[B,C,Hp,Wp] float64 -> [B, tiles_y * tiles_x, C]: sums over k_stem's 8 x 7 tiles clipped to the map (tile t = ty * tiles_x + tx)."""
    B, C, Hp, Wp = v.shape
    ty, tx = -(-Hp // S_PH), -(-Wp // S_PW)
    p = F.pad(v, (0, tx * S_PW - Wp, 0, ty * S_PH - Hp))
    return p.reshape(B, C, ty, S_PH, tx, S_PW).sum(dim=(3, 5)).permute(0, 2, 3, 1).reshape(B, ty * tx, C)


def _launch_stem(x, w_scaled, shift, cout):
    """Both entry points of the stem on guard-banded NaN-filled buffers.  Returns a dict of CPU tensors and flags; asserts nothing but
    the return codes, so that a cached record serves several tests."""
    from laudnet_amd import ops
    L, lib = _lib()
    B, _, H, W = x.shape
    Hp, Wp = _pooled(H), _pooled(W)
    splits = lib.ldn_stem_gap_splits(H, W)
    assert splits == -(-Hp // S_PH) * -(-Wp // S_PW)
    xn = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    frag = ops.pack_stem_weights(w_scaled.to(DEV))
    sh = shift.to(DEV).contiguous()
    n_out, n_gap = B * Hp * Wp * cout, B * splits * cout
    o0, o1, g1 = _Banded(n_out), _Banded(n_out), _Banded(n_gap)
    rc = lib.ldn_stem_conv_pool(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, o0.ptr(), Hp, Wp, L.stream_ptr())
    assert rc == 0, lib.ldn_last_error()
    rc = lib.ldn_stem_conv_pool_gap(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, o1.ptr(), Hp, Wp, g1.ptr(), L.stream_ptr())
    assert rc == 0, lib.ldn_last_error()
    out0, ok0 = o0.fetch()
    out1, ok1 = o1.fetch()
    gap, okg = g1.fetch()
    return dict(out=out0.view(B, Hp, Wp, cout), out_gap=out1.view(B, Hp, Wp, cout), gap=gap.view(B, splits, cout),
                guards=(ok0, ok1, okg), Hp=Hp, Wp=Wp)


def _check_stem(r, ref, tag):
    """The five checks of a stem launch pair against the float64 reference ref [B,C,Hp,Wp]."""
    assert all(r["guards"]), f"{tag}: a guard band was written (out, out with gap, gap) = {r['guards']}"
    for k in ("out", "out_gap", "gap"):
        nan = torch.isnan(r[k])
        assert not nan.any(), f"{tag}: {int(nan.sum())} elements of {k} were never written, first at {nan.nonzero()[0].tolist()}"
    want = ref.permute(0, 2, 3, 1)
    err = (r["out"].double() - want).abs()
    bound = 1e-4 + 1e-5 * want.abs()
    ratio = (err / bound).max().item()
    gwant = _tile_sums(ref)
    gabs = _tile_sums(ref.abs())
    npix = _tile_sums(torch.ones_like(ref))
    gbound = 1e-4 * npix + 1e-5 * gabs + 64 * 2.0 ** -24 * gabs
    gerr = (r["gap"].double() - gwant).abs()
    gratio = (gerr / gbound).max().item()
    print(f"[stem f64] {tag}: out max err {err.max().item():.3e} (ratio to bound {ratio:.3f}), "
          f"gap max err {gerr.max().item():.3e} (ratio to bound {gratio:.3f})")
    assert (err <= bound).all(), f"{tag}: output error / bound = {ratio:.3f}, first at {(err > bound).nonzero()[0].tolist()}"
    assert (gerr <= gbound).all(), (f"{tag}: per-tile GAP error / bound = {gratio:.3f}, first at [b, tile, c] = "
                                    f"{(gerr > gbound).nonzero()[0].tolist()}")
    assert _bits_equal(r["out_gap"], r["out"]), f"{tag}: the output of the launch with gap differs from the launch without"
    return ratio, gratio


def _inputs(B, H, W, cout, seed):
    w, gamma, beta, mean, var = _params(cout, seed)            # gamma[::5] < 0: the fold must happen before the max
    scale = gamma / torch.sqrt(var + 1e-5)
    w_scaled = (w * scale.view(-1, 1, 1, 1)).contiguous()
    shift = (beta - mean * scale).contiguous()
    x = seeded_randn((B, 3, H, W), seed + 7)
    return x, w_scaled, shift


@functools.lru_cache(maxsize=None)
def _case(B, H, W, cout):
    """(launch record, float64 reference) of a seeded case: computed once, shared, never modified."""
    x, w_scaled, shift = _inputs(B, H, W, cout, 100 + H + W)
    ref = _stem_ref64(x, w_scaled, shift)
    return _launch_stem(x, w_scaled, shift, cout), ref


# ------------------------------------------------------------------------------------------------- 1: steady state, several tiles
def _steady_geometry(which):
    """(H, W, tiles per image, B) of geometry 'A' (tiles in a row, last one 2 of 7 columns) or 'B' (tiles in a column, last one 1 of 8
    rows): three tiles per image, five where the CU count is a multiple of 3."""
    cus = _cus()
    if cus % 3:
        per, (H, W) = 3, ((29, 63) if which == "A" else (67, 27))
    else:
        per, (H, W) = 5, ((29, 119) if which == "A" else (131, 27))
    B = -(-(6 * cus + 37) // per)
    Hp, Wp = _pooled(H), _pooled(W)
    ty, tx = -(-Hp // S_PH), -(-Wp // S_PW)
    assert (ty, tx) == ((1, per) if which == "A" else (per, 1))
    assert (Wp - (tx - 1) * S_PW == 2) if which == "A" else (Hp - (ty - 1) * S_PH == 1)
    ntiles = B * per
    assert ntiles >= 6 * cus                                   # at least 3 passes at either per_cu
    assert ntiles % cus != 0 and ntiles % (2 * cus) != 0       # ragged end: some workgroups have a next tile when others do not
    assert cus % per != 0                                      # a workgroup's tile position within an image changes from pass to pass
    return H, W, per, B


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("geom", ["A", "B"])
def test_stem_steady_state(geom, cout):
    """At least three passes of every workgroup, ragged end, full and clipped tiles alternating in one workgroup, consecutive tiles
    of a workgroup in different images."""
    H, W, _, B = _steady_geometry(geom)
    r, ref = _case(B, H, W, cout)
    _check_stem(r, ref, f"steady {geom} B={B} {H}x{W} C={cout}")


# ------------------------------------------------------------------------------------------------- 2: one clipped tile per image
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("batch", ["6*cus+5", "cus+1", "2*cus+1"])
def test_stem_one_clipped_tile_per_image(batch, cout):
    """9 x 13 input -> 3 x 4 pooled: every tile is clipped on both axes and every next tile is another image's.  cus + 1 and
    2 cus + 1 images: at one of the two channel counts exactly one workgroup makes a second pass while all others finish after one."""
    cus = _cus()
    B = {"6*cus+5": 6 * cus + 5, "cus+1": cus + 1, "2*cus+1": 2 * cus + 1}[batch]
    H, W = 9, 13
    assert (_pooled(H), _pooled(W)) == (3, 4)
    r, ref = _case(B, H, W, cout)
    _check_stem(r, ref, f"clipped B={batch}={B} C={cout}")


# ------------------------------------------------------------------------------------------------- 3: the pool pads with -inf
@pytest.mark.parametrize("cout", [32, 64])
def test_stem_pool_padding_is_minus_inf(cout):
    """Every conv value negative (x > 0, w < 0), at the border too.  shift = +2 max|conv|: every output is max(window) + shift > 0 and
    a kernel that padded the pool with 0 would return shift along the border.  shift = -2 max|conv|: everything is exactly 0."""
    B, H, W = 2, 37, 53
    x = seeded_randn((B, 3, H, W), 301).abs() + 0.1
    w_scaled = -(seeded_randn((cout, 3, 7, 7), 302 + cout) * (2.0 / 147) ** 0.5).abs()
    conv = F.conv2d(x.double(), w_scaled.double(), None, 2, 3)
    assert (conv < 0).all()
    big = 2.0 * conv.abs().max().item()
    shift = torch.full((cout,), big, dtype=torch.float32)
    ref = _stem_ref64(x, w_scaled, shift)
    assert (ref > 0).all()
    border = F.relu(F.max_pool2d(F.pad(conv, (1, 1, 1, 1)), 3, 2, 0) + shift.double().view(1, -1, 1, 1))   # the zero-padded pool
    assert (border[:, :, 0] - ref[:, :, 0]).min().item() > 1e-2 and (border[:, :, :, 0] - ref[:, :, :, 0]).min().item() > 1e-2
    _check_stem(_launch_stem(x, w_scaled, shift, cout), ref, f"pad +shift C={cout}")
    r = _launch_stem(x, w_scaled, -shift, cout)
    assert all(r["guards"])
    for k in ("out", "out_gap", "gap"):
        assert not torch.isnan(r[k]).any(), k
        assert (r[k] == 0).all(), f"{k}: {int((r[k] != 0).sum())} non-zero values under shift = -2 max|conv|"


# ------------------------------------------------------------------------------------------------- 4: hand-off to the channel masker
def _masker_handoff(r, ref, cout, tag):
    from laudnet_amd import ops
    G = 16 if cout == 64 else 8
    gran = cout // G
    torch.manual_seed({32: 536, 64: 564}[cout])       # seeds at which the float64 masker keeps some groups and drops others
    mk = TR.ChannelMaskerMLPRef(cout, G).eval()
    with torch.no_grad():
        for prm in mk.parameters():
            prm.normal_()
        B = ref.shape[0]
        want = copy.deepcopy(mk).double().logits(ref).reshape(B, 2 * G)          # float64 module on the float64 reference output
    scale = want.abs().max().item()
    margin = (want[:, :G] - want[:, G:]).abs()
    near = margin <= 1e-4 * max(scale, 1.0)
    share = near.double().mean().item()
    print(f"[stem f64] {tag}: {int(near.sum())} of {near.numel()} decisions within the tie margin ({100 * share:.3f} %), scale {scale:.2f}")
    assert share <= 0.005, f"{tag}: {100 * share:.2f} % of the decisions are excused by the tie margin"     # from float64 alone
    keep = (want[:, :G] >= want[:, G:]).double().mean().item()
    assert 0.2 <= keep <= 0.8, f"{tag}: the float64 masker keeps {100 * keep:.1f} % of the groups: the decisions would check nothing"
    d = lambda t: t.detach().to(DEV).contiguous()
    gap = r["gap"].to(DEV).contiguous()
    mask, idx, cnt, logits = ops.channel_masker(None, d(mk.conv[0].weight), d(mk.conv[0].bias), d(mk.conv[2].weight), d(mk.conv[2].bias),
                                                G, gran, gap_partial=gap, hw=r["Hp"] * r["Wp"], want_logits=True)
    lerr = (logits.cpu().double() - want).abs()
    lbound = 2e-5 * max(scale, 1.0) + 1e-5 * want.abs()
    print(f"[stem f64] {tag}: logits max err {lerr.max().item():.3e} (ratio to bound {(lerr / lbound).max().item():.3f})")
    assert (lerr <= lbound).all(), f"{tag}: logits error / bound = {(lerr / lbound).max().item():.3f}"
    want_mask = (want[:, :G] >= want[:, G:]).float()
    assert not bool(((mask.cpu() != want_mask) & ~near).any()), f"{tag}: a decision differs outside the tie margin"
    widx, wcnt = IR.channel_lists(mask.cpu().numpy(), G * gran)                  # exactly the lists of the mask the kernel decided on
    assert np.array_equal(cnt.cpu().numpy(), wcnt)
    got = idx.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b, :wcnt[b]], widx[b, :wcnt[b]]), b


@pytest.mark.parametrize("cout", [32, 64])
def test_stem_gap_feeds_channel_masker(cout):
    """The partials of the steady-state launch (geometry A) through their only consumer, ldn_channel_masker(gap_partial=...)."""
    H, W, _, B = _steady_geometry("A")
    r, ref = _case(B, H, W, cout)
    _masker_handoff(r, ref, cout, f"masker B={B} {H}x{W} C={cout}")


def test_stem_gap_feeds_channel_masker_model_splits():
    """... and at the model's own geometry: 224 x 224 -> 56 x 56 pooled, 7 x 8 = 56 splits."""
    r, ref = _case(2, 224, 224, 64)
    assert r["gap"].shape[1] == 56
    _check_stem(r, ref, "model geometry B=2 224x224 C=64")
    _masker_handoff(r, ref, 64, "masker B=2 224x224 C=64")


# ------------------------------------------------------------------------------------------------- 5: refusals
def test_stem_refusals_launch_nothing():
    """A bad argument comes back as an error code naming it; nothing is launched (the NaN payloads and the guards stay as they were)."""
    from laudnet_amd import ops
    L, lib = _lib()
    B, H, W, cout = 1, 9, 13, 64
    Hp, Wp = _pooled(H), _pooled(W)
    x, w_scaled, shift = _inputs(B, H, W, cout, 5)
    xn = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    frag, sh = ops.pack_stem_weights(w_scaled.to(DEV)), shift.to(DEV)
    out, gap = _Banded(B * Hp * Wp * cout + 4), _Banded(B * cout + 4)
    st = L.stream_ptr()

    def refused(rc, *words):
        msg = lib.ldn_last_error() or b""
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    refused(lib.ldn_stem_conv_pool(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), 48, out.ptr(), Hp, Wp, st), b"cout", b"48")
    refused(lib.ldn_stem_conv_pool_gap(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), 48, out.ptr(), Hp, Wp, gap.ptr(), st), b"cout", b"48")
    refused(lib.ldn_stem_conv_pool(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, out.ptr(), Hp + 1, Wp, st), b"output must be 3x4")
    refused(lib.ldn_stem_conv_pool_gap(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, out.ptr(), Hp - 1, Wp, gap.ptr(), st),
            b"output must be 3x4")
    refused(lib.ldn_stem_conv_pool(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, out.ptr(4), Hp, Wp, st), b"out", b"aligned")
    refused(lib.ldn_stem_conv_pool_gap(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, out.ptr(4), Hp, Wp, gap.ptr(), st),
            b"out", b"aligned")
    refused(lib.ldn_stem_conv_pool_gap(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, out.ptr(), Hp, Wp, gap.ptr(4), st),
            b"gap", b"aligned")
    for buf in (out, gap):
        payload, ok = buf.fetch()
        assert ok and torch.isnan(payload).all()


# ------------------------------------------------------------------------------------------------- k_stem3
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,H,W,cout", [(2, 45, 75, 32), (2, 45, 75, 64), (1, 3, 511, 32)])
def test_stem3_f64(B, H, W, cout, relu):
    """k_stem3 (one workgroup per band of output rows).  45 x 75: Wo = 38, 6 rows per band, the last band has 5 rows = 190 pixels (its
    last two waves leave, the wave before them is partial); 3 x 511: Wo = 256, one row per band."""
    from laudnet_amd import ops
    L, lib = _lib()
    _, gamma, beta, mean, var = _params(cout, 60 + H)
    scale = gamma / torch.sqrt(var + 1e-5)
    w_scaled = (seeded_randn((cout, 3, 3, 3), 61 + H) * (2.0 / 27) ** 0.5 * scale.view(-1, 1, 1, 1)).contiguous()
    shift = (beta - mean * scale).contiguous()
    x = seeded_randn((B, 3, H, W), 62 + W)
    ref = F.conv2d(x.double(), w_scaled.double(), None, 2, 1) + shift.double().view(1, -1, 1, 1)
    if relu:
        ref = F.relu(ref)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(ref.shape) == (B, cout, Ho, Wo)
    xn = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    frag, sh = ops.pack_stem3_weights(w_scaled.to(DEV)), shift.to(DEV)
    out = _Banded(B * Ho * Wo * cout)
    rc = lib.ldn_stem3_conv(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, int(relu), out.ptr(), Ho, Wo, L.stream_ptr())
    assert rc == 0, lib.ldn_last_error()
    got, ok = out.fetch()
    assert ok, "a guard band was written"
    nan = torch.isnan(got)
    assert not nan.any(), f"{int(nan.sum())} elements were never written, first at flat index {int(nan.nonzero()[0])}"
    want = ref.permute(0, 2, 3, 1)
    err = (got.view(B, Ho, Wo, cout).double() - want).abs()
    bound = 1e-4 + 1e-5 * want.abs()
    print(f"[stem3 f64] {B}x{H}x{W} C={cout} relu={relu}: max err {err.max().item():.3e} (ratio to bound {(err / bound).max().item():.3f})")
    assert (err <= bound).all(), f"error / bound = {(err / bound).max().item():.3f}, first at {(err > bound).nonzero()[0].tolist()}"


def test_stem3_refuses_wide_images():
    """W = 514 (Wo = 257) does not fit a band: an error code, nothing launched."""
    from laudnet_amd import ops
    L, lib = _lib()
    B, H, W, cout = 1, 3, 514, 32
    Ho, Wo = 2, 257
    xn = seeded_randn((B, H, W, 3), 1).to(DEV)
    frag = ops.pack_stem3_weights(seeded_randn((cout, 3, 3, 3), 2).to(DEV))
    sh = torch.zeros(cout, device=DEV)
    out = _Banded(B * Ho * Wo * cout)
    rc = lib.ldn_stem3_conv(L.ptr(xn), B, H, W, L.ptr(frag), L.ptr(sh), cout, 1, out.ptr(), Ho, Wo, L.stream_ptr())
    msg = lib.ldn_last_error() or b""
    assert rc != 0 and b"wider than 512" in msg and b"514" in msg, (rc, msg)
    payload, ok = out.fetch()
    assert ok and torch.isnan(payload).all()
