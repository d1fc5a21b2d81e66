"""Float64 reference of ONE training block under frozen BatchNorm statistics, and inputs on which no ReLU can flip (CPU, plain torch).

`block_f64` restates the block from its formula (laudnet_amd/training.py's module docstring; laud_resnet.py:104-147; the layer-skip
LAD-RegNet block a -> grouped b -> SE -> c -> (+ proj) -> ReLU of laud_regnet.py:157-217) as differentiable torch ops in double precision:

    ResNet   out = relu(identity(x) + m3 * bn3(conv3(relu(bn2(c . conv2(relu(bn1(c . conv1(x)))))))))
    RegNet   out = relu(identity(x) + m3 * bn_c(c(gate . h_b))),  h_b = relu(bn_b(b(relu(bn_a(a(x)))))),  gate = sigmoid(fc2(relu(fc1(mean h_b))))

with the {0,1} masks as differentiable inputs (m3 [B, 1, S, S] upsampled to the output map, nearest; c [B, G] per channel group, applied
BEFORE bn1 / bn2).  It imports nothing of laudnet_amd and nothing of the oracle; tests/test_train_ref.py ties it to the oracle's autograd.

A kernel's gradient can only be held to a per-element bound where its ReLU gates are the reference's.  `forward_error_bound` bounds, to
first order, the error a float32 / bf16x3 evaluation can make in every pre-activation z that feeds a ReLU.  The bound it computes is

    E = |s| ((eps + (K + 4) 2^-24 + 2^-22) (|a| (*) |w|) + (E_prev . [a > 0]) (*) |w|) + 2^-22 |t| + 2^-23 |z|

K = the reduction length, (K + 4) 2^-24 the accumulation form of tests/wgrad_ref.py, eps = 2^-23 for fp32 and 2^-15 for bf16x3
(include/ldn_hip.h: about 2^-16 per product; doubled because both operands are split); the 2^-22 terms are the folding of (s, t) in float32.
E passes the SE gate with the sigmoid's slope 1/4.

THIS IS NOT THE FORMULA AS FIRST STATED for this test, E = |s| ((eps + (K + 4) 2^-24) (|a| (*) |w|) + E_prev (*) |w|) + 2^-23 |z|: it differs in the
factor [a > 0] -- the previous layer's bound E_prev is propagated only from the units whose ReLU is ON (gated=True; gated=False computes the
unrefined form, folding terms included).  That factor is 2 - 10 x in E and carries the case table, so its justification is an induction over the
layers in forward order, which is also the order `make_tie_free` works in:
  * layer 1 reads x, which is exact: E_1 holds as stated.  Once |z_1| >= 4 E_1 at every unit, every gate of layer 1 is the reference's, so an OFF
    unit is relu(negative) = exactly 0 on both sides: its error is 0, not E_1; an ON unit's error is at most E_1 (|relu(p) - relu(q)| <= |p - q|);
  * layer n + 1 therefore sees an input error of at most E_n . [h_n > 0], which is what the formula propagates; clearing it by 4 E_{n+1} makes
    its gates certain in turn.  The statement for layer n + 1 uses only the clearance of the layers before it, which the construction has
    already established and `clearance` re-checks on the final parameters for every ReLU at once.
Caveats.  E is FIRST-ORDER: products of two errors and the change of |a| (*) |w| under the error are dropped; the factor 4 is there for that (and
because the backward also reads the stored h).  The induction needs the clearance of EVERY earlier unit, dropped pixels and images included:
all sites are evaluated densely.  The squeeze of SE and the product with its gate are left unrefined (E of an off unit of h_b is counted): only
ever larger.  tests/test_train_ref.py asserts what the argument rests on: in the float32 run every unit that is off in float64 is exactly 0.
What the unrefined formula would give (measured, `gated=False`): the committed cases have clearance 0.83 - 17.5 under it (4 or more for four of
the narrow stride-2 cases only), 22 of the 27 cases cannot be made tie-free at their committed map, and wide_s1_spatial, wide_s1_layer,
wide_s2_spatial and wide_s2_layer on no map at all, down to 2 x 2 / 1 x 1 outputs.  So "4 E" below always means 4 x the REFINED bound.

`make_tie_free` moves one BatchNorm bias per ReLU layer and channel, in forward order, into a gap of that channel's pre-activations so that
|z| >= 4 E(bf16x3) at every unit of every ReLU, no bias moving by more than 0.25.  Units that are exactly equal on both sides need no clearance: a
dropped pixel over the identity shortcut (z = x, the final ReLU is plain torch everywhere) and a channel-masked unit (z = t[c]).

`CASES` is the table of tests/test_hip_training_f64.py; `tie_free_case` / `reference` build each case once per process.  `VARIANT_CASES`
puts zero, tiny (2^-24) and negative BatchNorm weights into eleven of them (tests/test_hip_training_bn_scales.py): nothing above assumes a
scale near 1 -- the bound carries |s|, and a channel whose scale is 0 is the constant t[c], cleared like any other unit."""
from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from fill import fill_state_dict, seeded_bernoulli, seeded_randn

EPS = {"fp32": 2.0 ** -23, "bf16x3": 2.0 ** -15}
CLEARANCE = 4.0        # |z| >= CLEARANCE * E(bf16x3) at every ReLU
MAX_MOVE = 0.25        # no BatchNorm / fc1 bias moves further than this
BN_EPS = 1e-5
U23, U22, U24 = 2.0 ** -23, 2.0 ** -22, 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ parameters
def _bn_keys(prefix, c):
    return {f"{prefix}.weight": (c,), f"{prefix}.bias": (c,), f"{prefix}.running_mean": (c,), f"{prefix}.running_var": (c,)}


def resnet_template(inplanes, planes, stride, proj):
    """shapes of a bottleneck's state dict (the maskers left out: the masks are inputs)"""
    t = {"conv1.weight": (planes, inplanes, 1, 1), **_bn_keys("bn1", planes), "conv2.weight": (planes, planes, 3, 3), **_bn_keys("bn2", planes),
         "conv3.weight": (4 * planes, planes, 1, 1), **_bn_keys("bn3", 4 * planes)}
    if proj:
        t.update({"downsample.0.weight": (4 * planes, inplanes, 1, 1), **_bn_keys("downsample.1", 4 * planes)})
    return t


def regnet_template(width_in, width_out, gw, se_ratio=0.25):
    wb, sq = width_out, int(round(se_ratio * width_in))
    t = {"f.a.0.weight": (wb, width_in, 1, 1), **_bn_keys("f.a.1", wb), "f.b.0.weight": (wb, gw, 3, 3), **_bn_keys("f.b.1", wb),
         "f.se.fc1.weight": (sq, wb, 1, 1), "f.se.fc1.bias": (sq,), "f.se.fc2.weight": (wb, sq, 1, 1), "f.se.fc2.bias": (wb,),
         "f.c.0.weight": (width_out, wb, 1, 1), **_bn_keys("f.c.1", width_out)}
    return t


def params_from_state_dict(sd, **cfg):
    """params = {"cfg": kind / mode / stride [/ gw], "sd": the block's tensors in float64 (maskers and counters left out)}"""
    keep = {k: v.detach().double().cpu().clone() for k, v in sd.items() if "masker" not in k and not k.endswith("num_batches_tracked")}
    return {"cfg": dict(cfg), "sd": keep}


def trainable(params):
    return [k for k in params["sd"] if not k.endswith(("running_mean", "running_var"))]


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _fold(sd, prefix):
    s = sd[prefix + ".weight"] * torch.rsqrt(sd[prefix + ".running_var"] + BN_EPS)
    return s, sd[prefix + ".bias"] - sd[prefix + ".running_mean"] * s


def _affine(y, s, t):
    return y * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)


def _conv_layer(rec, name, a, sd, wkey, bnkey, stride=1, groups=1, cm=None):
    """z = s (cm . conv(a)) + t, recorded for the error bound"""
    w = sd[wkey]
    pad = (w.shape[2] - 1) // 2
    y = F.conv2d(a, w, stride=stride, padding=pad, groups=groups)
    if cm is not None:
        y = y * cm
    s, t = _fold(sd, bnkey)
    z = _affine(y, s, t)
    rec[name] = SimpleNamespace(a=a, w=w, stride=stride, pad=pad, groups=groups, s=s, t=t, cm=cm, z=z, bias=bnkey + ".bias")
    return z


def _forward(params, x, masks, dtype, sd=None):
    """-> (out, rec): rec holds every layer's operands and pre-activations (what forward_error_bound walks)"""
    cfg = params["cfg"]
    sd = {k: v.to(dtype) for k, v in params["sd"].items()} if sd is None else sd
    x = x.to(dtype)
    rec = {}
    stride, mode = cfg["stride"], cfg["mode"]
    Ho, Wo = (x.shape[2] - 1) // stride + 1, (x.shape[3] - 1) // stride + 1
    m3 = None
    if mode != "channel":
        m3 = F.interpolate(masks["spatial"].to(dtype), size=(Ho, Wo), mode="nearest")
    if cfg["kind"] == "resnet":
        cm = None
        if mode in ("channel", "both"):
            c = masks["channel"].to(dtype)
            W = sd["conv1.weight"].shape[0]
            cm = c.repeat_interleave(W // c.shape[1], dim=1).view(c.shape[0], W, 1, 1)
        h1 = F.relu(_conv_layer(rec, "relu1", x, sd, "conv1.weight", "bn1", cm=cm))
        h2 = F.relu(_conv_layer(rec, "relu2", h1, sd, "conv2.weight", "bn2", stride=stride, cm=cm))
        br = _conv_layer(rec, "branch", h2, sd, "conv3.weight", "bn3")
        pkeys = ("downsample.0.weight", "downsample.1")
    else:
        gw = cfg["gw"]
        ha = F.relu(_conv_layer(rec, "relu_a", x, sd, "f.a.0.weight", "f.a.1"))
        hb = F.relu(_conv_layer(rec, "relu_b", ha, sd, "f.b.0.weight", "f.b.1", stride=stride, groups=ha.shape[1] // gw))
        w1, w2 = sd["f.se.fc1.weight"].flatten(1), sd["f.se.fc2.weight"].flatten(1)
        sq = hb.mean(dim=(2, 3))
        u = sq @ w1.t() + sd["f.se.fc1.bias"]
        v = torch.relu(u) @ w2.t() + sd["f.se.fc2.bias"]
        gate = torch.sigmoid(v)
        zc = hb * gate.view(gate.shape[0], -1, 1, 1)
        rec["se"] = SimpleNamespace(hb=hb, sq=sq, w1=w1, w2=w2, u=u, v=v, gate=gate, zc=zc, bias="f.se.fc1.bias")
        br = _conv_layer(rec, "branch", zc, sd, "f.c.0.weight", "f.c.1")
        pkeys = ("proj.0.weight", "proj.1")
    if m3 is not None:
        br = br * m3
    ident = x
    if pkeys[0] in sd:
        ident = _conv_layer(rec, "proj", x, sd, pkeys[0], pkeys[1], stride=stride)
    z = br + ident
    rec["final"] = SimpleNamespace(z=z, m3=m3, x=x)
    return F.relu(z), rec


def block_f64(params, x, masks, dtype=torch.float64):
    """The block's output [B, cout, Ho, Wo], differentiable in x, the masks (dict: "spatial" [B, 1, S, S] / "channel" [B, G]) and -- through
    `gradients` -- every parameter.  dtype: float64, or float32 for "the reference alone" runs."""
    return _forward(params, x, masks, dtype)[0]


def gradients(params, x, masks, gout, dtype=torch.float64):
    """-> (out, grads, gates): grads = {"x", "mask.spatial", "mask.channel", every trainable tensor's name} of sum(out * gout) by torch.autograd
    in `dtype`; gates = {ReLU site: z > 0}."""
    sd = {k: v.detach().to(dtype).clone() for k, v in params["sd"].items()}
    names = trainable(params)
    for k in names:
        sd[k].requires_grad_(True)
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    ml = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in masks.items()}
    out, rec = _forward(params, xl, ml, dtype, sd=sd)
    out.backward(gout.to(dtype))
    grads = {"x": xl.grad, **{f"mask.{k}": v.grad for k, v in ml.items()}, **{k: sd[k].grad for k in names}}
    gates = {k: (r.u if k == "se" else r.z).detach() > 0 for k, r in rec.items() if k not in ("branch", "proj")}
    return out.detach(), grads, gates


# ------------------------------------------------------------------------------------------------------------------ the error bound
def _conv_bound(r, E_in, eps, gated=True):
    """E of z = s (cm . conv(a)) + t from the bound E_in on a (None: a is exact).  gated: E_in counts only where a = relu(z_prev) is ON (the
    module docstring's induction); False = the unrefined E_prev (*) |w| over every unit."""
    conv = lambda t: F.conv2d(t, r.w.abs(), stride=r.stride, padding=r.pad, groups=r.groups)
    K = r.w[0].numel()
    E = (eps + (K + 4) * U24 + U22) * conv(r.a.abs())
    if E_in is not None:
        E = E + conv(E_in * (r.a > 0) if gated else E_in)
    E = E * r.s.abs().view(1, -1, 1, 1)
    if r.cm is not None:
        E = E * r.cm          # a masked channel is the constant t[c] on both sides
    return E + U22 * r.t.abs().view(1, -1, 1, 1) + U23 * r.z.abs()


def forward_error_bound(params, x, masks, mode, gated=True):
    """[(site, bias key, z, E, sel)] in forward order: the pre-activation z of every ReLU, the first-order bound E on its error under arithmetic
    `mode`, and sel = the units whose clearance that bias sets (the exactly-equal ones left out; the final ReLU appears once per bias that feeds it).  gated=False: the unrefined
    formula (E_prev over every unit, on or off) -- measured beside the refined one, never used to build a case."""
    eps = EPS[mode]
    with torch.no_grad():
        _, rec = _forward(params, x, masks, torch.float64)
        sites = []
        full = lambda r: torch.ones_like(r.z, dtype=torch.bool) if r.cm is None else (r.cm > 0.5).expand_as(r.z)
        if params["cfg"]["kind"] == "resnet":
            r1, r2 = rec["relu1"], rec["relu2"]
            E1 = _conv_bound(r1, None, eps, gated)
            E2 = _conv_bound(r2, E1, eps, gated)
            sites += [("relu1", r1.bias, r1.z, E1, full(r1)), ("relu2", r2.bias, r2.z, E2, full(r2))]
            Eb = _conv_bound(rec["branch"], E2, eps, gated)
        else:
            ra, rb, se = rec["relu_a"], rec["relu_b"], rec["se"]
            Ea = _conv_bound(ra, None, eps, gated)
            Eb_ = _conv_bound(rb, Ea, eps, gated)
            sites += [("relu_a", ra.bias, ra.z, Ea, full(ra)), ("relu_b", rb.bias, rb.z, Eb_, full(rb))]
            P = se.hb.shape[2] * se.hb.shape[3]
            # (the squeeze and the gate's product are NOT masked by h_b's gates: E of an off unit is counted although it is exactly zero --
            # only ever larger, and the SE site has three units per channel, so nothing is gained by refining it)
            Esq = Eb_.mean(dim=(2, 3)) + (P + 4) * U24 * se.hb.abs().mean(dim=(2, 3))
            fc = lambda a, Ea_, w, out: (eps + (w.shape[1] + 4) * U24) * (a.abs() @ w.abs().t()) + Ea_ @ w.abs().t() + U23 * out.abs()
            Eu = fc(se.sq, Esq, se.w1, se.u)                       # SE's inner ReLU is a gated layer of its own
            sites.append(("se", se.bias, se.u, Eu, torch.ones_like(se.u, dtype=torch.bool)))
            Ev = fc(torch.relu(se.u), Eu, se.w2, se.v)
            Eg = Ev / 4 + U22                                       # the sigmoid's slope is at most 1/4
            g4 = se.gate.view(se.gate.shape[0], -1, 1, 1)
            Ezc = Eb_ * g4 + se.hb.abs() * Eg.view(Eg.shape[0], -1, 1, 1) + U23 * se.zc.abs()
            Eb = _conv_bound(rec["branch"], Ezc, eps, gated)
        fin = rec["final"]
        kept = torch.ones_like(fin.z, dtype=torch.bool) if fin.m3 is None else (fin.m3 > 0.5).expand_as(fin.z)
        E = Eb if fin.m3 is None else Eb * fin.m3
        if "proj" in rec:
            rp = rec["proj"]
            E = E + _conv_bound(rp, None, eps, gated)
            if bool((~kept).any()):
                sites.append(("final", rp.bias, fin.z, E + U23 * fin.z.abs(), ~kept))      # the projection's bias first: the dropped pixels
        sites.append(("final", rec["branch"].bias, fin.z, E + U23 * fin.z.abs(), kept))    # (a dropped pixel over the identity shortcut: z = x, exact)
    return sites


def clearance(params, x, masks, mode="bf16x3", gated=True):
    """the smallest |z| / E over the selected units of every ReLU"""
    worst = float("inf")
    for _, _, z, E, sel in forward_error_bound(params, x, masks, mode, gated):
        if bool(sel.any()):
            worst = min(worst, float((z.abs() / E)[sel].min()))
    return worst


# ------------------------------------------------------------------------------------------------------------------ tie-free inputs
def _free_shift(z, need, cap):
    """a shift d of one channel's bias, |d| <= cap, with |z_i + d| >= need_i for every unit: the midpoint of the widest free gap BETWEEN two
    units' forbidden intervals (so the channel keeps units on both sides), else of the widest free stretch at either end; None if there is none"""
    order = np.argsort(-z - need)
    lo, hi = (-z - need)[order], np.maximum.accumulate((-z + need)[order])
    best = None
    for a, b in ((hi[:-1], lo[1:]), (np.array([-cap, hi[-1]]), np.array([lo[0], cap]))):
        a, b = np.clip(a, -cap, cap), np.clip(b, -cap, cap)
        if a.size and float((b - a).max()) > 0:
            i = int((b - a).argmax())
            best = 0.5 * (float(a[i]) + float(b[i]))
            break
    return best


def make_tie_free(params, x, masks, factor=CLEARANCE, cap=MAX_MOVE, gated=True):
    """-> (params with moved biases, the achieved smallest |z| / E(bf16x3), the largest move).  Raises ValueError where a channel has no gap
    within the cap."""
    P = copy.deepcopy(params)
    moved = 0.0
    n = len(forward_error_bound(P, x, masks, "bf16x3", gated))
    for k in range(n):                                              # forward order: a layer's bias is set on the final values of the layers before it
        site, key, z, E, sel = forward_error_bound(P, x, masks, "bf16x3", gated)[k]
        bias = P["sd"][key]
        C = z.shape[1]
        zc = z.transpose(0, 1).reshape(C, -1).numpy()
        # 10 % over the factor and the largest |z| a move can produce: E's own 2^-23 |z| term moves with the bias
        need = (1.1 * factor * (E + U23 * cap)).transpose(0, 1).reshape(C, -1).numpy()
        pick = sel.transpose(0, 1).reshape(C, -1).numpy()
        for c in range(C):
            if not pick[c].any():
                continue
            d = _free_shift(zc[c][pick[c]], need[c][pick[c]], cap)
            if d is None:
                raise ValueError(f"{site}: channel {c} of {key} has no gap of {factor} E within {cap}")
            new = (bias[c] + d).float().double()                    # the parameters stay float32 values: both sides hold the same numbers
            moved = max(moved, abs(float(new - bias[c])))
            bias[c] = new
    got = clearance(P, x, masks, gated=gated)
    if got < factor or moved > cap:
        raise ValueError(f"tie-free construction reached clearance {got:.2f} (needs {factor}) with a largest move of {moved:.3f} (cap {cap})")
    return P, got, moved


# ------------------------------------------------------------------------------------------------------------------ the case table
# ResNet: (inplanes, planes, stride); narrow = the fixtures' widths (channel algebra on conv_packed), wide = a full-width stage-1 block, mid =
# the narrowest widths whose channel algebra runs in k_dense's epilogue (every width a multiple of 32).  Batch 3 everywhere.
_RESNET = {"narrow_s1": (64, 16, 1), "narrow_s2": (32, 16, 2), "mid_s1": (128, 32, 1), "mid_s2": (128, 32, 2), "wide_s1": (256, 64, 1),
           "wide_s2": (256, 64, 2)}
# LAD-RegNet layer skip: tests/test_hip_training_regnet.py's blocks (width_in, width_out, group width, stride)
_REGNET = {"regnet_gw8_s1": (32, 32, 8, 1), "regnet_gw16_s2_proj": (32, 64, 16, 2), "regnet_gw24_s1": (48, 48, 24, 1)}
BATCH = 3
LAYER_MASK = [1.0, 0.0, 1.0]           # a skipped image between two kept ones
MODES = ("spatial", "layer", "channel", "both")
# case -> (the block's INPUT map, seed).  The intended maps are 10 x 10 (stride 1) and 12 x 12 -> 6 x 6 (stride 2) -- 300 rows, resp. 432 -> 108:
# more than one 256-row tile with a ragged remainder -- and 8 x 8 outputs for LAD-RegNet.  E is a WORST-CASE bound: it grows like the
# reduction lengths K1 K2 K3 while the pre-activations grow like their square roots, so the forbidden interval 4 E around every unit
# fills a channel's +-0.25 window once the channel has more than a few dozen units (narrow) / a dozen (wide: K = 256, 576, 64).  A case that
# cannot be made tie-free at the intended map runs on the LARGEST smaller map (and the first of four seeds) at which the construction
# succeeds (find_map; tests/test_train_ref.py holds this table to it); the factor 4 is never reduced.  Every narrow case keeps its intended
# map; the wide ones come down to 12 - 192 rows, which is why the mid cases exist: they cross the 256-row tile on the same kernels.  On the
# smallest maps the 2 x 2-pixel patch grid degenerates: wide_s1_spatial and wide_s2_spatial have ONE patch per image (a 2 x 2 output map), i.e. a
# seeded per-image mask -- layer skip under another name; the 64-wide path sees no second row tile in any case.
_MAPS = {
    "narrow_s1_spatial": (10, 700), "narrow_s1_layer": (10, 710), "narrow_s1_channel": (10, 720), "narrow_s1_both": (10, 730),
    "narrow_s2_spatial": (12, 740), "narrow_s2_layer": (12, 750), "narrow_s2_channel": (12, 760), "narrow_s2_both": (12, 770),
    "mid_s1_spatial": (6, 1780), "mid_s1_layer": (6, 3790), "mid_s1_channel": (8, 2800), "mid_s1_both": (10, 810),
    "mid_s2_spatial": (12, 820), "mid_s2_layer": (12, 1830), "mid_s2_channel": (12, 840), "mid_s2_both": (12, 850),
    "wide_s1_spatial": (2, 1860), "wide_s1_layer": (2, 870), "wide_s1_channel": (4, 880), "wide_s1_both": (4, 890),
    "wide_s2_spatial": (4, 2900), "wide_s2_layer": (4, 2910), "wide_s2_channel": (8, 1920), "wide_s2_both": (8, 930),
    "regnet_gw8_s1": (8, 2031), "regnet_gw16_s2_proj": (12, 3031), "regnet_gw24_s1": (3, 3031),
}


def _spec(name):
    if name in _REGNET:
        return ("regnet",) + _REGNET[name]
    shape, mode = name.rsplit("_", 1)
    return ("resnet", shape, mode) + _RESNET[shape]


def build_fixture(name, size, seed):
    """the block fixture of a case on a `size` x `size` INPUT map, in the form helpers.make_block takes (ResNet) / the constructor arguments
    (RegNet), with its masks"""
    spec = _spec(name)
    if spec[0] == "regnet":
        _, win, wout, gw, stride = spec
        return dict(kind="regnet", mode="layer", stride=stride, gw=gw, widths=(win, wout), output_size=size // stride, seed=seed, x_seed=seed + 1,
                    x_shape=[BATCH, win, size, size], masks={"spatial": torch.tensor(LAYER_MASK).view(BATCH, 1, 1, 1)},
                    has_downsample=win != wout or stride != 1)
    _, shape, mode, inplanes, planes, stride = spec
    out_size = size // stride
    grid = max(out_size // 2, 1)                                                        # 2 x 2-pixel patches
    use_s, use_c = mode in ("spatial", "both"), mode in ("channel", "both")
    kw = dict(inplanes=inplanes, planes=planes, stride=stride, spatial_mask_channel_group=1, channel_dyn_granularity=2 if use_c else 1,
              output_size=out_size, mask_spatial_granularity=(out_size // grid) if use_s else 1, dyn_mode=mode, channel_masker="MLP",
              channel_masker_layers=2, reduction=16)
    masks = {}
    if use_s:
        masks["spatial"] = seeded_bernoulli((BATCH, 1, grid, grid), 0.5, seed + 2)
    if mode == "layer":
        masks["spatial"] = torch.tensor(LAYER_MASK).view(BATCH, 1, 1, 1)
    if use_c:
        masks["channel"] = seeded_bernoulli((BATCH, planes // 2), 0.6, seed + 3)
    return dict(kind="resnet", mode=mode, stride=stride, kw=kw, seed=seed, x_seed=seed + 1, x_shape=[BATCH, inplanes, size, size], masks=masks,
                has_downsample=stride != 1)


CASES = [f"{shape}_{mode}" for shape in _RESNET for mode in MODES] + list(_REGNET)


def case_fixture(name):
    return build_fixture(name, *_MAPS[name])


def masks_keep_and_drop(masks):
    return all(bool((m > 0.5).any()) and bool((m < 0.5).any()) for m in masks.values())


def map_ladder(name):
    """the input maps a case is tried on, the intended one first"""
    spec = _spec(name)
    stride = spec[-1]
    outs = (8, 6, 4, 3, 2) if spec[0] == "regnet" else ((10, 8, 6, 4, 2) if stride == 1 else (6, 4, 2, 1))
    return [o * stride for o in outs]


def base_seed(name):
    return 31 if name in _REGNET else 700 + CASES.index(name) * 10


def find_map(name, seeds=4, gated=True):
    """the first (map, seed) of the ladder at which make_tie_free succeeds and every mask keeps and drops units"""
    for size in map_ladder(name):
        for k in range(seeds):
            fx = build_fixture(name, size, base_seed(name) + 1000 * k)
            if not masks_keep_and_drop(fx["masks"]):
                continue
            try:
                make_tie_free(case_params(fx), case_input(fx), fx["masks"], gated=gated)
            except ValueError:
                continue
            return size, fx["seed"]
    raise ValueError(f"{name}: no map of the ladder can be made tie-free")


def case_input(fx):
    return F.relu(seeded_randn(fx["x_shape"], fx["x_seed"]))


def case_params(fx):
    """the seeded parameters of a case (tests/golden/fill.py on this module's own template: the values a block of the same seed is filled with)"""
    if fx["kind"] == "regnet":
        tmpl = regnet_template(*fx["widths"], fx["gw"])
        if fx["has_downsample"]:
            tmpl.update({"proj.0.weight": (fx["widths"][1], fx["widths"][0], 1, 1), **_bn_keys("proj.1", fx["widths"][1])})
        cfg = dict(kind="regnet", mode="layer", stride=fx["stride"], gw=fx["gw"])
    else:
        tmpl = resnet_template(fx["kw"]["inplanes"], fx["kw"]["planes"], fx["stride"], fx["has_downsample"])
        cfg = dict(kind="resnet", mode=fx["mode"], stride=fx["stride"])
    sd = fill_state_dict({k: torch.zeros(v) for k, v in tmpl.items()}, fx["seed"])
    return params_from_state_dict(sd, **cfg)


# ------------------------------------------------------------------------------------------------------------------ BatchNorm scale variants
# Every seeded BatchNorm weight lies in [0.5, 1.5) (tests/golden/fill.py).  Real checkpoints hold zero, tiny and negative ones, and the
# detection backbone is constructed with zero_init_residual: every bn3.weight exactly 0.  A variant edits the seeded BatchNorm WEIGHTS of a case
# (so the folded scale of a zero weight is exactly 0) BEFORE make_tie_free runs, on the case's committed map and seed:
#   mixed      every BatchNorm of the block, the projection's included, by channel index c:  c % 8 == 1 -> 0,  c % 8 == 3 -> negated,
#              c % 8 == 5 -> +2^-24,  c % 8 == 7 -> -2^-24,  the rest as seeded
#   zero_last  the branch's last BatchNorm weight (bn3.weight / f.c.1.weight) 0 throughout: what zero_init_residual leaves
# find_map's rule (the largest map of the ladder) belongs to the base cases; the variants reuse their maps.
VARIANTS = ("mixed", "zero_last")
VARIANT_BASES = ["narrow_s1_spatial", "narrow_s1_layer", "narrow_s1_channel", "narrow_s1_both", "narrow_s2_spatial", "narrow_s2_channel",
                 "narrow_s2_both", "mid_s1_both", "mid_s2_channel", "regnet_gw8_s1", "regnet_gw16_s2_proj"]
VARIANT_CASES = [(n, v) for n in VARIANT_BASES for v in VARIANTS]
TINY = 2.0 ** -24


def last_bn(sd):
    """the branch's last BatchNorm of a state dict: "bn3" (ResNet) / "f.c.1" (LAD-RegNet)"""
    return "bn3" if "bn3.weight" in sd else "f.c.1"


def mixed_classes(n):
    """{class: bool [n]} of the `mixed` edit by channel index"""
    c = torch.arange(n) % 8
    return {"zero": c == 1, "negated": c == 3, "tiny": c == 5, "neg_tiny": c == 7}


def edit_bn_weights(sd, variant):
    """the variant's edit IN PLACE on a state dict (any float dtype): BatchNorm weights only (a `.weight` beside a `.running_var`)"""
    if variant == "zero_last":
        sd[last_bn(sd) + ".weight"].zero_()
    elif variant == "mixed":
        for k in [k for k in sd if k.endswith(".weight") and k[:-len("weight")] + "running_var" in sd and "masker" not in k]:
            w, cls = sd[k], mixed_classes(sd[k].numel())
            w[cls["zero"]] = 0.0
            w[cls["negated"]] = -w[cls["negated"]]
            w[cls["tiny"]] = TINY
            w[cls["neg_tiny"]] = -TINY
    else:
        raise ValueError(f"unknown BatchNorm scale variant {variant!r}")
    return sd


@functools.lru_cache(maxsize=None)
def tie_free_case(name, variant=None):
    """-> namespace(fx, params0 = as seeded [and edited by `variant`], params = tie-free, x, masks, clearance, moved); built once per process,
    never modified"""
    fx = case_fixture(name)
    x, params0 = case_input(fx), case_params(fx)
    if variant is not None:
        edit_bn_weights(params0["sd"], variant)
    params, got, moved = make_tie_free(params0, x, fx["masks"])
    return SimpleNamespace(name=name, variant=variant, fx=fx, params0=params0, params=params, x=x, masks=fx["masks"], clearance=got, moved=moved)


def case_gout(case, variant=None):
    """the upstream gradient of a case: the same for every variant (seed 77 at the output's shape)"""
    stride, cout = case.fx["stride"], case.params["sd"]["bn3.weight" if case.fx["kind"] == "resnet" else "f.c.1.weight"].shape[0]
    B, _, H, W = case.fx["x_shape"]
    return seeded_randn((B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1), 77)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64, variant=None):
    """-> (out, grads, gates) of the tie-free case in `dtype` (float64: THE reference, computed once and shared)"""
    case = tie_free_case(name, variant)
    return gradients(case.params, case.x, case.masks, case_gout(case, variant), dtype)


def worst_ratio(got, want):
    """max |got - want| / max |want|: the figure every gradient check of test_hip_training_f64.py bounds by 1e-3"""
    return float((got.double().cpu() - want).abs().max() / want.abs().max())
