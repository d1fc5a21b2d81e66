"""The contract of ldn_conv_rows_split / ldn_conv_rows_f32 (include/ldn_hip.h) restated as ONE plain float64 torch function, with every
optional epilogue term: the scale / shift / residual affine, the 16-class border shift table, the LayerNorm fold, the three activations,
post_sub and the per-image channel mask.  Nothing of the kernels' structure is in it (no tiles, no split products).  The same file holds
the table of cases that tests/test_dense_rows_ref.py (CPU: which kernel a case reaches, and whether its inputs tell eight plausible
mistakes from the truth) and tests/test_hip_dense_terms.py (GPU) share, and the deterministic inputs of a case.  No CUDA here."""
from __future__ import annotations

import math

import torch

MUTANTS = ("img_from_m", "ln_from_dst", "post_sub_before_act", "mask_before_post_sub", "class_from_m", "border_from_out",
           "residual_after_act", "relu_if_neg_le")


def border_class(q, geom, from_out=False):
    """The class of flat output pixel q: (top | bottom << 1) * 4 + (left | right << 1) of the 3x3 taps that fall into the padding."""
    Hi, Wi, Ho, Wo, stride = geom
    q = q % (Ho * Wo)
    oy, ox = q // Wo, q % Wo
    Hb, Wb = (Ho, Wo) if from_out else (Hi, Wi)
    top, bottom = (oy * stride - 1 < 0).long(), (oy * stride + 1 >= Hb).long()
    left, right = (ox * stride - 1 < 0).long(), (ox * stride + 1 >= Wb).long()
    return (top | bottom << 1) * 4 + (left | right << 1)


def conv_rows_f64(a, w, scale, shift, count, out_total, *, taps=1, a_rows=None, out_rows=None, residual=None, relu=1, relu_if_neg=None,
                  post_sub=None, chan_mask=None, rows_per_image=0, pix_map=None, geom=None, ln_stats=None, ln_c1=None, mutant=None):
    """-> (out [out_total, cout] float64, NaN where nothing is written; written [out_total, cout] bool).  Rows m < count only; list entries
    behind the count and rows that no list names are never touched.  mutant: one of MUTANTS, a deliberately wrong reading of the contract."""
    assert mutant is None or mutant in MUTANTS
    f64 = torch.float64
    cout = w.shape[0]
    m = torch.arange(count)
    src = a_rows.reshape(-1, taps)[:count].long() if a_rows is not None else m.view(-1, 1)
    g = torch.where((src >= 0).unsqueeze(-1), a.double()[src.clamp(min=0)], torch.zeros((), dtype=f64))      # [count, taps, cin]
    acc = torch.einsum("mtc,ntc->mn", g, w.double().reshape(cout, taps, -1))
    dst = out_rows[:count].long() if out_rows is not None else m
    if ln_stats is not None:
        s0 = dst % ln_stats.shape[0] if mutant == "ln_from_dst" else src[:, 0]
        st = ln_stats.double()[s0.clamp(min=0)]
        mean = torch.where(s0 >= 0, st[:, 0], torch.zeros((), dtype=f64))
        rstd = torch.where(s0 >= 0, st[:, 1], torch.ones((), dtype=f64))
        acc = (acc - mean.view(-1, 1) * ln_c1.double().view(1, -1)) * rstd.view(-1, 1)
    if shift.dim() == 2:
        cls = border_class(m if mutant == "class_from_m" else pix_map[:count].long(), geom, from_out=mutant == "border_from_out")
        sh = shift.double()[cls]
    else:
        sh = shift.double().view(1, -1)
    v = acc * (scale.double().view(1, -1) if scale is not None else 1.0) + sh
    res = residual.double()[dst] if residual is not None else 0.0
    if mutant != "residual_after_act":
        v = v + res
    if post_sub is not None and mutant == "post_sub_before_act":
        v = v - post_sub.double().view(1, -1)
    if relu == 1:
        v = v.clamp(min=0)
    elif relu == 2:
        neg = relu_if_neg[:count] <= 0 if mutant == "relu_if_neg_le" else relu_if_neg[:count] < 0
        v = torch.where(neg.view(-1, 1), v.clamp(min=0), v)
    elif relu == 3:
        v = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    else:
        assert relu == 0
    if mutant == "residual_after_act":
        v = v + res
    cm = chan_mask.double()[(m if mutant == "img_from_m" else dst) // rows_per_image] if chan_mask is not None else 1.0
    ps = post_sub.double().view(1, -1) if post_sub is not None and mutant != "post_sub_before_act" else 0.0
    v = v * cm - ps if mutant == "mask_before_post_sub" else (v - ps) * cm
    out = torch.full((out_total, cout), float("nan"), dtype=f64)
    written = torch.zeros(out_total, cout, dtype=torch.bool)
    out[dst] = v
    written[dst] = True
    return out, written


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# kind "pm": scale, residual, ReLU (relu 1, or relu 2 with relu_if_neg in {-1, 0, 1}), post_sub and chan_mask; taps == 9 adds the 16-class shift
#            table with pix_map and a geometry.  Bound 1e-4 max(1, |ref|max).
# kind "ln": the LayerNorm fold and the exact GELU with chan_mask, inputs scaled as test_hip_adavit.py::test_layernorm_and_gelu_as_epilogue_terms
#            (a quarter of the rows with mean / std = 3).  Bound 2e-4 absolute.
# Every case gathers through a list (taps == 1: a permutation with a few -1 entries; taps == 9: a random neighbour table) and scatters
# through a true permutation into a taller buffer, so that packed row, source row and destination row are three different numbers.
GEOMS = ((14, 10, 7, 5, 2), (13, 9, 7, 5, 2), (7, 5, 7, 5, 1), (12, 14, 6, 7, 2))     # stride 2 with even / odd Hi, non-square throughout
DEFAULT_COUNT = 283          # not a multiple of 32: the last 32-row group and the second 256-row tile are partial


def _case(kernel, form, taps, cin, cout, m_cap, counted, hint, kind):
    return dict(kernel=kernel, form=form, taps=taps, cin=cin, cout=cout, m_cap=m_cap, counted=counted, hint=hint, kind=kind)


def _table():
    shapes = [      # (kernel, form, taps, cin, cout, m_cap, counted, hint): the smallest shape found that reaches the kernel
        ("k_dense2<2,0,0,0,1,0,0>", "feat", 1, 64, 64, 300, 0, -1),
        ("k_dense2<4,0,0,0,1,0,0>", "feat", 1, 128, 128, 600, 1, -1),
        ("k_dense2<5,0,0,0,1,0,0>", "feat", 1, 64, 160, 300, 0, -1),
        ("k_dense2<6,0,0,0,1,0,0>", "feat", 1, 64, 192, 49153, 1, 49153),
        ("k_dense2<8,0,0,0,1,0,0>", "feat", 1, 64, 256, 49153, 1, 49153),
        ("k_dense2<2,0,0,0,1,1,0>", "feat", 1, 72, 40, 300, 1, -1),
        ("k_dense2<2,0,0,0,1,1,0>", "feat", 1, 136, 40, 300, 1, -1),
        ("k_dense2<5,0,0,0,1,1,0>", "feat", 1, 72, 144, 300, 1, -1),
        ("k_dense2<5,0,0,0,1,1,0>", "feat", 1, 24, 160, 300, 1, -1),
        ("k_dense2<5,0,0,0,1,1,0>", "feat", 1, 128, 320, 300, 1, -1),
        ("k_dense<2,0,0,0,256,0,0>", "feat", 1, 24, 40, 300, 1, -1),
        ("k_dense<2,0,1,0,256,0,0>", "feat", 1, 24, 64, 300, 1, -1),
        ("k_dense<4,0,0,0,256,0,0>", "feat", 1, 24, 100, 300, 1, -1),
        ("k_dense<4,0,0,0,256,0,0>", "feat", 1, 192, 576, 985, 1, -1),
        ("k_dense<4,0,1,0,256,0,0>", "feat", 1, 24, 128, 300, 1, -1),
        ("k_dense<5,0,0,0,256,0,0>", "feat", 1, 2056, 144, 300, 1, -1),
        ("k_dense<5,0,1,0,256,0,0>", "feat", 1, 2056, 160, 300, 1, -1),
        ("k_dense<6,0,1,0,256,0,0>", "feat", 1, 24, 192, 49153, 1, 49153),
        ("k_dense<8,0,1,0,256,0,0>", "feat", 1, 24, 256, 50001, 1, 50001),
        ("k_dense2<2,1,0,0,0,0,0>", "feat", 9, 64, 64, 300, 1, -1),
        ("k_dense2<4,1,0,0,0,0,0>", "feat", 9, 64, 128, 300, 1, -1),
        ("k_dense<2,1,0,0,256,0,0>", "feat", 9, 24, 40, 300, 1, -1),
        ("k_dense<2,1,1,0,256,0,0>", "feat", 9, 32, 64, 300, 1, -1),
        ("k_dense<4,1,0,0,256,0,0>", "feat", 9, 24, 100, 300, 1, -1),
        ("k_dense<4,1,1,0,256,0,0>", "feat", 9, 48, 128, 300, 1, -1),
        ("k_dense<2,0,0,1,256,0,0>", "f32+feat", 1, 24, 40, 300, 1, -1),
        ("k_dense<2,0,1,1,256,0,0>", "f32+feat", 1, 64, 64, 300, 1, -1),
        ("k_dense<4,0,0,1,256,0,0>", "f32+feat", 1, 24, 100, 300, 1, -1),
        ("k_dense<4,0,1,1,256,0,0>", "f32+feat", 1, 64, 128, 300, 1, -1),
        ("k_dense<5,0,0,1,256,0,0>", "f32+feat", 1, 40, 144, 300, 1, -1),
        ("k_dense<5,0,1,1,256,0,0>", "f32+feat", 1, 24, 160, 300, 1, -1),
        ("k_dense<8,0,1,1,256,0,0>", "f32+feat", 1, 24, 256, 98100, 1, -1),
        ("k_dense<2,1,0,1,256,0,0>", "f32+feat", 9, 24, 40, 300, 1, -1),
        ("k_dense<2,1,1,1,256,0,0>", "f32+feat", 9, 32, 64, 300, 1, -1),
        ("k_dense<4,1,0,1,256,0,0>", "f32+feat", 9, 24, 100, 300, 1, -1),
        ("k_dense<4,1,1,1,256,0,0>", "f32+feat", 9, 32, 128, 300, 1, -1),
    ]
    cases = []
    for j, s in enumerate(shapes):      # (j, the shape's number, deals out rows_per_image, the ReLU form and the geometry)
        cases.append(dict(_case(*s, "pm"), rows_per_image=(49, 197)[j % 2], relu=1 if j % 3 == 1 else 2))
        if s[2] == 1:
            cases.append(dict(_case(*s, "ln"), rows_per_image=(197, 49)[j % 2], relu=3))
        for c in cases[-2:]:
            c.setdefault("geom", GEOMS[j % len(GEOMS)] if c["taps"] == 9 else None)
    for i, c in enumerate(cases):
        c["index"] = i
        c["terms"] = (("ln", "gelu", "chan_mask") if c["kind"] == "ln" else
                      ("scale", "residual", "post_sub", "chan_mask") + (("relu_if_neg",) if c["relu"] == 2 else ()) + (("shift_table",) if c["taps"] == 9 else ()))
        c["lists"] = ("a_rows", "out_rows") + (("pix_map",) if c["taps"] == 9 else ())
        # the device-side count (counted cases), or m_cap; the wide-tile cases owe their kernel to the capacity and the hint alone
        c["count"] = min(DEFAULT_COUNT, c["m_cap"]) if c["counted"] else c["m_cap"]
        c["id"] = f"{c['form']}-{c['taps']}-{c['cin']}-{c['cout']}-{c['m_cap']}-{c['counted']}-{c['hint']}-{c['kind']}"
    return cases


CASES = _table()
# One case group per kernel family for the device-side counts 0, 1, 257 and m_cap (ids of CASES)
COUNT_FAMILIES = {"k_dense2 whole": "feat-1-128-128-600-1--1-pm", "k_dense2 ragged": "feat-1-72-40-300-1--1-pm", "k_dense": "feat-1-24-100-300-1--1-ln",
                  "3x3": "feat-9-64-128-300-1--1-pm", "fp32": "f32+feat-1-24-100-300-1--1-pm"}
COUNTS = (0, 1, 257, "m_cap")


def case_by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def plan_line(c):
    """The case as tests/dense_plan_cli.cpp reads it."""
    return f"{c['form']} {c['taps']} {c['cin']} {c['cout']} {c['m_cap']} {c['counted']} {c['hint']} 0"


def applicable_mutants(c):
    """The mistakes that concern a case: it sets the term, and the mistake is not the same function on it by construction (post_sub or the
    residual moved across an activation needs an activation; the Ho / Wo borders differ from the Hi / Wi ones under a stride only)."""
    t = c["terms"]
    out = []
    if "chan_mask" in t:
        out.append("img_from_m")
    if "ln" in t:
        out.append("ln_from_dst")
    if "post_sub" in t and c["relu"] != 0:
        out.append("post_sub_before_act")
    if "post_sub" in t and "chan_mask" in t:
        out.append("mask_before_post_sub")
    if "shift_table" in t:
        out.append("class_from_m")
        if c["geom"][4] > 1:
            out.append("border_from_out")
    if "residual" in t and c["relu"] != 0:
        out.append("residual_after_act")
    if "relu_if_neg" in t:
        out.append("relu_if_neg_le")
    return out


def tolerance(c, ref_max):
    """The GPU bound of a case: the project's op-level bounds of this kernel (see the docstring of tests/test_hip_dense_terms.py)."""
    return 2e-4 if c["kind"] == "ln" else 1e-4 * max(1.0, ref_max)


GARBAGE = {"a_rows": 0x3FFFFFF0, "out_rows": 0x2FFFFFF1, "pix_map": -0x12345677, "relu_if_neg": -0x7FFFFFFF}     # behind the count: never read


def _rand(shape, seed):
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(seed))


def _randn(shape, seed):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


def build_inputs(c, count=None):
    """Deterministic CPU inputs of a case (fp32 / int32 tensors, unpadded) -> dict.  count: the device-side count (default: the case's).
    The lists are m_cap long; their entries behind the count are GARBAGE.  `named_a`: bool [a_total], the A rows that the lists name
    within the count (the others may hold anything).  The keyword arguments of conv_rows_f64 are under "ref"."""
    count = c["count"] if count is None else count
    s = 1000 * (c["index"] + 1)
    taps, cin, cout, m_cap, rpi = c["taps"], c["cin"], c["cout"], c["m_cap"], c["rows_per_image"]
    n_max = m_cap if m_cap <= 1000 else DEFAULT_COUNT          # the largest count the case is ever run with
    assert count <= n_max
    B = n_max // rpi + 2
    out_total = B * rpi
    a_total = n_max + 64 if taps == 1 else 3 * n_max
    g = torch.Generator().manual_seed(s)
    ln = c["kind"] == "ln"
    a = _randn((a_total, cin), s + 1)
    if ln:
        a[: a_total // 4] += 3.0
        gamma, beta = _randn((cin,), s + 2) * 0.2 + 1.0, _randn((cin,), s + 3) * 0.1
        w0, b0 = _randn((cout, cin), s + 4) * (1.0 / cin) ** 0.5, _randn((cout,), s + 5) * 0.1
        wg = w0.double() * gamma.double().view(1, -1)
        w, scale = wg.float().reshape(cout, 1, cin).contiguous(), None
        shift = (w0.double() @ beta.double() + b0.double()).float()
        ln_c1 = wg.sum(1).float()
        ad = a.double()
        ln_stats = torch.stack((ad.mean(1), (ad.var(1, unbiased=False) + 1e-5).rsqrt()), 1).float()
        residual = post_sub = None
    else:
        w = (_randn((cout, taps, cin), s + 4) * (1.0 / (taps * cin)) ** 0.5).contiguous()
        scale = 0.75 + 0.5 * _rand((cout,), s + 2)
        shift = _randn((16, cout), s + 3) * 0.5 if taps == 9 else _randn((cout,), s + 3) * 0.1
        residual = _randn((out_total, cout), s + 5)
        post_sub = 0.5 + _rand((cout,), s + 6)                      # of the size of the activations
        ln_stats = ln_c1 = None
    chan_mask = (_rand((B, cout), s + 7) < 0.5).float()
    chan_mask[1] = 0.0                                               # one image drops every channel
    lst = lambda fill: torch.full((m_cap,), fill, dtype=torch.int32)
    out_rows = lst(GARBAGE["out_rows"])
    out_rows[:n_max] = torch.randperm(out_total, generator=g)[:n_max].to(torch.int32)
    if out_rows[0] // rpi == 1:                                      # (a count of 1 shall not write the all-dropped image alone)
        k = int(torch.nonzero(out_rows[:n_max] // rpi != 1)[0])
        out_rows[[0, k]] = out_rows[[k, 0]]
    if taps == 1:
        a_rows = lst(GARBAGE["a_rows"])
        a_rows[:n_max] = torch.randperm(a_total, generator=g)[:n_max].to(torch.int32)
        a_rows[5:n_max:41] = -1                                      # zero rows
    else:
        a_rows = torch.full((m_cap, 9), GARBAGE["a_rows"], dtype=torch.int32)
        a_rows[:n_max] = torch.randint(-1, a_total, (n_max, 9), generator=g).to(torch.int32)
    pix_map = relu_if_neg = None
    if taps == 9:
        pix_map = lst(GARBAGE["pix_map"])
        pix_map[:n_max] = torch.randint(0, B * c["geom"][2] * c["geom"][3], (n_max,), generator=g).to(torch.int32)
    if c["relu"] == 2:
        relu_if_neg = lst(GARBAGE["relu_if_neg"])
        relu_if_neg[:n_max] = torch.randint(-1, 2, (n_max,), generator=g).to(torch.int32)       # a third exactly 0
    for t, fill in ((out_rows, "out_rows"), (a_rows, "a_rows"), (pix_map, "pix_map"), (relu_if_neg, "relu_if_neg")):
        if t is not None:
            t[count:] = GARBAGE[fill]
    named_a = torch.zeros(a_total, dtype=torch.bool)
    live = a_rows[:count].reshape(-1).long()
    named_a[live[live >= 0]] = True
    ref = dict(taps=taps, a_rows=a_rows, out_rows=out_rows, residual=residual, relu=c["relu"], relu_if_neg=relu_if_neg, post_sub=post_sub,
               chan_mask=chan_mask, rows_per_image=rpi, pix_map=pix_map, geom=c["geom"], ln_stats=ln_stats, ln_c1=ln_c1)
    return dict(a=a, w=w, scale=scale, shift=shift, count=count, out_total=out_total, a_total=a_total, B=B, named_a=named_a, ref=ref)


def reference(c, inp, mutant=None):
    return conv_rows_f64(inp["a"], inp["w"], inp["scale"], inp["shift"], inp["count"], inp["out_total"], mutant=mutant, **inp["ref"])


def poisoned(inp):
    """A copy of the inputs with NaN wherever the contract says nothing is read: A rows and ln_stats rows that the lists do not name within
    the count, residual rows that are no destination.  (The mask row behind the last image and the pad columns belong to the device buffers.)"""
    nan = float("nan")
    p = dict(inp, ref=dict(inp["ref"]))
    p["a"] = torch.where(inp["named_a"].view(-1, 1), inp["a"], torch.full((), nan))
    r = p["ref"]
    if r["ln_stats"] is not None:
        first = r["a_rows"].reshape(-1, r["taps"])[: inp["count"], 0].long()
        named0 = torch.zeros(inp["a_total"], dtype=torch.bool)
        named0[first[first >= 0]] = True
        r["ln_stats"] = torch.where(named0.view(-1, 1), r["ln_stats"], torch.full((), nan))
    if r["residual"] is not None:
        is_dst = torch.zeros(inp["out_total"], dtype=torch.bool)
        is_dst[r["out_rows"][: inp["count"]].long()] = True
        r["residual"] = torch.where(is_dst.view(-1, 1), r["residual"], torch.full((), nan))
    return p
