"""CPU checks of the case table that tests/test_hip_dense_terms.py runs on the GPU (tests/dense_rows_ref.py): every kernel of LDN_DENSE_KERNELS
that carries the optional epilogue terms is reached by a case with those terms set, and the inputs of every case tell each of eight
plausible mistakes of the epilogue from the contract by far more than the GPU bound.  No GPU."""
import os
import subprocess

import pytest
import torch

import dense_rows_ref as R
from test_dense_plan import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dense_rows_ref") / "dense_plan_cli")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "dense_plan_cli.cpp"), "-o", exe], check=True)
    return exe


def _chosen(cli, lines):
    got = subprocess.run([cli], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(lines)
    return [ln.rsplit(" ", 1)[1] for ln in got]


def test_every_case_reaches_the_kernel_it_names(cli):
    for c, k in zip(R.CASES, _chosen(cli, [R.plan_line(c) for c in R.CASES])):
        assert k == c["kernel"], (c["id"], k)


def test_every_term_carrying_kernel_is_reached_with_its_terms_set(cli):
    """The carrying kernels, derived from the chooser itself: whatever a `feat` or `f32+feat` shape of the sweep grid of tests/dense_plan_cli.cpp,
    or of the table, reaches.  Each is reached by a case with post_sub + chan_mask; with taps == 1 also by one with the LayerNorm fold and by one
    with the GELU; with taps == 9 the post_sub + chan_mask case carries the shift table too.  15 bf16x3 1x1, 6 bf16x3 3x3 and 11 fp32 kernels."""
    cins, couts = (24, 32, 40, 64, 72, 136, 144, 256, 320, 512, 784, 1024, 2048, 2056, 2112), (32, 40, 64, 96, 100, 128, 144, 160, 168, 192, 216, 256, 320, 384, 512, 784, 1024, 2048)
    grid = [f"{form} {taps} {cin} {cout} {cap} {counted} {hint} 0" for form in ("feat", "f32+feat") for taps in (1, 9) for cin in cins for cout in couts
            for cap in (1, 256, 300, 3136, 12544, 50176, 200704, 802816) for counted in (0, 1) for hint in ((-1, 0, 100, cap // 2, 2 * cap) if counted else (-1,))]
    carrying = set(_chosen(cli, grid)) | {c["kernel"] for c in R.CASES}
    assert not [k for k in carrying if k.endswith(("?", "UNBUILT"))], "the chooser names an unbuilt kernel for a shape with a term set"
    bf1 = {k for k in carrying if k.startswith("k_dense2<") and k.split(",")[1] == "0" or k.startswith("k_dense<") and k.split(",")[1] == "0" and k.split(",")[3] == "0"}
    bf9 = {k for k in carrying if k.split(",")[1] == "1" and (k.startswith("k_dense2<") or k.split(",")[3] == "0")}
    f32 = {k for k in carrying if k.startswith("k_dense<") and k.split(",")[3] == "1"}
    assert (len(bf1), len(bf9), len(f32)) == (15, 6, 11) and len(carrying) == 32, sorted(carrying)
    for k in sorted(carrying):
        mine = [c for c in R.CASES if c["kernel"] == k]
        t9 = k.split(",")[1] == "1"
        assert any({"post_sub", "chan_mask"} <= set(c["terms"]) and (not t9 or "shift_table" in c["terms"]) for c in mine), f"{k}: no case with post_sub + chan_mask"
        if not t9:
            assert any("ln" in c["terms"] for c in mine) and any("gelu" in c["terms"] for c in mine), f"{k}: no case with the LayerNorm fold / the GELU"


def test_the_table_holds_what_makes_the_mistakes_visible():
    assert {c["rows_per_image"] for c in R.CASES} == {49, 197}
    geoms = {c["geom"] for c in R.CASES if c["taps"] == 9}
    assert any(g[4] == 2 and g[0] % 2 == 0 for g in geoms) and any(g[4] == 2 and g[0] % 2 == 1 for g in geoms) and all(g[0] != g[1] and g[2] != g[3] for g in geoms)
    for fam in ("k_dense2<", "k_dense<"):
        assert {c["relu"] for c in R.CASES if c["kernel"].startswith(fam) and c["kind"] == "pm"} == {1, 2}
    assert all(R.case_by_id(cid)["m_cap"] <= 1000 and R.case_by_id(cid)["counted"] for cid in R.COUNT_FAMILIES.values())
    for cid in R.COUNT_FAMILIES.values():      # a count of 1 writes one row with kept and dropped channels; a count of 0 writes nothing
        c = R.case_by_id(cid)
        ref, written = R.reference(c, R.build_inputs(c, 1))
        assert written.sum() == c["cout"] and (ref[written] == 0).any() and ref[written].abs().max() > 0.1
        assert not R.reference(c, R.build_inputs(c, 0))[1].any()


@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_inputs_tell_every_mistake_from_the_contract(c):
    """Each mistake that concerns the case moves more than 1 % of the written cells by more than 100 x the GPU bound; and the case's lists are
    what they claim: a true scatter permutation into a taller buffer, a gather that differs from it, a pix_map that is no identity, a mask that
    drops about half the channels and one whole image, relu_if_neg entries exactly 0, a post_sub of the size of the activations.  The reference
    itself reads nothing that the contract says is not read: NaN there changes no bit of it."""
    inp = R.build_inputs(c)
    n, r = inp["count"], inp["ref"]
    ref, written = R.reference(c, inp)
    assert written.any() and torch.isfinite(ref[written]).all() and torch.isnan(ref[~written]).all()
    ref_p, written_p = R.reference(c, R.poisoned(inp))
    assert torch.equal(written, written_p) and torch.equal(ref[written], ref_p[written])
    dst, m = r["out_rows"][:n].long(), torch.arange(n)
    assert dst.unique().numel() == n and inp["out_total"] > n and (dst != m).float().mean() > 0.9 and int(dst.max()) < inp["out_total"]
    assert (dst // c["rows_per_image"] != m // c["rows_per_image"]).float().mean() > 0.5
    src0 = r["a_rows"].reshape(-1, c["taps"])[:n, 0].long()
    assert (src0 != dst).float().mean() > 0.9 and (src0 != m).float().mean() > 0.9 and (c["taps"] == 9 or (src0 < 0).any())
    cm = r["chan_mask"]
    assert cm[1].sum() == 0 and 0.35 < cm[[0] + list(range(2, inp["B"]))].mean() < 0.65 and set(dst.div(c["rows_per_image"], rounding_mode="floor").tolist()) >= {0, 1, 2}
    if c["taps"] == 9:
        pm = r["pix_map"][:n].long()
        assert (pm != m).float().mean() > 0.9 and R.border_class(pm, c["geom"]).unique().numel() == (4 if c["geom"][4] == 2 and c["geom"][0] % 2 == 0 else 9)      # (an even map under stride 2 has no bottom / right border)
    if c["relu"] == 2:
        assert 0.2 < (r["relu_if_neg"][:n] == 0).float().mean() < 0.5 and (r["relu_if_neg"][:n] < 0).any() and (r["relu_if_neg"][:n] > 0).any()
    if r["post_sub"] is not None:
        assert 0.2 < r["post_sub"].mean() / ref[written].abs().mean().clamp(min=1e-9) < 20
    tol = R.tolerance(c, ref[written].abs().max().item())
    muts = R.applicable_mutants(c)
    assert len(muts) >= 2
    for mut in muts:
        got, w2 = R.reference(c, inp, mutant=mut)
        assert torch.equal(w2, written)
        frac = ((got[written] - ref[written]).abs() > 100 * tol).float().mean().item()
        assert frac > 0.01, f"{mut}: only {frac:.4f} of the written cells move by more than 100 x the bound {tol:.2e}"


def test_every_mistake_is_exercised_by_some_case_of_every_family():
    """Each of the eight mistakes concerns at least one case; the term-specific ones concern every case that sets the term (only a stride-1
    geometry cannot tell the Ho / Wo borders, and a case without an activation cannot tell the order around it: the table has no such case
    among those with post_sub or a residual)."""
    seen = {m for c in R.CASES for m in R.applicable_mutants(c)}
    assert seen == set(R.MUTANTS)
    for c in R.CASES:
        if "post_sub" in c["terms"] or "residual" in c["terms"]:
            assert c["relu"] != 0
    assert sum(c["taps"] == 9 and c["geom"][4] == 2 for c in R.CASES) >= 6
