"""The constructions of the xs_linear contract tests (tests/xs_contract.py) are sound, shown on the CPU with the documented rounding
chain restated in torch (``emulate``) before any kernel is blamed: the walk covers what tests/test_xs_contract_gpu.py claims, the
emulated chain EQUALS the fp64 answer in sections A, B and S and sits within the bounds of C and D, the layouts poison exactly what
their descriptors do not describe, and each of nine planted defects trips the check that is there to catch it.  Every case goes
through the code path of the GPU tests (xs_contract.run_case), the kernel replaced by ``emulate_into``."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402
import xs_contract as XC  # noqa: E402
from mvoc_amd._ffi import ACT_GEGLU, ACT_NONE  # noqa: E402

CPU = "cpu"


# ---- what the walk covers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", XC.K)
def test_walk_coverage(k):
    w = XC.walk(k)
    assert [p["i"] for p in w] == list(range(len(w))) and all(p["k"] == k for p in w)
    assert XC.walk(k) == w  # deterministic
    # every (act, residual, normalize) with every T (GEGLU: every n of GEGLU_N, T = 2, 4, 6 stages)
    seen = {(p["act"], p["resid"], p["normalize"], p["n"]) for p in w}
    for act, resid, nm in XC._combos():
        for n in (XC.GEGLU_N if act == ACT_GEGLU else [32 * t for t in XC.T]):
            assert (act, bool(resid), nm, n) in seen, (act, resid, nm, n)
    assert not any(p["act"] == ACT_GEGLU and p["resid"] for p in w)
    # every M with and without residual -- in the exact sections A and B each
    for sec in ("A", "B"):
        assert {(p["m"], p["resid"]) for p in XC.section_cases(sec, k)} >= {(m, r) for m in XC.M for r in (False, True)}, sec
    # every n_store trim with and without residual (GEGLU: its two trims)
    trims = {(p["act"] == ACT_GEGLU, p["trim"], p["resid"]) for p in w}
    assert trims >= {(False, t, r) for t in XC.TRIMS for r in (False, True)} | {(True, t, False) for t in XC.GEGLU_TRIMS}
    for p in w:
        assert p["n_store"] % 8 == 0 and XC.full_cols(p["n"], p["act"]) - 32 < p["n_store"] <= XC.full_cols(p["n"], p["act"])
    # every (ldo, ldr, address) placement with a residual, every (ldo, address) without
    assert {(p["ldo_pad"], p["ldr_pad"], p["addr"]) for p in w if p["resid"]} == set(XC.PLACEMENTS)
    assert {(p["ldo_pad"], p["addr"]) for p in w if not p["resid"]} == {(a, c) for a, _, c in XC.PLACEMENTS}
    # the sections partition the walk by (act, normalize); D takes all of it and the large-offset rows
    a, b, c, d = (XC.section_cases(s, k) for s in "ABCD")
    assert len(a) + len(b) + len(c) == len(w) + 1 and b[-1]["big_mean"] and len(d) == len(w) + 1 and d[-1]["offset"] and d[-1]["m"] == 257
    for sec in ("C", "D"):
        assert {p["m"] for p in XC.section_cases(sec, k)} == set(XC.M), sec
    s = XC.set_cases(k)
    assert {p["m"] for p in s} == {512, 768} and all(p["set_rows"] == 256 for p in s) and {p["resid"] for p in s} == {False, True}
    # the budget: every launch at most 768 rows by 192 columns
    assert all(p["m"] <= 768 and p["n"] <= 192 for p in w + s + d)
    keys = [XC.case_key(sec, p) for sec in XC.SECTIONS for p in XC.section_cases(sec, k)]
    assert len(set(keys)) == len(keys)


# ---- the emulated chain on every case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", XC.K)
@pytest.mark.parametrize("section", XC.SECTIONS)
def test_emulated_chain_meets_every_check(section, k):
    """A, B, S: equality with the fp64 answer (and |ref| < 2048 before the launch); C: within xs_ref's derived bound, and the share of
    |y| <= 8 at least a half; D: per 32-row group within the project's bounds -- asserted inside run_case, as on the GPU"""
    figures = []
    bits = XC.run_sections(k, CPU, XC.emulate_into, sections=(section,), figures=figures)
    assert len(bits) == len(XC.section_cases(section, k))
    if section == "D":
        assert len(figures) == len(bits) and max(f[1] for f in figures) < XC.D_BOUND_LN


def test_balanced_rows_normalise_to_exactly_one_with_the_rsqrt_off():
    """section B's premise: mean and variance exact in fp32, and every normalised value rounds to exactly +-1 in fp16 with the rsqrt off
    by +-2^-20 relative"""
    for k in XC.K:
        x, sign = XC.balanced_rows(XC.gen_of("balanced", k), 257, k)
        assert torch.equal(XC.layernorm_fold(x, XC.EPS), sign)
        xf = x.float()
        mu = xf.mean(1, keepdim=True)
        assert torch.equal(mu, xf.double().mean(1, keepdim=True).float()) and torch.equal(mu, mu.round())
        var = ((xf - mu) ** 2).mean(1, keepdim=True)
        assert torch.equal(var.double(), ((xf.double() - mu.double()) ** 2).mean(1, keepdim=True))
        for off in (1 - 2.0 ** -20, 1 + 2.0 ** -20):
            assert torch.equal(((xf - mu) * (torch.rsqrt(var + XC.EPS) * off)).half().float(), sign)


def test_activation_cases_exercise_the_activations():
    """the shares the constructions give (sparse draws, no LayerNorm): about 0.94 / 0.85 / 0.66 at K = 64 / 128 / 320"""
    for k, lo in zip(XC.K, (0.9, 0.8, 0.6)):
        shares = [XC.draw("C", p)["share"] for p in XC.section_cases("C", k) if not p["normalize"] and p["m"] >= 127]
        assert len(shares) >= 5 and sum(shares) / len(shares) > lo, (k, shares)


# ---- the layout ----------------------------------------------------------------------------------------------------------------------
def _base(**kw):
    p = dict(i=0, k=64, m=129, n=96, act=ACT_NONE, resid=True, normalize=0, trim=8, ldo_pad=8, ldr_pad=16, addr=16, set_rows=0, offset=False, big_mean=False)
    p.update(kw)
    p["n_store"] = XC.full_cols(p["n"], p["act"]) - p["trim"]
    return p


def test_layout_poisons_what_the_descriptor_does_not_describe():
    for p in (_base(), _base(act=ACT_GEGLU, n=128, resid=False, ldo_pad=0, addr=128), _base(m=512, set_rows=256, addr=0, trim=0, ldo_pad=0)):
        L = XC.XsLayout(CPU, p)
        L.fill(XC.draw("A" if p["act"] == ACT_NONE else "C", p))
        L.check_poison()
        d = L.desc()
        assert d.x % 16 == 0 and d.wp % 16 == 0 and d.out % 256 == p["addr"] and (not p["resid"] or d.resid % 256 == p["addr"])
        assert (d.ldo, d.n_store) == ((L.cols + p["ldo_pad"], L.cols) if (p["trim"] or p["ldo_pad"]) else (L.cols, 0))
        # the constants' tails are poison, the constants themselves are the case's; the extents are launch_census.xs_extents'
        ext, cols = LC.xs_extents(d)
        assert L.T["wp"].numel() == ext["wp"][0] and L.T["x"].numel() == ext["x"][0]
        assert int((~L.described("wp")).sum()) - (L.T["wp"].base_alloc.numel() - L.T["wp"].numel()) == 448 * L.nsets * (p["n"] // 32)
        raw = L.T["wp"].view(torch.int16).view(-1, L.nk + 1, 512)
        assert bool((raw[:, L.nk, 64:] == XC.NAN16).all()) and not bool((raw[:, :L.nk] == XC.NAN16).any())
        if p["resid"]:
            assert int(L.described("resid").sum()) == p["m"] * L.cols
            gaps = L.T["resid"].as_strided((p["m"] - 1, p["ldr_pad"]), (L.ldr, 1), L.T["resid"].storage_offset() + L.cols)
            assert bool((gaps.view(torch.int16) == XC.NAN16).all())
        assert bool((L.T["out"].base_alloc.view(torch.int16) == LC.OUT_SENTINEL).all())
        # a poisoned element that is lost, and a described one that is NaN, are both seen
        L.T["x"].base_alloc[3] = 0.0
        with pytest.raises(AssertionError, match="lost its poison"):
            L.check_poison()
        L.T["x"].base_alloc.view(torch.int16)[3] = XC.NAN16
        L.T["x"][5] = float("nan")
        with pytest.raises(AssertionError, match="described element is NaN"):
            L.check_poison()


# ---- planted defects: each is caught by the check that is there for it ---------------------------------------------------------------
DEFECTS = [
    ("row_copies_neighbour", "A", _base(), "differ from the exact answer"),
    ("tiles_swapped", "A", _base(), "differ from the exact answer"),
    ("next_tile_constants", "A", _base(), "differ from the exact answer"),
    ("previous_tile_residual", "A", _base(), "differ from the exact answer"),
    ("row_m_written", "A", _base(), "outside the operand's extent"),
    ("columns_past_n_store", "A", _base(), "undescribed elements"),
    ("constants_tail", "A", _base(), "not finite"),
    ("one_pass_variance", "B", XC.big_mean_case(320), "differ from the exact answer"),
    ("trim_every_tile", "A", _base(), "never written"),
]


@pytest.mark.parametrize("defect,section,p,message", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_is_caught(defect, section, p, message):
    XC.run_case(section, p, CPU, XC.emulate_into)  # sound without the defect
    with pytest.raises(AssertionError, match=message):
        XC.run_case(section, p, CPU, lambda L: XC.emulate_into(L, defect))


def test_planted_defects_at_other_shapes():
    """the same defects where they are hardest to see: a one-row tensor's row m, the last row's columns past n_store (they lie in the
    slack, not in a pitch gap), the tail read with GEGLU and with an activation"""
    with pytest.raises(AssertionError, match="outside the operand's extent"):
        XC.run_case("A", _base(m=1, resid=False), CPU, lambda L: XC.emulate_into(L, "row_m_written"))
    with pytest.raises(AssertionError, match="outside the operand's extent"):
        XC.run_case("A", _base(m=1, ldo_pad=0), CPU, lambda L: XC.emulate_into(L, "columns_past_n_store"))
    for p in (_base(act=ACT_GEGLU, n=128, resid=False), _base(act=XC.ACT_SILU), _base(act=XC.ACT_GELU, resid=False)):
        with pytest.raises(AssertionError, match="not finite|are NaN"):
            XC.run_case("C", p, CPU, lambda L: XC.emulate_into(L, "constants_tail"))
