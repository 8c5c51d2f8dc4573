"""The constructions of the GEMM contract tests (tests/gemm_contract.py) are sound, shown on the CPU with the documented rounding chain
restated in torch (``emulate``) before any kernel is blamed: the walk covers what tests/test_gemm_contract_gpu.py claims, the emulated
chain EQUALS the fp64 answer in sections A and L under two different K orders and sits within the bounds of C and D (D: under half of
each bound, the factor of two being for the accumulation order the emulation cannot know), the layouts poison exactly what their
descriptors do not describe, and each planted defect trips the check that is there to catch it.  Every case goes through the code path of
the GPU tests (gemm_contract.run_case), the kernel replaced by ``emulate_into``."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_contract as GC  # noqa: E402
import launch_census as LC  # noqa: E402
from mvoc_amd._ffi import ACT_GEGLU, ACT_NONE, ACT_SILU  # noqa: E402

CPU = "cpu"
FORCED = ("GENERAL", "GLDS", "G8")


# ---- what the walk covers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FORCED)
def test_walk_coverage(family):
    w = GC.walk(family)
    assert [p["i"] for p in w] == list(range(len(w))) and GC.walk(family) == w  # deterministic
    assert {p["tile"] for p in w} == set(GC.TILES[family])
    plain = [p for p in w if p["mode"] == "plain" and p["split_k"] == 1]
    for tile in GC.TILES[family]:
        mine = [p for p in plain if p["tile"] == tile]
        bn = GC.BN[tile]
        # every K of the family, hence every K-tile count from 1 to the ring depth + 2 (tiles 61 / 62 / 64 step 32: 2, 4, 6, 10)
        assert {p["k"] for p in mine} >= set(GC.FAMILY_K[family]), tile
        nks = {p["k"] // GC.K_STEP[family] for p in mine}
        assert nks >= set(range(1, GC.RING[family] + 3)), (tile, nks)
        # every M, in the exact section, with and without a residual
        a = [p for p in mine if GC.section_of(p) == "A"]
        assert {(p["m"], p["resid"]) for p in a} >= {(m, r) for m in GC.M for r in (False, True)}, tile
        # every N class of the tile's width with every trim
        trims = GC.TRIMS + ((GC.GENERAL_TAIL_TRIM,) if family == "GENERAL" else ())
        assert {(p["n"], p["trim"]) for p in mine if p["act"] != ACT_GEGLU} >= {(n, t) for n in GC.n_classes(bn) for t in trims}, tile
        if family == "GENERAL":
            assert any(GC.cols_of(p) % 4 == 2 for p in mine)
        # every epilogue form with every K
        forms = {(GC.epilogue_name(p), p["k"]) for p in mine}
        for name, e in GC.EPILOGUES:
            if e.get("ln") and family == "GENERAL":
                continue
            q = dict(act=ACT_NONE, bias=False, resid=False, ln=False, rowadd_div=0)
            q.update(e)
            for k in GC.FAMILY_K[family]:
                assert (GC.epilogue_name(q), k) in forms or (e.get("ln") and k % 64), (tile, name, k)
        # row-add divisors; a 256-row tile over five row-add rows
        divs = {p["rowadd_div"] for p in mine if p["m"] == 257}
        assert divs >= ({64, 100, 257} if family == "G8" else {1, 64, 100, 257}), (tile, divs)
        five = [p for p in mine if p.get("five_rows")]
        assert five and all(len({r // p["rowadd_div"] for r in range(256, min(512, p["m"]))}) == 5 for p in five)
        # GEGLU where the tile carries it: multiples of 64, with residual, with the LayerNorm fold
        g = [p for p in mine if p["act"] == ACT_GEGLU]
        if tile in GC.NO_GEGLU:
            assert not g
        else:
            assert {p["n"] for p in g} == set(GC.geglu_n(bn)) and all(p["n"] % 64 == 0 for p in g)
            assert {p["resid"] for p in g} == {False, True} and (family == "GENERAL" or any(p["ln"] for p in g))
        # gathers
        mine_all = [p for p in w if p["tile"] == tile]
        conv = [p for p in mine_all if p["mode"] == "conv" and p["upsample"] != 2 and not p["k_order"]]
        assert {p["geo"] for p in conv if not p["upsample"] and p["c1"] == p["cin"]} >= set(GC.CONV_GEO)
        assert {(p["geo"], p["stride"], p["pad_mode"]) for p in conv} >= {((2, 3, 5), 2, 0), ((3, 9, 7), 2, 0), ((2, 3, 5), 2, 1),
                                                                           ((3, 9, 7), 2, 1), ((5, 8, 8), 2, 1)}
        assert {p["up"] for p in conv if p["upsample"] == 1} == {(11, 7), (16, 16)}
        two = [p for p in mine_all if p["c1"] != p["cin"]]
        assert {p["mode"] for p in two} == {"plain", "conv", "temporal"} and all(p["c1"] != p["cin"] - p["c1"] for p in two)
        assert {(p["c1"], p["cin"] - p["c1"]) for p in two if p["mode"] == "conv"} == {(8, 24) if family == "GENERAL" else (64, 128)}
        if family == "GENERAL":
            assert any(p["cin"] == 8 and p["k"] == 96 for p in conv)
        assert {p["geo"] for p in mine_all if p["mode"] == "temporal" and not p["k_order"]} >= set(GC.TEMPORAL_GEO)
        # split-K
        sp = {(p["split_k"], p["k"] // (64 * p["split_k"])) for p in mine_all if p["split_k"] > 1}
        assert sp >= ({(2, 1), (2, 2), (4, 1), (4, 2)} if family != "GENERAL" else set()), (tile, sp)
    # epilogue forms of launch8, every one on each eight-phase tile that has it
    if family == "G8":
        assert {GC.g8_epi(p) for p in w if p["tile"] == 81} == {0, 1, 2, 3}
        assert {GC.g8_epi(p) for p in w if p["tile"] == 82} == {0, 1, 2}
        assert all(GC.g8_epi(p) == 0 for p in w if p["ln"] and p["rowadd_div"])
        st = [p for p in w if p["chan_sums"] and p["row_moments"] and p["split_k"] == 1]
        for tile in (81, 82):
            assert {(p["m"], p["n"]) for p in st if p["tile"] == tile and p["act"] == ACT_NONE and p["trim"] == 0 and not p["ln"]} >= \
                {(m, n) for m in GC.STATS_M for n in GC.STATS_N} | {(257, 256)}
            assert any(p["tile"] == tile and p["act"] != ACT_NONE for p in st) and any(p["tile"] == tile and p["trim"] for p in st)
        assert any(p["chan_sums"] and p["split_k"] > 1 for p in w)
        sub = [p for p in w if p["upsample"] == 2]
        assert {(p["m"], p["n"]) for p in sub} == {(m, n) for m in (1024, 2048) for n in GC.SUBPIXEL_N} and all(p["tile"] == 81 for p in sub)
        ko = [p for p in w if p["k_order"]]
        assert {(p["mode"], p["cin"], p["resid"]) for p in ko} == {(m, c, r) for m in ("conv", "temporal") for c in (64, 128) for r in (False, True)}
        assert all(p["tile"] == 82 and p["n"] == 320 and 1024 < p["m"] < 1280 and p["m"] % 256 for p in ko)
        assert not any(p["rowadd_div"] and p["rowadd_div"] < 64 for p in w)
    # every placement at least twice
    for p in w:
        assert p["ldo_pad"] in ((0, 8) if (family == "G8") else (0, 4, 8))
    seen = [(p["ldo_pad"], p["ldr_pad"], p["inner"], p["addr"], p["out_addr"]) for p in w]
    for pl in set(GC.placements(family)):
        if family == "G8":
            pl = pl[:4] + (pl[3],)
        assert seen.count(pl) >= 2, pl
    if family != "G8":
        assert sum(1 for p in w if p["ldo_pad"] == 4) >= 2 and sum(1 for p in w if p["out_addr"] == 8) >= 2
    # every gather mode at least twice, every section non-empty where the family has it
    for mode in ("plain", "conv", "temporal"):
        assert sum(1 for p in w if p["mode"] == mode) >= 2
    keys = [GC.case_key(s, p) for s in GC.SECTIONS for p in GC.section_cases(s, family)]
    assert len(set(keys)) == len(keys)


def test_walk_automatic():
    w = GC.walk("AUTO")
    assert all(p["tile"] == 0 for p in w) and [p["i"] for p in w] == list(range(len(w)))
    assert {p["k"] for p in w if p["mode"] == "plain"} >= {32, 64, 96, 128, 192, 256, 320}
    assert {p["m"] for p in w} >= set(GC.M) and {p["mode"] for p in w} == {"plain", "conv", "temporal"}
    low = [p for p in w if p["rowadd_div"] == 1 and p["m"] >= 1024 and p["k"] >= 256]
    assert low, "a row-add divisor below 64 at a shape the eight-phase tiles would take"
    # the forms only the eight-phase tiles carry, reached with tile = 0 as mvoc_amd.ops reaches them
    sub = [p for p in w if p["upsample"] == 2]
    assert {(p["m"], p["n"]) for p in sub} == {(m, n) for m in (1024, 2048) for n in GC.SUBPIXEL_N}
    ko = [p for p in w if p["k_order"]]
    assert {(p["mode"], p["cin"], p["resid"]) for p in ko} == {(m, c, r) for m in ("conv", "temporal") for c in (64, 128) for r in (False, True)}
    assert {p["m"] for p in ko} == {1058, 1026}
    sp = [p for p in w if p.get("expect_split")]
    assert len(sp) == 1 and sp[0]["split_k"] == 0 and sp[0]["workspace"] and sp[0]["k"] == 1024


def test_workload_cap():
    """every launch at most 2 048 rows by 704 columns by K = 1 728 (the two-source conv of the direct-to-LDS and eight-phase tiles,
    9 (64 + 128)); plain launches at most K = 1 024 (the automatic split); a few hundred small cases per GPU test function"""
    for family in GC.FAMILIES:
        w = GC.walk(family)
        for p in w:
            assert p["m"] <= GC.MAX_M and p["n"] <= GC.MAX_N and p["k"] <= GC.MAX_K, p
            assert p["mode"] == "conv" or p["k"] <= 1024
        for tile in GC.TILES[family]:
            for s in GC.SECTIONS:
                cases = GC.section_cases(s, family, tile)
                assert len(cases) <= 300, (family, tile, s, len(cases))  # (a case is a few milliseconds on the GPU)
                assert sum(p["m"] * p["n"] * p["k"] for p in cases) < 4e10


# ---- the emulated chain on every case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", GC.FAMILIES)
@pytest.mark.parametrize("section", GC.SECTIONS)
def test_emulated_chain_meets_every_check(section, family):
    """A, L: equality with the fp64 answer under two K orders; C: within gemm_epilogue's derived bound; D: per 32-row group under HALF
    of the project's bounds -- through run_case, as on the GPU"""
    figures = []
    cases = GC.section_cases(section, family)
    assert cases or (section == "L" and family == "GENERAL")
    for p in cases:
        bits = GC.run_case(section, p, CPU, GC.emulate_into, figures)
        if section in ("A", "L"):
            assert torch.equal(bits, GC.run_case(section, p, CPU, lambda L: GC.emulate_into(L, order=1)))
    if section == "D":
        assert len(figures) == len(cases)
        assert all(worst < 0.5 * lim for _, worst, lim in figures), max(figures, key=lambda f: f[1] / f[2])


# ---- the layout ----------------------------------------------------------------------------------------------------------------------
def _base(**kw):
    out = []
    q = dict(m=129, n=96, k=64, bias=True, resid=True, rowadd_div=64, trim=8)
    q.update(kw)
    p = GC._case(out, q.pop("family", "GLDS"), q.pop("tile", 13), **q)
    p.update(ldo_pad=8, ldr_pad=16, lda_pad=16, inner=True, addr=16, out_addr=16)
    return p


def test_layout_poisons_what_the_descriptor_does_not_describe():
    for p in (_base(), _base(ln=True, bias=False), _base(mode="conv", geo=(3, 9, 7), cin=64, c1=0, k=0, m=0),
              _base(family="G8", tile=81, m=256, n=288, trim=0, chan_sums=True, row_moments=True, split_k=2, workspace=True, k=128)):
        L = GC.GemmLayout(CPU, p)
        L.fill(GC.draw("A", p))
        L.check_poison()
        d = L.desc()
        assert d.a % 16 == 0 and d.w % 16 == 0 and d.out % 256 == 16 + 2 * GC.LEAD % 256
        assert int(L.described("a").sum()) == L.rows_a * p["c1"] and int(L.described("resid").sum()) == p["m"] * L.cols
        assert int(L.described("rowadd").sum()) == -(-p["m"] // 64) * L.cols
        gaps = L.T["resid"].as_strided((p["m"] - 1, L.ldr - L.cols), (L.ldr, 1), L.T["resid"].storage_offset() + L.cols)
        assert bool((gaps.view(torch.int16) == GC.NAN16).all())
        pads = L.T["a"].as_strided((L.rows_a - 1, L.lda - p["c1"]), (L.lda, 1), L.T["a"].storage_offset() + p["c1"])
        assert bool((pads.view(torch.int16) == GC.NAN16).all())
        ext = LC.gemm_extents(d)  # the operands span what launch_census counts, less the last row's padding
        for name in ("w", "bias", "ln_rowsum", "ln_bias", "ln_stats", "workspace"):
            if name in L.T:
                assert L.T[name].numel() == ext[name][0], name
        if "workspace" in L.T:
            assert d.workspace_bytes == 2 * p["m"] * p["n"] * 4
        # a poisoned element that is lost, and a described one that is NaN, are both seen
        L.T["a"].base_alloc[3] = 0.0
        with pytest.raises(AssertionError, match="lost its poison"):
            L.check_poison()
        L.T["a"].base_alloc.view(torch.int16)[3] = GC.NAN16
        L.T["a"][5] = float("nan")
        with pytest.raises(AssertionError, match="described element is NaN"):
            L.check_poison()


def test_padded_conv_k_holds_zeros():
    """k > 9 cin: the weight columns at and past 9 cin are described and zero (include/mvoc_hip.h)"""
    p = _base(family="GENERAL", tile=3, mode="conv", geo=(3, 9, 7), cin=8, c1=0, k=96, m=0, rowadd_div=0)
    L = GC.GemmLayout(CPU, p)
    L.fill(GC.draw("A", p))
    L.check_poison()
    w = L.views["w"](L.T["w"])
    assert w.shape == (96, 96) and bool((w[:, 72:] == 0).all()) and bool((w[:, :72] != 0).any())


# ---- planted defects: each is caught by the check that is there for it ---------------------------------------------------------------
_STATS = dict(family="G8", tile=81, m=256, n=288, k=128, trim=0, chan_sums=True, row_moments=True)
DEFECTS = [
    ("row_copies_neighbour", "A", _base(), "differ from the exact answer"),
    ("last_k_tile_dropped", "A", _base(), "differ from the exact answer"),
    ("rowadd_next_row", "A", _base(m=257), "differ from the exact answer|not finite|are NaN"),
    ("a_padding_column", "A", _base(), "not finite|are NaN"),
    ("resid_row_gap", "A", _base(), "not finite|are NaN"),
    ("bias_past_n", "A", _base(), "not finite|are NaN"),
    ("row_m_written", "A", _base(), "outside the operand's extent|undescribed elements"),
    ("columns_past_n_store", "A", _base(), "undescribed elements"),
    ("stats_when_unhonoured", "A", _base(**dict(_STATS, m=257)), "although the query function answers 0"),
    ("row_moments_padding", "A", _base(**_STATS), "outside the described extent"),
    ("workspace_overrun", "A", _base(split_k=2, workspace=True, k=128), "outside split_k"),
    ("stats_never_honoured", "A", _base(**_STATS), "the header's conditions give"),
    ("stats_never_honoured", "A", _base(m=256, n=128, k=128, trim=0, split_k=2, workspace=True, chan_sums=True), "the header's conditions give"),
    ("input_written", "A", _base(), "bias was written"),
]


@pytest.mark.parametrize("defect,section,p,message", DEFECTS, ids=[f"{i}_{d[0]}" for i, d in enumerate(DEFECTS)])
def test_planted_defect_is_caught(defect, section, p, message):
    GC.run_case(section, p, CPU, GC.emulate_into)  # sound without the defect
    with pytest.raises(AssertionError, match=message):
        GC.run_case(section, p, CPU, lambda L: GC.emulate_into(L, defect=defect))


def test_planted_defects_in_the_other_sections():
    for sec, p in (("C", _base(act=ACT_SILU)), ("C", _base(act=ACT_GEGLU, n=128, rowadd_div=0)), ("D", _base()), ("L", _base(ln=True, bias=False))):
        GC.run_case(sec, p, CPU, GC.emulate_into)
        with pytest.raises(AssertionError):
            GC.run_case(sec, p, CPU, lambda L: GC.emulate_into(L, defect="last_k_tile_dropped"))
        with pytest.raises(AssertionError, match="not finite|are NaN"):
            GC.run_case(sec, p, CPU, lambda L: GC.emulate_into(L, defect="a_padding_column"))


def test_return_codes_are_the_headers():
    p = _base()
    with pytest.raises(AssertionError, match="none of the header's"):
        GC.run_case("A", p, CPU, lambda L: (-9, 0, 0))
    with pytest.raises(AssertionError, match="refused with -2"):
        GC.run_case("A", p, CPU, lambda L: (-2, 0, 0))
