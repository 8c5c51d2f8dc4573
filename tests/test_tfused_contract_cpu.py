"""The fused temporal QKV-attention contract set (tests/tfused_contract.py) shown sound without a GPU:

  * the constructions' expectations are integers / exact means, re-derived in fp64 from the folded weights the product's packers made;
  * the undamaged CPU model of tfused.hip's rounding chain meets sections A, B and L on EVERY case the GPU file runs (and the issue's eight
    (B, u) pairs also with the mean one fp32 ulp off either way), and section R's bound on the inexact edges;
  * every named defect of the model fails a stated list of cases -- asserted, not printed; the one-pass variance at each of the three C;
  * section R's per-(sample, head) figure: tfused_contract.MODEL_HEAD_FIGURE = (9.08e-4 rel-L2, 5.20e-3 max abs) is the model's worst
    over all 666 cases of section R against fp64; HEAD_BOUND is twice that.  test_model_random_figures recomputes it over every case
    with hw <= 9 (which holds the worst slices: the fewer rows a slice has, the worse its rel-L2) and at hw 33.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_contract as AC  # noqa: E402
import launch_census as LC  # noqa: E402
import tfused_contract as TC  # noqa: E402

F64 = torch.float64


def test_geometry_covers_the_block_edges_of_both_forms():
    for frames in TC.FRAMES:
        hws = TC.hw_list(frames)
        assert set((1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33)) <= set(hws)
        for waves in (4, 8):
            ppb = TC.pixels_per_block(frames, waves)
            assert {ppb - 1, ppb, ppb + 1, 2 * ppb + 1} <= set(hws) | {0}, (frames, waves)
            assert max(hws) > 2 * ppb  # three blocks
    geos = TC.geometries()
    assert {g[1:] for g in geos} == {(c, f, hw, ns) for c in TC.C_ALL for f in TC.FRAMES for hw in TC.hw_list(f) for ns in TC.NSAMPLE}
    assert max(g[2] * g[3] * g[4] for g in geos) <= 4096  # a case is a few thousand rows at the most
    L = TC.section_geometries("L")
    assert {g[1:4] for g in L} == {g[1:4] for g in geos} and {g[4] for g in L} == set(TC.NSAMPLE)
    assert {g[0] % 6 for g in L} == set(range(6))  # every variant of the weights


def test_walsh_rows_are_balanced_and_orthogonal():
    w = TC.WALSH[32:]
    assert torch.equal(w @ w.t(), 64 * torch.eye(32, dtype=F64)) and not bool(w.sum(1).any())
    assert not bool((w @ TC.WALSH[1]).any())  # beta's pattern is orthogonal to every code


@pytest.mark.parametrize("c", TC.C_ALL)
def test_constructions_are_exact_in_fp64(c):
    """from the FOLDED weights (Linear.fold_layernorm's w_ln / ln_bias), a LayerNorm without eps and an argmax instead of a softmax: q
    and k are +-a one-hot rows, the only non-zero score of a query within its pixel is a^2 against frame sigma(f), v is an integer row,
    and the case's expectation is the selected v row; the uniform case's is the frame mean, a multiple of 1 / F"""
    for frames in TC.FRAMES:
        for geo in (g for g in TC.geometries() if g[1] == c and g[2] == frames and g[3] == 9):
            for case in (TC.exact_case(geo, TC.PAIRS[0]), TC.exact_case(geo, (1023, 2), large=True), TC.uniform_case(geo)):
                i, _, _, hw, ns = geo
                W = case["W"]
                x = case["x"].to(F64)
                xc = x - x.mean(-1, keepdim=True)
                xh = xc / (xc * xc).mean(-1, keepdim=True).sqrt()
                assert torch.equal(xh, case["xhat"])
                qkv = xh @ W["lin"].w_ln[:3 * c].to(F64).t() + W["ln_bias"][:3 * c].to(F64)
                assert torch.equal(qkv, qkv.round()) and float(qkv.abs().max()) < 2048
                q, k, v = (qkv[..., j * c:(j + 1) * c].reshape(ns, frames, hw, c // 64, 64) for j in range(3))
                s = torch.einsum("nfphd,ngphd->nphfg", q, k)
                if case["check"] == "ulp":
                    assert not bool(s.any())
                    assert torch.equal(case["exp"], v.mean(1, keepdim=True).expand_as(v).reshape(ns, frames, hw, c))
                    continue
                a = W["a"]
                assert torch.equal(s.sum(-1), torch.full_like(s.sum(-1), a * a)) and torch.equal((s != 0).sum(-1), torch.ones_like(s.sum(-1), dtype=torch.long))
                sel = s.argmax(-1)                                                      # [n, p, h, f]
                for hd in range(c // 64):
                    assert torch.equal(sel[:, :, hd], W["sigmas"][hd].expand(ns, hw, frames))
                got = torch.gather(v.permute(0, 2, 3, 1, 4), 3, sel[..., None].expand(ns, hw, c // 64, frames, 64))
                assert torch.equal(got.permute(0, 3, 1, 2, 4).reshape(ns, frames, hw, c), case["exp"])


def test_weights_use_every_permutation_kind_and_both_tiles():
    for c in TC.C_ALL:
        kinds, spread = set(), False
        for variant in range(6):
            W = TC.exact_weights(c, 8, variant, TC.A_SMALL[c])
            for sg, place in zip(W["sigmas"], W["places"]):
                ident, rev = torch.equal(sg, torch.arange(8)), torch.equal(sg, torch.arange(7, -1, -1))
                kinds.add("identity" if ident else "reversal" if rev else "random")
                spread |= bool((place >= 32).any()) and bool((place < 32).any())
            assert set(W["gamma"].tolist()) == {0.5, 1.0, 2.0}
        assert kinds == {"identity", "reversal", "random"} and spread


@pytest.mark.parametrize("c", TC.C_ALL)
@pytest.mark.parametrize("section", TC.EXACT_SECTIONS)
def test_model_meets_every_case(section, c):
    keys = set()
    for case in TC.section_cases(section, c):
        ref = TC.fp64_reference(case) if case["check"] == "random" else None
        why = TC.failure(case, TC.emulate(case), ref, AC.TFUSED_BOUND)
        assert why is None, why
        keys.add(case["key"])
    per_geo = {"A": 2, "B": 2, "L": len(TC.L_PAIRS) + 2}[section]
    assert len(keys) == per_geo * len(TC.section_geometries(section, c))  # the keys are distinct: the forced forms are compared by key


@pytest.mark.parametrize("c", TC.C_ALL)
def test_model_is_exact_with_the_mean_one_ulp_off(c):
    """the issue's eight pairs do not hang on the last bit of the mean (a division that is not correctly rounded, another order of
    the sum); DM2_PAIR does, by its construction, and is left out here"""
    for geo in (g for g in TC.geometries() if g[1] == c and g[3] == 17 and g[4] == 1):
        for pair in TC.PAIRS:
            case = TC.exact_case(geo, pair, section="L")
            for ulps in (-1, 1):
                why = TC.failure(case, TC.emulate(case, mean_ulps=ulps))
                assert why is None, (ulps, why)


# ---- the unfused twin --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.C_ALL)
def test_unfused_chain_model_meets_the_twin_check_and_cannot_be_bit_exact(c):
    """the documented arithmetic of row_stats -> folded GEMM -> temporal attention, in fp32 torch, on every exact case of A and L: it
    meets twin_failure's element-wise demand, and at every (B, u) pair but (8192, 32) it misses plain equality (the residue delta t where the
    normalised term and the constant cancel): the reason the GPU file holds the chain to twin_failure and not to torch.equal"""
    missed, share = set(), 1.0
    for section in ("A", "L"):
        for case in TC.section_cases(section, c):
            if case["check"] != "equal":
                continue
            out = TC.emulate_unfused(case)
            why = TC.twin_failure(case, out)
            assert why is None, why
            if TC.failure(case, out) is not None:
                missed.add(case["pair"])
            share = min(share, TC.twin_exact_share(case))
    assert missed == set(TC.L_PAIRS) - {(8192, 32)}  # whose delta = 2e-8 is below fp32's resolution: eps vanishes in 256 + eps
    assert share > 0.85  # the integer itself is due on at least this share of any case's elements (0.88 at u = 0.5, 0.97 and more elsewhere)


def test_twin_check_catches_a_wrong_selection():
    geo = next(g for g in TC.geometries() if g[1:] == (128, 16, 9, 3))
    case = TC.exact_case(geo, (0, 0.5), section="L")
    out = TC.emulate_unfused(case)
    assert TC.twin_failure(case, out) is None
    assert TC.twin_failure(case, out.flip(1)) is not None          # frames reversed
    assert TC.twin_failure(case, out.roll(1, 2)) is not None       # pixels shifted
    bumped = out.clone()
    bumped[1, 3, 4, 70] += 1                                       # one element off by one
    assert TC.twin_failure(case, bumped) is not None


# ---- defects -------------------------------------------------------------------------------------------------------------------------
PROBE = ("A", "A2C", "B", "L1023", "Ldm2", "L8192")   # six cases at one geometry per c (8 frames, hw >= 9, the weights' variant 5)
EXACT = ("A", "A2C", "L1023", "Ldm2", "L8192")
CAUGHT = {  # defect -> c -> the probe cases that must fail (every other probe case must pass)
    # (1024, 1) has the squares 2^20 and 2^20 + 2^11 + 1: a one-pass sum loses the ones as well
    "one_pass_variance": {64: ("L1023", "Ldm2"), 128: ("L1023", "Ldm2"), 320: ("L1023", "Ldm2", "L8192")},
    "dm2_dropped": {c: ("Ldm2",) for c in TC.C_ALL},
    "no_max_subtraction": {c: EXACT for c in TC.C_ALL},   # a = 16: exp2(46) overflows the fp16 probabilities; a = 2 C: fp32 itself
    "mask_dropped": {c: PROBE for c in TC.C_ALL},
    "qk_swapped": {c: EXACT for c in TC.C_ALL},
    "row0_q1": {c: EXACT for c in TC.C_ALL},
    "row0_k1": {c: EXACT for c in TC.C_ALL},
    "row0_v1": {c: PROBE for c in TC.C_ALL},
    "head_values_swapped": {64: (), 128: PROBE, 320: PROBE},   # one head at c = 64: nothing to swap
    "sigma_ignored": {c: EXACT for c in TC.C_ALL},
}


def probe_cases(c):
    geo = next(g for g in TC.geometries() if g[1] == c and g[2] == 8 and g[3] >= 9 and g[0] % 6 == 5)
    return dict(zip(PROBE, (TC.exact_case(geo, TC.PAIRS[0]), TC.exact_case(geo, TC.PAIRS[0], large=True), TC.uniform_case(geo),
                            TC.exact_case(geo, (1023, 2), section="L"), TC.exact_case(geo, TC.DM2_PAIR, section="L"),
                            TC.exact_case(geo, (8192, 32), section="L"))))


def test_every_defect_has_its_list():
    assert set(CAUGHT) == set(TC.DEFECTS)
    assert all(any(CAUGHT[d][c] for c in TC.C_ALL) for d in TC.DEFECTS)


@pytest.mark.parametrize("defect", TC.DEFECTS)
def test_defect_fails_exactly_its_cases(defect):
    for c in TC.C_ALL:
        cases = probe_cases(c)
        assert all(TC.failure(case, TC.emulate(case)) is None for case in cases.values())
        failed = tuple(name for name, case in cases.items() if TC.failure(case, TC.emulate(case, defect)) is not None)
        assert failed == CAUGHT[defect][c], (defect, c, failed)


def test_one_pass_variance_misses_at_each_c():
    """which (B, u) a one-pass fp32 E[x^2] - mean^2 gets wrong: (1023, 2) at every C; the dyadic pairs only at C = 320 (with a
    power-of-two C the one-pass sums of two-valued dyadic rows stay exact)"""
    big = ((512, 2), (1024, 4), (-2048, 8), (8192, 32))
    for c in TC.C_ALL:
        missed = tuple(p for p in TC.PAIRS if TC.one_pass_misses(c, p))
        assert missed == ((big if c == 320 else ()) + ((1023, 2),)), (c, missed)
        geo = next(g for g in TC.section_geometries("L", c) if g[3] == 9)
        case = TC.exact_case(geo, (1023, 2), section="L")
        assert TC.failure(case, TC.emulate(case, "one_pass_variance")) is not None
        assert TC.failure(case, TC.emulate(case)) is None


# ---- the packers, against the header's description --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.C_ALL)
def test_unpack_inverts_the_products_packer(c):
    W = TC.random_weights(c, 8, 0)
    assert torch.equal(TC.unpack(W["wp"], c), W["lin"].w_ln[:3 * c])
    assert not torch.equal(TC.unpack(W["wp"], c, "row0_v1"), W["lin"].w_ln[:3 * c])


# ---- section R's figure ----------------------------------------------------------------------------------------------------------------
def test_model_random_figures():
    """MODEL_HEAD_FIGURE was measured over all of section R; here: every case with hw <= 9 or hw = 33.  The model stays at or below the
    recorded figure, reaches 85 % of it (the figure is no loose guess), and the bound is twice the figure"""
    cases = (TC.random_case(g, dist) for g in TC.geometries() if g[3] <= 9 or g[3] == 33 for dist in TC.DISTRIBUTIONS)
    rel, mab = TC.model_figures(cases)
    print(f"CPU model against fp64, section R: worst (sample, head) rel-L2 {rel:.3e}, max abs {mab:.3e}")
    assert rel <= TC.MODEL_HEAD_FIGURE[0] * 1.0005 and mab <= TC.MODEL_HEAD_FIGURE[1] * 1.0005
    assert rel >= 0.85 * TC.MODEL_HEAD_FIGURE[0] and mab >= 0.85 * TC.MODEL_HEAD_FIGURE[1]
    assert TC.HEAD_BOUND == (2 * TC.MODEL_HEAD_FIGURE[0], 2 * TC.MODEL_HEAD_FIGURE[1])
    assert TC.HEAD_BOUND[0] < AC.TFUSED_BOUND[0] and TC.HEAD_BOUND[1] < AC.TFUSED_BOUND[1]  # per head is no looser than per sample


def test_layout_describes_what_the_header_says():
    """section D on the CPU: NaN everywhere outside the described elements, the addresses walk 0 / 16 / 128 (and 4 for the fp32 vectors)"""
    seen, seen_ln = set(), set()
    for geo in TC.geometries()[:12]:
        L = TC.TFLayout("cpu", TC.zero_rows_case(geo))
        L.check_poison()
        assert L.untouched()
        d = L.desc()
        seen |= {d.x % 256, d.wp % 256, d.out % 256}
        seen_ln |= {d.ln_rowsum % 256, d.ln_bias % 256}
        assert L.T["x"].numel() == geo[2] * geo[3] * geo[4] * geo[1] and L.T["wp"].numel() == 3 * geo[1] ** 2
        assert LC.unwritten(L.T["out"]) == L.T["out"].numel() and LC.stray_writes(L.T["out"]) == 0
    assert seen == set(TC.ADDR) and seen_ln == set(TC.LN_ADDR)


# ---- the host entry's refusals need no GPU: they return before anything is launched -------------------------------------------------------
@pytest.mark.parametrize("field,nbytes", [("x", 8), ("x", 2), ("wp", 8), ("out", 8), ("ln_rowsum", 2), ("ln_bias", 2), ("nsample", 0)])
def test_host_entry_refuses_before_any_launch(field, nbytes):
    import ctypes as C
    from mvoc_amd._ffi import lib
    L = TC.TFLayout("cpu", TC.zero_rows_case(TC.geometries()[0]))
    d = L.desc()
    if field == "nsample":
        d.nsample = 65536
    else:
        setattr(d, field, getattr(d, field) + nbytes)
    assert lib.mvoc_temporal_qkv_attn_f16(C.byref(d), None) == -2
    assert "temporal_qkv_attn" in lib.mvoc_last_error().decode()
    assert L.untouched()
