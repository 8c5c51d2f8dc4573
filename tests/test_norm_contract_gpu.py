"""What include/mvoc_hip.h promises about the seven entries of mvoc_amd/csrc/norm.hip, through the C ABI with hand-filled descriptors, on
constructions whose statistics are known without a reduction (tests/norm_contract.py; shown sound on the CPU by
tests/test_norm_contract_cpu.py), at the shapes where gn_geometry, gn_final_blocks and the inline_final gate change form:

  A  balanced data: moments == (R cpg, b, R cpg a^2) as fp32 values, row means == b, rstd within 2^-21, outputs within one fp16 rounding
     (+ the fp32 term; with SiLU: of either fp16 neighbour of the pre-activation) -- plain, and with one amplitude per row / per slab
  B  random data against fp64 at the project's own bounds, PER SAMPLE (GroupNorm) / per row (LayerNorm)
  C  in EVERY launch of A and B: undescribed input elements are NaN and none reaches a result, every described output element is
     written, nothing around an output is, the workspace (NaN all over before every call) is not written behind
     mvoc_groupnorm_workspace_bytes and its stale contents reach no result
  D  refusals: the code norm.hip returns, an error text that names the entry, nothing written; the unchanged descriptor then succeeds

The bug these tests found (fixed in norm.hip with them): test_groupnorm_fold_xs, constants.  gn_fold_xs_kernel builds a constant's mean
term from "the weight as rounded", but hipcc compiled the two copies of that expression differently: v_pk_mul_f32 + v_cvt_pk_f16_f32 for
the stored weight (fp32, then fp16: two roundings), v_fma_mixlo_f16 for the constant's copy (one rounding).  Where the fp32 product sits
on an fp16 tie (1 element in ~8 000) the constant used the fp16 neighbour of the stored weight: 7.6 / 14.5 / 7.8 times the bound at
c = 64 (R = 512) / 128 / 320, rows and sums route alike; a CPU restatement of the two roundings on the same draws gave 20 flips of 49 152
and 5.5 times the bound at c = 128, R = 512.  Both copies now go through gn_fold_weight, which pins the fp32 rounding: 0.07 at most.

Measured on an MI355X, worst error / bound per family: GroupNorm from rows balanced 0.500 (half an fp16 ulp, as derived), random 0.26
(2049 samples x 2 rows x 8 channels: 0.36); moments, apply_moments' merge: equal; apply_moments outputs 0.500; producer sums balanced
0.500, random 0.26; fold_xs weights 0.500, constants 0.07, consumer 0.20; LayerNorm balanced 0.500, random 0.38 (8 channels) to 0.22;
row_stats and row_stats_from_moments balanced 0.10 (rstd 1e-1 of 2^-21: v_rsq_f32 does better than its ulp), random 0.01 / 0.03.
The whole file, 114 tests: 7.6 s; the slowest test 1.2 s (the first one: library load), the 16-sample 66-slab walk 0.25 s.

That the file can fail (scratch perturbations of norm.hip, one at a time, on a copy, never committed; the tests named are ALL that tripped
among those run against it):
  * r1 clamped to R - 1 in gn_partial (the last row of every sample dropped) -> every test_groupnorm_moments_exact case (count, M2: "0.0 !=
    8.0" at R = 1), every test_groupnorm_rows_balanced case (its first failure: NaN outputs at R = 1), the four
    test_groupnorm_final_block_switch_and_sample_count_clamp cases (moments) and test_groupnorm_fold_xs[*-rows]
  * gn_fold_slab reading slab sl + 1 -> all 11 test_groupnorm_from_producer_sums* cases (the last slab reads the NaN behind the sums:
    "output elements are NaN"; with more samples the neighbour's slab: per-slab amplitudes)
  * gn_apply taking gamma one 8-channel chunk off -> test_groupnorm_rows_balanced, _rows_random_per_sample and _apply_moments_exact at
    every channel count above 8 (error / bound 1e2 .. 1e5)
  * row_stats_from_moments_kernel counting the partial last tile as tile_w -> test_row_stats_from_moments[256 / 320] (mean != b: inf) and
    both refusal cases (whose accepted descriptor has a partial tile)
`lanes` forced to 1 in gn_final is NOT a defect these tests can or should see: every lane count is a valid merge order, and on balanced
data every order returns the same bits.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402
import norm_contract as NC  # noqa: E402
from mvoc_amd._ffi import XsDesc, lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, H16, I16, I32 = torch.float32, torch.float16, torch.int16, torch.int32
_gen = NC.gen_of


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return lib.mvoc_last_error().decode()


def _ids(cg):
    return [f"{c}-{G}" for c, G, _ in cg]


def _need(case):
    need = lib.mvoc_groupnorm_workspace_bytes(case.nsample, case.R, case.c, case.G)
    assert need > 0 and need % 4 == 0
    return need


def _layout(case, **kw):
    return NC.GnLayout(case, DEV, _need(case), **kw)


def run_groupnorm(L, silu, what):
    L.d.silu = silu
    L.reset()
    rc = lib.mvoc_groupnorm_f16(C.byref(L.d), _stream())
    assert rc == 0, (what, _err())
    return L.out(what)


def run_moments(L, what):
    case = L.case
    mom = NC.poisoned32(case.nsample * case.G * 3, DEV)
    L.reset()
    rc = lib.mvoc_groupnorm_moments_f16(C.byref(L.d), mom.data_ptr(), _stream())
    assert rc == 0, (what, _err())
    L.check_workspace(what)
    return NC.check_out32(mom, what)


def check_case(case, what, sums=False):
    """section A or B (+ C) of mvoc_groupnorm_f16 on one case, SiLU off and on: worst error / bound"""
    L = _layout(case, sums=sums)
    worst = 0.0
    for silu in (0, 1):
        r = NC.gn_ratio(case, run_groupnorm(L, silu, what), silu)
        assert r < 1, f"{what} silu {silu}: error / bound = {r:.3f}"
        worst = max(worst, r)
    return worst


def _cases_of(c, G, c1):
    for ns in NC.GN_NSAMPLE:
        for R in NC.gn_rows_list(c):
            yield ns, R


# ---- GroupNorm from the rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,G,c1", NC.GN_CG, ids=_ids(NC.GN_CG))
def test_groupnorm_rows_balanced(c, G, c1):
    worst = 0.0
    for ns, R in _cases_of(c, G, c1):
        for slab_rows in (None, 1):
            case = NC.balanced_gn(ns, R, c, G, _gen("gn", c, G, ns, R, slab_rows), c1, device=DEV, slab_rows=slab_rows)
            worst = max(worst, check_case(case, f"balanced c {c} G {G} nsample {ns} R {R} slab_rows {slab_rows}"))
    print(f"groupnorm rows balanced c {c} G {G}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("c,G,c1", NC.GN_CG + NC.GN_CG_RANDOM, ids=_ids(NC.GN_CG + NC.GN_CG_RANDOM))
def test_groupnorm_rows_random_per_sample(c, G, c1):
    worst = 0.0
    for ns, R in _cases_of(c, G, c1):
        case = NC.random_gn(ns, R, c, G, _gen("gnr", c, G, ns, R), c1, device=DEV)
        worst = max(worst, check_case(case, f"random c {c} G {G} nsample {ns} R {R}"))
    print(f"groupnorm rows random c {c} G {G}: worst error / GN_BOUND {worst:.3f}")


@pytest.mark.parametrize("c,G,c1", NC.GN_CG, ids=_ids(NC.GN_CG))
def test_groupnorm_moments_exact(c, G, c1):
    for ns, R in _cases_of(c, G, c1):
        for slab_rows in (None, 1):
            case = NC.balanced_gn(ns, R, c, G, _gen("gn", c, G, ns, R, slab_rows), c1, device=DEV, slab_rows=slab_rows)
            what = f"moments c {c} G {G} nsample {ns} R {R} slab_rows {slab_rows}"
            NC.assert_moments(run_moments(_layout(case, affine=False, out=False), what), case, what)


@pytest.mark.parametrize("ns,R,c,G", NC.GN_FINAL_EXTRA + NC.GN_WANT_EXTRA, ids=lambda v: str(v))
def test_groupnorm_final_block_switch_and_sample_count_clamp(ns, R, c, G):
    """gn_final on four blocks below 16 samples (more than 64 chunks) and on one from 16; more samples than the chunk budget"""
    what = f"extra {(ns, R, c, G)}"
    for slab_rows in (None, 1):
        case = NC.balanced_gn(ns, R, c, G, _gen("gnx", ns, R, c, G, slab_rows), device=DEV, slab_rows=slab_rows)
        NC.assert_moments(run_moments(_layout(case, affine=False, out=False), what), case, what)
        r = check_case(case, what)
        print(f"{what} balanced: {r:.3f}")
    r = check_case(NC.random_gn(ns, R, c, G, _gen("gnxr", ns, R, c, G), device=DEV), what + " random")
    print(f"{what} random: {r:.3f}")


@pytest.mark.parametrize("c,G,c1", NC.GN_CG, ids=_ids(NC.GN_CG))
def test_groupnorm_apply_moments_exact(c, G, c1):
    """hand-built parts: the balanced rows split over 1, 2, 3 and 8 ranks, one of them with count 0: all means equal, the merge exact"""
    ry = 256 // min(c // 8, 256)
    worst = 0.0
    for R in sorted({4 * ry + 1, 37}):
        case = NC.balanced_gn(3, R, c, G, _gen("ap", c, G, R), c1, device=DEV)
        L = _layout(case)
        for nparts in NC.PARTS:
            what = f"apply_moments c {c} G {G} R {R} nparts {nparts}"
            parts = NC.put(NC.poisoned32(nparts * 3 * G * 3, DEV), NC.split_parts(case, nparts, _gen("split", c, R, nparts)).to(DEV))
            for silu in (0, 1):
                L.d.silu = silu
                L.reset()
                rc = lib.mvoc_groupnorm_apply_moments_f16(C.byref(L.d), parts.data_ptr(), nparts, _stream())
                assert rc == 0, (what, _err())
                out = L.out(what)
                r = NC.gn_out_ratio(case, out, silu)
                assert r < 1, f"{what} silu {silu}: error / bound = {r:.3f}"
                worst = max(worst, r)
                if nparts == 1:  # the header's promise: with one part the pair reproduces mvoc_groupnorm_f16 bit for bit
                    bits = out.view(I16).clone()
                    assert torch.equal(bits, run_groupnorm(L, silu, what).view(I16)), what
    print(f"apply_moments c {c} G {G}: worst error / bound {worst:.3f}")


# ---- GroupNorm from producer sums ----------------------------------------------------------------------------------------------------
def _sums_walk(c, G, c1, nslabs, nsamples):
    worst = {"balanced": 0.0, "random": 0.0}
    for nslab in nslabs:
        for ns in nsamples:
            R = 256 * nslab
            if (c // G) % 2 == 0:
                for slab_rows in (None, 256):
                    case = NC.balanced_gn(ns, R, c, G, _gen("s", c, nslab, ns, slab_rows), c1, device=DEV, slab_rows=slab_rows, unit_rows=256)
                    r = check_case(case, f"sums balanced c {c} G {G} nsample {ns} nslab {nslab} slab_rows {slab_rows}", sums=True)
                    worst["balanced"] = max(worst["balanced"], r)
                    del case
            case = NC.random_gn(ns, R, c, G, _gen("sr", c, nslab, ns), c1, device=DEV)
            worst["random"] = max(worst["random"], check_case(case, f"sums random c {c} G {G} nsample {ns} nslab {nslab}", sums=True))
            del case
    return worst


@pytest.mark.parametrize("c,G,c1", NC.SUMS_CG + NC.SUMS_CG_RANDOM, ids=_ids(NC.SUMS_CG + NC.SUMS_CG_RANDOM))
def test_groupnorm_from_producer_sums(c, G, c1):
    """1 .. 17 slabs: inline_final up to 16 slabs and 48 KB of sums where the groups divide 256, gn_final beyond; the float4 x 5 fold and its
    scalar remainder (cpg 10 / 12 / 40 / 60), cpg 5 and 8 on the scalar fold alone; x and out checked in full"""
    worst = _sums_walk(c, G, c1, NC.SUMS_NSLAB, (1, 3))
    print(f"sums c {c} G {G}: worst error / bound balanced {worst['balanced']:.3f}, random {worst['random']:.3f}")


@pytest.mark.parametrize("ns", NC.SUMS_LONG_NSAMPLE)
@pytest.mark.parametrize("c", NC.SUMS_LONG_C)
def test_groupnorm_from_producer_sums_many_slabs(c, ns):
    """64 / 65 / 66 slabs: gn_final on one block at 64, on four from 65 below 16 samples, on one at 16 samples"""
    worst = _sums_walk(c, 8 if c == 64 else 32, None, NC.SUMS_NSLAB_LONG, (ns,))
    print(f"sums long c {c} nsample {ns}: worst error / bound balanced {worst['balanced']:.3f}, random {worst['random']:.3f}")


# ---- GroupNorm folded into the linear that reads it ----------------------------------------------------------------------------------
def run_xs(x, wp, m, n, k, set_rows, what):
    out = NC.sentinel(m * n, DEV)
    d = XsDesc()
    d.x, d.wp, d.out = x.data_ptr(), wp.data_ptr(), out.data_ptr()
    d.m, d.n, d.k, d.n_store, d.ldo, d.wp_set_rows = m, n, k, n, n, set_rows
    rc = lib.mvoc_xs_linear_f16(C.byref(d), _stream())
    assert rc == 0, (what, _err())
    return NC.check_out16(out, what).reshape(m, n)


@pytest.mark.parametrize("sums", [False, True], ids=["rows", "sums"])
@pytest.mark.parametrize("c,n", NC.FOLD_CN)
def test_groupnorm_fold_xs(c, n, sums):
    ns, G = NC.FOLD_NSAMPLE, NC.FOLD_G
    worst = [0.0, 0.0, 0.0]
    for R in NC.FOLD_R:
        for balanced in (True, False):
            key = ("fold", c, R, balanced)
            case = (NC.balanced_gn if balanced else NC.random_gn)(ns, R, c, G, _gen(*key), device=DEV, eps=1e-6)
            L = _layout(case, sums=sums, out=False)
            gen = _gen("w", *key)
            w = (torch.randn(n, c, generator=gen) / c ** 0.5).to(H16).to(DEV)
            bias = torch.randn(n, generator=gen).to(H16).to(DEV)
            wbuf, bbuf = NC.put(NC.poisoned(n * c, DEV), w), NC.put(NC.poisoned(n, DEV), bias)
            for b, bb in ((bias, bbuf), (None, None)):
                what = f"fold_xs c {c} n {n} R {R} sums {sums} balanced {balanced} bias {b is not None}"
                wp = NC.sentinel(ns * (n // 32) * (c // 16 + 1) * 512, DEV)
                L.reset()
                rc = lib.mvoc_groupnorm_fold_xs_f16(C.byref(L.d), wbuf.data_ptr(), bb.data_ptr() if bb is not None else None, n, c,
                                                    wp.data_ptr(), _stream())
                assert rc == 0, (what, _err())
                L.check_workspace(what)
                assert LC.stray_writes(wp) == 0, what
                sets = [LC.unpack_xs_weights(wp.reshape(ns, -1)[s], n, c) for s in range(ns)]
                wk, ck = torch.stack([s_[0] for s_ in sets]), torch.stack([s_[1] for s_ in sets])
                assert LC.unwritten(wk) == 0 and not bool(torch.isnan(wk).any()) and not bool(torch.isnan(ck).any()), what
                if balanced:
                    wr, cr = NC.fold_ratios(case, w, b, wk, ck)
                    assert wr < 1 and cr < 1, f"{what}: weights {wr:.3f}, constants {cr:.3f} of their bounds"
                    worst[0], worst[1] = max(worst[0], wr), max(worst[1], cr)
                # the consumer on the RAW rows with its sample's set, per sample slice
                out = run_xs(L.T["x"], wp, ns * R, n, c, R, what)
                Lg = {"x": case.x, "gamma": case.gamma, "beta": case.beta, "w": w}
                if b is not None:
                    Lg["bias"] = b
                rel, _ = NC.slice_errors(out.reshape(ns, R, n), LC.gn_fold_ref(L.d, Lg).reshape(ns, R, n), (0,))
                assert rel < NC.FOLD_BOUND, f"{what}: worst sample rel-L2 {rel:.3g}"
                worst[2] = max(worst[2], rel / NC.FOLD_BOUND)
    print(f"fold_xs c {c} sums {sums}: worst error / bound weights {worst[0]:.3f}, constants {worst[1]:.3f}, consumer {worst[2]:.3f}")


# ---- LayerNorm, row statistics -------------------------------------------------------------------------------------------------------
def _row_cases(c, rows):
    yield NC.balanced_rows(rows, c, _gen("ln", c, rows), device=DEV)
    yield NC.random_rows(rows, c, _gen("lnr", c, rows), device=DEV)


@pytest.mark.parametrize("c", NC.LN_C)
def test_layernorm(c):
    worst = {True: 0.0, False: 0.0}
    for rows in NC.LN_ROWS:
        for case in _row_cases(c, rows):
            what = f"layernorm c {c} rows {rows} balanced {case.balanced}"
            x, g, b = (NC.put(NC.poisoned(t.numel(), DEV), t) for t in (case.x, case.gamma, case.beta))
            out = NC.sentinel(rows * c, DEV)
            rc = lib.mvoc_layernorm_f16(x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), rows, c, case.eps, _stream())
            assert rc == 0, (what, _err())
            r = NC.rows_ratio(case, NC.check_out16(out, what))
            assert r < 1, f"{what}: error / bound = {r:.3f}"
            worst[case.balanced] = max(worst[case.balanced], r)
    print(f"layernorm c {c}: worst error / bound balanced {worst[True]:.3f}, random {worst[False]:.3f}")


@pytest.mark.parametrize("c", NC.LN_C)
def test_row_stats(c):
    worst = {True: 0.0, False: 0.0}
    for rows in NC.LN_ROWS:
        for case in _row_cases(c, rows):
            what = f"row_stats c {c} rows {rows} balanced {case.balanced}"
            x = NC.put(NC.poisoned(rows * c, DEV), case.x)
            st = NC.poisoned32(rows * 2, DEV)
            rc = lib.mvoc_row_stats_f16(x.data_ptr(), st.data_ptr(), rows, c, case.eps, _stream())
            assert rc == 0, (what, _err())
            r = NC.stats_ratio(case, NC.check_out32(st, what))
            assert r < 1 if case.balanced else r <= 1, f"{what}: error / bound = {r:.3f}"
            worst[case.balanced] = max(worst[case.balanced], r)
    print(f"row_stats c {c}: worst error / bound balanced {worst[True]:.3f}, random {worst[False]:.3f}")


@pytest.mark.parametrize("tile_w", NC.TILE_W)
def test_row_stats_from_moments(tile_w):
    worst = {True: 0.0, False: 0.0}
    for n in NC.TILE_N:
        tiles = len(NC.tile_counts(n, tile_w))
        for ld in (tiles, tiles + 3):
            for rows in NC.TILE_ROWS:
                key = (n, tile_w, ld, rows)
                for case in (NC.balanced_tiles(rows, n, tile_w, ld, _gen("tile", *key), device=DEV),
                             NC.random_tiles(rows, n, tile_w, ld, _gen("tiler", *key), device=DEV)):
                    what = f"row_stats_from_moments {key} balanced {case.balanced}"
                    mom = NC.put(NC.poisoned32(rows * ld * 2, DEV), case.mom)  # the unused entries of a row are NaN as well
                    st = NC.poisoned32(rows * 2, DEV)
                    rc = lib.mvoc_row_stats_from_moments_f32(mom.data_ptr(), rows, ld, n, tile_w, case.eps, st.data_ptr(), _stream())
                    assert rc == 0, (what, _err())
                    r = NC.stats_ratio(case, NC.check_out32(st, what))
                    assert r < 1 if case.balanced else r <= 1, f"{what}: error / bound = {r:.3f}"
                    worst[case.balanced] = max(worst[case.balanced], r)
    print(f"row_stats_from_moments tile_w {tile_w}: worst error / bound balanced {worst[True]:.3f}, random {worst[False]:.3f}")


# ---- D: refusals ---------------------------------------------------------------------------------------------------------------------
def _set(**kw):
    def change(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return change


def _short_workspace(d):
    d.workspace_bytes = d.workspace_bytes - 1


def _untouched16(*bufs):
    torch.cuda.synchronize()
    return all(bool((b.base_alloc.view(I16) == LC.OUT_SENTINEL).all()) for b in bufs)


def _untouched32(*bufs):
    torch.cuda.synchronize()
    return all(bool((b.base_alloc.view(I32) == NC.NAN32).all()) for b in bufs)


def _rows_layout():
    return _layout(NC.balanced_gn(2, 37, 192, 24, _gen("refuse"), 128, device=DEV))


def _sums_layout():
    return _layout(NC.balanced_gn(1, 256, 1920, 32, _gen("refuse sums"), 960, device=DEV, unit_rows=256), sums=True)


GN_REFUSALS = [
    ("c 12", _rows_layout, _set(c=12, c1=12, groups=1, x2=None), -2),
    ("c 2568", _rows_layout, _set(c=2568, c1=2568, groups=24, x2=None), -2),
    ("groups 0", _rows_layout, _set(groups=0), -2),
    ("groups 257", _rows_layout, _set(groups=257), -2),
    ("c % groups != 0", _rows_layout, _set(groups=7), -2),
    ("c1 < c without x2", _rows_layout, _set(x2=None), -1),
    ("nsample 65536", _rows_layout, _set(nsample=65536), -2),
    ("workspace one byte short", _rows_layout, _short_workspace, -1),
    ("chan_sums with R 255", _sums_layout, _set(rows_per_sample=255), -2),
    ("chan_sums without chan_sums2", _sums_layout, _set(chan_sums2=None), -2),
    ("chan_sums with c1 % cpg != 0", _sums_layout, _set(c1=1280), -2),
]


@pytest.mark.parametrize("what,make,change,code", GN_REFUSALS, ids=[r[0].replace(" ", "_") for r in GN_REFUSALS])
def test_groupnorm_refusals(what, make, change, code):
    L = make()
    d = LC.copy_desc(L.d)
    change(d)
    L.reset()
    assert lib.mvoc_groupnorm_f16(C.byref(d), _stream()) == code, (what, _err())
    assert "groupnorm" in _err(), _err()
    assert _untouched16(L.T["out"]) and _untouched32(L.T["workspace"]), what
    r = NC.gn_out_ratio(L.case, run_groupnorm(L, 0, what), 0)  # the unchanged descriptor is accepted
    assert r < 1, (what, r)


@pytest.mark.parametrize("what,kw,code", [("x2 set", dict(x2=True), -2), ("k != c", dict(k=128), -2), ("n 48", dict(n=48), -2)],
                         ids=["x2_set", "k_ne_c", "n_48"])
def test_fold_xs_refusals(what, kw, code):
    c, n, R, ns = 64, 64, 256, 2
    case = NC.balanced_gn(ns, R, c, 32, _gen("refuse fold"), device=DEV)
    L = _layout(case, out=False)
    w = NC.put(NC.poisoned(n * c, DEV), (torch.randn(n, c, generator=_gen("refuse w")) / 8).to(H16).to(DEV))
    wp = NC.sentinel(ns * (n // 32) * (c // 16 + 1) * 512, DEV)
    d = LC.copy_desc(L.d)
    if kw.get("x2"):
        d.x2 = L.T["x"].data_ptr()
    L.reset()
    rc = lib.mvoc_groupnorm_fold_xs_f16(C.byref(d), w.data_ptr(), None, kw.get("n", n), kw.get("k", c), wp.data_ptr(), _stream())
    assert rc == code, (what, _err())
    assert "groupnorm_fold_xs" in _err(), _err()
    assert _untouched16(wp) and _untouched32(L.T["workspace"]), what
    assert lib.mvoc_groupnorm_fold_xs_f16(C.byref(L.d), w.data_ptr(), None, n, c, wp.data_ptr(), _stream()) == 0, _err()
    sets = [LC.unpack_xs_weights(wp.reshape(ns, -1)[s], n, c) for s in range(ns)]
    wr, cr = NC.fold_ratios(case, w.reshape(n, c), None, torch.stack([s_[0] for s_ in sets]), torch.stack([s_[1] for s_ in sets]))
    assert wr < 1 and cr < 1, (wr, cr)


@pytest.mark.parametrize("c", [4, 2056])
def test_layernorm_and_row_stats_refusals(c):
    rows = 5
    case = NC.balanced_rows(rows, 64, _gen("refuse ln"), device=DEV)
    x, g, b = (NC.put(NC.poisoned(t.numel(), DEV), t) for t in (case.x, case.gamma, case.beta))
    out, st = NC.sentinel(rows * 64, DEV), NC.poisoned32(rows * 2, DEV)
    assert lib.mvoc_layernorm_f16(x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), rows, c, case.eps, _stream()) == -2, _err()
    assert "layernorm" in _err(), _err()
    assert lib.mvoc_row_stats_f16(x.data_ptr(), st.data_ptr(), rows, c, case.eps, _stream()) == -1, _err()
    assert "row_stats" in _err(), _err()
    assert _untouched16(out) and _untouched32(st)
    assert lib.mvoc_layernorm_f16(x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), rows, 64, case.eps, _stream()) == 0, _err()
    assert lib.mvoc_row_stats_f16(x.data_ptr(), st.data_ptr(), rows, 64, case.eps, _stream()) == 0, _err()
    assert NC.rows_ratio(case, NC.check_out16(out, "layernorm")) < 1 and NC.stats_ratio(case, NC.check_out32(st, "row_stats")) < 1


@pytest.mark.parametrize("what,tile_w,ld_off", [("tile_w 128", 128, 0), ("ld one short", 256, -1)], ids=["tile_w_128", "ld_short"])
def test_row_stats_from_moments_refusals(what, tile_w, ld_off):
    rows, n = 5, 640
    case = NC.balanced_tiles(rows, n, 256, 3, _gen("refuse tiles"), device=DEV)
    mom, st = NC.put(NC.poisoned32(rows * 3 * 2, DEV), case.mom), NC.poisoned32(rows * 2, DEV)
    ld = -(-n // tile_w) + ld_off if tile_w == 256 else 5
    assert lib.mvoc_row_stats_from_moments_f32(mom.data_ptr(), rows, ld, n, tile_w, case.eps, st.data_ptr(), _stream()) == -1, (what, _err())
    assert "row_stats_from_moments" in _err(), _err()
    assert _untouched32(st), what
    assert lib.mvoc_row_stats_from_moments_f32(mom.data_ptr(), rows, 3, n, 256, case.eps, st.data_ptr(), _stream()) == 0, _err()
    assert NC.stats_ratio(case, NC.check_out32(st, what)) < 1
