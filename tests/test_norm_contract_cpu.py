"""The constructions of the norm contract tests (tests/norm_contract.py) are sound: shown on the CPU, with the documented fp32 chains
restated in torch (``emulate_*``: one-pass chunk moments with random chunk cuts and a random element order, the Chan merge in a random
order, the slab fold, sc / sh, the r16-then-SiLU step, two-pass row statistics, the tile merge), before any kernel is blamed.  Over the
lists tests/test_norm_contract_gpu.py launches, every construction meets its bound on the emulation alone: balanced moments equal
(R cpg, b, R cpg a^2) as fp32 values, row means equal b, rstd within 2^-21, outputs within ulp16 + the fp32 term (SiLU: of either
neighbour).  Then defects are planted one at a time and the checkers must fail.

Truncated for time (the emulation has none of the host geometry these sizes exist for): rows_per_sample 300 runs at channel counts up to
320 and as 45 rows above; the gn_final block-switch cases (15 / 16 samples x 300 x 1280) run with 45 rows; producer sums run with at most
3 slabs from 1280 channels up; the 64 / 65 / 66-slab cases run at 64 channels with one sample.

What a checker can and cannot see is part of the record: on the plain balanced construction every set of whole rows of a group has the
same mean and variance, so a dropped row or a skipped slab shows in the moments (count and M2) and in NO output; the output checker sees
them on the variant with one amplitude per row / per slab (``slab_rows``).  Each defect is therefore asserted against every checker that
can see it, and the one blind spot is asserted too."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402
import norm_contract as NC  # noqa: E402

F32, F64, H16 = torch.float32, torch.float64, torch.float16
_gen = NC.gen_of


def _cpu_rows(R, c):
    return 45 if R == 300 and c > 320 else R


def _gn_emulated(case, gen, silu, sums=False, **defect):
    """(moments, output) of the emulated chain of a case"""
    stat_kw = {k: v for k, v in defect.items() if k in ("drop_last", "take_next", "chan_shift", "skip")}
    app_kw = {k: v for k, v in defect.items() if k in ("gamma_shift", "sample_shift")}
    if sums:
        cs = LC.chan_sums64(case.x).to(F32).reshape(case.nsample, case.R // 256, case.c, 2)
        mom = NC.emulate_moments_sums(cs, case.G, gen, **stat_kw)
    else:
        mom = NC.emulate_moments_rows(case.x, case.nsample, case.R, case.G, gen, **stat_kw)
    mean, rstd = NC.finalize32(mom, case.eps)
    return mom, NC.emulate_apply(case.x, mean, rstd, case.gamma, case.beta, case.R, silu, **app_kw)


def _check_balanced(case, gen, what, sums=False):
    worst = 0.0
    for silu in (0, 1):
        mom, out = _gn_emulated(case, gen, silu, sums)
        NC.assert_moments(mom, case, what)
        r = NC.gn_out_ratio(case, out, silu)
        assert r < 1, f"{what} silu {silu}: error / bound {r:.3f}"
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("c,G,c1", NC.GN_CG, ids=[f"{c}-{G}" for c, G, _ in NC.GN_CG])
def test_balanced_groupnorm_from_rows_is_exact(c, G, c1):
    for ns in NC.GN_NSAMPLE:
        for R in NC.gn_rows_list(c):
            R = _cpu_rows(R, c)
            for slab_rows in (None, 1):
                case = NC.balanced_gn(ns, R, c, G, _gen("gn", c, G, ns, R, slab_rows), c1, slab_rows=slab_rows)
                _check_balanced(case, _gen("emu", c, G, ns, R), f"c {c} G {G} nsample {ns} R {R} slab_rows {slab_rows}")


@pytest.mark.parametrize("ns,R,c,G", NC.GN_FINAL_EXTRA + NC.GN_WANT_EXTRA, ids=lambda v: str(v))
def test_balanced_groupnorm_extra_cases_are_exact(ns, R, c, G):
    case = NC.balanced_gn(ns, _cpu_rows(R, c), c, G, _gen("gnx", ns, R, c, G))
    _check_balanced(case, _gen("emux", ns, R), f"extra {(ns, R, c, G)}")


@pytest.mark.parametrize("c,G,c1", NC.GN_CG + NC.GN_CG_RANDOM, ids=[f"{c}-{G}" for c, G, _ in NC.GN_CG + NC.GN_CG_RANDOM])
def test_random_groupnorm_from_rows_meets_the_project_bound_per_sample(c, G, c1):
    for R in NC.gn_rows_list(c):
        R = _cpu_rows(R, c)
        case = NC.random_gn(3, R, c, G, _gen("gnr", c, G, R), c1)
        for silu in (0, 1):
            _, out = _gn_emulated(case, _gen("emur", c, R), silu)
            r = NC.gn_random_ratio(case, out, silu)
            assert r < 1, f"random c {c} G {G} R {R} silu {silu}: {r:.3f} of GN_BOUND"


def _cpu_nslab(nslab, c):
    return min(nslab, 3) if c >= 1280 else nslab


@pytest.mark.parametrize("c,G,c1", NC.SUMS_CG + NC.SUMS_CG_RANDOM, ids=[f"{c}-{G}" for c, G, _ in NC.SUMS_CG + NC.SUMS_CG_RANDOM])
def test_groupnorm_from_producer_sums(c, G, c1):
    long_ = NC.SUMS_NSLAB_LONG if c == 64 else ()
    for nslab in sorted({_cpu_nslab(n, c) for n in NC.SUMS_NSLAB}) + list(long_):
        ns = 1 if nslab >= 15 else 3
        R = 256 * nslab
        if (c // G) % 2:
            case = NC.random_gn(ns, R, c, G, _gen("sr", c, nslab), c1)
            _, out = _gn_emulated(case, _gen("emusr", c, nslab), 1, sums=True)
            assert NC.gn_random_ratio(case, out, 1) < 1
            continue
        for slab_rows in (None, 256):
            case = NC.balanced_gn(ns, R, c, G, _gen("s", c, nslab, slab_rows), c1, slab_rows=slab_rows, unit_rows=256)
            _check_balanced(case, _gen("emus", c, nslab), f"sums c {c} G {G} nslab {nslab} slab_rows {slab_rows}", sums=True)


def test_split_parts_merge_exactly():
    """mvoc_groupnorm_apply_moments_f16's input: the parts of a balanced sample merge to the sample's moments bit for bit, in index order,
    with a part of count 0 among them"""
    case = NC.balanced_gn(3, 37, 64, 8, _gen("parts"))
    for nparts in NC.PARTS:
        for trial in range(4):
            parts = NC.split_parts(case, nparts, _gen("split", nparts, trial))
            assert nparts == 1 or int((parts[:, 0, 0, 0] == 0).sum()) >= 1
            acc = tuple(torch.zeros(3, 8) for _ in range(3))
            for p in range(nparts):
                acc = NC.chan_merge32(acc, parts[p, ..., 0], parts[p, ..., 1], parts[p, ..., 2])
            NC.assert_moments(torch.stack(acc, -1), case, f"nparts {nparts}")


@pytest.mark.parametrize("c,n", NC.FOLD_CN)
def test_folded_weights_and_constants_meet_their_bounds(c, n):
    for R in NC.FOLD_R:
        case = NC.balanced_gn(NC.FOLD_NSAMPLE, R, c, NC.FOLD_G, _gen("fold", c, R), eps=1e-6)
        gen = _gen("foldw", c, R)
        w = (torch.randn(n, c, generator=gen) / c ** 0.5).to(H16)
        bias = torch.randn(n, generator=gen).to(H16)
        mom = NC.emulate_moments_rows(case.x, case.nsample, R, case.G, gen)
        mean, rstd = NC.finalize32(mom, case.eps)
        for b in (bias, None):
            wk, ck = NC.emulate_fold(w, b, case.gamma, case.beta, mean, rstd, case.cpg)
            wr, cr = NC.fold_ratios(case, w, b, wk, ck)
            assert wr < 1 and cr < 1, (c, R, wr, cr)
            # a weight scaled with the statistics of the previous sample is seen
            wk2, ck2 = NC.emulate_fold(w, b, case.gamma, case.beta, torch.roll(mean, 1, 0), torch.roll(rstd, 1, 0), case.cpg)
            wr2, cr2 = NC.fold_ratios(case, w, b, wk2, ck2)
            assert wr2 >= 1 and cr2 >= 1, (c, R, wr2, cr2)


@pytest.mark.parametrize("c", NC.LN_C)
def test_layernorm_and_row_statistics(c):
    for rows in NC.LN_ROWS:
        rows = min(rows, 129)  # 1001 rows exist for the grid, which the emulation does not have
        gen = _gen("emuln", c, rows)
        case = NC.balanced_rows(rows, c, _gen("ln", c, rows))
        st = torch.stack(NC.emulate_row_stats(case.x, case.eps, gen), 1)
        assert NC.stats_ratio(case, st) < 1
        assert NC.rows_ratio(case, NC.emulate_layernorm(case.x, case.gamma, case.beta, case.eps, gen)) < 1
        case = NC.random_rows(rows, c, _gen("lnr", c, rows))
        assert NC.stats_ratio(case, torch.stack(NC.emulate_row_stats(case.x, case.eps, gen), 1)) <= 1
        assert NC.rows_ratio(case, NC.emulate_layernorm(case.x, case.gamma, case.beta, case.eps, gen)) < 1
        if c > 8:  # a row's statistics without its last 8 channels are seen (balanced: only where the dropped chunk is unbalanced)
            short = torch.stack(NC.emulate_row_stats(case.x[:, :-8], case.eps, gen), 1)
            assert NC.stats_ratio(case, short) > 1


@pytest.mark.parametrize("tile_w", NC.TILE_W)
def test_row_statistics_from_tile_moments(tile_w):
    for n in NC.TILE_N:
        tiles = len(NC.tile_counts(n, tile_w))
        for ld in (tiles, tiles + 3):
            for rows in (1, 9):
                case = NC.balanced_tiles(rows, n, tile_w, ld, _gen("tile", n, tile_w, ld, rows))
                assert bool(torch.isnan(case.mom[:, tiles:]).all()) and not bool(torch.isnan(case.mom[:, :tiles]).any())
                assert NC.stats_ratio(case, NC.emulate_tiles(case.mom, n, tile_w, case.eps)) < 1
                rcase = NC.random_tiles(rows, n, tile_w, ld, _gen("tiler", n, tile_w, ld, rows))
                assert NC.stats_ratio(rcase, NC.emulate_tiles(rcase.mom, n, tile_w, rcase.eps)) <= 1
                if n % tile_w:  # defect: the partial last tile counted as a whole one
                    assert NC.stats_ratio(case, NC.emulate_tiles(case.mom, n, tile_w, case.eps, full_last=True)) > 1
                    assert NC.stats_ratio(rcase, NC.emulate_tiles(rcase.mom, n, tile_w, rcase.eps, full_last=True)) > 1


# ---- planted defects -------------------------------------------------------------------------------------------------------------------
def _moments_fail(mom, case):
    try:
        NC.assert_moments(mom, case, "defect")
    except AssertionError:
        return True
    return False


DEFECT_SHAPES = ((64, 8, None), (192, 24, 128), (320, 32, None))


@pytest.mark.parametrize("c,G,c1", DEFECT_SHAPES, ids=[f"{c}-{G}" for c, G, _ in DEFECT_SHAPES])
def test_row_set_defects_are_seen(c, G, c1):
    ns, R = 3, 37
    plain = NC.balanced_gn(ns, R, c, G, _gen("d", c), c1)
    per_row = NC.balanced_gn(ns, R, c, G, _gen("dv", c), c1, slab_rows=1)
    gen = _gen("demu", c)
    # the last row of a sample dropped from the statistics: count and M2 on both constructions, outputs on the per-row amplitudes only
    for case in (plain, per_row):
        mom, out = _gn_emulated(case, gen, 0, drop_last=True)
        assert _moments_fail(mom, case)
        assert (NC.gn_out_ratio(case, out, 0) >= 1) == (case is per_row)
    # the first row of the next sample included; a group boundary shifted by 8 channels
    for defect in ({"take_next": True}, {"chan_shift": 8}):
        for silu in (0, 1):
            mom, out = _gn_emulated(plain, gen, silu, **defect)
            assert _moments_fail(mom, plain), defect
            assert NC.gn_out_ratio(plain, out, silu) >= 1, defect


@pytest.mark.parametrize("c,G,c1", DEFECT_SHAPES, ids=[f"{c}-{G}" for c, G, _ in DEFECT_SHAPES])
def test_apply_defects_are_seen_by_both_classes(c, G, c1):
    """sample s normalised with the statistics of sample s - 1; gamma indexed 8 channels off: the balanced checker and the per-sample random
    checker both fail"""
    ns, R = 3, 37
    gen = _gen("aemu", c)
    for defect in ({"sample_shift": 1}, {"gamma_shift": 8}):
        for silu in (0, 1):
            case = NC.balanced_gn(ns, R, c, G, _gen("a", c), c1)
            assert NC.gn_out_ratio(case, _gn_emulated(case, gen, silu, **defect)[1], silu) >= 1, defect
            case = NC.random_gn(ns, R, c, G, _gen("ar", c), c1)
            assert NC.gn_random_ratio(case, _gn_emulated(case, gen, silu)[1], silu) < 1
            assert NC.gn_random_ratio(case, _gn_emulated(case, gen, silu, **defect)[1], silu) >= 1, defect


def test_second_source_taken_from_the_first_is_seen():
    """x2's channels read from x (the concat's wrong source): statistics and outputs of the groups behind c1 change"""
    c, G, c1 = 192, 24, 128
    case = NC.balanced_gn(3, 37, c, G, _gen("x2"), c1)
    wrong = torch.cat([case.x[:, :c1], case.x[:, :c - c1]], 1)
    gen = _gen("x2emu")
    mom = NC.emulate_moments_rows(wrong, 3, 37, G, gen)
    assert _moments_fail(mom, case)
    mean, rstd = NC.finalize32(mom, case.eps)
    for silu in (0, 1):
        assert NC.gn_out_ratio(case, NC.emulate_apply(wrong, mean, rstd, case.gamma, case.beta, 37, silu), silu) >= 1
    rcase = NC.random_gn(3, 37, c, G, _gen("x2r"), c1)
    wrong = torch.cat([rcase.x[:, :c1], rcase.x[:, :c - c1]], 1)
    mean, rstd = NC.finalize32(NC.emulate_moments_rows(wrong, 3, 37, G, gen), rcase.eps)
    assert NC.gn_random_ratio(rcase, NC.emulate_apply(wrong, mean, rstd, rcase.gamma, rcase.beta, 37, 0), 0) >= 1


@pytest.mark.parametrize("nslab", [2, 5, 17])
def test_a_skipped_slab_is_seen(nslab):
    """producer sums have no moments output: the per-slab amplitudes make a skipped slab visible in the outputs (every slab tried); the
    plain construction cannot see it, which is asserted as well"""
    c, G = 64, 8
    gen = _gen("skipemu", nslab)
    plain = NC.balanced_gn(1, 256 * nslab, c, G, _gen("skip", nslab), unit_rows=256)
    varied = NC.balanced_gn(1, 256 * nslab, c, G, _gen("skipv", nslab), slab_rows=256, unit_rows=256)
    for skip in range(nslab):
        mom, out = _gn_emulated(plain, gen, 0, sums=True, skip=skip)
        assert _moments_fail(mom, plain) and NC.gn_out_ratio(plain, out, 0) < 1
        mom, out = _gn_emulated(varied, gen, 0, sums=True, skip=skip)
        assert _moments_fail(mom, varied) and NC.gn_out_ratio(varied, out, 0) >= 1, skip


def test_layout_poisons_what_the_descriptor_does_not_describe():
    case = NC.balanced_gn(2, 256, 192, 24, _gen("layout"), 128)
    L = NC.GnLayout(case, "cpu", 4096, sums=True)
    for name, t in L.T.items():
        base = t.base_alloc
        off = (t.data_ptr() - base.data_ptr()) // base.element_size()
        outside = torch.cat([base[:off], base[off + t.numel():]])
        assert outside.numel() >= 4096 and bool(torch.isnan(outside).all()), name  # (a 256-byte aligned GPU allocation has 128 bytes in front too)
        if name not in ("out", "workspace"):
            assert not bool(torch.isnan(t).any()), name
    assert L.T["x"].numel() == 2 * 256 * 128 and L.T["x2"].numel() == 2 * 256 * 64 and L.T["chan_sums2"].numel() == 2 * 64 * 2
    assert L.T["workspace"].numel() * 4 == 4096 + NC.WS_EXCESS and bool(torch.isnan(L.T["workspace"]).all())
    assert NC.intact32(L.T["workspace"], 1024) == 0
    L.T["workspace"][1024] = 0.0
    assert NC.intact32(L.T["workspace"], 1024) == 1
