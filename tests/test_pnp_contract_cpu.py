"""CPU: that tests/pnp_contract.py can fail, and that what it compares against is the reference's arithmetic.

  * the one blend reference is bit-equal to oracle/pnp_ref.py on the shapes both define and to the captures of the reference's own
    processors (tests/golden/*_proc_bg*.npz); the glue references to oracle/loops_ref.py + oracle/sched_ref.py
  * the nearest rule is F.interpolate(mode="nearest") for every size pair 1..96, and the walk holds pairs on which it is not the
    exact quotient
  * the conditions of the walk: work-item totals 255 / 256 / 257 / 513 per item geometry and entry, every pair of factor levels
    per entry, fewer than 1 500 launches per layout, no NaN in a random result, under a quarter of the atlas compared as NaN
  * every mutation of the reference named below trips the walk's own comparison in at least one case (the test says where)
  * every one of the seven + four scalar-product sites of the loop glue is held: rounding that one product once changes at least
    32 elements of a case of the walk"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_contract as PC  # noqa: E402

torch.set_grad_enabled(False)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _same(a, b):
    return np.array_equal(PC.bits(np.asarray(a)), PC.bits(np.asarray(b)))


# ---- the nearest rule --------------------------------------------------------------------------------------------------------------
def test_nearest_rule_is_interpolate_and_not_the_exact_quotient():
    differ = []
    for n_in in range(1, 97):
        src = torch.arange(n_in, dtype=torch.float32)[None, None]
        for n_out in range(1, 97):
            want = F.interpolate(src, size=n_out, mode="nearest")[0, 0].long().numpy()
            assert np.array_equal(PC.near(n_out, n_in), want), (n_in, n_out)
            if PC.float_rule_differs(n_in, n_out):
                differ.append((n_in, n_out))
    assert len(differ) == 74 and {(26, 22), (14, 46), (39, 33), (21, 69), (54, 38)} <= set(differ)
    for g in PC.FLOAT_RULE_GEOMS:  # (F, H, W, mh, mw): one axis of each is such a pair
        assert PC.float_rule_differs(g[3], g[1]) or PC.float_rule_differs(g[4], g[2]), g
    for layout in PC.LAYOUTS:
        for entry in PC.ENTRIES:
            w = PC.walk_cases(layout, entry)
            assert {(c.F, c.H, c.W, c.mh, c.mw) for c in w["index"]} == set(PC.FLOAT_RULE_GEOMS)
            assert all(c.nobj == 1 and c.kind == "index" for c in w["index"])
    # under the index mask the result IS the sampled cell
    c = PC.walk_cases("tokens", "pos")["index"][0]
    out = PC.blend_reference(c)[0, c.c_chunk(0)]
    cells = (1 + np.arange(c.mh * c.mw)).reshape(c.mh, c.mw)
    assert np.array_equal(out[0, :, :, 0].astype(np.int64), cells[PC.near(c.H, c.mh)][:, PC.near(c.W, c.mw)])


# ---- the reference against the oracle and the reference's captures ------------------------------------------------------------------
def _given(layout, X, masks, base, ndst, strides="spatial"):
    """a positional case on given data: X [T][chunk][F][H][W][C], masks [nobj][F][mh][mw]"""
    T, nchunk, Fr, H, W, C = X.shape
    nobj = masks.shape[0]
    c = PC.Case(layout, "pos", (Fr, H, W) + masks.shape[2:], C, nobj, ndst, base, "ident", (1, 1), "none", "given", T == 2, strides)
    assert c.nchunk == nchunk
    c.X, c.masks, c.table, c._built = X, masks[None], None, True
    return c


@pytest.mark.parametrize("bg", [0, 1])
@pytest.mark.parametrize("ndst", [1, 2])
def test_reference_equals_oracle(bg, ndst):
    from oracle import pnp_ref
    rng = np.random.default_rng(3)
    Fr, H, W, C, nobj = 3, 5, 7, 8, 2
    nchunk = nobj + 1 + ndst
    X = rng.standard_normal((2, nchunk, Fr, H, W, C)).astype(PC.F16)
    u8 = rng.integers(0, 256, (nobj, Fr, 10, 14))
    hard, soft = (u8 > 10).astype(PC.F16), (u8.astype(np.float32) / np.float32(255)).astype(PC.F16)
    # spatial Q/K [chunks * F, HW, C], bool masks
    q, k = (_t(X[t].reshape(nchunk * Fr, H * W, C)) for t in (0, 1))
    rq, rk = pnp_ref.inject_qk_spatial(q, k, [_t(m) > 0 for m in hard], Fr, H, W, inject_background=bool(bg), ndst=ndst)
    got = PC.blend_reference(_given("tokens", X, hard, bg, ndst))
    assert _same(got[0].reshape(nchunk * Fr, H * W, C), rq.numpy()) and _same(got[1].reshape(nchunk * Fr, H * W, C), rk.numpy())
    # temporal Q/K [chunks * HW, F, C], soft masks
    to_t = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1, 4)).reshape(nchunk * H * W, Fr, C)
    rq, rk = pnp_ref.inject_qk_temporal(_t(to_t(X[0])), _t(to_t(X[1])), [_t(m) for m in soft], H, W, inject_background=bool(bg), ndst=ndst)
    got = PC.blend_reference(_given("tokens", X, soft, bg, ndst, "temporal"))
    assert _same(to_t(got[0]), rq.numpy()) and _same(to_t(got[1]), rk.numpy())
    if bg:  # features [chunks * F, C, H, W], masks at the features' size, base chunk 0
        to_n = lambda a: np.ascontiguousarray(a.transpose(0, 1, 4, 2, 3)).reshape(nchunk * Fr, C, H, W)
        same_size = hard[:, :, :H, :W]
        ref = pnp_ref.inject_feature_nchw(_t(to_n(X[0])), [_t(m) > 0 for m in same_size], ndst=ndst)
        got = PC.blend_reference(_given("nchw", X[:1], same_size, 1, ndst))
        assert _same(to_n(got[0]), ref.numpy())


@pytest.mark.parametrize("kind", ["g1_spatial", "g2_temporal"])
@pytest.mark.parametrize("bg", [0, 1])
def test_reference_equals_the_captures(golden_dir, kind, bg):
    g = np.load(os.path.join(golden_dir, f"{kind}_proc_bg{bg}.npz"))
    Fr, H, W = int(g["frames"]), int(g["height"]), int(g["width"])
    q, k = g["q_off"][:, 0], g["k_off"][:, 0]
    C = q.shape[-1]
    if kind == "g1_spatial":
        masks = g["mask_bool"][:, 0, 0].astype(PC.F16)
        to_x = lambda a: a.reshape(5, Fr, H, W, C)
        back = lambda a: a.reshape(5 * Fr, H * W, C)
    else:
        masks = g["mask_float"][:, 0, 0].astype(PC.F16)
        to_x = lambda a: np.ascontiguousarray(a.reshape(5, H, W, Fr, C).transpose(0, 3, 1, 2, 4))
        back = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1, 4)).reshape(5 * H * W, Fr, C)
    X = np.stack([to_x(q), to_x(k)])
    got = PC.blend_reference(_given("tokens", X, masks, bg, 2, "spatial" if kind == "g1_spatial" else "temporal"))
    assert _same(back(got[0]), g["q_on"][:, 0]) and _same(back(got[1]), g["k_on"][:, 0])


def test_glue_references_equal_the_oracle():
    from oracle import loops_ref, sched_ref
    from mvoc_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    rng = np.random.default_rng(5)
    n = 4096
    x, vu, vc = (rng.standard_normal(n).astype(PC.F16) for _ in range(3))
    for cls, rcls in ((DDIMScheduler, sched_ref.DDIMSchedulerRef), (DDIMInverseScheduler, sched_ref.DDIMInverseSchedulerRef)):
        s, rs = cls(), rcls()
        s.set_timesteps(50)
        rs.set_timesteps(50)
        for t in (rs.timesteps[0], rs.timesteps[17], rs.timesteps[-1]):
            coef = s.coefficients(int(t), 9.0)
            for cfg in (False, True):
                v = loops_ref.cfg_combine(_t(vu), _t(vc), 9.0) if cfg else _t(vc)
                ref = rs.step(v, t, _t(x)).prev_sample
                assert _same(PC.ddim_reference(x, vu if cfg else None, vc, coef), ref.numpy()), (cls.__name__, int(t), cfg)
    lat, bgl = (rng.standard_normal(n).astype(PC.F16) for _ in range(2))
    objs = rng.standard_normal((2, n)).astype(PC.F16)
    masks = (rng.integers(0, 256, (2, n)).astype(np.float32) / np.float32(255)).astype(PC.F16)
    for ratio in (0.0, 0.8, 0.01, 0.3):
        for rnf in (False, True):
            ref = loops_ref.latent_fusion(_t(lat), _t(bgl), [_t(o) for o in objs], [_t(m) for m in masks], ratio, rnf)
            assert _same(PC.fusion_reference(lat, bgl, objs, masks, ratio, rnf), ref.numpy()), (ratio, rnf)


def test_plane_references():
    src = (1 + np.arange(2 * 3 * 4 * 5)).reshape(2, 3, 4, 5).astype(PC.F16)
    off = np.array([[0, 0], [1, -2], [PC.I32MIN, 0]], np.int32)
    out = PC.shift_planes_reference(src, off)
    assert _same(out[:, 0], src[:, 0]) and not out[:, 2].any()
    want = np.zeros((2, 4, 5), PC.F16)
    want[:, 1:, :3] = src[:, 1, :3, 2:]
    assert _same(out[:, 1], want)
    maps = np.stack([np.concatenate([np.arange(4) - d[0], np.arange(5) - d[1]]) for d in off.astype(np.int64)]).astype(np.int32)
    assert _same(PC.gather_planes_reference(src, maps), out)  # translation maps are the shift


# ---- the conditions of the walk -----------------------------------------------------------------------------------------------------
def test_work_item_totals():
    for layout in PC.LAYOUTS:
        for entry in PC.ENTRIES:
            tot = PC.walk_cases(layout, entry)["totals"]
            groups = {"tokens": [tot]} if layout == "tokens" else {"nchw": [tot[:4], tot[4:]]}
            for grp in groups[layout]:
                got = [c.work_items() for c in grp]
                assert got[:3] == [255, 256, 257] and got[3] >= 513, (layout, entry, got)
            if layout == "nchw":
                assert all((c.H * c.W) % 8 == 0 for c in tot[:4]) and all((c.H * c.W) % 8 for c in tot[4:])
    c = PC.nchw_misaligned_case()
    assert c.H * c.W == 24 and c.lead % 16 == 2 and c.work_items() == c.F * c.C * 24


def test_pairwise_coverage_and_size():
    for layout in PC.LAYOUTS:
        launches = 0
        for entry in PC.ENTRIES:
            names = sorted(PC.factors(layout, entry))
            seen = set()
            for c in PC.walk_cases(layout, entry)["pairs"]:
                assert all(c.fac[a] in PC.factors(layout, entry)[a] for a in names)
                seen |= PC.pairs_of(c.fac, names)
            missing = PC.required_pairs(layout, entry) - seen
            assert not missing, (layout, entry, sorted(map(sorted, missing))[:4])
            launches += len(PC.all_cases(layout, entry))
        print(f"{layout}: {launches} launches")
        assert launches < 1500
    # what BAD_PAIRS leaves out is what cannot be: two objects on one chunk need two objects
    assert PC.BAD_PAIRS == {frozenset({("nobj", 1), ("srcmap", "shared")})}


def _dest(c):
    d = np.zeros((c.T, c.nchunk, c.F, c.H, c.W, c.C), bool)
    d[:, PC.dest_chunks(c)] = True
    return d


def test_nan_share_and_poison():
    atlas_share = []
    for layout in PC.LAYOUTS:
        for entry in PC.ENTRIES:
            for c in PC.all_cases(layout, entry):
                P = PC.pack(c)
                nan_ref = np.isnan(P.expect.view(PC.F16)) & P.dest
                if c.kind == "atlas":
                    atlas_share.append(nan_ref.sum() / P.dest.sum())
                else:
                    assert not nan_ref.any(), c  # on random data no NaN reaches a result
                # everything outside the logical elements is NaN before the call, and so is what the contract does not read
                outside = np.ones(P.feat.size, bool)
                outside[P.offs] = False
                assert (P.feat[outside] == PC.NAN_BITS).all() and outside.sum() >= 2 * PC.GUARD
                X = c.X
                for k in range(c.nvar):
                    if c.nd == 2:
                        assert np.isnan(X[:, c.u_chunk(k)]).all()
                    if c.base == 1 or not c.on(k):
                        assert np.isnan(X[:, c.c_chunk(k)]).all()
                    if c.nm > 1 and not c.on(k):
                        assert np.isnan(c.masks[k]).all() and (P.table[P.t_off:].reshape(-1)[k * c.table[0].size:(k + 1) * c.table[0].size] == PC.I32MIN).all()
                if c.base != 1 and 0 not in c.obj_chunk:
                    assert np.isnan(X[:, 0]).all()
    print(f"atlas: {100 * min(atlas_share):.1f} % .. {100 * max(atlas_share):.1f} % of the destination elements are compared as NaN")
    assert max(atlas_share) < 0.25
    # the atlas is the full cross product, and a select is a different function on it
    c = PC.walk_cases("tokens", "pos")["atlas"][0]
    b, o, m = PC.atlas_values(c)
    combos = {(int(x), int(y), int(z)) for x, y, z in zip(PC.bits(b).ravel(), PC.bits(o).ravel(),
                                                         PC.bits(np.broadcast_to(m[:, :, None], b.shape)).ravel())}
    assert len(combos) == 16 * 16 * 6 == 1536
    ref, sel = PC.blend_reference(c), PC.blend_reference(c, ("select",))
    d = _dest(c) & ~np.isnan(ref)
    share = (PC.bits(ref)[d] != PC.bits(sel)[d]).mean()
    frame = ref[0, c.c_chunk(0), 0]  # frame 0 of the atlas: nothing moved
    pure = np.where(np.broadcast_to(m[:, :, None], b.shape).astype(np.float32) > 0.5, o, b)
    ok = ~np.isnan(frame)
    pure_share = (PC.bits(frame)[ok] != PC.bits(pure)[ok]).mean()
    print(f"atlas: the blend differs from a select in {100 * pure_share:.1f} % of its non-NaN elements, and in {100 * share:.1f} % "
          "from a blend that selects only where the mask is exactly 0 or 1")
    assert pure_share > 0.25 and share > 0.01


# ---- the mutations ------------------------------------------------------------------------------------------------------------------
def _first_trip(mut, entries=PC.ENTRIES, kinds=("atlas", "index", "totals", "pairs")):
    for kind in kinds:
        for layout in PC.LAYOUTS:
            for entry in entries:
                for c in PC.walk_cases(layout, entry)[kind]:
                    ref, got = PC.blend_reference(c), PC.blend_reference(c, (mut,))
                    bad, _ = PC.compare(PC.bits(got), PC.bits(ref), _dest(c))
                    if bad:
                        return kind, c, bad
    return None


BLEND_MUTATIONS = [  # (mutation, entries it can show on, the kind of case that must catch it or None)
    ("near_ceil", PC.ENTRIES, None),
    ("near_exact", PC.ENTRIES, "index"),
    ("reverse_objects", PC.ENTRIES, None),
    ("base_chunk0", PC.ENTRIES, None),
    ("skip_absent", ("placed", "placed_variants", "resampled", "resampled_variants"), "atlas"),
    ("select", PC.ENTRIES, "atlas"),
    ("flush", PC.ENTRIES, "atlas"),
    ("product_plus_zero", PC.ENTRIES, "atlas"),  # what pnp_blend.h says hipcc once made of the float blend behind a select
    ("table0", PC.PER_VARIANT, None),
    ("swap_blocks", PC.ENTRIES[2:], None),
]


@pytest.mark.parametrize("mut,entries,kind", BLEND_MUTATIONS, ids=[m[0] for m in BLEND_MUTATIONS])
def test_blend_mutations_trip(mut, entries, kind):
    """per entry: a mistake in one kernel family must not hide behind another's cases"""
    for entry in entries:
        hit = _first_trip(mut, (entry,), (kind,) if kind else ("atlas", "index", "totals", "pairs"))
        assert hit, f"{mut} passes every {entry} case"
        print(f"{mut} on {entry}: tripped the {hit[0]} case {hit[1]} ({hit[2]} elements)")


def test_near_exact_trips_only_the_float_rule_geometries():
    """no other geometry of the walk could see a nearest rule rewritten in integers: the reason they are in it"""
    for layout in PC.LAYOUTS:
        for c in PC.walk_cases(layout, "sel")["pairs"]:
            if (c.F, c.H, c.W, c.mh, c.mw) not in PC.FLOAT_RULE_GEOMS:
                assert _same(PC.blend_reference(c), PC.blend_reference(c, ("near_exact",)))


# ---- loop glue ------------------------------------------------------------------------------------------------------------------------
def _count(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return int(((PC.bits(a) != PC.bits(b)) & ~(np.isnan(a) & np.isnan(b))).sum())


@pytest.mark.parametrize("site", PC.DDIM_SITES)
def test_every_ddim_product_is_held(site):
    x, vu, vc, coef = PC.ddim_isolating_case(site)
    n = _count(PC.ddim_reference(x, vu, vc, coef), PC.ddim_reference(x, vu, vc, coef, once=(site,)))
    print(f"ddim {site}: rounding it once changes {n} of 65536 elements")
    assert n >= 32
    for other in PC.DDIM_SITES:  # the case isolates the site: no other product's rounding shows in it
        if other != site:
            assert _count(PC.ddim_reference(x, vu, vc, coef), PC.ddim_reference(x, vu, vc, coef, once=(other,))) == 0, other


@pytest.mark.parametrize("site", PC.FUSION_SITES)
def test_every_fusion_product_is_held(site):
    lat, bg, objs, masks, mix, rnf = PC.fusion_isolating_case(site)
    n = _count(PC.fusion_reference(lat, bg, objs, masks, mix, rnf), PC.fusion_reference(lat, bg, objs, masks, mix, rnf, once=(site,)))
    print(f"fusion {site}: rounding it once changes {n} of 65536 elements")
    assert n >= 32


def test_isolating_scalars_come_from_the_search():
    assert PC.flips(PC.S_ISO) >= 32
    for site, mix in PC.MIX_ISO.items():
        scalar = np.float32(mix) if site.startswith("mix") else np.float32(1.0 - mix)
        assert PC.flips(scalar) >= 32, site
    for round_value in (9.0, 0.8, 0.5):  # what the older tests multiply by: no operand flips
        assert PC.flips(round_value) == 0


def test_glue_mutations_trip():
    rows = PC.scheduler_rows()
    assert len(rows) == 6 + len(PC.HAND_ROWS)
    hit = [name for name, nvar, x, vu, vc, coef in PC.ddim_cases(rows)
           if nvar > 1 and _count(PC.ddim_variants_reference(x, vu, vc, coef), PC.ddim_variants_reference(x, vu, vc, coef, row0=True))]
    print(f"coefficient row 0 for every variant: tripped {len(hit)} cases, first {hit[:3]}")
    assert hit
    # the two ways to form 1 - mix differ by an fp32 ulp at some ratios only, and an ulp of the factor shows in few products: the
    # isolating case "omix_form" holds it over all 65 536 operands
    lat, bg, objs, masks, mix, rnf = PC.fusion_isolating_case("omix_form")
    assert np.float32(1.0 - mix) != np.float32(1.0) - np.float32(mix)
    n = _count(PC.fusion_reference(lat, bg, objs, masks, mix, rnf), PC.fusion_reference(lat, bg, objs, masks, mix, rnf, omix_f32=True))
    print(f"1.0f - f32(mix) for f32(1.0 - mix): changes {n} of 65536 elements of the omix_form case")
    assert n >= 32
    # every size, variant count, object count and both fusion switches are in the glue walk
    d = PC.ddim_cases(rows)
    assert {(x.shape[1], nvar, vu is None) for _, nvar, x, vu, vc, _ in d if x.shape[1] < 1024} == \
        {(n, v, u) for n in PC.GLUE_N for v in (0,) + PC.GLUE_NVAR for u in (False, True)}
    f = PC.fusion_cases()
    assert {(lat.shape[1], nvar, len(objs), rnf) for _, nvar, lat, _, objs, _, _, rnf in f if lat.shape[1] < 1024} == \
        {(n, v, o, r) for n in PC.GLUE_N for v in (0,) + PC.GLUE_NVAR for o in (0, 1, 2, 4) for r in (0, 1)}
    kinds = {(len(objs), name.rsplit("_", 1)[1]) for name, _, _, _, objs, _, _, _ in f if name[0] == "n" and len(objs)}
    assert kinds == {(o, k) for o in (1, 2, 4) for k in ("hard", "soft")}
