"""CPU: bilinear sampling of warped objects on an exact fp16 chain -- everything that needs no kernel.

* the rule ``ops.level_warp_taps`` (Python ints) against an independent ``fractions.Fraction`` evaluation of the same coordinates;
  weights 0 with the nearest map's pixel for the identity, integer translations and quarter turns; the 2 x 2 mean of scale 1/2 and
  the 64 / 192 pattern of scale 2; the vectorised int64 form against the Python ints, and the bound that decides between them.
* the packed device form and its builders.
* the resolver under ``interp="bilinear"``, the engine attribute ``warp_filter`` and the blend functions' fourth table keyword.
* the drivers' parsing, and that the new entries are declared, exported and bound.
"""
import itertools
import math
import os
import re
import sys
import types
from fractions import Fraction

import pytest
import torch

from test_warp_cpu import GRIDS, _diagonal_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 65536
ROT = [(56756, 32768), (46341, 46341), (0, D), (-D, 0), (63303, -16962)]


def _fraction_taps(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw):
    """the rule restated with rationals: the destination pixel centre in latent units relative to the anchor, moved back by the
    level's offset, through the inverse matrix, back to this level; minus half a pixel; floor and round-half-up of the rest"""
    from mvoc_amd import ops
    myy, myx, mxy, mxx = m
    dfy, dfx = ops.level_offset(dy, H, Lh), ops.level_offset(dx, W, Lw)
    out = []
    for iy in range(H):
        uy = Fraction(2 * (iy - dfy) + 1, 2) * Fraction(Lh, H) - Fraction(ay2, 2)  # latent rows from the anchor
        for ix in range(W):
            ux = Fraction(2 * (ix - dfx) + 1, 2) * Fraction(Lw, W) - Fraction(ax2, 2)
            sy = (Fraction(ay2, 2) + (myy * uy + myx * ux) / den) * Fraction(H, Lh) - Fraction(1, 2)
            sx = (Fraction(ax2, 2) + (mxy * uy + mxx * ux) / den) * Fraction(W, Lw) - Fraction(1, 2)
            y0, x0 = math.floor(sy), math.floor(sx)
            out.append((y0, x0, math.floor((sy - y0) * 256 + Fraction(1, 2)), math.floor((sx - x0) * 256 + Fraction(1, 2))))
    return out


def _cases(step):
    """every ``step``-th diagonal case of tests/test_warp_cpu.py (its grid list), under a rotation that changes with it"""
    for i, ((Lh, Lw), (H, W), (py, qy, px, qx), (fy, fx), (ay2, ax2), (dy, dx)) in enumerate(_diagonal_cases()):
        if i % step:
            continue
        c, s = ROT[(i // step) % len(ROT)]
        gy, gx = (-1 if fy else 1) * qy * px, (-1 if fx else 1) * qx * py
        yield (dy, dx, (gy * c, gy * s, -gx * s, gx * c), py * px * D, ay2, ax2, H, W, Lh, Lw)


def test_the_rule_equals_a_fraction_evaluation_of_the_same_coordinates():
    from mvoc_amd import ops
    n, grids = 0, set()
    for args in _cases(11):
        got = ops.level_warp_taps(*args, form="py")
        assert got == _fraction_taps(*args), args
        assert all(0 <= qy <= 256 and 0 <= qx <= 256 for _, _, qy, qx in got)
        grids.add((args[8:], args[6:8]))
        n += 1
    assert n > 100 and grids == set(GRIDS)
    # the diagonal cases themselves (no rotation), every 13th
    for i, ((Lh, Lw), (H, W), (py, qy, px, qx), (fy, fx), (ay2, ax2), (dy, dx)) in enumerate(_diagonal_cases()):
        if i % 13 == 0:
            args = (dy, dx, ((-1 if fy else 1) * qy * px, 0, 0, (-1 if fx else 1) * qx * py), py * px, ay2, ax2, H, W, Lh, Lw)
            assert ops.level_warp_taps(*args, form="py") == _fraction_taps(*args), args


def _is_nearest_with_zero_weights(args):
    from mvoc_amd import ops
    H, W = args[6], args[7]
    taps, near = ops.level_warp_taps(*args, form="py"), ops.level_warp_map(*args, form="py")
    for (y0, x0, qy, qx), s in zip(taps, near):
        assert qy == 0 and qx == 0, args
        inside = 0 <= y0 < H and 0 <= x0 < W
        assert (y0 * W + x0 if inside else -1) == s, args
    return True


def test_identity_translations_and_quarter_turns_have_weight_zero_on_the_nearest_pixel():
    for (Lh, Lw), (H, W) in GRIDS:
        assert _is_nearest_with_zero_weights((0, 0, (1, 0, 0, 1), 1, Lh, Lw, H, W, Lh, Lw))  # the identity, at every level
    # every integer latent translation at S = L (and beyond the frame: everything absent)
    for L in (8, 6):
        for dy, dx in itertools.product(range(-L - 1, L + 2), repeat=2):
            assert _is_nearest_with_zero_weights((dy, dx, (1, 0, 0, 1), 1, L, L, L, L, L, L))
    assert _is_nearest_with_zero_weights((3, -7, (1, 0, 0, 1), 1, 5, 12, 5, 12, 5, 12))
    # the four quarter turns about the centre of a square grid
    for L, S in [(64, 64), (64, 32), (64, 8), (8, 8), (6, 3)]:
        for c, s in [(1, 0), (0, 1), (-1, 0), (0, -1)]:
            assert _is_nearest_with_zero_weights((0, 0, (c, s, -s, c), 1, L, L, S, S, L, L))


def test_scale_one_half_is_the_two_by_two_mean_and_scale_two_the_64_192_pattern():
    from mvoc_amd import ops
    for L, S in [(8, 8), (64, 32), (6, 6)]:
        # scale 1/2 about the centre: the inverse matrix is 2 -- destination i reads 2 (i - S/2) + S/2 + 1/2, half-way between
        # two source pixels on both axes
        taps = ops.level_warp_taps(0, 0, (2, 0, 0, 2), 1, L, L, S, S, L, L, form="py")
        for iy in range(S):
            for ix in range(S):
                y0, x0, qy, qx = taps[iy * S + ix]
                assert (qy, qx) == (128, 128) and (y0, x0) == (2 * iy - S // 2, 2 * ix - S // 2)
        # scale 2 about the centre: the inverse matrix is 1/2 -- destination i reads i/2 + S/4 - 1/4 = (2i + S - 1) / 4: the
        # fractions alternate 3/4, 1/4 (weights 192, 64 of the lower / right tap)
        taps = ops.level_warp_taps(0, 0, (1, 0, 0, 1), 2, L, L, S, S, L, L, form="py")
        for iy in range(S):
            for ix in range(S):
                y0, x0, qy, qx = taps[iy * S + ix]
                want = lambda i: ((2 * i + S - 1) // 4, 64 * ((2 * i + S - 1) % 4))
                assert (y0, qy) == want(iy) and (x0, qx) == want(ix)
                assert {qy, qx} <= {64, 192}
        assert {t[2] for t in taps} == {64, 192}


def test_the_int64_form_equals_the_python_ints_and_the_bound_hands_over():
    from mvoc_amd import ops
    n = 0
    for args in _cases(7):
        assert ops.warp_taps_bound(*args) < 2 ** 62
        a, b = ops.level_warp_taps(*args, form="py"), ops.level_warp_taps(*args, form="i64")
        assert a == b and ops.level_warp_taps(*args) == a, args
        n += 1
    assert n > 150
    # the bound carries the factor of 512 the weights add (513 with the rounding term) to the nearest rule's
    worst = (92, 162, (64 * D, 64 * D, -64 * D, 64 * D), 64 * 64 * D, 180, 320, 90, 160, 90, 160)
    assert ops.warp_taps_bound(*worst) == 513 * ops.warp_numerator_bound(*worst) < 2 ** 62  # production's worst case is vectorised
    # ... and is an upper bound on what the rule forms (Python ints show the true maximum at the corners)
    for dy, dx, m, den, ay2, ax2, H, W, Lh, Lw in [worst, (3, -2, (5, -7, 11, 13), 17, 3, 25, 12, 20, 90, 160)]:
        dfy, dfx = ops.level_offset(dy, H, Lh), ops.level_offset(dx, W, Lw)
        top = 0
        for iy, ix in itertools.product((0, H - 1), (0, W - 1)):
            ny, nx = (2 * (iy - dfy) + 1) * Lh - ay2 * H, (2 * (ix - dfx) + 1) * Lw - ax2 * W
            for N, Dn in ((ay2 * den * H * W + m[0] * ny * W + m[1] * nx * H, 2 * den * W * Lh),
                          (ax2 * den * H * W + m[2] * ny * W + m[3] * nx * H, 2 * den * H * Lw)):
                T = 2 * N - Dn
                i0 = T // (2 * Dn)
                top = max(top, abs(T), abs(i0 * 2 * Dn), 256 * (T - i0 * 2 * Dn) + Dn)
        assert top <= ops.warp_taps_bound(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw)
    # the hand-over: the identity with terms so large that the bound sits just below / just above 2^62
    ident = lambda big: (0, 0, (big, 0, 0, big), big, 8, 8, 8, 8, 8, 8)
    per_unit = ops.warp_taps_bound(*ident(1))
    assert ops.warp_taps_bound(*ident(10 ** 6)) == per_unit * 10 ** 6  # linear in the common factor
    big = -(-2 ** 62 // per_unit)  # the smallest factor at which the bound reaches 2^62
    below, above = ident(big - 1), ident(big)
    assert ops.warp_taps_bound(*below) < 2 ** 62 <= ops.warp_taps_bound(*above)
    assert ops.warp_numerator_bound(*above) < 2 ** 62  # the nearest rule would still vectorise here: the factor matters
    want = [(i // 8, i % 8, 0, 0) for i in range(64)]
    assert ops.level_warp_taps(*below, form="i64") == ops.level_warp_taps(*below, form="py") == ops.level_warp_taps(*below) == want
    assert ops.level_warp_taps(*above) == ops.level_warp_taps(*above, form="py") == want
    with pytest.raises(RuntimeError, match="int64 form is not exact"):
        ops.level_warp_taps(*above, form="i64")
    with pytest.raises(RuntimeError, match="int64 form is not exact"):
        ops.level_warp_taps(*ident(2 ** 56), form="i64")
    assert ops.level_warp_taps(*ident(2 ** 56)) == want
    with pytest.raises(RuntimeError, match="is not one of"):
        ops.level_warp_taps(*below, form="fast")
    with pytest.raises(RuntimeError, match="must be positive"):
        ops.level_warp_taps(0, 0, (1, 0, 0, 1), 0, 8, 8, 4, 4, 8, 8)


# ---- the packed form and its builders --------------------------------------------------------------------------------------------
def test_the_packed_form():
    from mvoc_amd import ops
    H, W = 4, 6
    taps = [(-1, -1, 5, 7), (0, 0, 0, 0), (3, 5, 256, 256), (4, 0, 1, 1), (0, 6, 1, 1), (-2, 0, 9, 9), (0, -2, 9, 9), (-1, 5, 0, 128)]
    words = ops.pack_taps(taps, H, W)
    assert words[0] == [0, (5 << 16) | 7]  # the tap (0, 0) alone is inside: present, fields 0 and 0
    assert words[1] == [(1 << 16) | 1, 0] and words[2] == [(4 << 16) | 6, (256 << 16) | 256]
    assert [w[0] for w in words[3:7]] == [-1] * 4  # y0 = H, x0 = W, y0 = -2, x0 = -2: no tap inside
    assert words[7] == [6, 128]
    assert [ops.tap_present(y0, x0, H, W) for y0, x0, _, _ in taps] == [True, True, True, False, False, False, False, True]
    # a row field of 2^15 or more is a negative int32 word
    big = ops.pack_taps([(40000, 2, 0, 0)], 50000, 8)
    assert big == [[((40001 << 16) | 3) - 2 ** 32, 0]] and -2 ** 31 <= big[0][0] < 0
    for h, w in ((65535, 8), (8, 65535), (70000, 70000)):
        with pytest.raises(RuntimeError, match="16-bit tap fields"):
            ops.pack_taps([], h, w)
        with pytest.raises(RuntimeError, match="16-bit tap fields"):
            ops.warp_taps(((8, 8, ((1, 0, 0, 1, 1, 0, 0),)),), h, w, 8, 8)
    assert ops.pack_taps([], 65534, 65534) == []


def test_warp_taps_cache_per_distinct_frame_and_equal_the_packed_rule():
    from mvoc_amd import ops
    fr = (56756, 32768, -32768, 56756, 65536, 0, 0)
    moved = fr[:5] + (1, -1)
    warp = ((8, 8, (fr, moved, fr)), (6, 10, ((1, 0, 0, 1, 1, 0, 0),) * 3))
    tab = ops.warp_taps(warp, 4, 6, 8, 8)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (2, 3, 24, 2) and tab.is_contiguous() and not tab.is_cuda
    assert torch.equal(tab[0, 0], tab[0, 2]) and not torch.equal(tab[0, 0], tab[0, 1])
    for j, (ay2, ax2, frames) in enumerate(warp):
        for f, v in enumerate(frames):
            rule = ops.level_warp_taps(v[5], v[6], v[:4], v[4], ay2, ax2, 4, 6, 8, 8, form="py")
            assert tab[j, f].tolist() == ops.pack_taps(rule, 4, 6), (j, f)
    assert tab[1, 0].tolist() == [[((i // 6 + 1) << 16) | (i % 6 + 1), 0] for i in range(24)]  # the identity
    assert (tab[0, :, :, 0] == -1).any() and (tab[0, :, :, 0] != -1).any()  # the turned object leaves the plane somewhere
    assert torch.equal(ops.warp_tap_table(warp, 4, 6, 8, 8, "cpu"), tab)
    # beyond int64 the Python ints build the table
    huge = ((8, 8, ((2 ** 70, 0, 0, 2 ** 70, 2 ** 70, 0, 0),)),)
    assert torch.equal(ops.warp_taps(huge, 4, 4, 8, 8), ops.warp_taps(((8, 8, ((1, 0, 0, 1, 1, 0, 0),)),), 4, 4, 8, 8))
    with pytest.raises(RuntimeError, match="same number"):
        ops.warp_taps(((8, 8, (fr,)), (8, 8, (fr, fr))), 4, 4, 8, 8)
    with pytest.raises(RuntimeError, match="same number"):
        ops.warp_taps((), 4, 4, 8, 8)


# ---- the resolver ------------------------------------------------------------------------------------------------------------------
def test_the_resolver_under_the_bilinear_filter():
    from mvoc_amd.pipeline import resolve_obj_transforms
    args = (2, 3, 8, 8)
    # positional callers and "nearest" are unchanged
    for tr in (None, [{}, {}], [{"offset": (8, 16)}, {}], [{"scale": 2, "flip": "v"}, {}], [{"rotate": 30}, {}]):
        assert resolve_obj_transforms(tr, *args) == resolve_obj_transforms(tr, *args, 8, "nearest") == \
            resolve_obj_transforms(tr, *args, interp="nearest")
    bil = lambda tr: resolve_obj_transforms(tr, *args, interp="bilinear")
    assert bil(None) == (None, None, None)
    assert bil([{}, {"rotate": 360}]) == (None, None, None)  # identity: no mode
    assert bil([{"offset": (8, 16)}, {"rotate": 0}]) == resolve_obj_transforms([{"offset": (8, 16)}, {}], *args)  # the placement
    assert bil([{"offset": (8, 16)}, {}])[0] is not None
    # everything else is a warp for all objects: axis-aligned scale and mirror included
    for tr in ([{"scale": 2, "flip": "v"}, {}], [{"flip": "h"}, {}], [{"rotate": 180}, {}], [{"scale": "1/2", "offset": (8, 0)}, {}]):
        pl, t, warp = bil(tr)
        assert pl is None and t is None and len(warp) == 2 and all(len(o[2]) == 3 for o in warp)
        assert resolve_obj_transforms(tr, *args)[1] is not None  # (nearest: the transform mode)
        assert all(f[1] == 0 and f[2] == 0 for o in warp for f in o[2])  # diagonal matrices
    assert bil([{"scale": 2, "flip": "v"}, {}])[2][0] == (8, 8, ((-1, 0, 0, 1, 2, 0, 0),) * 3)
    assert bil([{"rotate": 180}, {}])[2][0] == (8, 8, ((-1, 0, 0, -1, 1, 0, 0),) * 3)
    assert bil([{"rotate": 30}, {}]) == resolve_obj_transforms([{"rotate": 30}, {}], *args)  # a turn is the same warp
    with pytest.raises(ValueError, match="interp 'cubic' is not 'nearest' or 'bilinear'"):
        resolve_obj_transforms([{}, {}], *args, interp="cubic")


def test_the_filter_argument_is_checked_by_name():
    from mvoc_amd.pipeline import TRANSFORM_FILTERS, _transform_filter
    assert TRANSFORM_FILTERS == (None, "nearest", "bilinear")
    assert _transform_filter(None) is None and _transform_filter("nearest") is None and _transform_filter("bilinear") == "bilinear"
    for bad in ("linear", "Bilinear", 1, True, ""):
        with pytest.raises(ValueError, match="obj_transform_filter .* is not one of None, 'nearest', 'bilinear'"):
            _transform_filter(bad)


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
WARP = ((8, 8, ((0, 1, -1, 0, 1, 0, 0),)),) * 2  # two objects, one frame
MASKS = [None, None]


def _engine(variants=2):
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cpu")
    eng.variants = variants
    return eng


def test_the_filter_is_an_attribute_of_the_engine_and_no_sixth_mode():
    from mvoc_amd.unet import PLACEMENT_MODES
    eng = _engine()
    assert len(PLACEMENT_MODES) == 5 and "warp_filter" not in [m.attr for m in PLACEMENT_MODES]
    assert eng.warp_filter is None and eng._tap_tables == (None, {}) and set(eng._level_tables) == {m.attr for m in PLACEMENT_MODES}
    with eng.scoped(warp=WARP, warp_filter="bilinear"):
        assert eng.warp_filter == "bilinear"
    assert eng.warp_filter is None and eng.warp is None
    assert eng.place_kw(MASKS, 8, 8) == {}


def test_the_filter_without_a_warp_is_refused_at_the_site_after_the_modes_own_refusals():
    import test_warp_cpu as twc
    eng = _engine()
    eng.warp_filter = "bilinear"
    with pytest.raises(RuntimeError, match="warp_filter is set but warp is not"):
        eng.place_kw(MASKS, 8, 8)
    eng.placement = (((1, 0),), ((0, 1),))
    with pytest.raises(RuntimeError, match="warp_filter is set but warp is not"):
        eng.place_kw(MASKS, 8, 8)
    # mixes, the frame shard and the object count are the warp's, in the warp's order
    eng.warp = WARP
    with pytest.raises(RuntimeError) as e:
        eng.place_kw(MASKS, 8, 8)
    assert str(e.value).startswith("warp is set together with placement / variant_placements / transform / variant_transforms")
    eng.placement = None
    with pytest.raises(RuntimeError, match="warp holds 2 objects, the hooks carry 3 masks"):
        eng.place_kw([None] * 3, 8, 8)
    eng.shard = types.SimpleNamespace(rank=0, world=1)
    with pytest.raises(RuntimeError, match="a warp does not combine with the frame shard"):
        eng.place_kw(MASKS, 8, 8)
    eng.shard = None
    eng.warp_filter = "cubic"
    with pytest.raises(RuntimeError, match="warp_filter is 'cubic'"):
        eng.place_kw(MASKS, 8, 8)
    assert twc.WARP == WARP


def test_the_blend_functions_route_and_refuse_a_tap_table_before_any_launch():
    from mvoc_amd import ops
    t3, t4 = torch.zeros(2, 2, 16, dtype=torch.int32), torch.zeros(2, 2, 16, 2, dtype=torch.int32)
    entry = lambda **kw: ops._blend_entry("pnp_blend_x", kw.get("place"), kw.get("resample"), kw.get("mask_dim", 4),
                                          kw.get("no_background", False), kw.get("src_map"), kw.get("nvar", 1), kw.get("active"),
                                          kw.get("warp"), kw.get("warp_taps"))
    assert entry(warp_taps=t4) == "_bilinear" and entry(warp_taps=t4, nvar=3, active=0b101, src_map=(2, (1, 1))) == "_bilinear"
    assert entry() == "" and entry(resample=t3) == "_resampled" and entry(place=t3) == "_placed" and entry(warp=t3) == "_warped"
    for other in ("place", "resample", "warp"):
        with pytest.raises(RuntimeError, match="warp_taps= is given together with place= / resample= / warp="):
            entry(warp_taps=t4, **{other: t3})
    with pytest.raises(RuntimeError, match="warp_taps= does not take a .* mask stack"):
        entry(warp_taps=t4, mask_dim=5)
    with pytest.raises(RuntimeError, match="warp_taps= with no_background"):
        entry(warp_taps=t4, no_background=True)
    with pytest.raises(RuntimeError, match="must be a device tensor"):  # the table's form is checked on the device table
        ops._check_table("pnp_blend_x", "warp_taps", t4, None, 1, types.SimpleNamespace(nobj=2, frames=2, height=4, width=4))
    import inspect
    for fn in (ops.pnp_blend_tokens, ops.pnp_blend_nchw):
        assert inspect.signature(fn).parameters["warp_taps"].default is None


# ---- drivers -------------------------------------------------------------------------------------------------------------------
def test_demo_job_takes_the_filter():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import demo_job
    finally:
        sys.path.pop(0)
    import inspect
    assert inspect.signature(demo_job.run_variants).parameters["transform_filter"].default is None
    src = open(os.path.join(REPO, "tools", "demo_job.py")).read()
    assert '"--transform-filter"' in src and 'choices=("nearest", "bilinear")' in src and 'res["obj_transform_filter"]' in src
    assert "--transform-filter bilinear" in open(os.path.join(REPO, "README.md")).read()
    # the option alone reaches run_variants (and its refusal) instead of being dropped with the plain job
    assert re.search(r"if a\.variants or .* or a\.transform_filter:", src)
    # refused before any work is done: without --transform, and next to --variant-transform
    tf = demo_job.parse_transform("rotate=30;")
    with pytest.raises(SystemExit, match="--transform-filter needs --transform"):
        demo_job.run_variants(variants=1, transform_filter="bilinear")
    with pytest.raises(SystemExit, match="--transform-filter needs --transform"):
        demo_job.run_variants(variants=1, transform_filter="nearest")
    with pytest.raises(SystemExit, match="--transform-filter bilinear does not combine with --variant-transform"):
        demo_job.run_variants(variants=2, transform=tf, variant_transform=[tf, None], transform_filter="bilinear")
    # the result line names the filter only when the option was given: a run without it prints what it printed before
    assert 'res["obj_transform_filter"] = transform_filter\n' in src and 'or "nearest"' not in src


def test_composite_py_hands_the_filter_to_the_sampling_call(tmp_path):
    import test_resample_cpu as trc
    rotated = [{"rotate": 30, "scale": "3/2"}, {"rotate": [0, 15]}]
    gen = trc.composite.__wrapped__()  # the fixture's generator: composite.py imported from this repository, then put away again
    composite = next(gen)
    try:
        ct = trc._template(tmp_path)
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, obj_transform=rotated, obj_transform_filter="bilinear"))
        assert composite.transform_kwargs(config, variants) == {"obj_transforms": rotated, "obj_transform_filter": "bilinear"}
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, obj_transform=rotated))
        assert composite.transform_kwargs(config, variants) == {"obj_transforms": rotated}  # without the key: today's call
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, obj_transform_filter="bilinear"))
        with pytest.raises(ValueError, match="obj_transform_filter is 'bilinear' without obj_transform"):
            composite.transform_kwargs(config, variants)
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, obj_transform_filter="nearest"))
        assert composite.transform_kwargs(config, variants) == {}
        # a variant with its own transform: the call would run variant_obj_transforms, which has no filter -- refused here, with
        # the shared obj_transform or without it; "nearest" is the call without the key
        var = [{"transform": [{"scale": 2}, {}]}, {}]
        for extra in ({"obj_transform": rotated}, {}):
            config, variants = composite.merge_variants(ct, dict(trc.ENTRY, variants=var, obj_transform_filter="bilinear", **extra))
            with pytest.raises(ValueError, match="obj_transform_filter is 'bilinear' and a variant sets 'transform'"):
                composite.transform_kwargs(config, variants)
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, variants=var, obj_transform=rotated))
        plain = composite.transform_kwargs(config, variants)
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, variants=var, obj_transform=rotated, obj_transform_filter="nearest"))
        assert composite.transform_kwargs(config, variants) == plain and list(plain) == ["variant_obj_transforms"]
        # variants that all use the shared obj_transform keep the filter
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, variants=[{}, {}], obj_transform=rotated, obj_transform_filter="bilinear"))
        assert composite.transform_kwargs(config, variants) == {"obj_transforms": rotated, "obj_transform_filter": "bilinear"}
        # a misspelt value is refused whatever else the entry sets
        for extra in ({}, {"obj_transform": rotated}, {"variants": var}, {"obj_offset": [[8, 8], [0, 0]]}):
            config, variants = composite.merge_variants(ct, dict(trc.ENTRY, obj_transform_filter="cubic", **extra))
            with pytest.raises(ValueError, match="obj_transform_filter 'cubic' is not one of 'nearest', 'bilinear'"):
                composite.transform_kwargs(config, variants)
    finally:
        gen.close()


# ---- declared, exported, bound ---------------------------------------------------------------------------------------------------
ENTRIES = ("mvoc_pnp_blend_scatter_tokens_bilinear", "mvoc_pnp_blend_scatter_nchw_bilinear", "mvoc_gather_planes_bilinear_f16")


def test_the_entries_are_declared_exported_and_bound():
    from mvoc_amd import _ffi, build
    header = open(os.path.join(REPO, "include", "mvoc_hip.h")).read()
    assert "pnp_bilinear.hip" in build.SOURCES
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _ffi.SIGNATURES and callable(getattr(_ffi.lib, name)), name
    assert _ffi.SIGNATURES[ENTRIES[0]] == _ffi.SIGNATURES["mvoc_pnp_blend_scatter_tokens_warped"]
    assert _ffi.SIGNATURES[ENTRIES[1]] == _ffi.SIGNATURES["mvoc_pnp_blend_scatter_nchw_warped"]
    assert _ffi.SIGNATURES[ENTRIES[2]] == _ffi.SIGNATURES["mvoc_gather_planes_warped_f16"]
    assert _ffi.ABI_VERSION == 100 and "#define MVOC_VERSION 100" in header  # the descriptor and the version stay
