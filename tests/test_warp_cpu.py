"""CPU: rotation of objects at composition time through an exact 2-D nearest index map -- everything that needs
no kernel.

* the rule ``ops.level_warp_map`` (Python ints): a diagonal matrix is the outer combination of ``level_axis_map`` of DESIGN.md 6n,
  a quarter turn about the centre of a square grid is ``rot90``; the vectorised int64 form against the Python ints, and the bound
  that decides between them.
* angle -> matrix: the pins of 30, 45 and the exact multiples of 90 degrees; the resolver's downgrade table and its messages.
* the engine's fifth placement mode: its mix and frame-shard refusals and the order of the checks.
* the drivers' parsing, and that the new entries are declared, exported and bound.
"""
import itertools
import os
import re
import sys
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (latent grid, site): the levels of 64 x 64 and 90 x 160 latents, and two grids with nothing in common
GRIDS = [((64, 64), (64, 64)), ((64, 64), (32, 32)), ((64, 64), (8, 8)), ((90, 160), (45, 80)), ((90, 160), (23, 40)),
         ((90, 160), (12, 20)), ((5, 12), (3, 23)), ((8, 8), (8, 8)), ((6, 10), (3, 5))]
SCALES = [(1, 1, 1, 1), (3, 2, 3, 2), (1, 2, 3, 4), (64, 1, 1, 64), (5, 3, 2, 7)]  # (py, qy, px, qx)


def _diagonal_cases():
    for ((Lh, Lw), (H, W)), scale, flips in itertools.product(GRIDS, SCALES, itertools.product((False, True), repeat=2)):
        for (ay2, ax2), (dy, dx) in itertools.product([(Lh, Lw), (3, Lw + 5)], [(0, 0), (3, -2), (-Lh - 2, 1), (1, Lw + 2)]):
            yield (Lh, Lw), (H, W), scale, flips, (ay2, ax2), (dy, dx)


def test_a_diagonal_matrix_is_the_outer_combination_of_the_per_axis_maps():
    from mvoc_amd import ops
    n = 0
    for (Lh, Lw), (H, W), (py, qy, px, qx), (fy, fx), (ay2, ax2), (dy, dx) in _diagonal_cases():
        ym, xm = ops.level_axis_map(dy, py, qy, fy, ay2, H, Lh), ops.level_axis_map(dx, px, qx, fx, ax2, W, Lw)
        want = [y * W + x if y >= 0 and x >= 0 else -1 for y in ym for x in xm]
        m = ((-1 if fy else 1) * qy * px, 0, 0, (-1 if fx else 1) * qx * py)
        got = ops.level_warp_map(dy, dx, m, py * px, ay2, ax2, H, W, Lh, Lw, form="py")
        assert got == want, ((Lh, Lw), (H, W), (py, qy, px, qx), (fy, fx), (ay2, ax2), (dy, dx))
        n += 1
    assert n == len(GRIDS) * len(SCALES) * 4 * 2 * 4 == 1440


@pytest.mark.parametrize("L,S", [(64, 64), (64, 32), (64, 8), (8, 8), (6, 3)])
def test_quarter_turns_about_the_centre_are_rot90(L, S):
    """the orientation: the inverse matrix of a rotation by theta is [[cos, sin], [-sin, cos]] in (y, x) order, and positive angles
    turn the object counter-clockwise on screen -- ``torch.rot90`` with k = 1"""
    from mvoc_amd import ops
    src = torch.arange(S * S).reshape(S, S)
    for k, (c, s) in enumerate([(1, 0), (0, 1), (-1, 0), (0, -1)]):
        for form in ("py", "i64"):
            got = ops.level_warp_map(0, 0, (c, s, -s, c), 1, L, L, S, S, L, L, form=form)
            assert sorted(got) == list(range(S * S))  # a permutation, nothing absent
            assert torch.equal(torch.tensor(got).reshape(S, S), torch.rot90(src, k)), (k, form)


def test_thirty_and_forty_five_degrees_show_the_counted_pixels_and_are_not_separable():
    from mvoc_amd import ops
    D = 65536
    for (c, s), present in (((56756, 32768), 56), ((46341, 46341), 52)):
        got = ops.level_warp_map(0, 0, (c, s, -s, c), D, 8, 8, 8, 8, 8, 8)
        assert sum(v >= 0 for v in got) == present
        rows = [{v // 8 for v in got[iy * 8:iy * 8 + 8] if v >= 0} for iy in range(8)]
        assert any(len(r) > 1 for r in rows)  # one destination row reads several source rows: no (ymap, xmap) pair says this


def test_the_int64_form_equals_the_python_ints():
    from mvoc_amd import ops
    D = 65536
    rot = [(56756, 32768), (46341, 46341), (0, D), (-D, 0), (63303, -16962)]
    n = 0
    for i, ((Lh, Lw), (H, W), (py, qy, px, qx), (fy, fx), (ay2, ax2), (dy, dx)) in enumerate(_diagonal_cases()):
        if i % 7:  # every seventh diagonal case, under a rotation that changes with it
            continue
        c, s = rot[(i // 7) % len(rot)]
        gy, gx = (-1 if fy else 1) * qy * px, (-1 if fx else 1) * qx * py
        m, den = (gy * c, gy * s, -gx * s, gx * c), py * px * D
        args = (dy, dx, m, den, ay2, ax2, H, W, Lh, Lw)
        assert ops.warp_numerator_bound(*args) < 2 ** 62
        a, b = ops.level_warp_map(*args, form="py"), ops.level_warp_map(*args, form="i64")
        assert a == b, args
        assert ops.level_warp_map(*args) == a
        n += 1
    assert n > 150


def test_the_bound_decides_the_form_and_covers_production():
    from mvoc_amd import ops
    D = 65536
    # production's worst case: the finest level of 90 x 160 latents, scale terms of 64, offsets beyond the frame
    worst = (92, 162, (64 * D, 64 * D, -64 * D, 64 * D), 64 * 64 * D, 180, 320, 90, 160, 90, 160)
    assert ops.warp_numerator_bound(*worst) < 2 ** 56
    # a denominator beyond int64: the Python ints answer, the int64 form is refused
    big = 2 ** 56
    args = (0, 0, (big, 0, 0, big), big, 8, 8, 8, 8, 8, 8)
    assert ops.warp_numerator_bound(*args) >= 2 ** 62
    assert ops.level_warp_map(*args) == list(range(64))  # the identity, whatever the size of its terms
    with pytest.raises(RuntimeError, match="int64 form is not exact"):
        ops.level_warp_map(*args, form="i64")
    # the bound is an upper bound on what the rule forms (checked where Python ints show the true maximum)
    for dy, dx, m, den, ay2, ax2, H, W, Lh, Lw in [worst, (3, -2, (5, -7, 11, 13), 17, 3, 25, 12, 20, 90, 160)]:
        dfy, dfx = ops.level_offset(dy, H, Lh), ops.level_offset(dx, W, Lw)
        top = 0
        for iy, ix in itertools.product((0, H - 1), (0, W - 1)):
            ny, nx = (2 * (iy - dfy) + 1) * Lh - ay2 * H, (2 * (ix - dfx) + 1) * Lw - ax2 * W
            top = max(top, abs(ay2 * den * H * W + m[0] * ny * W + m[1] * nx * H), abs(ax2 * den * H * W + m[2] * ny * W + m[3] * nx * H))
        assert top <= ops.warp_numerator_bound(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw)


def test_warp_maps_cache_per_distinct_frame_and_refuse_ragged_values():
    from mvoc_amd import ops
    fr = (56756, 32768, -32768, 56756, 65536, 0, 0)
    moved = fr[:5] + (1, -1)
    warp = ((8, 8, (fr, moved, fr)), (6, 10, ((1, 0, 0, 1, 1, 0, 0),) * 3))
    rows = ops.warp_maps(warp, 4, 4, 8, 8)
    assert len(rows) == 2 and [len(o) for o in rows] == [3, 3] and all(len(r) == 16 for o in rows for r in o)
    assert rows[0][0] is rows[0][2] and rows[0][0] != rows[0][1]  # one computation per distinct frame value
    assert rows[1][0] == list(range(16))
    assert rows[0][1] == ops.level_warp_map(1, -1, fr[:4], fr[4], 8, 8, 4, 4, 8, 8)
    tab = ops.warp_table(warp, 4, 4, 8, 8, "cpu")
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (2, 3, 16) and tab.is_contiguous() and tab.tolist() == rows
    with pytest.raises(RuntimeError, match="same number"):
        ops.warp_maps(((8, 8, (fr,)), (8, 8, (fr, fr))), 4, 4, 8, 8)
    with pytest.raises(RuntimeError, match="same number"):
        ops.warp_maps((), 4, 4, 8, 8)
    with pytest.raises(RuntimeError, match="must be positive"):
        ops.level_warp_map(0, 0, (1, 0, 0, 1), 0, 8, 8, 4, 4, 8, 8)


# ---- angle -> matrix, the resolver ---------------------------------------------------------------------------------------------
def test_angle_pins():
    from mvoc_amd.pipeline import WARP_DEN, _rotation
    D = WARP_DEN
    assert D == 65536
    assert _rotation(30, "x") == (56756, 32768) and _rotation(45, "x") == (46341, 46341)
    assert _rotation(30.0, "x") == _rotation("30", "x") == _rotation("60/2", "x") == (56756, 32768)
    for deg, want in ((0, (D, 0)), (90, (0, D)), (180, (-D, 0)), (270, (0, -D)), (360, (D, 0)), (-90, (0, -D)), (450, (0, D)),
                      (-180.0, (-D, 0)), ("720", (D, 0))):
        assert _rotation(deg, "x") == want, deg
    assert _rotation(390, "x") == _rotation(30, "x") and _rotation(-330, "x") == _rotation(30, "x")
    c, s = _rotation(-15, "x")
    assert (c, s) == (63303, -16962)
    for bad in (True, None, "a", "1/0", [30], {}):
        with pytest.raises(ValueError, match="rotate .* is not an int, a float or a 'p/q' string"):
            _rotation(bad, "obj_transforms: object 0")


def test_the_warp_value_is_the_reduced_inverse_matrix():
    from mvoc_amd import ops
    from mvoc_amd.pipeline import resolve_obj_transforms
    pl, tr, warp = resolve_obj_transforms([{"rotate": 30, "scale": "3/2", "flip": "h", "offset": (8, -16)}, {}], 2, 2, 8, 8)
    assert pl is None and tr is None
    # diag(2/3, -2/3) . [[C, S], [-S, C]] / D over 3 * 3 * D, reduced by the gcd; the second object turns by nothing
    assert warp == ((8, 8, ((14189, 8192, 8192, -14189, 24576, -2, 1),) * 2), (8, 8, ((1, 0, 0, 1, 1, 0, 0),) * 2))
    hash(warp)
    # a path of angles: one matrix per frame
    _, _, w2 = resolve_obj_transforms([{"rotate": [0, "45/2", 90]}], 1, 3, 8, 8)
    assert [f[:5] for f in w2[0][2]] == [(1, 0, 0, 1, 1), (60547, 25080, -25080, 60547, 65536), (0, 1, -1, 0, 1)]
    # the maps of a quarter turn built this way are rot90
    _, _, w3 = resolve_obj_transforms([{"rotate": 90}], 1, 1, 6, 6)
    got = torch.tensor(ops.warp_maps(w3, 6, 6, 6, 6)[0][0]).reshape(6, 6)
    assert torch.equal(got, torch.rot90(torch.arange(36).reshape(6, 6), 1))


def test_the_resolver_downgrades_diagonal_matrices_to_the_older_modes_exactly():
    from mvoc_amd.pipeline import normalize_obj_transforms, resolve_obj_transforms
    args = (2, 3, 8, 8)
    assert resolve_obj_transforms(None, *args) == (None, None, None)
    table = [  # (with rotate, the call without the key)
        ([{"rotate": 0}, {"rotate": 360.0}], [{}, {}]),
        ([{"rotate": [0, 360, -720]}, None], [{}, None]),
        ([{"rotate": 0, "offset": (8, 16)}, {}], [{"offset": (8, 16)}, {}]),
        ([{"rotate": 180}, {"rotate": "-180", "scale": "3/2"}], [{"flip": "hv"}, {"flip": "hv", "scale": "3/2"}]),
        ([{"rotate": 180, "flip": "hv"}, {"rotate": 540, "flip": "h", "anchor": [40, 24]}], [{}, {"flip": "v", "anchor": [40, 24]}]),
        ([{"scale": 2, "flip": "v"}, {}], [{"scale": 2, "flip": "v"}, {}]),
    ]
    kinds = set()
    for rotated, plain in table:
        want = normalize_obj_transforms(plain, *args)
        assert resolve_obj_transforms(rotated, *args) == want + (None,), rotated
        kinds.add(tuple(v is not None for v in want))
    assert kinds == {(False, False), (True, False), (False, True)}  # no mode, placement, transform: all three were met
    # anything that is not diagonal in every frame, or not the same diagonal in every frame, is a warp -- for every object
    for rotated in ([{"rotate": 30}, {}], [{"rotate": [0, 180, 0]}, {}], [{}, {"rotate": 90, "scale": 2}]):
        pl, tr, warp = resolve_obj_transforms(rotated, *args)
        assert pl is None and tr is None and len(warp) == 2 and all(len(o[2]) == 3 for o in warp)
    # normalize_obj_transforms keeps refusing the key it never took
    with pytest.raises(ValueError, match=r"object 0 has the unknown key\(s\) 'rotate'; the keys are offset, scale, flip, anchor"):
        normalize_obj_transforms([{"rotate": 30}, {}], *args)


def test_the_resolver_and_the_variant_form_name_what_they_refuse():
    from mvoc_amd.pipeline import resolve_obj_transforms, resolve_variant_obj_transforms
    args = (2, 3, 8, 8)
    for bad, text in [
        ([{"rotate": "x"}, {}], "object 0: rotate 'x' is not an int"),
        ([{}, {"rotate": [0, 90]}], "object 1: rotate has 2 per-frame angles, the clip 3 frames"),
        ([{}, {"rotate": [0, 90, None]}], "object 1: rotate None is not"),
        ([{"spin": 3}, {}], r"object 0 has the unknown key\(s\) 'spin'"),
        ([{}], "1 entries for 2 objects"),
    ]:
        with pytest.raises(ValueError, match=text):
            resolve_obj_transforms(bad, *args)
    with pytest.raises(ValueError, match="variant 1: object 0: rotate: per-variant rotation is not built"):
        resolve_variant_obj_transforms([None, [{"rotate": 30}, {}]], 2, *args)
    with pytest.raises(ValueError, match="per-variant rotation is not built"):
        resolve_variant_obj_transforms([[{}, {"rotate": 0}], None], 2, *args)
    # without the key the variant form is what it was
    assert resolve_variant_obj_transforms([None, [{"scale": 2}, {}]], 2, *args)[3] is not None


# ---- the engine's fifth mode ----------------------------------------------------------------------------------------------------
WARP = ((8, 8, ((0, 1, -1, 0, 1, 0, 0),)),) * 2  # two objects, one frame
OTHERS = (("variant_transforms", ((((2, 1, 2, 1, False, False, 8, 8, ((0, 0),)),) * 2,) * 2)),
          ("transform", ((2, 1, 2, 1, False, False, 8, 8, ((0, 0),)),) * 2),
          ("variant_placements", ((((1, 0),), ((0, 1),)),) * 2), ("placement", (((1, 0),), ((0, 1),))))
MASKS = [None, None]


def _engine(variants=2):
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cpu")
    eng.variants = variants
    return eng


def test_the_warp_mode_is_first_in_the_table_and_names_its_kernels():
    from mvoc_amd import ops
    from mvoc_amd.unet import PLACEMENT_MODES
    m = PLACEMENT_MODES[0]
    assert (m.attr, m.per_variant, m.kw, m.builder, m.mover) == ("warp", False, "warp", "warp_table", "warp")
    assert callable(getattr(ops, m.builder)) and callable(getattr(ops, m.mover + "_planes"))
    assert [x.attr for x in PLACEMENT_MODES[1:]] == ["variant_transforms", "transform", "variant_placements", "placement"]
    assert m.mix.startswith("warp is {set} together with")
    assert _engine().warp is None


def test_a_warp_next_to_any_other_mode_raises_the_warp_sentence():
    eng = _engine()
    for n in (1, 2, 3, 4):
        for subset in itertools.combinations(OTHERS, n):
            eng.warp = WARP
            for attr, value in subset:
                setattr(eng, attr, value)
            with pytest.raises(RuntimeError) as e:
                eng.place_kw(MASKS, 8, 8)
            assert str(e.value).startswith("warp is set together with placement / variant_placements / transform / variant_transforms")
            eng.warp = None
            for attr, _ in subset:
                setattr(eng, attr, None)
    assert eng.place_kw(MASKS, 8, 8) == {}


def test_a_warp_is_refused_under_a_frame_shard_before_the_object_count():
    eng = _engine()
    eng.warp = WARP
    with pytest.raises(RuntimeError, match="warp holds 2 objects, the hooks carry 3 masks"):
        eng.place_kw([None] * 3, 8, 8)
    eng.shard = types.SimpleNamespace(rank=0, world=1)
    for call in (lambda: eng.place_kw([None] * 3, 8, 8), lambda: eng.pnp_batch(3 + 2 * eng.variants, MASKS)):
        with pytest.raises(RuntimeError, match="frame shard") as e:
            call()
        assert str(e.value).startswith("a warp does not combine with the frame shard") and "a warp crosses slabs" in str(e.value)


def test_the_blend_functions_route_and_refuse_a_warp_table_before_any_launch():
    from mvoc_amd import ops
    t3 = torch.zeros(2, 2, 16, dtype=torch.int32)
    entry = lambda **kw: ops._blend_entry("pnp_blend_x", kw.get("place"), kw.get("resample"), kw.get("mask_dim", 4),
                                          kw.get("no_background", False), kw.get("src_map"), kw.get("nvar", 1), kw.get("active"),
                                          kw.get("warp"))
    assert entry(warp=t3) == "_warped" and entry(warp=t3, nvar=3, active=0b101, src_map=(2, (1, 1))) == "_warped"
    assert entry() == "" and entry(resample=t3) == "_resampled" and entry(place=t3) == "_placed"  # today's calls stay
    with pytest.raises(RuntimeError, match="warp= is given together with place= / resample="):
        entry(warp=t3, place=t3)
    with pytest.raises(RuntimeError, match="warp= is given together with place= / resample="):
        entry(warp=t3, resample=t3)
    with pytest.raises(RuntimeError, match="warp= does not take a .* mask stack"):
        entry(warp=t3, mask_dim=5)
    with pytest.raises(RuntimeError, match="warp= with no_background"):
        entry(warp=t3, no_background=True)
    with pytest.raises(RuntimeError, match="must be a device tensor"):  # the table's form is checked on the device table
        ops._check_table("pnp_blend_x", "warp", t3, None, 1, types.SimpleNamespace(nobj=2, frames=2, height=4, width=4))


# ---- drivers -------------------------------------------------------------------------------------------------------------------
def test_demo_job_reads_rotate():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import demo_job
    finally:
        sys.path.pop(0)
    assert demo_job.parse_transform("rotate=30,scale=3/2;rotate=-15") == [{"rotate": 30, "scale": "3/2"}, {"rotate": -15}]
    assert demo_job.parse_transform("rotate=45/2;rotate=17.5,flip=h;") == [{"rotate": "45/2"}, {"rotate": 17.5, "flip": "h"}, {}]
    assert demo_job.parse_transform("rotate=0,10,20,offset=8,0") == [{"rotate": [0, 10, 20], "offset": [8, 0]}]
    assert demo_job.parse_transform("scale=3/2,flip=h,offset=64,0;scale=1/2") == [{"scale": "3/2", "flip": "h", "offset": [64, 0]},
                                                                                  {"scale": "1/2"}]
    with pytest.raises(SystemExit, match="cannot read rotate=x"):
        demo_job.parse_transform("rotate=x")


def test_composite_py_hands_rotate_to_the_sampling_call(tmp_path):
    import test_resample_cpu as trc
    from mvoc_amd.pipeline import resolve_obj_transforms
    rotated = [{"rotate": 30, "scale": "3/2"}, {"rotate": [0, 15]}]
    gen = trc.composite.__wrapped__()  # the fixture's generator: composite.py imported from this repository, then put away again
    composite = next(gen)
    try:
        ct = trc._template(tmp_path)
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, obj_transform=rotated))
        kw = composite.transform_kwargs(config, variants)
        assert kw == {"obj_transforms": rotated} and type(kw["obj_transforms"][1]["rotate"]) is list
        assert resolve_obj_transforms(kw["obj_transforms"], 2, 2, 64, 48) == resolve_obj_transforms(rotated, 2, 2, 64, 48)
        assert resolve_obj_transforms(kw["obj_transforms"], 2, 2, 64, 48)[2] is not None
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, obj_transform=rotated, obj_offset=[[8, 8], [0, 0]]))
        with pytest.raises(ValueError, match="obj_transform and obj_offset are both set"):
            composite.transform_kwargs(config, variants)
    finally:
        gen.close()


# ---- declared, exported, bound ---------------------------------------------------------------------------------------------------
ENTRIES = ("mvoc_pnp_blend_scatter_tokens_warped", "mvoc_pnp_blend_scatter_nchw_warped", "mvoc_gather_planes_warped_f16")


def test_the_entries_are_declared_exported_and_bound():
    from mvoc_amd import _ffi, build
    header = open(os.path.join(REPO, "include", "mvoc_hip.h")).read()
    assert "pnp_warp.hip" in build.SOURCES
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _ffi.SIGNATURES and callable(getattr(_ffi.lib, name)), name
    assert _ffi.SIGNATURES[ENTRIES[0]] == _ffi.SIGNATURES["mvoc_pnp_blend_scatter_tokens_resampled"]
    assert _ffi.SIGNATURES[ENTRIES[1]] == _ffi.SIGNATURES["mvoc_pnp_blend_scatter_nchw_resampled"]
    assert _ffi.SIGNATURES[ENTRIES[2]] == _ffi.SIGNATURES["mvoc_gather_planes_f16"]
    assert _ffi.ABI_VERSION == 100 and "#define MVOC_VERSION 100" in header  # the descriptor and the version stay
