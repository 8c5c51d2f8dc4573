"""CPU: per-variant object placement -- the normalisation and three-way resolution of the sampling call's
``variant_obj_offsets``, ``ops.place_table_variants`` against ``level_offsets``, composite.py's per-variant ``placement`` key,
``demo_job.py --variant-place`` and the two new entry points declared, exported and bound.  No kernel is launched."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

from test_placement_cpu import ENTRY, REPO, _template, composite  # noqa: F401  (the fixture and the entry of the 6k tests)

F = 3
A = [(16, -8), [(0, 0), (8, 0), (16, 24)]]  # object 0 by one pair, object 1 along a path (dx, dy in image pixels)
B = [(-8, 8), (0, 16)]
A_LAT = (((-1, 2),) * F, ((0, 0), (0, 1), (3, 2)))  # (dy, dx) on the latent grid
B_LAT = (((1, -1),) * F, ((2, 0),) * F)
ZERO = (((0, 0),) * F,) * 2


# ---- variant_obj_offsets of the sampling call -------------------------------------------------------------------------------
def test_no_argument_and_all_none_or_zero_resolve_to_a_call_without_it():
    from mvoc_amd.pipeline import resolve_variant_obj_offsets as res
    assert res(None, 3, 2, F) == (None, None)
    assert res([None, None, None], 3, 2, F) == (None, None)
    assert res([None, [(0, 0), (0, 0)], [[(0, 0)] * F, (0, 0)]], 3, 2, F) == (None, None)


def test_equal_items_resolve_to_the_shared_placement():
    from mvoc_amd.pipeline import normalize_obj_offsets, resolve_variant_obj_offsets as res
    shared, per = res([A, A, A], 3, 2, F)
    assert per is None and shared == A_LAT == normalize_obj_offsets(A, 2, F)
    # equal after normalisation: a pair and the path that repeats it are one placement
    shared, per = res([[(8, 8), (0, 0)], [[(8, 8)] * F, [(0, 0)] * F]], 2, 2, F)
    assert per is None and shared == (((1, 1),) * F, ((0, 0),) * F)
    assert res([B], 1, 2, F) == (B_LAT, None)  # one variant: always the shared call


def test_different_items_resolve_per_variant_with_zeros_for_the_unplaced():
    from mvoc_amd.pipeline import resolve_variant_obj_offsets as res
    shared, per = res([A, None, B], 3, 2, F)
    assert shared is None and per == (A_LAT, ZERO, B_LAT)
    hash(per)  # the engine keys its table cache and the graph variants by it
    shared, per = res([None, [(0, 0), (0, 0)], B], 3, 2, F)  # None and zeros are the same thing
    assert shared is None and per == (ZERO, ZERO, B_LAT)
    # a placed variant among unplaced ones is per-variant, never shared
    assert res([A, None], 2, 2, F) == (None, (A_LAT, ZERO))


@pytest.mark.parametrize("bad,nvar,msg", [
    ([A, B], 3, r"variant_obj_offsets: 2 entries for 3 variants"),
    ([A, B, A, B], 3, r"variant_obj_offsets: 4 entries for 3 variants"),
    ("8,8", 3, r"variant_obj_offsets: needs a list of 3 items"),
    ([A, None, [(8, 8), (8, 4)]], 3, r"variant 2: obj_offsets: object 1, frame 0: \(8, 4\) is not a multiple of 8"),
    ([[[(8, 8), (8, 8), (9, 8)], (0, 0)], None, None], 3, r"variant 0: obj_offsets: object 0, frame 2: \(9, 8\) is not a multiple of 8"),
    ([None, [(8, 8)], None], 3, r"variant 1: obj_offsets: 1 entries for 2 objects"),
    ([None, [(8, 8), [(0, 0), (8, 8)]]], 2, r"variant 1: obj_offsets: object 1 has 2 per-frame offsets, the clip 3 frames"),
])
def test_bad_variant_offsets_name_the_variant_and_the_object(bad, nvar, msg):
    from mvoc_amd.pipeline import resolve_variant_obj_offsets as res
    with pytest.raises(ValueError, match=msg):
        res(bad, nvar, 2, F)


def test_both_arguments_are_refused_before_anything_runs():
    """the sampling call checks the pair of arguments where it normalises them: with both given nothing else is touched"""
    import inspect
    from mvoc_amd.pipeline import I2VGenXLPipeline
    fn = I2VGenXLPipeline.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection
    assert inspect.signature(fn).parameters["variant_obj_offsets"].default is None
    pipe = I2VGenXLPipeline.__new__(I2VGenXLPipeline)  # no engine: the refusal comes before the conditioner is used
    pipe.conditioner = None
    with pytest.raises(ValueError, match="obj_offsets and variant_obj_offsets are both given"):
        fn(pipe, prompt=["a", "b"], obj_ddim_latents_path=["o0", "o1"], obj_offsets=A, variant_obj_offsets=[A, B], num_frames=F)


# ---- the device table ---------------------------------------------------------------------------------------------------
def test_place_table_variants_is_level_offsets_per_variant():
    from mvoc_amd import ops
    mh, mw = 90, 160  # the latent grid of a 720 x 1280 clip; its levels have 45, 23 and 12 rows
    pls = (A_LAT, ZERO, B_LAT, (((-89, 159), (45, -80), (7, 3)), ((1, 1), (-1, -1), (44, 79))))
    for H, W in ((90, 160), (45, 80), (23, 40), (12, 20)):
        tab = ops.place_table_variants(pls, H, W, mh, mw, "cpu")
        assert tab.dtype == torch.int32 and tuple(tab.shape) == (4, 2, F, 2) and tab.is_contiguous()
        for k, pl in enumerate(pls):
            assert tab[k].tolist() == [list(map(list, o)) for o in ops.level_offsets(pl, H, W, mh, mw)], (H, W, k)
            assert torch.equal(tab[k], ops.place_table(pl, H, W, mh, mw, "cpu"))  # one rule, no second one
        assert not tab[1].any()
    assert ops.place_table_variants(pls, 23, 40, mh, mw, "cpu")[3, 0].tolist() == [[-23, 40], [12, -20], [2, 1]]


def test_place_table_variants_refuses_what_place_table_refuses():
    from mvoc_amd import ops
    with pytest.raises(RuntimeError, match=r"place_table_variants: variant 1: place_table: offset .* of object 0, frame 0 does not fit int32"):
        ops.place_table_variants((ZERO, (((2 ** 31, 0),) * F, ((0, 0),) * F)), 8, 8, 8, 8, "cpu")
    with pytest.raises(RuntimeError, match=r"variant 0: place_table: offset .* does not fit int32"):
        ops.place_table_variants(((((0, -2 ** 31 - 1),) * F, ((0, 0),) * F), ZERO), 8, 8, 8, 8, "cpu")
    with pytest.raises(RuntimeError, match="differ in shape"):
        ops.place_table_variants((ZERO, ZERO[:1]), 8, 8, 8, 8, "cpu")
    with pytest.raises(RuntimeError, match="at least one"):
        ops.place_table_variants((), 8, 8, 8, 8, "cpu")
    assert "place_table_variants" in ops.__all__


def test_engine_defaults_to_no_variant_placements():
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cpu")
    assert eng.variant_placements is None and eng.variant_masks is None
    assert eng.place_kw([None, None], 8, 8) == {}
    m = torch.zeros(2, F, 8, 8)
    assert eng.site_masks(m, 0) is m and eng.site_masks(m, 1) is m  # the sites' calls carry today's masks


def test_engine_refuses_bad_variant_placements():
    import types
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cpu")
    masks = [None, None]
    eng.variant_placements, eng.variants = (A_LAT, ZERO, B_LAT), 2
    with pytest.raises(RuntimeError, match="variant_placements holds 3 placements, the call 2 variants"):
        eng.place_kw(masks, 8, 8)
    eng.variants = 3
    with pytest.raises(RuntimeError, match=r"variant_placements\[0\] holds offsets for 2 objects, the hooks carry 3 masks"):
        eng.place_kw([None] * 3, 8, 8)
    eng.placement = A_LAT
    with pytest.raises(RuntimeError, match="variant_placements and placement are both set"):
        eng.place_kw(masks, 8, 8)
    eng.placement, eng.shard = None, types.SimpleNamespace(rank=0, world=1)
    with pytest.raises(RuntimeError, match="variant_placements do not combine with the frame shard"):
        eng.place_kw(masks, 8, 8)
    with pytest.raises(RuntimeError, match="variant_placements do not combine with the frame shard"):
        eng.pnp_batch(9, masks)
    eng.shard = None
    with pytest.raises(RuntimeError, match="variant_masks is not"):
        eng.site_masks(torch.zeros(2, F, 8, 8), 1)
    eng.variant_masks = (torch.zeros(3, 2, F, 8, 8), torch.zeros(2, 2, F, 8, 8))
    assert eng.site_masks(torch.zeros(2, F, 8, 8), 0) is eng.variant_masks[0]
    with pytest.raises(RuntimeError, match=r"variant_masks\[1\] is \(2, 2, 3, 8, 8\), expected \[K = 3, 2, 3, 8, 8\]"):
        eng.site_masks(torch.zeros(2, F, 8, 8), 1)


# ---- composite.py -------------------------------------------------------------------------------------------------------
def test_composite_variant_placement_reaches_the_call(composite, tmp_path):  # noqa: F811
    ct = _template(tmp_path)
    assert "placement" in composite.VARIANT_KEYS and "obj_offset" not in composite.VARIANT_KEYS
    var = [{"seed": 1, "placement": [[64, 0], [-32, 16]]}, {"seed": 2}, {"seed": 3, "placement": [[0, 0], [[0, 0], [8, 0]]]}]
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=var))
    kw = composite.variant_placement_kwargs(config, variants)
    assert kw == {"variant_obj_offsets": [[[64, 0], [-32, 16]], None, [[0, 0], [[0, 0], [8, 0]]]]}
    assert all(type(v) is int for v in kw["variant_obj_offsets"][0][0]) and type(kw["variant_obj_offsets"][2][1][1]) is list
    from mvoc_amd.pipeline import resolve_variant_obj_offsets
    shared, per = resolve_variant_obj_offsets(kw["variant_obj_offsets"], 3, 2, 2)
    assert shared is None and per == ((((0, 8),) * 2, ((2, -4),) * 2), (((0, 0),) * 2,) * 2, (((0, 0),) * 2, ((0, 0), (0, 1))))
    # a variant without the key inherits the entry's obj_offset
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_offset=[[8, 8], [0, 0]], variants=var))
    assert composite.variant_placement_kwargs(config, variants) == {
        "variant_obj_offsets": [[[64, 0], [-32, 16]], [[8, 8], [0, 0]], [[0, 0], [[0, 0], [8, 0]]]]}
    # the suffix of the output directory does not know the key
    assert composite.output_suffix(variants[0]) == composite.output_suffix(config)


def test_composite_without_a_variant_placement_keeps_the_shared_path(composite, tmp_path):  # noqa: F811
    ct = _template(tmp_path)
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_offset=[[8, 8], [0, 0]], variants=[{"seed": 1}, {"seed": 2}]))
    assert composite.variant_placement_kwargs(config, variants) == composite.placement_kwargs(config) == {"obj_offsets": [[8, 8], [0, 0]]}
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1}, {"seed": 2}]))
    assert composite.variant_placement_kwargs(config, variants) == {}
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_offset=[[8, 8], [0, 0]]))
    assert variants is None and composite.variant_placement_kwargs(config, None) == {"obj_offsets": [[8, 8], [0, 0]]}


def test_composite_variant_still_may_not_set_obj_offset(composite, tmp_path):  # noqa: F811
    ct = _template(tmp_path)
    with pytest.raises(ValueError, match=r"variants\[1\] overrides 'obj_offset'.*a variant may set .*placement"):
        composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1, "placement": [[8, 8], [0, 0]]},
                                                           {"seed": 2, "obj_offset": [[8, 8], [0, 0]]}]))


# ---- demo_job.py -----------------------------------------------------------------------------------------------------------
def test_demo_job_parses_variant_place():
    spec = importlib.util.spec_from_file_location("demo_job_variant_place", os.path.join(REPO, "tools", "demo_job.py"))
    dj = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dj)
    assert dj.parse_variant_place("64,0;-32,16|0,0;0,0|-8,8;0,24", 3) == [[[64, 0], [-32, 16]], [[0, 0], [0, 0]], [[-8, 8], [0, 24]]]
    assert dj.parse_variant_place("8,8", 1) == [[[8, 8]]]
    for bad, k, msg in (("64,0;0,0|0,0;0,0", 0, "needs --variants"), ("64,0;0,0|0,0;0,0", 3, "2 placements for 3 variants"),
                        ("64,0;0,0|a,b;0,0", 2, "variant 1"), ("64,0;0,0|1,2,3;0,0", 2, "variant 1"),
                        ("64,0;0,0|0,0", 2, "one dx,dy per object"), ("64,0;0,0|", 2, "variant 1")):
        with pytest.raises(SystemExit, match=msg):
            dj.parse_variant_place(bad, k)


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_variant_placement_entry_points_are_declared_exported_and_bound():
    from mvoc_amd import _ffi
    hdr = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "mvoc_hip.h")).read())
    pd, i32, u32, vp = C.POINTER(_ffi.PnpDesc), _ffi.i32, C.c_uint32, _ffi.vp
    decl = ("(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, "
            "const int32_t* place, void* stream);")
    for name in ("mvoc_pnp_blend_scatter_tokens_placed_variants", "mvoc_pnp_blend_scatter_nchw_placed_variants"):
        assert f"int {name}{decl}" in hdr, name
        assert hasattr(_ffi.lib, name), name
        res, got = _ffi.SIGNATURES[name]
        assert res is i32 and got == [pd, i32, C.POINTER(i32), i32, u32, vp, vp], name
        assert getattr(_ffi.lib, name).argtypes == got
    assert "8 * nvar*nobj*frames" in hdr  # the byte formula of the profiler is stated with the entries
    assert _ffi.lib.mvoc_version() == 100
