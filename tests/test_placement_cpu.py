"""CPU: placement of objects at composition time -- the level-offset rule against exact rational rounding,
the normalisation of the sampling call's ``obj_offsets``, composite.py's ``obj_offset`` key, and the three new entry points
declared, exported and bound.  No kernel is launched."""
import ctypes as C
import importlib
import math
import os
import re
import sys
from fractions import Fraction

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the level-offset rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_h", [8, 9, 64, 90])
def test_level_offset_is_round_half_up_of_the_exact_ratio(mask_h):
    from mvoc_amd import ops
    levels = [mask_h] + [-(-mask_h // d) for d in (2, 4, 8)]  # mask_h, ceil(mask_h / 2), / 4, / 8 (90 -> 45, 23, 12)
    n = 0
    for H in levels:
        for dy in range(-mask_h - 1, mask_h + 2):
            want = math.floor(Fraction(dy * H, mask_h) + Fraction(1, 2))  # round-half-up, exact
            assert ops.level_offset(dy, H, mask_h) == want, (mask_h, H, dy)
            n += 1
        assert ops.level_offset(0, H, mask_h) == 0
    assert n == 4 * (2 * mask_h + 3)
    for dy in range(-mask_h - 1, mask_h + 2):  # the latent grid itself: the offset as given
        assert ops.level_offset(dy, mask_h, mask_h) == dy


def test_level_offsets_form_each_axis_on_its_own():
    from mvoc_amd import ops
    pl = (((3, -5), (0, 1)), ((-9, 9), (8, -8)))
    got = ops.level_offsets(pl, 5, 12, 9, 16)
    assert got == tuple(tuple((ops.level_offset(dy, 5, 9), ops.level_offset(dx, 12, 16)) for dy, dx in obj) for obj in pl)
    assert got[0][0] == (2, -4) and got[1][1] == (4, -6)  # 15/9 = 1.67 -> 2; -60/16 = -3.75 -> -4; 40/9 = 4.4 -> 4; -6.0


# ---- obj_offsets of the sampling call ------------------------------------------------------------------------------------
def test_offsets_broadcast_a_pair_and_keep_a_path():
    from mvoc_amd.pipeline import normalize_obj_offsets
    F = 3
    got = normalize_obj_offsets([(16, -8), [(0, 0), (8, 0), (16, 24)]], 2, F)
    # public (dx, dy) in image pixels -> (dy, dx) on the latent grid, one pair per frame
    assert got == (((-1, 2),) * F, ((0, 0), (0, 1), (3, 2)))
    hash(got)  # the engine keys its caches and the graph variants by it
    assert normalize_obj_offsets([[8, 8]], 1, F) == (((1, 1),) * F,)
    assert normalize_obj_offsets([(32, 0), (0, 0)], 2, 2, factor=16) == (((0, 2),) * 2, ((0, 0),) * 2)


def test_offsets_that_move_nothing_are_none():
    from mvoc_amd.pipeline import normalize_obj_offsets
    assert normalize_obj_offsets(None, 2, 4) is None
    assert normalize_obj_offsets([(0, 0), (0, 0)], 2, 4) is None
    assert normalize_obj_offsets([(0, 0), [(0, 0)] * 4], 2, 4) is None
    assert normalize_obj_offsets([(0, 0), [(0, 0), (0, 0), (0, 8), (0, 0)]], 2, 4) is not None


@pytest.mark.parametrize("bad,msg", [
    ([(8, 8), [(0, 0), (8, 8)]], r"object 1 has 2 per-frame offsets, the clip 3 frames"),
    ([(8, 8), (8, 4)], r"object 1, frame 0: \(8, 4\) is not a multiple of 8"),
    ([[(8, 8), (8, 8), (9, 8)], (0, 0)], r"object 0, frame 2: \(9, 8\) is not a multiple of 8"),
    ([(8, 8), (8.0, 8)], r"object 1 needs \(dx, dy\)"),
    ([(8, 8), (8, 8, 8)], r"object 1 needs \(dx, dy\)"),
    ([(8, 8), "8,8"], r"object 1 needs \(dx, dy\)"),
])
def test_bad_offsets_name_the_object(bad, msg):
    from mvoc_amd.pipeline import normalize_obj_offsets
    with pytest.raises(ValueError, match=msg):
        normalize_obj_offsets(bad, 2, 3)


def test_a_wrong_object_count_is_refused():
    from mvoc_amd.pipeline import normalize_obj_offsets
    with pytest.raises(ValueError, match=r"3 entries for 2 objects"):
        normalize_obj_offsets([(8, 8)] * 3, 2, 3)
    with pytest.raises(ValueError, match=r"1 entries for 2 objects"):
        normalize_obj_offsets([(0, 0)], 2, 3)  # (checked before the all-zero shortcut)


def test_engine_defaults_to_no_placement():
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cpu")
    assert eng.placement is None
    assert eng.place_kw([None, None], 8, 8) == {}  # the sites' calls carry no extra argument


# ---- composite.py -------------------------------------------------------------------------------------------------------
@pytest.fixture
def composite():
    ref = os.path.join(REPO, "i2vgen-xl")
    sys.path.insert(0, ref)
    mods = ("utils", "pnp_utils", "composite", "inverse", "pipelines", "pipelines.pipeline_i2vgen_xl", "common")
    saved = {m: sys.modules.pop(m) for m in mods if m in sys.modules}
    try:
        mod = importlib.import_module("composite")
        assert mod.__file__.startswith(REPO)
        yield mod
    finally:
        sys.path.remove(ref)
        for m in mods:
            sys.modules.pop(m, None)
        sys.modules.update(saved)


def _template(tmp):
    from mvoc_amd.config import OmegaConf
    ct = OmegaConf.load(os.path.join(REPO, "tests", "data", "composite_template.yaml"))
    ct.data_dir = str(tmp)
    return ct


ENTRY = dict(active=True, video_name="boat", edited_video_name="boat_surf", edited_first_frame_path="edit/first.png",
             editing_prompt="a boat and a surfer", obj_ddim_latents_path=["inv/o0", "inv/o1"], obj_mask_path=["m/0", "m/1"],
             obj_width_height=[[64, 64], [64, 64]], edited_contorl_frame_path=["f/o0", "f/o1"],
             edited_contorl_frame_path_main="f/main", edited_contorl_frame_path_background="f/bg")


def test_composite_obj_offset_reaches_the_call(composite, tmp_path):
    ct = _template(tmp_path)
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_offset=[[16, -8], [[0, 0], [8, 0]]]))
    assert variants is None
    kw = composite.placement_kwargs(config)
    assert kw == {"obj_offsets": [[16, -8], [[0, 0], [8, 0]]]}
    assert all(type(v) is int for v in kw["obj_offsets"][0]) and type(kw["obj_offsets"][1][1]) is list  # plain lists of ints
    from mvoc_amd.pipeline import normalize_obj_offsets
    assert normalize_obj_offsets(kw["obj_offsets"], 2, 2) == (((-1, 2), (-1, 2)), ((0, 0), (0, 1)))
    # shared by an entry's variants: the entry's key reaches every variant's merged config
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_offset=[[8, 8], [0, 0]], variants=[{"seed": 1}, {"seed": 2}]))
    assert composite.placement_kwargs(config) == {"obj_offsets": [[8, 8], [0, 0]]}
    assert all(composite.placement_kwargs(v) == {"obj_offsets": [[8, 8], [0, 0]]} for v in variants)


def test_composite_without_obj_offset_passes_no_argument(composite, tmp_path):
    ct = _template(tmp_path)
    config, _ = composite.merge_variants(ct, ENTRY)
    assert composite.placement_kwargs(config) == {}
    assert "obj_offset" not in config
    # the suffix of the output directory does not know the key
    placed, _ = composite.merge_variants(ct, dict(ENTRY, obj_offset=[[8, 8], [0, 0]]))
    assert composite.output_suffix(placed) == composite.output_suffix(config)


def test_composite_variant_may_not_set_obj_offset(composite, tmp_path):
    ct = _template(tmp_path)
    with pytest.raises(ValueError, match=r"variants\[1\] overrides 'obj_offset'"):
        composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1}, {"seed": 2, "obj_offset": [[8, 8], [0, 0]]}]))


def test_demo_job_parses_place():
    spec = importlib.util.spec_from_file_location("demo_job_place", os.path.join(REPO, "tools", "demo_job.py"))
    dj = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dj)
    assert dj.parse_place("64,0;-32,16") == [[64, 0], [-32, 16]]
    for bad in ("64;0", "a,b", "1,2,3"):
        with pytest.raises(SystemExit):
            dj.parse_place(bad)


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_placement_entry_points_are_declared_exported_and_bound():
    from mvoc_amd import _ffi
    hdr = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "mvoc_hip.h")).read())
    pd, i32, u32, vp = C.POINTER(_ffi.PnpDesc), _ffi.i32, C.c_uint32, _ffi.vp
    placed = ("(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, "
              "const int32_t* place, void* stream);")
    want = {
        "mvoc_pnp_blend_scatter_tokens_placed": (placed, [pd, i32, C.POINTER(i32), i32, u32, vp, vp]),
        "mvoc_pnp_blend_scatter_nchw_placed": (placed, [pd, i32, C.POINTER(i32), i32, u32, vp, vp]),
        "mvoc_shift_planes_f16": ("(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w, "
                                  "const int32_t* offsets, void* stream);", [vp, vp, i32, i32, i32, i32, vp, vp]),
    }
    for name, (decl, args) in want.items():
        assert f"int {name}{decl}" in hdr, name
        assert hasattr(_ffi.lib, name), name
        res, got = _ffi.SIGNATURES[name]
        assert res is i32 and got == args, name
        assert getattr(_ffi.lib, name).argtypes == args
    assert _ffi.lib.mvoc_version() == 100


def test_the_sel_entries_and_the_descriptor_are_unchanged():
    from mvoc_amd import _ffi
    pd = C.POINTER(_ffi.PnpDesc)
    assert [f[0] for f in _ffi.PnpDesc._fields_] == ["x", "x2", "masks", "chunk_stride", "f_stride", "p_stride", "nobj", "frames",
                                                    "height", "width", "channels", "mask_h", "mask_w", "base_chunk0", "ndst"]
    for name in ("mvoc_pnp_blend_scatter_tokens_variants_sel", "mvoc_pnp_blend_scatter_nchw_variants_sel"):
        assert _ffi.SIGNATURES[name][1] == [pd, _ffi.i32, C.POINTER(_ffi.i32), _ffi.i32, C.c_uint32, _ffi.vp]
