"""CPU-only: per-variant object transforms -- how ``variant_obj_transforms`` resolves to the older arguments, the
per-variant table rule, the engine's defaults and refusals, the drivers' key flow, the C ABI and the compiler's resource remarks
of the new translation unit."""
import ctypes as C
import importlib
import inspect
import os
import re
import sys
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = 3
A = [{"scale": "3/2", "flip": "h", "offset": [(8, 0), (16, -8), (24, -16)]}, {"scale": [1, 0.5], "flip": "v", "anchor": [40, 24]}]
B = [{"scale": "1/2", "anchor": [16, 48]}, {"offset": (-16, 8)}]
MOVE_A = [{"offset": (8, -8)}, {}]
MOVE_B = [{}, {"offset": [(0, 8), (8, 8), (16, 8)], "scale": "2/2"}]
IDENT = [{"scale": 1.0, "flip": None, "anchor": [8, 16]}, None]


def _resolve(items, nvar=3, n_obj=2):
    from mvoc_amd.pipeline import resolve_variant_obj_transforms
    return resolve_variant_obj_transforms(items, nvar, n_obj, F, 8, 8)


# ---- resolution -------------------------------------------------------------------------------------------------------------
def test_identity_variants_are_a_call_without_the_argument():
    assert _resolve(None) == (None, None, None, None)
    assert _resolve([None, IDENT, [{}, {}]]) == (None, None, None, None)


def test_equal_variants_are_the_shared_obj_transforms_call():
    from mvoc_amd.pipeline import normalize_obj_transforms, normalize_obj_offsets
    pl, tr = normalize_obj_transforms(A, 2, F, 8, 8)
    assert pl is None and tr is not None
    assert _resolve([A, [dict(d) for d in A], A]) == (None, None, tr, None)
    # ... which itself falls to obj_offsets when it only translates
    want = normalize_obj_offsets([(8, -8), (0, 0)], 2, F)
    assert normalize_obj_transforms(MOVE_A, 2, F, 8, 8) == (want, None)
    assert _resolve([MOVE_A] * 3) == (want, None, None, None)


def test_translation_only_variants_are_the_variant_obj_offsets_call():
    from mvoc_amd.pipeline import resolve_variant_obj_offsets
    older = resolve_variant_obj_offsets([[(8, -8), (0, 0)], None, [(0, 0), [(0, 8), (8, 8), (16, 8)]]], 3, 2, F)
    assert older[0] is None and older[1] is not None
    assert _resolve([MOVE_A, IDENT, MOVE_B]) == (None, older[1], None, None)


def test_differing_variants_keep_every_variant_as_a_full_transform():
    from mvoc_amd.pipeline import normalize_obj_transforms
    got = _resolve([A, None, MOVE_B])
    assert got[:3] == (None, None, None)
    vt = got[3]
    assert len(vt) == 3 and vt[0] == normalize_obj_transforms(A, 2, F, 8, 8)[1]
    zero = ((0, 0),) * F
    assert vt[1] == ((1, 1, 1, 1, False, False, 8, 8, zero),) * 2  # identity: scale 1/1, no flip, the frame centre, zero offsets
    assert vt[2] == ((1, 1, 1, 1, False, False, 8, 8, zero), (1, 1, 1, 1, False, False, 8, 8, ((1, 0), (1, 1), (1, 2))))  # no downgrade
    hash(vt)
    assert _resolve([A, B, A])[3] == (vt[0], normalize_obj_transforms(B, 2, F, 8, 8)[1], vt[0])


@pytest.mark.parametrize("items, msg", [
    ([A, None, [{"scale": 0}, {}]], r"variant 2: obj_transforms: object 0: scale 0"),
    ([A, [{}, {"flip": "x"}], None], r"variant 1: obj_transforms: object 1: flip 'x'"),
    ([[{}, {}, {}], None, None], r"variant 0: obj_transforms: 3 entries for 2 objects"),
    ([None, None, [{"offset": (4, 0)}, {}]], r"variant 2: obj_transforms: object 0: offset"),
    ([A, "x", None], r"variant 1: obj_transforms: needs a list of 2 dicts"),
    ([A, B], r"variant_obj_transforms: 2 entries for 3 variants"),
    ({"scale": 2}, r"variant_obj_transforms: needs a list of 3 items"),
])
def test_bad_items_name_the_variant_and_the_object(items, msg):
    with pytest.raises(ValueError, match=msg):
        _resolve(items)


def test_the_call_refuses_argument_mixes_before_anything_runs():
    from mvoc_amd.pipeline import I2VGenXLPipeline
    fn = I2VGenXLPipeline.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection
    assert inspect.signature(fn).parameters["variant_obj_transforms"].default is None
    pipe = I2VGenXLPipeline.__new__(I2VGenXLPipeline)  # no engine: the refusal comes before the conditioner is used
    pipe.conditioner = None
    for kw in ({"obj_offsets": [(8, 8), (0, 0)]}, {"variant_obj_offsets": [[(8, 8), (0, 0)]]}, {"obj_transforms": [{"scale": 2}, {}]}):
        with pytest.raises(ValueError, match="variant_obj_transforms is given together with obj_transforms / obj_offsets / variant_obj_offsets"):
            fn(pipe, prompt="a", obj_ddim_latents_path=["o0", "o1"], variant_obj_transforms=[A], num_frames=F, **kw)
    pipe.vae_scale_factor = 8
    with pytest.raises(ValueError, match="variant_obj_transforms: 2 entries for 1 variants"):
        fn(pipe, prompt="a", obj_ddim_latents_path=["o0", "o1"], variant_obj_transforms=[A, B], num_frames=F, height=64, width=64)


# ---- the table rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(5, 12, 9, 16), (4, 4, 8, 8)])
def test_table_row_k_is_the_resample_table_of_transform_k(grid):
    from mvoc_amd import ops
    from mvoc_amd.pipeline import normalize_obj_transforms
    H, W, mh, mw = grid
    ident = _resolve([A, None, B])[3][1]
    vt = (normalize_obj_transforms(A, 2, F, mh, mw)[1], ident, normalize_obj_transforms(B, 2, F, mh, mw)[1])
    tab = ops.resample_table_variants(vt, H, W, mh, mw, "cpu")
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (3, 2, F, H + W) and tab.is_contiguous()
    for k, tr in enumerate(vt):
        assert torch.equal(tab[k], ops.resample_table(tr, H, W, mh, mw, "cpu")), k
        assert tab[k].tolist() == ops.transform_maps(tr, H, W, mh, mw)
    assert not torch.equal(tab[0], tab[2])
    with pytest.raises(RuntimeError, match="at least one variant"):
        ops.resample_table_variants((), H, W, mh, mw, "cpu")
    with pytest.raises(RuntimeError, match="variant 1: transform_maps"):
        ops.resample_table_variants((vt[0], ()), H, W, mh, mw, "cpu")
    with pytest.raises(RuntimeError, match="differ in shape"):
        ops.resample_table_variants((vt[0], vt[0][:1]), H, W, mh, mw, "cpu")


# ---- engine -----------------------------------------------------------------------------------------------------------------
def test_engine_defaults_and_refusals():
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cpu")
    assert eng.variant_transforms is None and eng.place_kw([None, None], 8, 8) == {}
    tr = ((2, 1, 2, 1, False, False, 8, 8, ((0, 0),)),) * 2
    eng.variant_transforms, eng.variants = (tr, tr), 2
    for attr, val in (("placement", (((1, 0),),) * 2), ("variant_placements", ((((1, 0),),) * 2,) * 2), ("transform", tr)):
        setattr(eng, attr, val)
        with pytest.raises(RuntimeError, match="variant_transforms is set together with placement / variant_placements / transform"):
            eng.place_kw([None, None], 8, 8)
        setattr(eng, attr, None)
    eng.variants = 3
    with pytest.raises(RuntimeError, match="variant_transforms holds 2 transforms, the call 3 variants"):
        eng.place_kw([None, None], 8, 8)
    eng.variants = 2
    with pytest.raises(RuntimeError, match=r"variant_transforms\[0\] holds 2 objects, the hooks carry 3 masks"):
        eng.place_kw([None, None, None], 8, 8)
    with pytest.raises(RuntimeError, match="variant_transforms is set but variant_masks is not"):
        eng.site_masks(torch.zeros(2, 1, 8, 8), 0)
    eng.shard = types.SimpleNamespace(rank=0, world=1)
    with pytest.raises(RuntimeError, match="frame shard"):
        eng.place_kw([None, None], 8, 8)
    with pytest.raises(RuntimeError, match="frame shard"):
        eng.pnp_batch(7, [None, None])


# ---- composite.py and tools/demo_job.py ---------------------------------------------------------------------------------------
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
T_A = [{"scale": "3/2", "flip": "h", "offset": [64, 0]}, {"scale": [0.5, 2], "anchor": [12, 40]}]
T_B = [{"scale": "1/2"}, {}]


def test_composite_variant_transform_reaches_the_call(composite, tmp_path):
    ct = _template(tmp_path)
    assert "transform" in composite.VARIANT_KEYS
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1, "transform": T_A}, {"seed": 2}, {"seed": 3, "transform": T_B}]))
    kw = composite.transform_kwargs(config, variants)
    assert kw == {"variant_obj_transforms": [T_A, None, T_B]}
    assert all(type(d) is dict for d in kw["variant_obj_transforms"][0]) and type(kw["variant_obj_transforms"][0][0]["offset"]) is list
    # a variant without the key takes the entry's obj_transform
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_transform=T_B, variants=[{"seed": 1, "transform": T_A}, {"seed": 2}]))
    assert composite.transform_kwargs(config, variants) == {"variant_obj_transforms": [T_A, T_B]}
    plain, _ = composite.merge_variants(ct, ENTRY)
    assert composite.output_suffix(config) == composite.output_suffix(plain)


def test_composite_without_the_key_passes_what_it_passed(composite, tmp_path):
    ct = _template(tmp_path)
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1}, {"seed": 2}]))
    assert composite.transform_kwargs(config, variants) == {}
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_transform=T_A, variants=[{"seed": 1}, {"seed": 2}]))
    assert composite.transform_kwargs(config, variants) == {"obj_transforms": T_A}
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1, "placement": [[8, 8], [0, 0]]}, {"seed": 2}]))
    assert composite.transform_kwargs(config, variants) == {"variant_obj_offsets": [[[8, 8], [0, 0]], None]}
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_transform=T_A, variants=[{"seed": 1}, {"seed": 2, "placement": [[8, 8], [0, 0]]}]))
    with pytest.raises(ValueError, match="obj_transform is set and a variant sets 'placement'"):
        composite.transform_kwargs(config, variants)


def test_composite_key_errors(composite, tmp_path):
    ct = _template(tmp_path)
    with pytest.raises(ValueError, match=r"variants\[1\] overrides 'obj_transform'"):
        composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1}, {"seed": 2, "obj_transform": T_A}]))
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_offset=[[8, 8], [0, 0]], variants=[{"seed": 1, "transform": T_A}, {"seed": 2}]))
    with pytest.raises(ValueError, match=r"put the offset into the transform \('offset'\)"):
        composite.transform_kwargs(config, variants)
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1, "transform": T_A}, {"seed": 2, "placement": [[8, 8], [0, 0]]}]))
    with pytest.raises(ValueError, match=r"a variant sets 'placement': put the offset into the transform \('offset'\)"):
        composite.transform_kwargs(config, variants)


def test_demo_job_parses_variant_transform():
    spec = importlib.util.spec_from_file_location("demo_job_variant_transform", os.path.join(REPO, "tools", "demo_job.py"))
    dj = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dj)
    got = dj.parse_variant_transform("scale=3/2,flip=h;scale=1/2||offset=64,0;", 3)
    assert got == [[{"scale": "3/2", "flip": "h"}, {"scale": "1/2"}], None, [{"offset": [64, 0]}, {}]]
    assert dj.parse_variant_transform(" |scale=2;", 2) == [None, [{"scale": 2}, {}]]
    with pytest.raises(SystemExit, match="needs --variants K"):
        dj.parse_variant_transform("scale=2;", 0)
    with pytest.raises(SystemExit, match="2 transforms for 3 variants"):
        dj.parse_variant_transform("scale=2;|", 3)
    with pytest.raises(SystemExit, match="--variant-transform, variant 1: --transform, object 0"):
        dj.parse_variant_transform("scale=2;|64,0;", 2)
    with pytest.raises(SystemExit, match="one item per object"):
        dj.parse_variant_transform("scale=2;|scale=2", 2)


# ---- ABI and compiler report ------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from mvoc_amd import _ffi, build
    assert "pnp_variants2.hip" in build.SOURCES
    hdr = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "mvoc_hip.h")).read())
    pd, i32, u32, vp = C.POINTER(_ffi.PnpDesc), _ffi.i32, C.c_uint32, _ffi.vp
    decl = ("(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, "
            "const int32_t* maps, void* stream);")
    for name in ("mvoc_pnp_blend_scatter_tokens_resampled_variants", "mvoc_pnp_blend_scatter_nchw_resampled_variants"):
        assert f"int {name}{decl}" in hdr, name
        assert hasattr(_ffi.lib, name), name
        res, got = _ffi.SIGNATURES[name]
        assert res is i32 and got == [pd, i32, C.POINTER(i32), i32, u32, vp, vp], name
        assert getattr(_ffi.lib, name).argtypes == got
    assert _ffi.lib.mvoc_version() == 100 and _ffi.ABI_VERSION == 100


def _remarks(obj):
    from mvoc_amd import build
    build.build(verbose=False)
    seen, name = {}, None
    for line in open(os.path.join(REPO, "mvoc_amd", "csrc", obj + ".res.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]"):
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m and name:
                seen[name][key] = int(m.group(1))
    return seen


def test_the_twelve_kernels_run_without_scratch_at_their_twins_occupancy():
    new, old = _remarks("pnp_variants2.o"), _remarks("pnp.o")
    assert len(new) == 12, sorted(new)
    forms = set()
    for name, r in sorted(new.items()):
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        m = re.search(r"\d+pnp_(tokens|nchw)_resampled_variants_kernelIL?i?(\d*)E?Li([1-4])E", name)
        assert m, name
        layout, vec, nobj = m.group(1), m.group(2), int(m.group(3))
        forms.add((layout, vec, nobj))
        if layout == "tokens" or vec == "1":
            assert r["Occupancy [waves/SIMD]"] == 8, (name, r)
        else:  # nchw<8, NOBJ>: not below the _placed_variants twin of the same build
            twin = name.replace("34pnp_nchw_resampled_variants_kernel", "31pnp_nchw_placed_variants_kernel")
            assert twin != name and twin in old, name
            assert r["Occupancy [waves/SIMD]"] >= old[twin]["Occupancy [waves/SIMD]"], (name, r, old[twin])
    assert forms == {("tokens", "", n) for n in (1, 2, 3, 4)} | {("nchw", v, n) for v in ("8", "1") for n in (1, 2, 3, 4)}, forms
