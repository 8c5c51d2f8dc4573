"""CPU: K variants over one set of source chunks -- the four new entry points are declared, exported and
bound; the batch layout planner as a pure function; composite.py's merge of an entry's ``variants``.  No kernel is launched."""
import ctypes as C
import importlib
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_variant_entry_points_are_declared_exported_and_bound():
    from mvoc_amd import _ffi
    hdr = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "mvoc_hip.h")).read())
    pd, i32, i64, f64, vp = C.POINTER(_ffi.PnpDesc), _ffi.i32, _ffi.i64, _ffi.f64, _ffi.vp
    want = {
        "mvoc_pnp_blend_scatter_tokens_variants":
            ("(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, void* stream);",
             [pd, i32, C.POINTER(i32), i32, vp]),
        "mvoc_pnp_blend_scatter_nchw_variants":
            ("(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, void* stream);",
             [pd, i32, C.POINTER(i32), i32, vp]),
        "mvoc_ddim_step_variants_f16":
            ("(const void* x, const void* v_uncond, const void* v_cond, const float* coef_dev, void* out, int64_t n_per, "
             "int32_t nvar, void* stream);", [vp, vp, vp, vp, vp, i64, i32, vp]),
        "mvoc_latent_fusion_variants_f16":
            ("(const void* latents, const void* bg, const void* objs, const void* masks, void* out, int32_t nobj, "
             "int64_t n_per, int32_t nvar, double mix_ratio, int32_t obj_random_noise_fusion, void* stream);",
             [vp, vp, vp, vp, vp, i32, i64, i32, f64, i32, vp]),
    }
    for name, (decl, args) in want.items():
        assert f"int {name}{decl}" in hdr, name
        assert hasattr(_ffi.lib, name), name
        res, got = _ffi.SIGNATURES[name]
        assert res is i32 and got == args, name
        assert getattr(_ffi.lib, name).argtypes == args
    assert _ffi.lib.mvoc_version() == 100


def test_existing_pnp_descriptor_and_entries_are_unchanged():
    from mvoc_amd import _ffi
    assert [f[0] for f in _ffi.PnpDesc._fields_] == ["x", "x2", "masks", "chunk_stride", "f_stride", "p_stride", "nobj", "frames",
                                                    "height", "width", "channels", "mask_h", "mask_w", "base_chunk0", "ndst"]
    pd = C.POINTER(_ffi.PnpDesc)
    assert _ffi.SIGNATURES["mvoc_pnp_blend_scatter_tokens"][1] == [pd, _ffi.vp]
    assert _ffi.SIGNATURES["mvoc_pnp_blend_scatter_nchw_mapped"][1] == [pd, _ffi.i32, C.POINTER(_ffi.i32), _ffi.vp]
    assert _ffi.SIGNATURES["mvoc_ddim_step_f16"][1] == [_ffi.vp] * 5 + [_ffi.i64, _ffi.vp]


# ---- layout ----------------------------------------------------------------------------------------------------------
def _maps(n_obj):
    out = [None, (1, (0,) * n_obj)]
    if n_obj >= 2:
        out += [(2, (1,) * n_obj), (2, (1, 0) + (1,) * (n_obj - 2)), (n_obj, tuple(range(1, n_obj)) + (0,))]
    return out


@pytest.mark.parametrize("do_cfg", [True, False])
@pytest.mark.parametrize("n_obj", [1, 2, 3, 4])
def test_layout_chunk_indices(n_obj, do_cfg):
    from mvoc_amd.pipeline import variant_layout
    for smap in _maps(n_obj):
        nsrc = n_obj + 1 if smap is None else smap[0]
        chunks = tuple(range(1, n_obj + 1)) if smap is None else smap[1]
        for K in range(1, 9):
            lay = variant_layout(n_obj, K, do_cfg, smap)
            ndst = 2 if do_cfg else 1
            assert lay["nsrc"] == nsrc and lay["ndst"] == ndst and lay["nb"] == nsrc + ndst * K
            assert lay["src"] == [0] + list(chunks) and lay["obj_chunks"] == chunks
            # blocks: [s.., u_1..u_K, c_1..c_K]; the c block at a constant offset K behind the u block
            if do_cfg:
                assert lay["u"] == list(range(nsrc, nsrc + K))
                assert lay["c"] == [u + K for u in lay["u"]]
            else:
                assert lay["u"] is None and lay["c"] == list(range(nsrc, nsrc + K))
            used = sorted(set(lay["src"]) | set(lay["u"] or []) | set(lay["c"]))
            assert used == list(range(lay["nb"]))  # every chunk of the batch has exactly one meaning
            assert lay["c"][-1] == lay["nb"] - 1


@pytest.mark.parametrize("do_cfg", [True, False])
@pytest.mark.parametrize("n_obj", [1, 2, 3, 4])
def test_layout_one_variant_is_the_positional_batch(n_obj, do_cfg):
    """[bg, obj_1..obj_n, (uncond,) cond]: what check_pnp_batch and the unmapped kernels address today"""
    from mvoc_amd.pipeline import variant_layout
    from mvoc_amd.unet import I2VGenXLUNet
    lay = variant_layout(n_obj, 1, do_cfg)
    nb = n_obj + (3 if do_cfg else 2)
    assert lay["nb"] == nb and lay["src"] == list(range(n_obj + 1)) and lay["c"] == [nb - 1]
    assert lay["u"] == ([nb - 2] if do_cfg else None)
    assert I2VGenXLUNet.check_pnp_batch(nb, [None] * n_obj) == lay["ndst"]
    for K in (2, 5, 8):
        layk = variant_layout(n_obj, K, do_cfg)
        assert I2VGenXLUNet.check_pnp_batch(layk["nb"], [None] * n_obj, None, K) == lay["ndst"]
        with pytest.raises(RuntimeError, match="UNet batch"):
            I2VGenXLUNet.check_pnp_batch(layk["nb"] + 1 + 2 * K, [None] * n_obj, None, K)
        m = (1, (0,) * n_obj)
        assert I2VGenXLUNet.check_pnp_batch(variant_layout(n_obj, K, do_cfg, m)["nb"], [None] * n_obj, 1, K) == lay["ndst"]


def test_layout_refuses_what_the_kernels_refuse():
    from mvoc_amd.pipeline import variant_layout
    for K in (0, 9, -1):
        with pytest.raises(ValueError, match="variants"):
            variant_layout(2, K)
    with pytest.raises(ValueError, match="source map"):
        variant_layout(2, 2, True, (2, (0, 2)))
    with pytest.raises(ValueError, match="source map"):
        variant_layout(2, 2, True, (1, (0,)))
    with pytest.raises(ValueError, match="objects"):
        variant_layout(5, 2)


def test_gemm_offset_line():
    """16 x 64 x 64: B <= 12 keeps the widest level-0 tensor [B * 65536, 1280] fp16 under 2 GB -- K <= 4 with two objects"""
    from mvoc_amd.pipeline import crosses_gemm_offset_line, variant_layout
    for K in range(1, 9):
        nb = variant_layout(2, K)["nb"]
        assert crosses_gemm_offset_line(nb, 16, 64, 64, 320) == (K > 4), (K, nb)
    assert not crosses_gemm_offset_line(12, 16, 64, 64, 320) and crosses_gemm_offset_line(13, 16, 64, 64, 320)


# ---- composite.py -----------------------------------------------------------------------------------------------------
@pytest.fixture
def composite():
    ref = os.path.join(REPO, "i2vgen-xl")
    sys.path.insert(0, ref)
    saved = {m: sys.modules.pop(m) for m in ("utils", "pnp_utils", "composite", "inverse", "pipelines", "pipelines.pipeline_i2vgen_xl",
                                             "common") if m in sys.modules}
    try:
        mod = importlib.import_module("composite")
        assert mod.__file__.startswith(REPO)
        yield mod
    finally:
        sys.path.remove(ref)
        for m in ("utils", "pnp_utils", "composite", "inverse", "pipelines", "pipelines.pipeline_i2vgen_xl", "common"):
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


def test_composite_entry_without_variants_is_untouched(composite, tmp_path):
    from mvoc_amd.config import OmegaConf
    ct = _template(tmp_path)
    config, variants = composite.merge_variants(ct, ENTRY)
    assert variants is None
    # exactly the merge and the path resolution of a single composition
    want = OmegaConf.merge(ct, OmegaConf.create(ENTRY))
    d = str(tmp_path)
    assert config.editing_prompt == want.editing_prompt == "a boat and a surfer" and config.cfg == 9.0 and config.seed == 6
    assert config.edited_first_frame_path == os.path.join(d, "edit/first.png")
    assert config.obj_ddim_latents_path == [os.path.join(d, "inv/o0"), os.path.join(d, "inv/o1")]
    assert config.edited_contorl_frame_path_main == os.path.join(d, "f/main")
    assert config.bg_ddim_latents_path == os.path.join(d, want.bg_ddim_latents_path)
    assert config.output_dir == want.output_dir
    assert "variants" not in config
    assert ENTRY.get("variants") is None  # the caller's entry is not edited


def test_composite_variants_merge_overrides_and_output_dirs(composite, tmp_path):
    ct = _template(tmp_path)
    vs = [{}, {"editing_prompt": "a boat and a swimmer", "seed": 11}, {"cfg": 7.5, "editing_negative_prompt": "dull"},
          {"edited_first_frame_path": "edit/other.png", "edited_contorl_frame_path_main": "f/main2"}]
    entry = dict(ENTRY, variants=vs)
    config, variants = composite.merge_variants(ct, entry)
    assert len(variants) == 4 and "variants" in entry
    d = str(tmp_path)
    assert [v.editing_prompt for v in variants] == ["a boat and a surfer", "a boat and a swimmer"] + ["a boat and a surfer"] * 2
    assert [v.seed for v in variants] == [6, 11, 6, 6]
    assert [v.cfg for v in variants] == [9.0, 9.0, 7.5, 9.0]
    assert [v.editing_negative_prompt for v in variants] == ["blurry", "blurry", "dull", "blurry"]
    assert variants[3].edited_first_frame_path == os.path.join(d, "edit/other.png")
    assert variants[3].edited_contorl_frame_path_main == os.path.join(d, "f/main2")
    assert variants[0].edited_first_frame_path == config.edited_first_frame_path
    for v in variants:  # shared keys: the entry's
        assert v.obj_ddim_latents_path == config.obj_ddim_latents_path and v.n_steps == config.n_steps
        assert v.output_dir == config.output_dir
    for k, v in enumerate(variants):
        od = composite.variant_output_dir(v, k)
        assert od == os.path.join(v.output_dir, composite.output_suffix(v), f"variant_{k:02d}")
    # the suffix follows the variant's own merged config (its cfg)
    assert "_cfg_7.5_" in composite.variant_output_dir(variants[2], 2) and "_cfg_9.0_" in composite.variant_output_dir(variants[1], 1)
    assert composite.variant_output_dir(variants[0], 0).startswith(os.path.join(config.output_dir, composite.output_suffix(config)))


@pytest.mark.parametrize("key,value", [("pnp_f_t", 0.4), ("pnp_temp_attn_t", 1.0), ("obj_mask_path", ["m/2", "m/3"]), ("n_steps", 10),
                                       ("random_noise_ratio", 0.1), ("fusion_step", [0, 1]), ("inject_background", True)])
def test_composite_variant_may_not_override_a_shared_key(composite, tmp_path, key, value):
    ct = _template(tmp_path)
    with pytest.raises(ValueError, match=rf"variants\[1\] overrides '{key}'"):
        composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1}, {"seed": 2, key: value}]))


def test_composite_variant_count_is_bounded(composite, tmp_path):
    ct = _template(tmp_path)
    with pytest.raises(ValueError, match="1 to 8"):
        composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": i} for i in range(9)]))
    with pytest.raises(ValueError, match="1 to 8"):
        composite.merge_variants(ct, dict(ENTRY, variants=[]))
