"""CPU: scale and mirror of objects at composition time -- the per-axis index-map rule (its two reductions to the
placement of DESIGN.md 6k, known answers, monotonicity), the normalisation of the sampling call's ``obj_transforms``,
composite.py's ``obj_transform`` key, tools/demo_job.py's ``--transform``, and the three new entry points declared, exported and
bound.  No kernel is launched."""
import ctypes as C
import importlib
import inspect
import os
import re
import sys
from fractions import Fraction

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# latent axis L -> feature axes S (the levels of 64, 90 and 160 rows, and two odd pairs: a level LARGER than the mask grid too)
GRIDS = [(64, 64), (64, 32), (64, 8), (90, 45), (90, 23), (90, 12), (160, 80), (160, 40), (160, 20), (5, 3), (12, 23)]
ANCHORS = lambda L: sorted({L, 0, 1, L - 3, 2 * L, 2 * L + 5, -7})  # twice the anchor: the centre, edges, odd, outside


# ---- the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,S", GRIDS)
def test_unit_scale_without_a_flip_is_the_translation_of_6k_for_every_anchor(L, S):
    from mvoc_amd import ops
    n = 0
    for d in range(-L - 2, L + 3):
        df = ops.level_offset(d, S, L)
        want = [i - df if 0 <= i - df < S else -1 for i in range(S)]
        for a2 in ANCHORS(L):
            for p in (1, 3, 64):  # an unreduced p == q says the same
                assert ops.level_axis_map(d, p, p, False, a2, S, L) == want, (d, a2, p)
                n += 1
    assert n == (2 * L + 5) * len(ANCHORS(L)) * 3


@pytest.mark.parametrize("L,S", GRIDS)
def test_unit_scale_with_a_flip_about_the_centre_is_the_exact_mirror(L, S):
    from mvoc_amd import ops
    for d in range(-L - 2, L + 3):
        df = ops.level_offset(d, S, L)
        want = [S - 1 - (i - df) if 0 <= S - 1 - (i - df) < S else -1 for i in range(S)]
        assert ops.level_axis_map(d, 1, 1, True, L, S, L) == want, d
        assert ops.level_axis_map(d, 5, 5, True, L, S, L) == want, d


def test_known_answers_on_an_eight_row_axis():
    from mvoc_amd import ops
    m = lambda p, q, flip=False, d=0: ops.level_axis_map(d, p, q, flip, 8, 8, 8)
    assert m(2, 1) == [2, 2, 3, 3, 4, 4, 5, 5]
    assert m(1, 2) == [-1, -1, 1, 3, 5, 7, -1, -1]
    assert m(3, 2) == [1, 2, 3, 3, 4, 5, 5, 6]
    assert m(2, 1, True) == [5, 5, 4, 4, 3, 3, 2, 2]
    assert m(2, 1, d=1) == [1, 2, 2, 3, 3, 4, 4, 5]
    assert m(1, 1) == list(range(8)) and m(1, 1, True) == list(range(7, -1, -1))


def test_the_rule_is_the_floor_of_the_exact_rational():
    """source centre = anchor + sign * (destination centre - offset - anchor) * q / p at the level, floor = nearest on centres"""
    from mvoc_amd import ops
    for (L, S), (p, q), flip, a2, d in [((90, 23), (3, 2), False, 90, 7), ((90, 23), (7, 5), True, 31, -11), ((12, 23), (1, 3), True, 12, 2),
                                        ((64, 8), (64, 1), False, 64, 0), ((64, 8), (1, 64), False, 64, 0), ((5, 3), (2, 3), True, 3, -1)]:
        df = ops.level_offset(d, S, L)
        a = Fraction(a2 * S, 2 * L)
        want = []
        for i in range(S):
            c = a + (-1 if flip else 1) * (Fraction(2 * (i - df) + 1, 2) - a) * Fraction(q, p)
            s = c.numerator // c.denominator
            want.append(s if 0 <= s < S else -1)
        assert ops.level_axis_map(d, p, q, flip, a2, S, L) == want, (L, S, p, q, flip, a2, d)


@pytest.mark.parametrize("L,S", GRIDS)
def test_every_map_is_monotone_and_in_range(L, S):
    from mvoc_amd import ops
    scales = [(1, 1), (2, 1), (1, 2), (3, 2), (2, 3), (64, 1), (1, 64), (63, 64), (64, 63), (7, 5)]
    for (p, q), flip, a2, d in [(s, f, a, d) for s in scales for f in (False, True) for a in ANCHORS(L) for d in (0, 1, -3, L // 2, -L - 2)]:
        m = ops.level_axis_map(d, p, q, flip, a2, S, L)
        assert len(m) == S and all(type(v) is int and -1 <= v < S for v in m)
        present = [v for v in m if v >= 0]
        steps = [b - a for a, b in zip(present, present[1:])]
        assert all(s <= 0 for s in steps) if flip else all(s >= 0 for s in steps), (p, q, flip, a2, d, m)
        first = [i for i, v in enumerate(m) if v >= 0]
        assert not first or first == list(range(first[0], first[-1] + 1))  # the object covers ONE run of destinations


def test_maps_and_table_lay_out_y_then_x_per_frame():
    from mvoc_amd import ops
    tr = ((3, 2, 1, 2, False, True, 9, 16, ((1, -2), (0, 3))), (1, 1, 1, 1, False, False, 9, 16, ((0, 0), (2, 2))))
    rows = ops.transform_maps(tr, 5, 12, 9, 16)
    assert len(rows) == 2 and all(len(o) == 2 and all(len(r) == 17 for r in o) for o in rows)
    for j, (py, qy, px, qx, fy, fx, ay2, ax2, offs) in enumerate(tr):
        for f, (dy, dx) in enumerate(offs):
            assert rows[j][f][:5] == ops.level_axis_map(dy, py, qy, fy, ay2, 5, 9)
            assert rows[j][f][5:] == ops.level_axis_map(dx, px, qx, fx, ax2, 12, 16)
    tab = ops.resample_table(tr, 5, 12, 9, 16, "cpu")
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (2, 2, 17) and tab.tolist() == rows
    with pytest.raises(RuntimeError, match="same number"):
        ops.transform_maps((tr[0], tr[1][:8] + (((0, 0),),)), 5, 12, 9, 16)
    with pytest.raises(RuntimeError, match="positive"):
        ops.level_axis_map(0, 0, 1, False, 8, 8, 8)


def _gather(src, ymap, xmap):
    """the gather in torch: out[.., y, x] = src[.., ymap[y], xmap[x]] or 0"""
    ym, xm = torch.tensor(ymap), torch.tensor(xmap)
    out = src[..., ym.clamp(min=0), :][..., xm.clamp(min=0)]
    keep = (ym >= 0)[:, None] & (xm >= 0)[None, :]
    return torch.where(keep, out, torch.zeros((), dtype=src.dtype))


def test_a_torch_restatement_of_the_gather():
    from mvoc_amd import ops
    src = torch.arange(1, 1 + 8 * 8, dtype=torch.float32).view(8, 8)
    up = _gather(src, ops.level_axis_map(0, 2, 1, False, 8, 8, 8), ops.level_axis_map(0, 2, 1, False, 8, 8, 8))
    assert torch.equal(up, src[2:6, 2:6].repeat_interleave(2, 0).repeat_interleave(2, 1))  # the centre, every pixel twice
    down = _gather(src, ops.level_axis_map(0, 1, 2, False, 8, 8, 8), ops.level_axis_map(0, 1, 2, False, 8, 8, 8))
    assert torch.equal(down[2:6, 2:6], src[1::2, 1::2]) and not down[:2].any() and not down[:, 6:].any()
    mirror = _gather(src, list(range(8)), ops.level_axis_map(0, 1, 1, True, 8, 8, 8))
    assert torch.equal(mirror, src.flip(1))
    moved = _gather(src, ops.level_axis_map(2, 1, 1, False, 8, 8, 8), ops.level_axis_map(-3, 1, 1, False, 8, 8, 8))
    want = torch.zeros_like(src)
    want[2:, :5] = src[:6, 3:]
    assert torch.equal(moved, want)


# ---- obj_transforms of the sampling call -----------------------------------------------------------------------------------
def test_identity_transforms_are_none():
    from mvoc_amd.pipeline import normalize_obj_transforms as norm
    assert norm(None, 2, 3, 8, 8) == (None, None)
    assert norm([{}, {}], 2, 3, 8, 8) == (None, None)
    assert norm([None, {"scale": 1, "flip": None, "offset": (0, 0)}], 2, 3, 8, 8) == (None, None)
    assert norm([{"scale": "2/2", "anchor": [4, 12]}, {"scale": [1.0, "1"], "offset": [(0, 0)] * 3}], 2, 3, 8, 8) == (None, None)


def test_translation_only_transforms_are_the_placement_of_obj_offsets():
    from mvoc_amd.pipeline import normalize_obj_offsets, normalize_obj_transforms as norm
    offs = [(16, -8), [(0, 0), (8, 0), (16, 24)]]
    pl, tr = norm([{"offset": offs[0]}, {"offset": offs[1], "scale": 1.0, "anchor": [8, 8]}], 2, 3, 8, 8)
    assert tr is None and pl == normalize_obj_offsets(offs, 2, 3)
    pl, tr = norm([{}, {"offset": [8, 8]}], 2, 3, 8, 8)
    assert tr is None and pl == normalize_obj_offsets([(0, 0), (8, 8)], 2, 3)


def test_transforms_carry_scale_flip_anchor_and_offsets_on_the_latent_grid():
    from mvoc_amd.pipeline import normalize_obj_transforms as norm
    pl, tr = norm([{"scale": "3/2", "flip": "h", "offset": (64, 0)}, {"scale": [0.5, 2], "flip": "v", "anchor": [12, 40]}], 2, 2, 64, 48)
    assert pl is None
    # (py, qy, px, qx, flip_y, flip_x, ay2, ax2, ((dy, dx) per frame)); public pairs are (x, y), the default anchor the centre
    assert tr == ((3, 2, 3, 2, False, True, 64, 48, ((0, 8), (0, 8))), (2, 1, 1, 2, True, False, 10, 3, ((0, 0), (0, 0))))
    hash(tr)
    assert norm([{"flip": "hv"}], 1, 1, 8, 8)[1] == ((1, 1, 1, 1, True, True, 8, 8, ((0, 0),)),)
    # one flipped object makes the call a transform; the other objects keep their identity rows
    assert norm([{}, {"flip": "h"}], 2, 1, 8, 8)[1][0] == (1, 1, 1, 1, False, False, 8, 8, ((0, 0),))
    assert norm([{"scale": 2}], 1, 1, 8, 8, factor=16)[1][0][:4] == (2, 1, 2, 1)


def test_float_string_and_int_forms_of_a_scale_agree():
    from mvoc_amd.pipeline import normalize_obj_transforms as norm
    one = lambda s: norm([{"scale": s}], 1, 1, 8, 8)[1][0][:4]
    assert one(1.5) == one("3/2") == one("6/4") == one([1.5, "3/2"]) == (3, 2, 3, 2)
    assert one(2) == one(2.0) == one("2") == one("4/2") == (2, 1, 2, 1)
    assert one(0.1) == one("1/10") == (1, 10, 1, 10)  # the decimal form, not the binary expansion of the float
    assert one(0.125) == one("1/8") and one(64) == (64, 1, 64, 1) and one("1/64") == (1, 64, 1, 64)


@pytest.mark.parametrize("bad,msg", [
    ([{}], r"1 entries for 2 objects"),
    ("scale=2", r"needs a list of 2 dicts"),
    ([{}, 3], r"object 1 needs a dict"),
    ([{}, {"zoom": 2}], r"object 1 has the unknown key\(s\) 'zoom'"),
    ([{"scale": 65}, {}], r"object 0: scale 65 = 65/1 needs 1 <= p, q <= 64"),
    ([{}, {"scale": "1/65"}], r"object 1: scale '1/65' = 1/65 needs"),
    ([{}, {"scale": 0}], r"object 1: scale 0 = 0/1 needs"),
    ([{}, {"scale": -2}], r"object 1: scale -2 = -2/1 needs"),
    ([{}, {"scale": 0.3333}], r"object 1: scale 0.3333 = 3333/10000 needs"),
    ([{}, {"scale": "a/b"}], r"object 1: scale 'a/b' is not an int"),
    ([{}, {"scale": "1/0"}], r"object 1: scale '1/0' is not an int"),
    ([{}, {"scale": True}], r"object 1: scale True is not an int"),
    ([{}, {"scale": [1, 2, 3]}], r"object 1: scale \[1, 2, 3\] needs one value or \[sx, sy\]"),
    ([{"flip": "x"}, {}], r"object 0: flip 'x' is not one of"),
    ([{}, {"anchor": [6, 8]}], r"object 1: anchor \(6, 8\) is not a multiple of 4"),
    ([{}, {"anchor": [8]}], r"object 1: anchor \[8\] needs \[ax, ay\]"),
    ([{}, {"anchor": [8.0, 8]}], r"object 1: anchor \[8.0, 8\] needs \[ax, ay\]"),
    ([{}, {"offset": (8, 4)}], r"object 1: offset: frame 0: \(8, 4\) is not a multiple of 8"),
    ([{}, {"offset": [(0, 0), (8, 8)]}], r"object 1: offset: has 2 per-frame offsets, the clip 3 frames"),
    ([{"offset": "8,8"}, {}], r"object 0: offset: needs \(dx, dy\)"),
])
def test_bad_transforms_name_the_object(bad, msg):
    from mvoc_amd.pipeline import normalize_obj_transforms as norm
    with pytest.raises(ValueError, match=msg):
        norm(bad, 2, 3, 8, 8)


def test_the_call_refuses_transforms_next_to_offsets():
    from mvoc_amd.pipeline import I2VGenXLPipeline
    fn = I2VGenXLPipeline.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection
    assert inspect.signature(fn).parameters["obj_transforms"].default is None
    pipe = I2VGenXLPipeline.__new__(I2VGenXLPipeline)  # no engine: the refusal comes before the conditioner is used
    pipe.conditioner = None
    for kw in ({"obj_offsets": [(8, 8), (0, 0)]}, {"variant_obj_offsets": [[(8, 8), (0, 0)]]}):
        with pytest.raises(ValueError, match="obj_transforms is given together with obj_offsets / variant_obj_offsets"):
            fn(pipe, prompt="a", obj_ddim_latents_path=["o0", "o1"], obj_transforms=[{"scale": 2}, {}], num_frames=3, **kw)


def test_engine_defaults_to_no_transform_and_refuses_a_mix():
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cpu")
    assert eng.transform is None and eng.place_kw([None, None], 8, 8) == {}
    tr = ((2, 1, 2, 1, False, False, 8, 8, ((0, 0),)),) * 2
    eng.transform, eng.placement = tr, (((1, 0),),) * 2
    with pytest.raises(RuntimeError, match="together with placement / variant_placements"):
        eng.place_kw([None, None], 8, 8)
    eng.placement, eng.variant_placements = None, ((((1, 0),),) * 2,)
    with pytest.raises(RuntimeError, match="together with placement / variant_placements"):
        eng.place_kw([None, None], 8, 8)
    eng.variant_placements = None
    with pytest.raises(RuntimeError, match="transform holds 2 objects, the hooks carry 3 masks"):
        eng.place_kw([None, None, None], 8, 8)
    import types
    eng.shard = types.SimpleNamespace(rank=0, world=1)
    with pytest.raises(RuntimeError, match="frame shard"):
        eng.place_kw([None, None], 8, 8)
    with pytest.raises(RuntimeError, match="frame shard"):
        eng.pnp_batch(5, [None, None])


# ---- composite.py and tools/demo_job.py ------------------------------------------------------------------------------------
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
TRANSFORM = [{"scale": "3/2", "flip": "h", "offset": [64, 0]}, {"scale": [0.5, 2], "anchor": [12, 40]}]


def test_composite_obj_transform_reaches_the_call(composite, tmp_path):
    from mvoc_amd.pipeline import normalize_obj_transforms as norm
    ct = _template(tmp_path)
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_transform=TRANSFORM))
    kw = composite.transform_kwargs(config, variants)
    assert kw == {"obj_transforms": TRANSFORM}
    assert all(type(d) is dict for d in kw["obj_transforms"]) and type(kw["obj_transforms"][0]["offset"]) is list
    assert norm(kw["obj_transforms"], 2, 2, 64, 48) == norm(TRANSFORM, 2, 2, 64, 48)
    # shared by an entry's variants
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_transform=TRANSFORM, variants=[{"seed": 1}, {"seed": 2}]))
    assert composite.transform_kwargs(config, variants) == {"obj_transforms": TRANSFORM}
    # the suffix of the output directory does not know the key; obj_width_height stays what the reference makes of it: unused
    plain, _ = composite.merge_variants(ct, ENTRY)
    assert composite.output_suffix(config) == composite.output_suffix(plain)


def test_composite_without_obj_transform_passes_what_it_passed(composite, tmp_path):
    ct = _template(tmp_path)
    config, variants = composite.merge_variants(ct, ENTRY)
    assert composite.transform_kwargs(config, variants) == {} and "obj_transform" not in config
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_offset=[[8, 8], [0, 0]]))
    assert composite.transform_kwargs(config, variants) == {"obj_offsets": [[8, 8], [0, 0]]}
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1, "placement": [[8, 8], [0, 0]]}, {"seed": 2}]))
    assert composite.transform_kwargs(config, variants) == composite.variant_placement_kwargs(config, variants) \
        == {"variant_obj_offsets": [[[8, 8], [0, 0]], None]}


def test_composite_key_errors(composite, tmp_path):
    ct = _template(tmp_path)
    with pytest.raises(ValueError, match=r"variants\[1\] overrides 'obj_transform'"):
        composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1}, {"seed": 2, "obj_transform": TRANSFORM}]))
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_transform=TRANSFORM, obj_offset=[[8, 8], [0, 0]]))
    with pytest.raises(ValueError, match="obj_transform and obj_offset are both set"):
        composite.transform_kwargs(config, variants)
    config, variants = composite.merge_variants(ct, dict(ENTRY, obj_transform=TRANSFORM,
                                                         variants=[{"seed": 1}, {"seed": 2, "placement": [[8, 8], [0, 0]]}]))
    with pytest.raises(ValueError, match="a variant sets 'placement'"):
        composite.transform_kwargs(config, variants)


def test_demo_job_parses_transform():
    from mvoc_amd.pipeline import normalize_obj_transforms as norm
    spec = importlib.util.spec_from_file_location("demo_job_transform", os.path.join(REPO, "tools", "demo_job.py"))
    dj = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dj)
    got = dj.parse_transform("scale=3/2,flip=h,offset=64,0;scale=1/2")
    assert got == [{"scale": "3/2", "flip": "h", "offset": [64, 0]}, {"scale": "1/2"}]
    assert norm(got, 2, 1, 64, 64)[1] == ((3, 2, 3, 2, False, True, 64, 64, ((0, 8),)), (1, 2, 1, 2, False, False, 64, 64, ((0, 0),)))
    assert dj.parse_transform("scale=2,3/2,anchor=8,-4;") == [{"scale": [2, "3/2"], "anchor": [8, -4]}, {}]
    for bad in ("64,0", "offset=64", "scale=1,2,3", "anchor=a,b"):
        with pytest.raises(SystemExit):
            dj.parse_transform(bad)


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_resample_entry_points_are_declared_exported_and_bound():
    from mvoc_amd import _ffi
    hdr = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "mvoc_hip.h")).read())
    pd, i32, u32, vp = C.POINTER(_ffi.PnpDesc), _ffi.i32, C.c_uint32, _ffi.vp
    resampled = ("(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, "
                 "const int32_t* maps, void* stream);")
    want = {
        "mvoc_pnp_blend_scatter_tokens_resampled": (resampled, [pd, i32, C.POINTER(i32), i32, u32, vp, vp]),
        "mvoc_pnp_blend_scatter_nchw_resampled": (resampled, [pd, i32, C.POINTER(i32), i32, u32, vp, vp]),
        "mvoc_gather_planes_f16": ("(const void* src, void* dst, int32_t nplane, int32_t frames, int32_t h, int32_t w, "
                                   "const int32_t* maps, void* stream);", [vp, vp, i32, i32, i32, i32, vp, vp]),
    }
    for name, (decl, args) in want.items():
        assert f"int {name}{decl}" in hdr, name
        assert hasattr(_ffi.lib, name), name
        res, got = _ffi.SIGNATURES[name]
        assert res is i32 and got == args, name
        assert getattr(_ffi.lib, name).argtypes == args
    assert _ffi.lib.mvoc_version() == 100 and _ffi.ABI_VERSION == 100
    assert [f[0] for f in _ffi.PnpDesc._fields_] == ["x", "x2", "masks", "chunk_stride", "f_stride", "p_stride", "nobj", "frames",
                                                    "height", "width", "channels", "mask_h", "mask_w", "base_chunk0", "ndst"]


def test_no_resample_kernel_uses_scratch():
    """the compiler's resource-usage remarks of the build: every instantiation of the new kernels without scratch or spills, and
    none above the registers of its _placed twin plus the two table loads"""
    from mvoc_amd import build
    build.build(verbose=False)
    seen, name = {}, None
    for line in open(os.path.join(REPO, "mvoc_amd", "csrc", "pnp.o.res.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m and name:
                seen[name][key] = int(m.group(1))
    new = {n: r for n, r in seen.items() if "resampled_kernel" in n or "gather_planes_kernel" in n}
    assert len(new) == 4 + 8 + 1, sorted(new)
    for n, r in new.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (n, r)
        twin = n.replace("25pnp_nchw_resampled_kernel", "22pnp_nchw_placed_kernel").replace("27pnp_tokens_resampled_kernel", "24pnp_tokens_placed_kernel")
        if twin != n:
            assert r["VGPRs"] <= seen[twin]["VGPRs"] + 2, (n, r, seen[twin])
