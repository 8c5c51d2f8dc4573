"""CPU-only: matte edges at composition time.  The rule of the mask filter restated once -- torch on the CPU for fp16
(``ref_pass_f16``) and numpy int64 for uint8 (``ref_pass_u8``), with clamped gathers and the fixed tap order: the yardstick of
tests/test_mask_edit_gpu.py as well -- its properties, ``normalize_obj_mask_edit`` and its refusals, the refusals of both C
entries (they return before any HIP call), the declarations, the drivers' key and option, and the README line.  No kernel is
launched."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def _taps(n, d):
    return np.clip(np.arange(n) + d, 0, n - 1)


def ref_pass_f16(v, op, r, axis):
    """one pass over the fp16 CPU tensor ``v`` [..., h, w] along ``axis`` (0: y, 1: x).  max / min: the first tap, then every later
    tap that is strictly greater / smaller replaces it; mean: a fp32 sum in the order -r .. r, times inv (formed in double, rounded
    once to float), rounded once to fp16"""
    assert v.dtype == torch.float16 and not v.is_cuda
    dim = v.dim() - 1 if axis else v.dim() - 2
    tap = lambda d: v.index_select(dim, torch.from_numpy(_taps(v.shape[dim], d)))
    if op == "mean":
        acc = torch.zeros(v.shape, dtype=torch.float32)
        for d in range(-r, r + 1):
            acc = acc + tap(d).float()
        inv = torch.tensor(1.0 / (2 * r + 1), dtype=torch.float64).to(torch.float32)
        return (acc * inv).half()
    o = tap(-r)
    for d in range(-r + 1, r + 1):
        t = tap(d)
        o = torch.where((t > o) if op == "max" else (t < o), t, o)
    return o


def ref_pass_u8(v, op, r, axis):
    """one pass over the uint8 numpy array ``v`` [..., h, w] in int64; mean: (2 sum + n) // (2 n), n = 2 r + 1"""
    assert v.dtype == np.uint8
    ax = v.ndim - 1 if axis else v.ndim - 2
    a = v.astype(np.int64)
    taps = np.stack([np.take(a, _taps(v.shape[ax], d), axis=ax) for d in range(-r, r + 1)])
    if op == "mean":
        n = 2 * r + 1
        out = (2 * taps.sum(0) + n) // (2 * n)
    else:
        out = taps.max(0) if op == "max" else taps.min(0)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def ref_pass(v, op, r, axis):
    return ref_pass_f16(v, op, r, axis) if torch.is_tensor(v) else ref_pass_u8(v, op, r, axis)


def ref_edit(v, grow, feather, scale=1):
    """the edit: grow / shrink along x then y, then feather along x then y, radii times ``scale``; the intermediate in v's type"""
    if grow:
        op = "max" if grow > 0 else "min"
        v = ref_pass(ref_pass(v, op, abs(grow) * scale, 1), op, abs(grow) * scale, 0)
    if feather:
        v = ref_pass(ref_pass(v, "mean", feather * scale, 1), "mean", feather * scale, 0)
    return v


def ref_edit_masks(masks, edit):
    """what ``edit_obj_masks`` must return, on the CPU: the soft mask under the edit, the hard mask as fp16 0 / 1 under the grow
    passes alone, back as bool"""
    return [(ref_edit(s, g, f), ref_edit(h.half(), g, 0) != 0) for (s, h), (g, f) in zip(masks, edit)]


def _planes(shape, seed, kind="k255"):
    g = torch.Generator().manual_seed(seed)
    if kind == "k255":
        return (torch.randint(0, 256, shape, generator=g).float() / 255).half()
    bits = torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.float16)
    return torch.where(torch.isfinite(v), v, torch.zeros_like(v))  # arbitrary FINITE fp16, both zeros included


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- properties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 6), (16, 16)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_radius_zero_is_the_identity_and_full_and_empty_planes_are_preserved(hw):
    h, w = hw
    f16 = _planes((2, h, w), 1, "any")
    u8 = np.random.default_rng(2).integers(0, 256, (2, h, w), dtype=np.uint8)
    for op in ("max", "min", "mean"):
        for axis in (0, 1):
            assert _same_bits(ref_pass_f16(f16, op, 0, axis), f16) and np.array_equal(ref_pass_u8(u8, op, 0, axis), u8)
    for grow, feather in [(1, 0), (-1, 0), (0, 2), (8, 8), (-8, 3)]:
        for fill in (0.0, 1.0):
            plane = torch.full((2, h, w), fill, dtype=torch.float16)
            assert _same_bits(ref_edit(plane, grow, feather), plane), (grow, feather, fill)
        for fill in (0, 255):
            plane = np.full((2, h, w), fill, np.uint8)
            assert np.array_equal(ref_edit(plane, grow, feather, 8), plane), (grow, feather, fill)


def test_the_fp16_mean_of_a_full_plane_is_exact_at_every_radius_the_entry_takes():
    """n ones sum to n exactly, and n * float(1 / n) rounds to 1 in fp16 for every window 2 r + 1 up to 129"""
    one = torch.ones(1, 1, 3, dtype=torch.float16)
    for r in range(65):
        assert _same_bits(ref_pass_f16(one, "mean", r, 1), one), r


@pytest.mark.parametrize("r", [1, 2, 8])
def test_shrink_is_the_complement_of_growing_the_complement_on_binary_planes(r):
    g = torch.Generator().manual_seed(r)
    m = (torch.rand(3, 9, 11, generator=g) > 0.6).half()
    assert _same_bits(ref_edit(m, -r, 0), 1 - ref_edit(1 - m, r, 0))
    m8 = (m.numpy() * 255).astype(np.uint8)
    assert np.array_equal(ref_edit(m8, -r, 0), 255 - ref_edit(255 - m8, r, 0))
    # growing covers the mask, shrinking is covered by it, and a pixel r away from the mask along an axis is reached
    assert (ref_edit(m, r, 0) >= m).all() and (ref_edit(m, -r, 0) <= m).all()
    dot = torch.zeros(1, 21, 21, dtype=torch.float16)
    dot[0, 10, 10] = 1
    grown = ref_edit(dot, r, 0)
    assert grown.sum() == (2 * r + 1) ** 2 and grown[0, 10 - r:11 + r, 10 - r:11 + r].all()


def test_the_hard_mask_stays_binary_and_unfeathered_and_the_soft_mask_takes_both():
    g = torch.Generator().manual_seed(3)
    hard = torch.rand(1, 4, 2, 8, 8, generator=g) > 0.5
    soft = _planes((1, 4, 2, 8, 8), 4)
    (s1, h1), (s2, h2), (s3, h3) = ref_edit_masks([(soft, hard)] * 3, ((2, 3), (0, 3), (-1, 0)))
    assert h1.dtype == torch.bool and torch.equal(h1, ref_edit(hard.half(), 2, 0) != 0)
    assert torch.equal(h2, hard) and not _same_bits(s2, soft)      # feather alone leaves the hard mask
    assert _same_bits(s1, ref_edit(ref_edit(soft, 2, 0), 0, 3))    # grow, then feather
    assert _same_bits(s3, ref_edit(soft, -1, 0)) and torch.equal(h3, ref_edit(hard.half(), -1, 0) != 0)
    assert set(ref_edit(hard.half(), 2, 0).unique().tolist()) <= {0.0, 1.0}


def test_the_passes_of_an_edit_and_the_image_site_radius():
    from mvoc_amd import ops
    assert ops.edit_passes(0, 0) == [] and ops.edit_passes(0, 0, 8) == []
    assert ops.edit_passes(2, 0) == [("max", 2, 1), ("max", 2, 0)]
    assert ops.edit_passes(-3, 1) == [("min", 3, 1), ("min", 3, 0), ("mean", 1, 1), ("mean", 1, 0)]
    assert ops.edit_passes(0, 8, 8) == [("mean", 64, 1), ("mean", 64, 0)]
    for grow, feather in [(1, 2), (-8, 8), (5, 0)]:  # the image site: every radius is s times the latent one, same order
        lat, img = ops.edit_passes(grow, feather), ops.edit_passes(grow, feather, 8)
        assert [(op, 8 * r, ax) for op, r, ax in lat] == img
    assert ops.MASK_EDIT_MAX * 8 == ops.MASK_FILTER_MAX_RADIUS == 64 and ops.MASK_OPS == {"max": 0, "min": 1, "mean": 2}
    t = torch.zeros(2, 2, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="`src` must be a device tensor"):
        ops.mask_filter(t, "max", 1, 0)
    with pytest.raises(RuntimeError, match="`src` must be a device tensor"):
        ops.edit_planes(t, 1, 0)
    assert ops.edit_planes(t, 0, 0) is t  # nothing to do: src itself, on any device
    # a block of 8 x 8 image pixels grown by R * 8 is the latent pixel grown by R, seen at the image site
    lat = np.zeros((1, 6, 6), np.uint8)
    lat[0, 2, 3] = 255
    img = np.kron(lat, np.ones((8, 8), np.uint8))
    assert np.array_equal(ref_edit(img, 1, 0, 8), np.kron(ref_edit(lat, 1, 0), np.ones((8, 8), np.uint8)))


# ---- normalize_obj_mask_edit ---------------------------------------------------------------------------------------------------
def test_normalize_accepts_the_three_forms_and_all_zeros_is_none():
    from mvoc_amd.pipeline import mask_edit_launches, normalize_obj_mask_edit as norm
    assert norm(None, 2) is None and norm([None, None], 2) is None and norm({}, 3) is None
    assert norm([{"grow": 0}, {"feather": 0, "grow": 0}], 2) is None and norm({"grow": 0, "feather": 0}, 2) is None
    assert norm({"grow": 1, "feather": 2}, 2) == ((1, 2), (1, 2))
    assert norm([{"grow": -8}, None], 2) == ((-8, 0), (0, 0)) and norm(({"feather": 8}, {}), 2) == ((0, 8), (0, 0))
    assert norm([{"grow": 8, "feather": 8}], 1) == ((8, 8),)
    assert mask_edit_launches(None) == 0 and mask_edit_launches(((1, 2), (-1, 0))) == 4 + 2 + 2 + 2
    assert mask_edit_launches(((1, 2), (0, 3)), hard=False) == 4 + 2 and mask_edit_launches(((0, 3),)) == 2


@pytest.mark.parametrize("bad,msg", [
    ([{"grow": 1}], r"obj_mask_edit: 1 entries for 2 objects \(one per object, or one dict for all\)"),
    ([{}, {}, {}], r"obj_mask_edit: 3 entries for 2 objects"),
    (3, r"obj_mask_edit: needs None, one dict for all objects or a list of 2 items, got int"),
    ("grow=1", r"obj_mask_edit: needs None, one dict for all objects or a list of 2 items, got str"),
    ([{"grow": 1}, 2], r"obj_mask_edit: object 1 needs None or a dict with the keys grow, feather, got 2"),
    ([None, {"blur": 1}], r"obj_mask_edit: object 1 has the unknown key 'blur' \(the keys are grow, feather\)"),
    ({"grow": 1, "Feather": 1}, r"obj_mask_edit: object 0 has the unknown key 'Feather'"),
    ([{"grow": 1.0}, None], r"obj_mask_edit: object 0: grow = 1.0 is not an int \(latent pixels\)"),
    ([None, {"feather": True}], r"obj_mask_edit: object 1: feather = True is not an int"),
    ([{"grow": "2"}, None], r"obj_mask_edit: object 0: grow = '2' is not an int"),
    ([{"grow": None}, None], r"obj_mask_edit: object 0: grow = None is not an int"),
    ([{"grow": 9}, None], r"obj_mask_edit: object 0: grow = 9 is not in \[-8, 8\] latent pixels"),
    ([None, {"grow": -9}], r"obj_mask_edit: object 1: grow = -9 is not in \[-8, 8\] latent pixels"),
    ([None, {"feather": -1}], r"obj_mask_edit: object 1: feather = -1 is not in \[0, 8\] latent pixels"),
    ({"feather": 9}, r"obj_mask_edit: object 0: feather = 9 is not in \[0, 8\] latent pixels"),
])
def test_bad_edits_name_the_object(bad, msg):
    from mvoc_amd.pipeline import normalize_obj_mask_edit as norm
    with pytest.raises(ValueError, match=msg):
        norm(bad, 2)


def test_the_sampling_call_takes_the_argument_and_refuses_before_any_work():
    from mvoc_amd.pipeline import I2VGenXLPipeline, PipelineOutput, edit_obj_masks
    fn = I2VGenXLPipeline.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection
    p = inspect.signature(fn).parameters
    assert p["obj_mask_edit"].default is None
    assert list(p)[-3:] == ["obj_mask_edit", "compose_main_images", "obj_alpha"]  # behind every argument of the calls before 6t
    assert list(inspect.signature(I2VGenXLPipeline.compose_main_frames).parameters)[-1] == "mask_edit"
    assert inspect.signature(I2VGenXLPipeline.compose_main_frames).parameters["mask_edit"].default is None
    assert PipelineOutput(frames=1).mask_edit_info is None
    pipe = object.__new__(I2VGenXLPipeline)
    with pytest.raises(ValueError, match=r"obj_mask_edit: object 1: grow = 9 is not in \[-8, 8\] latent pixels"):
        fn(pipe, prompt="p", obj_ddim_latents_path=["a", "b"], obj_mask_edit=[None, {"grow": 9}])
    with pytest.raises(ValueError, match="obj_mask_edit: 1 entries for 2 objects"):
        fn(pipe, prompt="p", obj_ddim_latents_path=["a", "b"], obj_mask_edit=[{"grow": 1}])
    masks = [(torch.zeros(1, 4, 2, 4, 4, dtype=torch.float16), torch.zeros(1, 4, 2, 4, 4, dtype=torch.bool))] * 2
    assert edit_obj_masks(masks, None) is masks
    same = edit_obj_masks(masks, ((0, 0), (0, 0)))
    assert all(a is c and b is d for (a, b), (c, d) in zip(same, masks))  # an object that is not edited keeps its very tensors
    with pytest.raises(ValueError, match="edit_obj_masks: 1 edits for 2 objects"):
        edit_obj_masks(masks, ((1, 0),))
    with pytest.raises(ValueError, match=r"an object's masks are \(fp16, bool\) \[..., h, w\] of one shape, got torch.float32"):
        edit_obj_masks([(masks[0][0].float(), masks[0][1])], ((1, 0),))
    with pytest.raises(RuntimeError, match="`src` must be a device tensor"):  # no CPU path behind the edit
        edit_obj_masks(masks, ((1, 0), (0, 0)))


# ---- the C entries: refusals by code and full text, before any HIP call -------------------------------------------------------------
SRC, DST = 0x1000, 0x2000  # never dereferenced: every call below is refused
ENTRIES = ("mask_filter_f16", "mask_filter_u8")


def _refused(name, code, text, src=SRC, dst=DST, nplane=1, h=4, w=4, op=0, radius=1, axis=0):
    from mvoc_amd._ffi import lib
    args = (src, dst, nplane, h, w, op, radius, axis) + ((0.5,) if name.endswith("f16") else ()) + (None,)
    rc = getattr(lib, "mvoc_" + name)(*args)
    assert (rc, lib.mvoc_last_error().decode()) == (code, f"{name}: {text}"), (name, text)


NULL = (-1, "null operand")
ALIAS = (-1, "in place (src == dst) is not supported")
DIMS = lambda nplane, h, w: (-1, f"bad dims (nplane {nplane}, h {h}, w {w})")
OPAXIS = lambda op, axis: (-1, f"op {op} not in [0, 2] or axis {axis} not in [0, 1]")
RADIUS = lambda r: (-2, f"radius {r} not in [0, 64]")
HW = (-2, "h * w does not fit an int")
GRID = (-2, "grid too large")


@pytest.mark.parametrize("name", ENTRIES)
def test_every_refusal_of_the_entries_by_code_and_full_text(name):
    _refused(name, *NULL, src=None)
    _refused(name, *NULL, dst=None)
    _refused(name, *ALIAS, src=DST)
    for kw in (dict(nplane=0), dict(nplane=-2), dict(h=0), dict(w=-3)):
        a = dict(dict(nplane=1, h=4, w=4), **kw)
        _refused(name, *DIMS(a["nplane"], a["h"], a["w"]), **kw)
    for kw in (dict(op=3), dict(op=-1), dict(axis=2), dict(axis=-1)):
        a = dict(dict(op=0, axis=0), **kw)
        _refused(name, *OPAXIS(a["op"], a["axis"]), **kw)
    _refused(name, *RADIUS(65), radius=65)
    _refused(name, *RADIUS(-1), radius=-1)
    _refused(name, *HW, h=65536, w=32768)   # 2^31 exactly
    _refused(name, *HW, h=46341, w=46341)   # 46341^2 = 2^31 + 4633: the first square that does not fit
    _refused(name, *GRID, nplane=2 ** 31 - 1, h=1000, w=1000)
    _refused(name, *GRID, nplane=2 ** 31 - 1, h=256, w=1)  # (2^31 - 1) blocks exactly


@pytest.mark.parametrize("name", ENTRIES)
def test_of_two_faults_the_earlier_one_is_reported(name):
    _refused(name, *NULL, src=None, dst=None)                             # null operand | src == dst
    _refused(name, *ALIAS, src=DST, h=0)                                  # src == dst | dims
    _refused(name, *DIMS(1, 0, 4), h=0, op=3)                             # dims | op / axis
    _refused(name, *OPAXIS(3, 0), op=3, radius=65)                        # op / axis | radius
    _refused(name, *RADIUS(65), radius=65, h=46341, w=46341)              # radius | h * w
    _refused(name, *HW, h=46341, w=46341, nplane=2 ** 31 - 1)             # h * w | grid


# ---- declared, exported, bound ---------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_exported_and_bound_and_the_unit_sits_before_pnp_bilinear():
    from mvoc_amd import _ffi, build, ops
    assert build.SOURCES[-3] == "mask_edit.hip"
    assert build.SOURCES == ["runtime.hip", "gemm.hip", "gemm8.hip", "attention.hip", "tfused.hip", "xslin.hip", "norm.hip", "pnp.hip",
                             "pnp_variants2.hip", "pnp_warp.hip", "stem.hip", "comm.hip", "mask_edit.hip", "pnp_bilinear.hip", "collage.hip"]
    header = open(os.path.join(REPO, "include", "mvoc_hip.h")).read()
    assert re.search(r"int mvoc_mask_filter_f16\(const void\* src, void\* dst, int32_t nplane, int32_t h, int32_t w, int32_t op, "
                     r"int32_t radius,\s+int32_t axis, float inv, void\* stream\);", header)
    assert re.search(r"int mvoc_mask_filter_u8\(const void\* src, void\* dst, int32_t nplane, int32_t h, int32_t w, int32_t op, "
                     r"int32_t radius,\s+int32_t axis, void\* stream\);", header)
    assert "#define MVOC_VERSION 100" in header and _ffi.lib.mvoc_version() == 100
    assert len(_ffi.lib.mvoc_mask_filter_f16.argtypes) == 10 and len(_ffi.lib.mvoc_mask_filter_u8.argtypes) == 9
    assert _ffi.lib.mvoc_mask_filter_f16.argtypes[8] is _ffi.f32
    for name in ("mask_filter", "edit_passes", "edit_planes"):
        assert callable(getattr(ops, name))
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 6u." in design and "mvoc_mask_filter_f16" in design
    assert "obj_mask_edit" in open(os.path.join(REPO, "INTEGRATION.md")).read()


# ---- drivers -----------------------------------------------------------------------------------------------------------------------
def test_composite_py_takes_obj_mask_edit_and_refuses_it_in_a_variant(tmp_path):
    import test_resample_cpu as trc
    gen = trc.composite.__wrapped__()  # the fixture's generator: composite.py imported from this repository, then put away again
    composite = next(gen)
    try:
        ct = trc._template(tmp_path)
        config, variants = composite.merge_variants(ct, trc.ENTRY)
        assert composite.mask_edit_kwargs(config) == {}  # without the key: today's call
        config, _ = composite.merge_variants(ct, dict(trc.ENTRY, obj_mask_edit=None))
        assert composite.mask_edit_kwargs(config) == {}
        config, _ = composite.merge_variants(ct, dict(trc.ENTRY, obj_mask_edit={"grow": 1, "feather": 2}))
        got = composite.mask_edit_kwargs(config)
        assert got == {"obj_mask_edit": {"grow": 1, "feather": 2}} and type(got["obj_mask_edit"]) is dict
        config, _ = composite.merge_variants(ct, dict(trc.ENTRY, obj_mask_edit=[{"grow": -1}, None]))
        got = composite.mask_edit_kwargs(config)
        assert got == {"obj_mask_edit": [{"grow": -1}, None]} and type(got["obj_mask_edit"]) is list
        assert composite.transform_kwargs(config, None) == {} and composite.compose_main_kwargs(config, None) == {}
        config, _ = composite.merge_variants(ct, dict(trc.ENTRY, obj_mask_edit=[{"grow": 9}, None]))
        with pytest.raises(ValueError, match=r"obj_mask_edit: object 0: grow = 9 is not in \[-8, 8\] latent pixels"):
            composite.mask_edit_kwargs(config)
        config, _ = composite.merge_variants(ct, dict(trc.ENTRY, obj_mask_edit=[{"grow": 1}]))
        with pytest.raises(ValueError, match="obj_mask_edit: 1 entries for 2 objects"):
            composite.mask_edit_kwargs(config)
        with pytest.raises(ValueError, match=r"variants\[1\] overrides 'obj_mask_edit', which all variants of an entry share"):
            composite.merge_variants(ct, dict(trc.ENTRY, variants=[{"seed": 1}, {"obj_mask_edit": {"grow": 1}}]))
        assert "obj_mask_edit" not in composite.VARIANT_KEYS
        src = open(os.path.join(REPO, "i2vgen-xl", "composite.py")).read()
        assert "**transform_kwargs(config, variants), **mask_edit)" in src
    finally:
        gen.close()


def test_demo_job_takes_mask_edit_and_refuses_before_any_work():
    spec = importlib.util.spec_from_file_location("demo_job_mask_edit", os.path.join(REPO, "tools", "demo_job.py"))
    demo_job = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo_job)
    parse = demo_job.parse_mask_edit
    assert parse("grow=1,feather=2;grow=-1") == [{"grow": 1, "feather": 2}, {"grow": -1}]
    assert parse(";feather=8") == [None, {"feather": 8}] and parse(" grow = -8 ; ") == [{"grow": -8}, None]
    for text, msg in [("grow=1,blur=2;", "--mask-edit, object 0: 'blur=2' is not grow=N or feather=N"),
                      (";grow", "--mask-edit, object 1: 'grow' is not grow=N or feather=N"),
                      ("grow=1.5;", r"--mask-edit, object 0: cannot read grow=1.5 \(an integer, latent pixels\)"),
                      ("grow=9;", r"--mask-edit, object 0: grow=9 is not in \[-8, 8\] latent pixels"),
                      (";feather=-1", r"--mask-edit, object 1: feather=-1 is not in \[0, 8\] latent pixels"),
                      ("grow=1,grow=2;", "--mask-edit, object 0: grow is given twice"),
                      ("grow=1,,feather=1;", "--mask-edit, object 0: '' is not grow=N or feather=N")]:
        with pytest.raises(SystemExit, match=msg):
            parse(text)
    assert inspect.signature(demo_job.run_variants).parameters["mask_edit"].default is None
    with pytest.raises(SystemExit, match=r"--mask-edit: 1 items for 2 objects \(separate the objects with ;\)"):
        demo_job.run_variants(variants=1, mask_edit=[{"grow": 1}])
    with pytest.raises(SystemExit, match="--transform-filter needs --transform"):  # the older refusals still come first
        demo_job.run_variants(variants=1, transform_filter="bilinear", mask_edit=[{"grow": 1}])
    src = open(os.path.join(REPO, "tools", "demo_job.py")).read()
    assert '"--mask-edit"' in src and 'centry["obj_mask_edit"]' in src and 'res["mask_edit"]' in src
    assert src.index("parse_mask_edit(a.mask_edit)") < src.index("if a.variants or ")  # parsed before any work
    assert "--mask-edit" in open(os.path.join(REPO, "README.md")).read()
