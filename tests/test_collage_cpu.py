"""CPU-only: the main conditioning frames composed from the placed objects.  The rule of the collage restated in
plain numpy int64 (``ref_collage``: the yardstick of tests/test_collage_gpu.py as well), the tap tables of ``ops.collage_taps``
against ``ops.warp_taps`` / ``ops.level_warp_map``, ``pipeline.collage_warps`` against each placement mode's own rule at the image
site, the drivers' keys and refusals, and the entry declared, exported and bound.  No kernel is launched."""
import importlib.util
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 65536
ROT30 = (56756, 32768)    # round(cos 30 * D), round(sin 30 * D)
LATENTS = [(8, 8), (5, 12), (6, 10)]  # the image site is 8 Lh x 8 Lw


# ---- the rule, in integers ------------------------------------------------------------------------------------------------------
def ref_collage(bg, objs, alpha, taps):
    """bg uint8 [F, H, W, 3], objs uint8 [nobj, F, H, W, 3], alpha uint8 [nobj, F, H, W], taps int32 [nobj, F, H * W, 2] (numpy)
    -> uint8 [F, H, W, 3].  Word 0 = ((y0 + 1) << 16) | (x0 + 1), word 1 = (qy << 16) | qx with 9 bits read per weight and a value
    above 256 counted as 256 (so every sample is a byte); a tap outside the plane is 0 for colour and alpha alike;
        S(v) = ((v00 (256 - qx) + v01 qx) (256 - qy) + (v10 (256 - qx) + v11 qx) qy + 32768) >> 16
        a = S(alpha_j);  o = (o (255 - a) + S(objs_j) a + 127) // 255       for j = 0 .. nobj - 1, o = bg at first"""
    bg, objs, alpha, taps = (np.asarray(v) for v in (bg, objs, alpha, taps))
    F, H, W, _ = bg.shape
    o = bg.astype(np.int64)
    fi = np.arange(F)[:, None, None]
    for j in range(objs.shape[0]):
        t = taps[j].astype(np.int64).reshape(F, H, W, 2) & 0xffffffff
        r0, c0 = (t[..., 0] >> 16) - 1, (t[..., 0] & 0xffff) - 1
        qy, qx = np.minimum((t[..., 1] >> 16) & 0x1ff, 256)[..., None], np.minimum(t[..., 1] & 0x1ff, 256)[..., None]
        v = np.concatenate([objs[j], alpha[j][..., None]], -1).astype(np.int64)  # colour and alpha: four channels, one sampler

        def tap(r, c):
            inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
            return np.where(inside[..., None], v[fi, np.where(inside, r, 0), np.where(inside, c, 0)], 0)
        s = ((tap(r0, c0) * (256 - qx) + tap(r0, c0 + 1) * qx) * (256 - qy)
             + (tap(r0 + 1, c0) * (256 - qx) + tap(r0 + 1, c0 + 1) * qx) * qy + 32768) >> 16
        assert s.min() >= 0 and s.max() <= 255
        a = s[..., 3:]
        o = (o * (255 - a) + s[..., :3] * a + 127) // 255
    assert o.min() >= 0 and o.max() <= 255
    return o.astype(np.uint8)


def identity_warp(nobj, frames, Lh, Lw, offs=(0, 0)):
    return tuple((Lh, Lw, ((1, 0, 0, 1, 1) + tuple(offs),) * frames) for _ in range(nobj))


def quarter_turn(Lh, Lw, frames=1):
    return ((Lh, Lw, ((0, 1, -1, 0, 1, 0, 0),) * frames),)  # the inverse matrix of a turn by +90 degrees (tests/test_warp_cpu.py)


def _images(nobj, F, H, W, seed=0):
    g = np.random.default_rng(seed)
    return (g.integers(0, 256, (F, H, W, 3), dtype=np.uint8), g.integers(0, 256, (nobj, F, H, W, 3), dtype=np.uint8),
            g.integers(0, 256, (nobj, F, H, W), dtype=np.uint8))


@pytest.mark.parametrize("filt", [None, "bilinear"])
def test_the_rule_on_identity_taps_is_a_select_and_zero_alpha_returns_the_background(filt):
    from mvoc_amd import ops
    F, H, W = 2, 16, 24
    bg, objs, alpha = _images(1, F, H, W)
    taps = ops.collage_taps(identity_warp(1, F, 2, 3), H, W, 2, 3, filt).numpy()
    hard = np.where(alpha > 127, 255, 0).astype(np.uint8)
    assert np.array_equal(ref_collage(bg, objs, hard, taps), np.where(hard[0][..., None] > 0, objs[0], bg))
    assert np.array_equal(ref_collage(bg, objs, np.zeros_like(alpha), taps), bg)
    soft = ref_collage(bg, objs, alpha, taps).astype(np.int64)  # between the two, rounded to nearest
    a = alpha[0][..., None].astype(np.int64)
    assert np.array_equal(soft, (bg.astype(np.int64) * (255 - a) + objs[0].astype(np.int64) * a + 127) // 255)


@pytest.mark.parametrize("filt", [None, "bilinear"])
def test_a_quarter_turn_about_the_centre_of_a_square_frame_is_rot90(filt):
    from mvoc_amd import ops
    F, S = 2, 16
    bg, objs, alpha = _images(1, F, S, S, seed=1)
    taps = ops.collage_taps(quarter_turn(2, 2, F), S, S, 2, 2, filt).numpy()
    full = np.full_like(alpha, 255)
    assert np.array_equal(ref_collage(bg, objs, full, taps), np.rot90(objs[0], 1, axes=(1, 2)))
    hard = np.where(alpha > 127, 255, 0).astype(np.uint8)
    want = np.where(np.rot90(hard[0], 1, axes=(1, 2))[..., None] > 0, np.rot90(objs[0], 1, axes=(1, 2)), bg)
    assert np.array_equal(ref_collage(bg, objs, hard, taps), want)


def test_the_later_of_two_overlapping_objects_is_in_front():
    from mvoc_amd import ops
    F, H, W = 1, 8, 8
    bg, objs, alpha = _images(2, F, H, W, seed=2)
    alpha[:] = 0
    alpha[0, :, 1:6, 1:6] = 255
    alpha[1, :, 3:8, 3:8] = 255
    out = ref_collage(bg, objs, alpha, ops.collage_taps(identity_warp(2, F, 1, 1), H, W, 1, 1).numpy())
    assert np.array_equal(out[:, 3:6, 3:6], objs[1][:, 3:6, 3:6]) and np.array_equal(out[:, 1:3, 1:6], objs[0][:, 1:3, 1:6])
    assert np.array_equal(out[:, 0], bg[:, 0]) and np.array_equal(out[:, 6:8, 6:8], objs[1][:, 6:8, 6:8])
    # half-transparent in front: the object behind shows through, and the order matters
    alpha[1, :, 3:8, 3:8] = 128
    out = ref_collage(bg, objs, alpha, ops.collage_taps(identity_warp(2, F, 1, 1), H, W, 1, 1).numpy()).astype(np.int64)
    assert np.array_equal(out[:, 3:6, 3:6], (objs[0][:, 3:6, 3:6].astype(np.int64) * 127 + objs[1][:, 3:6, 3:6].astype(np.int64) * 128 + 127) // 255)


def directed_words(F, H, W):
    """two tables of one object that name their words outright -> (taps, what the frame must show) pairs: every pixel samples the
    2 x 2 block at (0, 0) with the weight fields 511 / 300 (both above 256: all the weight on pixel (1, 1)); every word absent"""
    heavy = np.zeros((1, F, H * W, 2), np.int32)
    heavy[..., 0] = (1 << 16) | 1
    heavy[..., 1] = (511 << 16) | 300
    absent = heavy.copy()
    absent[..., 0] = -1
    return heavy, absent


def test_the_yardstick_itself_counts_a_weight_field_above_256_as_256_and_leaves_the_background_at_absent_words():
    """a self-check of ``ref_collage`` alone (no code of the package runs): tests/test_collage_gpu.py sends the same two tables
    through the kernel"""
    F, H, W = 1, 2, 3
    bg, objs, alpha = _images(1, F, H, W, seed=3)
    alpha[:] = 255
    heavy, absent = directed_words(F, H, W)
    assert (ref_collage(bg, objs, alpha, heavy) == objs[0][:, 1:2, 1:2]).all()
    assert np.array_equal(ref_collage(bg, objs, alpha, absent), bg)


# ---- the tap tables -------------------------------------------------------------------------------------------------------------
def _warps(Lh, Lw):
    turn = (ROT30[0] * 2, ROT30[1] * 2, -ROT30[1] * 2, ROT30[0] * 2, 3 * D)  # 30 degrees at scale 3/2 (not reduced: any den is legal)
    path = tuple(turn + (f - 1, 2 * f) for f in range(3))
    half = ((2, 0, 0, 2, 1, 0, 1),) * 3                                    # scale 1/2 about an off-centre anchor
    return [(((Lh, Lw, path), (3, Lw + 5, half))), identity_warp(2, 3, Lh, Lw), identity_warp(1, 3, Lh, Lw, (-1, 2)),
            ((Lh, Lw, ((-1, 0, 0, 1, 1, 0, 0),) * 3),)]


@pytest.mark.parametrize("lat", LATENTS, ids=lambda l: f"{l[0]}x{l[1]}")
def test_collage_taps_are_warp_taps_for_bilinear_and_the_nearest_pixel_with_zero_weights_else(lat):
    from mvoc_amd import ops
    Lh, Lw = lat
    H, W = 8 * Lh, 8 * Lw
    for warp in _warps(Lh, Lw):
        got = ops.collage_taps(warp, H, W, Lh, Lw, "bilinear")
        assert got.dtype == torch.int32 and not got.is_cuda and tuple(got.shape) == (len(warp), 3, H * W, 2)
        assert torch.equal(got, ops.warp_taps(warp, H, W, Lh, Lw))
        for filt in (None, "nearest"):
            got = ops.collage_taps(warp, H, W, Lh, Lw, filt)
            assert got.dtype == torch.int32 and tuple(got.shape) == (len(warp), 3, H * W, 2)
            for j, (ay2, ax2, frames) in enumerate(warp):
                for f, (myy, myx, mxy, mxx, den, dy, dx) in enumerate(frames):
                    px = ops.level_warp_map(dy, dx, (myy, myx, mxy, mxx), den, ay2, ax2, H, W, Lh, Lw)
                    want = ops.pack_taps([(s // W, s % W, 0, 0) if s >= 0 else (-2, -2, 0, 0) for s in px], H, W)
                    assert got[j, f].tolist() == want, (warp, j, f)
    with pytest.raises(RuntimeError, match="collage_taps: filter 'cubic' is not one of None, 'nearest', 'bilinear'"):
        ops.collage_taps(identity_warp(1, 1, Lh, Lw), H, W, Lh, Lw, "cubic")
    with pytest.raises(RuntimeError, match="collage_taps: every object needs the same number"):
        ops.collage_taps(((Lh, Lw, ()),), H, W, Lh, Lw)
    with pytest.raises(RuntimeError, match="collage_taps: 65535 x 8: a site of 65535 rows or columns or more"):
        ops.collage_taps(identity_warp(1, 1, Lh, Lw), 65535, 8, Lh, Lw)


def test_collage_taps_compute_one_row_per_distinct_frame_value_and_make_no_copies_of_a_static_row(monkeypatch):
    from mvoc_amd import ops
    calls = []
    real = ops._level_tap_words
    monkeypatch.setattr(ops, "_level_tap_words", lambda *a: (calls.append(a), real(*a))[1])
    static = identity_warp(2, 5, 8, 8, (1, -1))
    t = ops.collage_taps(static, 64, 64, 8, 8, "bilinear")
    assert len(calls) == 2 and t.stride(1) == 0 and tuple(t.shape) == (2, 5, 4096, 2)  # the frame axis is a view of one row
    assert torch.equal(t, ops.warp_taps(static, 64, 64, 8, 8))
    calls.clear()
    fr = (1, 0, 0, 1, 1)
    moving = ((8, 8, (fr + (0, 0), fr + (1, 0), fr + (0, 0), fr + (1, 0), fr + (0, 0))),)
    t = ops.collage_taps(moving, 64, 64, 8, 8, "bilinear")
    assert len(calls) == 2 and t.is_contiguous() and torch.equal(t, ops.warp_taps(moving, 64, 64, 8, 8))
    # at 512 x 512 the int64 form serves: no nested lists (pack_taps / level_warp_map are the list forms)
    monkeypatch.setattr(ops, "pack_taps", lambda *a: pytest.fail("the list form was taken"))
    monkeypatch.setattr(ops, "level_warp_map", lambda *a, **k: pytest.fail("the list form was taken"))
    for filt in (None, "bilinear"):
        t = ops.collage_taps(((64, 64, ((ROT30[0], ROT30[1], -ROT30[1], ROT30[0], D, 0, 0),) * 16),), 512, 512, 64, 64, filt)
        assert tuple(t.shape) == (1, 16, 512 * 512, 2) and t.stride(1) == 0


# ---- collage_warps ----------------------------------------------------------------------------------------------------------------
def _nearest_pixels(warp, H, W, Lh, Lw):
    """per object and frame the source pixel of every destination pixel under the collage's nearest table (-1: absent)"""
    from mvoc_amd import ops
    t = ops.collage_taps(warp, H, W, Lh, Lw).to(torch.int64)
    w0 = t[..., 0]
    assert (t[..., 1] == 0).all()
    return torch.where(w0 < 0, w0, (((w0 >> 16) & 0xffff) - 1) * W + (w0 & 0xffff) - 1).tolist()


@pytest.mark.parametrize("lat", LATENTS, ids=lambda l: f"{l[0]}x{l[1]}")
def test_collage_warps_agree_with_each_modes_own_rule_at_the_image_site(lat):
    from mvoc_amd import ops
    from mvoc_amd.pipeline import collage_warps, resolve_obj_transforms, resolve_variant_obj_offsets, resolve_variant_obj_transforms
    Lh, Lw = lat
    H, W, F, n = 8 * Lh, 8 * Lw, 2, 2
    none = dict(placement=None, variant_placements=None, transform=None, variant_transforms=None, warp=None)
    # no mode: the identity permutation
    (w,) = collage_warps(none, 3, n, F, Lh, Lw)
    assert _nearest_pixels(w, H, W, Lh, Lw) == [[list(range(H * W))] * F] * n
    assert collage_warps(None, 1, n, F, Lh, Lw) == [w]
    # a placement: level_offsets at the image site, which is 8 d exactly
    placement = (((1, -2), (0, 3)), ((-1, 0),) * 2)
    (w,) = collage_warps(dict(none, placement=placement), 2, n, F, Lh, Lw)
    offs = ops.level_offsets(placement, H, W, Lh, Lw)
    assert offs == tuple(tuple((8 * dy, 8 * dx) for dy, dx in obj) for obj in placement)
    got = _nearest_pixels(w, H, W, Lh, Lw)
    for j in range(n):
        for f, (dy, dx) in enumerate(offs[j]):
            want = [(y - dy) * W + (x - dx) if 0 <= y - dy < H and 0 <= x - dx < W else -1 for y in range(H) for x in range(W)]
            assert got[j][f] == want, (j, f)
    # per-variant placements: K of them
    pl, vpl = resolve_variant_obj_offsets([[(8, 0), (0, -16)], None, [(8, 0), (0, 8)]], 3, n, F)
    assert pl is None
    ws = collage_warps(dict(none, variant_placements=vpl), 3, n, F, Lh, Lw)
    assert len(ws) == 3 and ws == [collage_warps(dict(none, placement=p), 1, n, F, Lh, Lw)[0] for p in vpl] and ws[0] != ws[2]
    assert _nearest_pixels(ws[1], H, W, Lh, Lw) == [[list(range(H * W))] * F] * n
    # a transform: the outer combination of level_axis_map
    tr = [{"scale": "3/2", "flip": "h", "offset": [(8, 0), (16, -8)]}, {"scale": [2, "1/2"], "anchor": [12, 20]}]
    _, transform, warp = resolve_obj_transforms(tr, n, F, Lh, Lw)
    assert transform is not None and warp is None
    (w,) = collage_warps(dict(none, transform=transform), 1, n, F, Lh, Lw)
    got = _nearest_pixels(w, H, W, Lh, Lw)
    maps = ops.transform_maps(transform, H, W, Lh, Lw)
    for j in range(n):
        for f in range(F):
            ym, xm = maps[j][f][:H], maps[j][f][H:]
            assert got[j][f] == [ym[y] * W + xm[x] if ym[y] >= 0 and xm[x] >= 0 else -1 for y in range(H) for x in range(W)], (j, f)
    # per-variant transforms: K of them, each its own
    _, _, _, vtr = resolve_variant_obj_transforms([tr, None], 2, n, F, Lh, Lw)
    ws = collage_warps(dict(none, variant_transforms=vtr), 2, n, F, Lh, Lw)
    assert len(ws) == 2 and ws[0] == w and _nearest_pixels(ws[1], H, W, Lh, Lw) == [[list(range(H * W))] * F] * n
    with pytest.raises(ValueError, match="collage_warps: 2 per-variant values for 3 variants"):
        collage_warps(dict(none, variant_transforms=vtr), 3, n, F, Lh, Lw)
    # a warp: itself, so level_warp_map
    _, _, warp = resolve_obj_transforms([{"rotate": 30, "scale": "3/2"}, {"rotate": [0, -15]}], n, F, Lh, Lw)
    (w,) = collage_warps(dict(none, warp=warp), 2, n, F, Lh, Lw)
    assert w == warp
    got = _nearest_pixels(w, H, W, Lh, Lw)
    for j, (ay2, ax2, frames) in enumerate(warp):
        for f, fr in enumerate(frames):
            assert got[j][f] == ops.level_warp_map(fr[5], fr[6], fr[:4], fr[4], ay2, ax2, H, W, Lh, Lw), (j, f)


# ---- the call's refusals that need no device -----------------------------------------------------------------------------------------
def test_the_sampling_call_takes_the_two_arguments_and_refuses_before_any_work():
    from mvoc_amd.pipeline import I2VGenXLPipeline, PipelineOutput, _frames_rgb_u8
    from PIL import Image
    fn = I2VGenXLPipeline.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection
    p = inspect.signature(fn).parameters
    assert p["compose_main_images"].default is False and p["obj_alpha"].default is None
    assert list(p)[-2:] == ["compose_main_images", "obj_alpha"]  # behind every existing argument
    assert PipelineOutput(frames=1).main_frames is None
    pipe = object.__new__(I2VGenXLPipeline)
    with pytest.raises(ValueError, match="compose_main_images=True builds main_first_image from the sources"):
        fn(pipe, prompt="p", main_first_image=object(), compose_main_images=True, obj_alpha=[])
    with pytest.raises(ValueError, match="compose_main_images=True builds main_image_list from the sources"):
        fn(pipe, prompt="p", main_image_list=[object()], compose_main_images=True, obj_alpha=[])
    with pytest.raises(ValueError, match="needs the objects' image-size masks: obj_mask paths or obj_alpha"):
        fn(pipe, prompt="p", compose_main_images=True)
    # the sampling call still runs without autograd whatever the caller's mode is, and so does the new stage
    seen = []

    class Probe:
        @property
        def shape(self):
            seen.append(torch.is_grad_enabled())
            raise KeyError("probe")

        def __len__(self):
            return self.shape
    with torch.enable_grad():
        with pytest.raises(KeyError, match="probe"):
            fn(pipe, prompt_embeds=Probe())
        with pytest.raises(KeyError, match="probe"):
            I2VGenXLPipeline.compose_main_frames(pipe, None, 1, 1, 1, 8, 8, [], Probe())
        assert torch.is_grad_enabled()
    assert seen == [False, False]
    ok = [Image.new("RGB", (24, 16))] * 2
    assert tuple(_frames_rgb_u8(ok, 2, 16, 24, "x").shape) == (2, 16, 24, 3)
    with pytest.raises(ValueError, match=r"objs_image_list\[1\], frame 1 is 16 x 24, the call 24 x 16 .*does not resize"):
        _frames_rgb_u8([ok[0], Image.new("RGB", (16, 24))], 2, 16, 24, "objs_image_list[1]")
    with pytest.raises(ValueError, match="background_image_list has 2 frames, the clip 3"):
        _frames_rgb_u8(ok, 3, 16, 24, "background_image_list")


def test_mask_alpha_frames_follow_the_listing_rule_of_mask_preprocess(tmp_path):
    from PIL import Image
    from mvoc_amd.utils import mask_alpha_frames
    g = np.random.default_rng(4)
    imgs = [g.integers(0, 256, (16, 24), dtype=np.uint8) for _ in range(11)]
    for i, im in enumerate(imgs):  # "10.png" sorts after "9.png": by number, not by name
        Image.fromarray(im).save(tmp_path / f"{i}.png")
    got = mask_alpha_frames(str(tmp_path), 11)
    assert got.dtype == np.uint8 and np.array_equal(got, np.stack(imgs))
    assert np.array_equal(mask_alpha_frames(str(tmp_path), 3), np.stack(imgs[:3]))
    assert np.array_equal(mask_alpha_frames(str(tmp_path / "4.png"), 2), np.stack([imgs[4]] * 2))
    with pytest.raises(ValueError, match="11 masks .* for 12 frames"):
        mask_alpha_frames(str(tmp_path), 12)


# ---- drivers -----------------------------------------------------------------------------------------------------------------------
def test_composite_py_takes_compose_main_and_refuses_a_variants_own_main_frames(tmp_path):
    import test_resample_cpu as trc
    gen = trc.composite.__wrapped__()  # the fixture's generator: composite.py imported from this repository, then put away again
    composite = next(gen)
    try:
        ct = trc._template(tmp_path)
        config, variants = composite.merge_variants(ct, trc.ENTRY)
        assert composite.compose_main_kwargs(config, variants) == {}  # without the key: today's call
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, compose_main=False))
        assert composite.compose_main_kwargs(config, variants) == {}
        entry = dict(trc.ENTRY, compose_main=True, edited_first_frame_path="", edited_contorl_frame_path_main="")
        config, variants = composite.merge_variants(ct, entry)
        assert composite.compose_main_kwargs(config, variants) == {"compose_main_images": True}
        assert composite.transform_kwargs(config, variants) == {}  # the placement keys do not know the new one
        config, variants = composite.merge_variants(ct, dict(entry, variants=[{"seed": 1}, {"transform": [{"scale": 2}, {}]}]))
        assert composite.compose_main_kwargs(config, variants) == {"compose_main_images": True}
        for key in ("edited_first_frame_path", "edited_contorl_frame_path_main"):
            config, variants = composite.merge_variants(ct, dict(entry, variants=[{}, {key: "other"}]))
            with pytest.raises(ValueError, match=rf"variants\[1\] overrides '{key}' and the entry sets compose_main"):
                composite.compose_main_kwargs(config, variants)
            config, variants = composite.merge_variants(ct, dict(trc.ENTRY, variants=[{}, {key: "other"}]))
            assert composite.compose_main_kwargs(config, variants) == {}  # without the key a variant may show its own
        with pytest.raises(ValueError, match="variants\\[0\\] overrides 'compose_main', which all variants of an entry share"):
            composite.merge_variants(ct, dict(trc.ENTRY, variants=[{"compose_main": True}]))
        config, variants = composite.merge_variants(ct, dict(trc.ENTRY, compose_main="yes"))
        with pytest.raises(ValueError, match="compose_main 'yes' is not true or false"):
            composite.compose_main_kwargs(config, variants)
        src = open(os.path.join(REPO, "i2vgen-xl", "composite.py")).read()
        assert 'f"main_{i:05d}.png"' in src and "None if compose else first(config)" in src
    finally:
        gen.close()


def test_demo_job_takes_compose_main():
    spec = importlib.util.spec_from_file_location("demo_job_compose_main", os.path.join(REPO, "tools", "demo_job.py"))
    demo_job = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo_job)
    assert inspect.signature(demo_job.run_variants).parameters["compose_main"].default is False
    src = open(os.path.join(REPO, "tools", "demo_job.py")).read()
    assert '"--compose-main"' in src and 'centry["compose_main"] = True' in src and 'res["compose_main"]' in src
    assert re.search(r"if a\.variants or .* or a\.transform_filter:", src)  # the older options' line keeps its ending
    assert "if a.compose_main and not a.variants:" in src                  # the option alone reaches run_variants
    assert "--compose-main" in open(os.path.join(REPO, "README.md")).read()
    # the refusals in front of any work still come first
    with pytest.raises(SystemExit, match="--transform-filter needs --transform"):
        demo_job.run_variants(variants=1, transform_filter="bilinear", compose_main=True)


# ---- declared, exported, bound ---------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound_and_its_unit_is_last():
    from mvoc_amd import _ffi, build, ops
    assert build.SOURCES[-1] == "collage.hip" and build.SOURCES[-2] == "pnp_bilinear.hip"
    header = open(os.path.join(REPO, "include", "mvoc_hip.h")).read()
    assert re.search(r"int mvoc_collage_rgb_u8\(const void\* bg, const void\* objs, const void\* alpha, void\* out, int32_t nobj, "
                     r"int32_t frames, int32_t h,\s+int32_t w, const int32_t\* taps, void\* stream\);", header)
    assert "#define MVOC_VERSION 100" in header
    fn = _ffi.lib.mvoc_collage_rgb_u8
    assert len(fn.argtypes) == 10 and _ffi.lib.mvoc_version() == 100
    # the refusals of the host entry need no device: codes and texts, in the promised order
    err = lambda: _ffi.lib.mvoc_last_error().decode()
    assert fn(None, 8, 8, 16, 1, 1, 1, 1, 8, None) == -1 and err() == "collage: null operand"
    assert fn(8, 16, 24, 8, 1, 1, 1, 1, 32, None) == -1 and err() == "collage: out aliases an input (in place is not supported)"
    assert ops.COLLAGE_MAX_OBJECTS == 16
    for name in ("collage", "collage_taps", "collage_tap_table"):
        assert callable(getattr(ops, name))
    with pytest.raises(RuntimeError, match="`bg` must be a device tensor"):
        ops.collage(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), None, None, None)
