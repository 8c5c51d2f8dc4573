"""GPU: the collage kernel (mvoc_collage_rgb_u8) against the integer restatement of its rule in
tests/test_collage_cpu.py (``ref_collage``) -- exact equality everywhere -- its refusals by code and full text, and the sampling
call's ``compose_main_images`` on the toy composition of tests/test_placement_gpu.py: the run equals the run that is handed the
CPU reference's collage as explicit main images."""
import types

import numpy as np
import pytest
import torch

import test_collage_cpu as tcc
import test_placement_gpu as tpg

pytestmark = pytest.mark.gpu
tv = tpg.tv
D = tcc.D


# ---- kernel against reference ---------------------------------------------------------------------------------------------------
def _flush(t, slack):
    """``t`` copied to the device so that it ends where its allocation's tensor ends (``slack`` elements lie in front of it)"""
    buf = torch.empty(slack + t.numel(), dtype=t.dtype, device="cuda")
    view = buf[slack:].view(t.shape)
    view.copy_(t)
    return view


def _tables(nobj, F, H, W):
    from mvoc_amd import ops
    Lh, Lw = max(1, H // 2), max(1, W // 3)
    c, s = tcc.ROT30
    turn = (2 * c, 2 * s, -2 * s, 2 * c, 3 * D)  # 30 degrees at scale 3/2
    path = lambda j: tuple(turn + (f - j, j - 2 * f) for f in range(F))
    half = lambda j: (3, Lw + 1 + j, ((2, 0, 0, 2, 1, 0, j),) * F)
    g = torch.Generator().manual_seed(H * 1000 + W + nobj)
    garbage = torch.randint(-2 ** 63, 2 ** 63 - 1, (nobj, F, H * W), generator=g, dtype=torch.int64).view(torch.int32).view(nobj, F, H * W, 2)
    return {"turn-path": ops.collage_taps(tuple((Lh, Lw, path(j)) for j in range(nobj)), H, W, Lh, Lw, "bilinear"),
            "half-off-centre": ops.collage_taps(tuple(half(j) for j in range(nobj)), H, W, Lh, Lw, "bilinear"),
            "identity": ops.collage_taps(tcc.identity_warp(nobj, F, Lh, Lw), H, W, Lh, Lw, "bilinear"),
            "nearest": ops.collage_taps(tuple((Lh, Lw, path(j)) for j in range(nobj)), H, W, Lh, Lw, None),
            "garbage": garbage}


@pytest.mark.parametrize("nobj", [1, 2, 4])
@pytest.mark.parametrize("hw", [(5, 6), (4, 6), (1, 255), (1, 257), (16, 16)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_the_kernel_gives_the_bytes_of_the_rule(hw, nobj):
    from mvoc_amd import ops
    F, (H, W) = 2, hw
    bg, objs, alpha = tcc._images(nobj, F, H, W, seed=H * W + nobj)
    alpha[:, :, : (H + 1) // 2] = np.where(alpha[:, :, : (H + 1) // 2] > 127, 255, 0)  # hard and soft alphas
    dbg, dobjs, dalpha = _flush(torch.from_numpy(bg), 3), _flush(torch.from_numpy(objs), 5), _flush(torch.from_numpy(alpha), 7)
    n = F * H * W * 3
    seen = {}
    for name, taps in _tables(nobj, F, H, W).items():
        taps = taps.contiguous()
        want = tcc.ref_collage(bg, objs, alpha, taps.numpy())
        buf = torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[64:64 + n].view(F, H, W, 3)
        assert ops.collage(dbg, dobjs, dalpha, _flush(taps, 6), out=out) is out
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:64] == 0xA5).all() and (host[64 + n:] == 0xA5).all(), name  # the sentinels around out survive
        assert np.array_equal(host[64:64 + n].reshape(F, H, W, 3), want), name
        seen[name] = want
    assert not np.array_equal(seen["identity"], bg)
    # a fresh output tensor: the same bytes
    assert np.array_equal(ops.collage(dbg, dobjs, dalpha, _tables(nobj, F, H, W)["identity"].contiguous().cuda()).cpu().numpy(), seen["identity"])


def test_the_kernel_counts_a_weight_field_above_256_as_256_and_leaves_the_background_at_absent_words():
    """directed words, not random ones: weight fields 511 / 300 put all the weight on the lower-right tap (the kernel clamps; the
    fp16 family of DESIGN.md 6r does not), and absent words (-1) leave the background whatever the alpha"""
    from mvoc_amd import ops
    F, H, W = 2, 3, 5
    bg, objs, alpha = tcc._images(1, F, H, W, seed=21)
    alpha[:] = 255
    dev = [torch.from_numpy(v).cuda() for v in (bg, objs, alpha)]
    heavy, absent = tcc.directed_words(F, H, W)
    got = ops.collage(*dev, torch.from_numpy(heavy).cuda()).cpu().numpy()
    assert (got == objs[0][:, 1:2, 1:2]).all() and np.array_equal(got, tcc.ref_collage(bg, objs, alpha, heavy))
    got = ops.collage(*dev, torch.from_numpy(absent).cuda()).cpu().numpy()
    assert np.array_equal(got, bg) and np.array_equal(got, tcc.ref_collage(bg, objs, alpha, absent))
    # soft alpha under the clamped weights: the blend of pixel (1, 1) alone
    alpha[:] = 77
    got = ops.collage(dev[0], dev[1], torch.from_numpy(alpha).cuda(), torch.from_numpy(heavy).cuda()).cpu().numpy()
    want = (bg.astype(np.int64) * (255 - 77) + objs[0][:, 1:2, 1:2].astype(np.int64) * 77 + 127) // 255
    assert np.array_equal(got, want) and np.array_equal(got, tcc.ref_collage(bg, objs, alpha, heavy))


def test_collage_tap_table_is_collage_taps_on_the_device_and_ops_collage_checks_its_arguments():
    from mvoc_amd import ops
    static = tcc.identity_warp(2, 3, 2, 2, (1, -1))
    moving = ((2, 2, tuple((1, 0, 0, 1, 1, f % 2, 0) for f in range(3))),) * 2
    for warp in (static, moving):
        for filt in (None, "bilinear"):
            t = ops.collage_tap_table(warp, 16, 16, 2, 2, filt, "cuda")
            assert t.is_cuda and t.is_contiguous() and torch.equal(t.cpu(), ops.collage_taps(warp, 16, 16, 2, 2, filt))
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device="cuda")
    bg, objs, alpha, taps = u8(3, 16, 16, 3), u8(2, 3, 16, 16, 3), u8(2, 3, 16, 16), t
    for bad, text in [(dict(bg=u8(3, 16, 16, 4)), r"bg must be contiguous \[F, H, W, 3\]"),
                      (dict(bg=bg.half()), "`bg` must be torch.uint8"),
                      (dict(objs=u8(2, 3, 16, 15, 3)), r"objs must be contiguous \[nobj, F = 3, H = 16, W = 16, 3\]"),
                      (dict(alpha=u8(2, 3, 16, 16, 1)), r"alpha must be contiguous \[nobj = 2, F = 3, H = 16, W = 16\]"),
                      (dict(alpha=u8(2, 3, 16, 32)[..., ::2]), "alpha must be contiguous"),
                      (dict(taps=taps[:, :, :, :1]), r"taps must be a contiguous int32 \[nobj = 2, F = 3, h \* w = 256, 2\] table"),
                      (dict(taps=taps.long()), "`taps` must be torch.int32"),
                      (dict(taps=_flush(taps.cpu(), 5)), "taps must be 8-byte aligned"),  # contiguous, at an odd int32 offset
                      (dict(out=u8(3, 16, 16)), "out must be contiguous and of bg's shape"),
                      (dict(out=bg), "out overlaps bg")]:
        with pytest.raises(RuntimeError, match=text):
            ops.collage(**dict(dict(bg=bg, objs=objs, alpha=alpha, taps=taps), **bad))


# ---- refusals of the entry -----------------------------------------------------------------------------------------------------
BG, OBJS, ALPHA, OUT, TAPS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000  # never dereferenced: every call below is refused
NULL = (-1, "collage: null operand")
ALIAS = (-1, "collage: out aliases an input (in place is not supported)")
DIMS = lambda nobj, frames, h, w: (-1, f"collage: nobj {nobj} not in [1, 16] or bad dims (frames {frames}, h {h}, w {w})")
FIELDS = lambda h, w: (-2, f"collage: h {h} or w {w} does not fit the 16-bit tap fields (< 65535)")
HW = (-2, "collage: h * w does not fit an int")
GRID = (-2, "collage: grid too large")


def _refused(want, bg=BG, objs=OBJS, alpha=ALPHA, out=OUT, nobj=1, frames=1, h=4, w=4, taps=TAPS):
    from mvoc_amd._ffi import lib
    rc = lib.mvoc_collage_rgb_u8(bg, objs, alpha, out, nobj, frames, h, w, taps, None)
    assert (rc, lib.mvoc_last_error().decode()) == want


def test_every_refusal_of_the_entry_by_code_and_full_text():
    for name in ("bg", "objs", "alpha", "out", "taps"):
        _refused(NULL, **{name: None})
    for name in ("bg", "objs", "alpha", "taps"):
        _refused(ALIAS, **{name: OUT})
    for kw in (dict(nobj=0), dict(nobj=17), dict(nobj=-1), dict(frames=0), dict(h=0), dict(w=-3)):
        a = dict(dict(nobj=1, frames=1, h=4, w=4), **kw)
        _refused(DIMS(a["nobj"], a["frames"], a["h"], a["w"]), **kw)
    _refused(FIELDS(65535, 4), h=65535)
    _refused(FIELDS(4, 70000), w=70000)
    _refused(HW, h=65534, w=65534)
    _refused(HW, h=46341, w=46341)  # 46341^2 = 2^31 + 4633: the first square that does not fit
    _refused(GRID, h=30000, w=30000, frames=1000)
    _refused(GRID, h=65534, w=32767, frames=2 ** 31 - 1)


def test_of_two_faults_the_earlier_one_is_reported():
    _refused(NULL, taps=None, bg=OUT)                                   # null operand | alias
    _refused(ALIAS, bg=OUT, nobj=0)                                     # alias | nobj / dims
    _refused(DIMS(17, 1, 65535, 4), nobj=17, h=65535)                   # nobj / dims | 16-bit fields
    _refused(FIELDS(65535, 65535), h=65535, w=65535)                    # 16-bit fields | h * w
    _refused(HW, h=65534, w=65534, frames=2 ** 31 - 1)                  # h * w | grid


# ---- pipeline -----------------------------------------------------------------------------------------------------------------------
F_, LAT, SIZE, STEPS = 3, 8, 64, 2
ROTATED = [{"rotate": 30, "scale": "3/2"}, {"rotate": [0, 15, -15], "offset": (8, -16)}]
VARIANT_TRANSFORMS = [[{"scale": "3/2", "flip": "h"}, {"offset": (8, -16)}], None]


def _sources():
    from PIL import Image
    g = np.random.default_rng(11)
    clips = [[Image.fromarray(g.integers(0, 256, (SIZE, SIZE, 3), dtype=np.uint8)) for _ in range(F_)] for _ in range(3)]
    alpha = g.integers(0, 256, (2, F_, SIZE, SIZE), dtype=np.uint8)
    alpha[:, :, :24] = 0
    alpha[:, :, 40:] = 255
    return clips, alpha


def _reference_frames(placed, K, filt):
    """the collage the CPU reference builds under what the resolvers returned -> per variant a list of images"""
    from PIL import Image
    from mvoc_amd import ops
    from mvoc_amd.pipeline import collage_warps
    clips, alpha = _sources()
    rgb = lambda fr: np.stack([np.asarray(im) for im in fr])
    out = []
    for warp in collage_warps(placed, K, 2, F_, LAT, LAT):
        taps = ops.collage_taps(warp, SIZE, SIZE, LAT, LAT, filt).contiguous().numpy()
        out.append([Image.fromarray(fr) for fr in tcc.ref_collage(rgb(clips[0]), np.stack([rgb(clips[1]), rgb(clips[2])]), alpha, taps)])
    return out * K if len(out) == 1 else out


def _job(K=1, shard=False, **kw):
    """the toy composition of tests/test_placement_gpu.py (three sources, two objects, fusion on the first step) with real images
    and the synthetic conditioner, which keys on image bytes"""
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    _, eng = tv._toy_pair()
    g = torch.Generator().manual_seed(5)
    s = DDIMScheduler()
    s.set_timesteps(STEPS)
    dirs = ["/virtual/bg", "/virtual/o1", "/virtual/o2"]
    src = {d: {int(t): torch.randn(1, 4, F_, LAT, LAT, generator=g).half() for t in s.timesteps} for d in dirs}
    x0 = torch.randn(K, 4, F_, LAT, LAT, generator=g).half()
    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False)
    pnp_utils.register_temp_attention_pnp(pipe, s.timesteps[:2], False)
    pnp_utils.register_spatial_attention_pnp(pipe, s.timesteps[:2], False)
    pnp_utils.register_temp_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_out_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_resnet_injection(pipe, s.timesteps[:1])
    pipe.latent_cache.write_files = False
    for d, lat in src.items():
        for t, v in lat.items():
            pipe.latent_cache.put(d, t, v.cuda())
    clips, alpha = _sources()
    cpu_masks, _ = tv._hook_masks(F_, LAT, LAT)
    var = dict(prompt="edit0", guidance_scale=9.0, negative_prompt="neg") if K == 1 else \
        dict(prompt=[f"edit{k}" for k in range(K)], guidance_scale=[tv.GUIDANCE[k % 2] for k in range(K)], negative_prompt=["neg"] * K)
    if kw.get("compose_main_images") and "obj_alpha" not in kw:
        kw["obj_alpha"] = list(alpha)
    if shard:
        eng.shard = types.SimpleNamespace(rank=0, world=1)
    try:
        res = pipe.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection(
            background_first_image=clips[0][0], background_image_list=clips[0], objs_first_image=[clips[1][0], clips[2][0]],
            objs_image_list=[clips[1], clips[2]], height=SIZE, width=SIZE, num_frames=F_, num_inference_steps=STEPS, target_fps=8,
            output_type="latent", ddim_inv_prompt="", bg_inv_latents_path=dirs[0], obj_ddim_latents_path=dirs[1:],
            obj_ddim_latents_idx_offset=[0, 0], obj_masks_tensors=[(a.clone(), b.clone()) for a, b in cpu_masks],
            ddim_init_latents_t_idx=0, fusion_steps=(0, 1), random_noise_ratio=0.3, obj_random_noise_fusion=True,
            latents=x0.cuda(), **var, **kw)
    finally:
        eng.shard = None
    torch.cuda.synchronize()
    return res


def _same_images(a, b):
    return len(a) == len(b) and all(x.size == y.size and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("filt", [None, "nearest", "bilinear"])
def test_a_rotated_call_composes_the_frames_the_reference_builds_and_runs_as_if_handed_them(filt):
    from mvoc_amd.pipeline import resolve_obj_transforms
    kw = dict(obj_transforms=ROTATED, **({} if filt is None else {"obj_transform_filter": filt}))
    _, _, warp = resolve_obj_transforms(ROTATED, 2, F_, LAT, LAT, **({"interp": "bilinear"} if filt == "bilinear" else {}))
    (want,) = _reference_frames({"warp": warp}, 1, "bilinear" if filt == "bilinear" else None)
    got = _job(compose_main_images=True, **kw)
    assert len(got.main_frames) == 1 and _same_images(got.main_frames[0], want)
    explicit = _job(main_first_image=want[0], main_image_list=want, **kw)
    assert explicit.main_frames is None
    assert torch.equal(got.frames, explicit.frames) and torch.isfinite(got.frames).all()
    (upright,) = _reference_frames(None, 1, None)
    assert not _same_images(want, upright)  # the turned collage is not the upright one


def test_two_variants_with_their_own_transforms_see_their_own_collages():
    from mvoc_amd.pipeline import resolve_variant_obj_transforms
    _, _, _, vtr = resolve_variant_obj_transforms(VARIANT_TRANSFORMS, 2, 2, F_, LAT, LAT)
    want = _reference_frames({"variant_transforms": vtr}, 2, None)
    assert not _same_images(want[0], want[1])
    got = _job(K=2, compose_main_images=True, variant_obj_transforms=VARIANT_TRANSFORMS)
    assert len(got.main_frames) == 2 and all(_same_images(got.main_frames[k], want[k]) for k in range(2))
    explicit = _job(K=2, main_first_image=[w[0] for w in want], main_image_list=want, variant_obj_transforms=VARIANT_TRANSFORMS)
    assert torch.equal(got.frames, explicit.frames) and not torch.equal(got.frames[0], got.frames[1])
    # variants that share a warp receive the SAME objects
    shared = _job(K=2, compose_main_images=True, obj_transforms=ROTATED)
    assert shared.main_frames[0] is shared.main_frames[1]


def test_no_placement_composes_the_identity_collage_and_the_defaults_are_the_call_without_the_arguments():
    (want,) = _reference_frames(None, 1, None)
    got = _job(compose_main_images=True)
    assert _same_images(got.main_frames[0], want)
    explicit = _job(main_first_image=want[0], main_image_list=want)
    assert torch.equal(got.frames, explicit.frames)
    defaults = _job(main_first_image=want[0], main_image_list=want, compose_main_images=False, obj_alpha=None)
    assert torch.equal(defaults.frames, explicit.frames) and defaults.main_frames is None


def test_the_calls_refusals():
    clips, alpha = _sources()
    with pytest.raises(ValueError, match="compose_main_images=True builds main_first_image from the sources"):
        _job(compose_main_images=True, main_first_image=clips[0][0])
    with pytest.raises(ValueError, match="compose_main_images=True builds main_image_list from the sources"):
        _job(compose_main_images=True, main_image_list=clips[0])
    with pytest.raises(ValueError, match="needs the objects' image-size masks: obj_mask paths or obj_alpha"):
        _job(compose_main_images=True, obj_alpha=None)
    with pytest.raises(ValueError, match=r"the alpha of object 1 is torch.uint8 \(3, 32, 64\), the call needs uint8 \[F = 3, height = 64, width = 64\]"):
        _job(compose_main_images=True, obj_alpha=[alpha[0], alpha[1][:, ::2]])
    with pytest.raises(ValueError, match="obj_alpha holds 1 arrays for 2 objects"):
        _job(compose_main_images=True, obj_alpha=[alpha[0]])
    with pytest.raises(RuntimeError, match="compose_main_images does not combine with the frame shard: the section masks are cut to "
                                           "pixel slabs and a collage crosses slabs"):
        _job(compose_main_images=True, shard=True)
