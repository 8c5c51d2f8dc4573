#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by IMPORTING THE REFERENCE (this container only).

The reference (``/root/reference``, SobeyMIL/MVOC @ 2024_08_07) is pure Python on top of
diffusers==0.27.2 / torchvision / cv2 / omegaconf, none of which is installed here.  A ``sys.meta_path``
finder fabricates empty stand-in modules for those top-level names so that the reference's own files
``i2vgen-xl/pnp_utils.py``, ``i2vgen-xl/pipelines/pipeline_i2vgen_xl.py`` and ``i2vgen-xl/utils.py`` import
unchanged; the class names the reference dispatches on with ``isinstance`` are pre-seeded with the
ORACLE's module classes (``oracle/unet_ref.py``), so the reference's hook code and forward
re-implementations execute for real against duck-typed modules.  What is recorded is therefore the output
of the reference's code, not of the oracle's.

Outputs are small ``.npz`` files (inputs, weights, masks, outputs).  Neither reference source nor
bytecode is copied anywhere; only this script and the data it produced are committed.

    python tools/gen_golden.py            # rewrites tests/golden/*.npz
"""
import importlib.abc
import importlib.machinery
import logging
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.environ.get("MVOC_GOLDEN_OUT") or os.path.join(REPO, "tests", "golden")  # (override: tests/test_oracle_golden.py regenerates into a scratch dir)
sys.path.insert(0, REPO)

from oracle import unet_ref as U  # noqa: E402
from oracle.sched_ref import DDIMSchedulerRef  # noqa: E402

STUB_ROOTS = ("diffusers", "torchvision", "cv2", "omegaconf", "transformers")


class _StubModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (), {})
        setattr(self, name, cls)
        return cls


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in STUB_ROOTS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _StubModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def install_stubs():
    for k in [k for k in sys.modules if k.split(".")[0] in STUB_ROOTS]:
        del sys.modules[k]
    sys.meta_path.insert(0, _StubFinder())
    import diffusers.utils as du
    import diffusers.utils.logging as dul
    du.USE_PEFT_BACKEND = True
    du.replace_example_docstring = lambda *_a, **_k: (lambda f: f)
    du.is_torch_version = lambda *a: True
    du.logging = dul
    dul.get_logger = logging.getLogger
    import diffusers.models.attention_processor as ap
    ap.AttnProcessor2_0 = U.AttnProcessor2_0
    ap.Attention = U.Attention
    import diffusers.models.attention as att
    att.BasicTransformerBlock = U.BasicTransformerBlock
    att._chunked_feed_forward = None
    import diffusers.models.transformers.transformer_2d as t2d
    t2d.Transformer2DModel = U.Transformer2DModel
    t2d.Transformer2DModelOutput = lambda sample: (sample,)
    import diffusers.models.transformers.transformer_temporal as tt
    tt.TransformerTemporalModel = U.TransformerTemporalModel
    tt.TransformerTemporalModelOutput = lambda sample: (sample,)
    import diffusers.models.upsampling as up
    up.Upsample2D = U.Upsample2D
    import diffusers.models.downsampling as dn
    dn.Downsample2D = U.Downsample2D
    import diffusers.models.unets.unet_i2vgen_xl as ui
    ui.UNet3DConditionOutput = lambda sample: (sample,)
    # the three cv2 / torchvision calls utils.mask_preprocess makes (shimmed: flagged in DESIGN.md)
    import cv2
    cv2.THRESH_BINARY = 0
    cv2.threshold = lambda img, thr, mx, _type: (thr, ((np.asarray(img) > thr) * mx).astype(np.uint8))
    import torchvision
    import torchvision.transforms as TT

    class PILToTensor:
        def __call__(self, img):
            a = np.asarray(img)
            return torch.from_numpy(a.copy())[None] if a.ndim == 2 else torch.from_numpy(a.copy()).permute(2, 0, 1)

    TT.PILToTensor = PILToTensor
    torchvision.transforms = TT
    sys.path[:0] = [os.path.join(REF, "i2vgen-xl"), REF]


class _Pipe:
    """what the reference's register_* functions expect: an object with ``.unet``"""

    def __init__(self, unet):
        self.unet = unet


def _np(t):
    return t.detach().cpu().numpy()


def _masks(num_frames, h, w, seed, soft=True):
    """two moving-rectangle object masks, as (float fp16 [1,4,F,h,w], bool [1,4,F,h,w]) pairs with soft edges"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for j in range(2):
        m = torch.zeros(num_frames, h, w)
        for f in range(num_frames):
            y0 = (1 + j * (h // 2) + f) % max(h - 2, 1)
            x0 = (j * (w // 3) + f) % max(w - 3, 1)
            m[f, y0:y0 + max(h // 3, 1), x0:x0 + max(w // 2, 1)] = 1.0
        u8 = (m * 255).to(torch.uint8)
        if soft:  # a few sub-threshold / partial values like a BICUBIC-resized mask has
            noise = torch.randint(0, 256, m.shape, generator=g, dtype=torch.int32)
            edge = torch.rand(m.shape, generator=g) < 0.25
            u8 = torch.where(edge, noise.to(torch.uint8), u8)
        fl = (u8.float() / 255.0).to(torch.float16)
        bl = u8 > 10
        out.append((fl[None, None].repeat(1, 4, 1, 1, 1), bl[None, None].repeat(1, 4, 1, 1, 1)))
    return out


def gen_processors(pnp_utils):
    """G1 (spatial) / G2 (temporal): the reference's two PnP attention processors, fp16, on/off schedule,
    inject_background in {False, True}.  Q and K handed to SDPA are captured as well."""
    torch.manual_seed(1)
    C, heads, Fr, H, W, hl, wl = 64, 1, 3, 4, 6, 8, 12
    cfg = U.UNetConfig.small4()
    unet = U.I2VGenXLUNet(cfg)
    sched = torch.tensor([981, 961])
    masks = _masks(Fr, hl, wl, seed=3)
    captured = {}
    real_sdpa = torch.nn.functional.scaled_dot_product_attention

    def rec_sdpa(q, k, v, **kw):
        captured["q"], captured["k"] = q.clone(), k.clone()
        return real_sdpa(q, k, v, **kw)

    for kind in ("spatial", "temporal"):
        for inject_background in (False, True):
            attn = U.Attention(C, heads=heads, dim_head=64).half()
            U.init_weights_(attn, seed=11, scale_out=False)
            # borrow the registration code path: it installs the processor class on up_blocks[...].attn1
            pipe = _Pipe(unet)
            if kind == "spatial":
                pnp_utils.register_spatial_attention_pnp(pipe, sched, inject_background)
                proc = unet.up_blocks[1].attentions[1].transformer_blocks[0].attn1.processor
                hs = torch.randn(5 * Fr, H * W, C).half()
            else:
                pnp_utils.register_temp_attention_pnp(pipe, sched, inject_background)
                proc = unet.up_blocks[1].temp_attentions[1].transformer_blocks[0].attn1.processor
                hs = torch.randn(5 * H * W, Fr, C).half()
            proc.mask = masks
            res = {}
            for tag, t in (("on", 981), ("off", 1)):
                proc.t = t
                pnp_utils.F.scaled_dot_product_attention = rec_sdpa
                try:
                    out = proc(attn, hs.clone(), height=H, width=W)
                finally:
                    pnp_utils.F.scaled_dot_product_attention = real_sdpa
                res[f"out_{tag}"] = _np(out)
                res[f"q_{tag}"] = _np(captured["q"])  # [b, heads, tokens, 64]
                res[f"k_{tag}"] = _np(captured["k"])
            np.savez_compressed(
                os.path.join(OUT, f"g{1 if kind == 'spatial' else 2}_{kind}_proc_bg{int(inject_background)}.npz"),
                hidden_states=_np(hs), to_q=_np(attn.to_q.weight), to_k=_np(attn.to_k.weight),
                to_v=_np(attn.to_v.weight), to_out_w=_np(attn.to_out[0].weight), to_out_b=_np(attn.to_out[0].bias),
                mask_float=np.stack([_np(m[0]) for m in masks]), mask_bool=np.stack([_np(m[1]) for m in masks]),
                frames=Fr, height=H, width=W, heads=heads, **res)


def gen_feature_injection(pnp_utils):
    """G3 resnet / G4 temporal conv / G5 conv_out: the reference's patched forwards, fp16, on/off schedule."""
    torch.manual_seed(2)
    Fr, H, W = 3, 8, 12
    cfg = U.UNetConfig.small4()
    unet = U.I2VGenXLUNet(cfg).half()
    U.init_weights_(unet, seed=5)
    pipe = _Pipe(unet)
    sched = torch.tensor([981, 961])
    masks = _masks(Fr, H, W, seed=4)
    pnp_utils.register_resnet_injection(pipe, sched)
    pnp_utils.register_temp_conv_injection(pipe, sched)
    pnp_utils.register_out_conv_injection(pipe, sched)
    rn = unet.up_blocks[3].resnets[0]  # 128+64 -> 64 channels, has a 1x1 shortcut
    tc = unet.up_blocks[3].temp_convs[0]
    co = unet.conv_out
    cin = rn.norm1.num_channels
    cmid = tc.conv1[0].num_channels
    x_rn = torch.randn(5 * Fr, cin, H, W).half()
    temb = torch.randn(5 * Fr, unet.time_embedding.linear_2.out_features).half()
    x_tc = torch.randn(5 * Fr, cmid, H, W).half()
    x_co = torch.randn(5 * Fr, unet.conv_out.in_channels, H, W).half()
    res = {}
    for tag, t in (("on", 961), ("off", 21)):
        for m in (rn, tc, co):
            m.t, m.mask = t, masks
        res[f"resnet_{tag}"] = _np(rn.forward(x_rn.clone(), temb.clone()))
        res[f"tconv_{tag}"] = _np(tc.forward(x_tc.clone(), num_frames=Fr))
        res[f"convout_{tag}"] = _np(co.forward(x_co.clone()))
    sd = {}
    for prefix, mod in (("resnet.", rn), ("tconv.", tc), ("convout.", co)):
        for k, v in mod.state_dict().items():
            sd[prefix + k] = _np(v)
    np.savez_compressed(os.path.join(OUT, "g3_g4_g5_feature_injection.npz"), x_resnet=_np(x_rn), temb=_np(temb),
                        x_tconv=_np(x_tc), x_convout=_np(x_co), frames=Fr,
                        mask_float=np.stack([_np(m[0]) for m in masks]), mask_bool=np.stack([_np(m[1]) for m in masks]),
                        **res, **{"w:" + k: v for k, v in sd.items()})


def gen_transformer_forwards(pnp_utils):
    """G6: the reference's re-implemented forwards of TransformerTemporalModel / BasicTransformerBlock /
    Attention / Transformer2DModel (bound by modify_diffuser_attention_forward) driven on oracle modules, fp32."""
    torch.manual_seed(3)
    Fr, H, W, C, ctx = 3, 4, 6, 64, 64
    holder = torch.nn.Module()
    holder.spa = U.Transformer2DModel(1, 64, C, ctx, 8)
    holder.tmp = U.TransformerTemporalModel(1, 64, C, 8)
    U.init_weights_(holder, seed=7)
    x = torch.randn(2 * Fr, C, H, W)
    enc = torch.randn(2 * Fr, 9, ctx)
    pnp_utils.modify_diffuser_attention_forward(holder)  # rebinds .forward on every matching submodule
    assert "partial" in type(holder.spa.forward).__name__ or hasattr(holder.spa.forward, "func")
    with torch.no_grad():
        o_spa = holder.spa.forward(x, encoder_hidden_states=enc, return_dict=False)[0]
        o_tmp = holder.tmp.forward(x, num_frames=Fr, return_dict=False)[0]
    sd = {"w:" + k: _np(v) for k, v in holder.state_dict().items()}
    np.savez_compressed(os.path.join(OUT, "g6_transformer_forwards.npz"), x=_np(x), enc=_np(enc), frames=Fr,
                        out_spatial=_np(o_spa), out_temporal=_np(o_tmp), **sd)


def gen_unet_ext(pnp_utils, pipeline_mod):
    """G7: ``I2VGenXLUnetExtension.forward`` (the reference's custom UNet forward) on the toy UNet, fp32:
    (a) plain, batch 2; (b) batch 5 with all five PnP hook families registered by the reference's own
    ``register_*`` functions, masks pushed by its ``register_time_all``, on- and off-schedule."""
    torch.manual_seed(4)
    cfg = U.UNetConfig.small4()
    unet = U.I2VGenXLUNet(cfg)
    U.init_weights_(unet, seed=9)
    for p_ in unet.parameters():  # make every weight fp16-representable: the HIP path stores fp16 weights
        p_.copy_(p_.half().float())
    Fr, h, w = 4, 8, 8
    ext = pipeline_mod.I2VGenXLUnetExtension.forward

    def inputs(b):
        g = torch.Generator().manual_seed(100 + b)
        return dict(sample=torch.randn(b, 4, Fr, h, w, generator=g), fps=torch.tensor([8] * b),
                    image_latents_first=torch.randn(b, 4, Fr, h, w, generator=g),
                    image_latents=torch.randn(b, 4, Fr, h, w, generator=g),
                    image_embeddings=torch.randn(b, Fr, cfg.cross_attention_dim, generator=g),
                    encoder_hidden_states=torch.randn(b, 7, cfg.cross_attention_dim, generator=g))

    save = {"cfg_block_out_channels": np.array(cfg.block_out_channels), "frames": Fr}
    with torch.no_grad():
        i2 = inputs(2)
        o = ext(unet, i2["sample"], 961, i2["fps"], i2["image_latents_first"], i2["image_latents"],
                i2["image_embeddings"], i2["encoder_hidden_states"], return_dict=False)[0]
        save.update({"plain_" + k: _np(v) for k, v in i2.items()})
        save["plain_out"] = _np(o)
        save["plain_t"] = 961

        # PnP: the reference's registration order (composite.py:54-60)
        pipe = _Pipe(unet)
        full = DDIMSchedulerRef()
        full.set_timesteps(50)
        pnp_utils.modify_diffuser_attention_forward(unet)
        pnp_utils.register_temp_attention_pnp(pipe, full.timesteps[:50], False)
        pnp_utils.register_spatial_attention_pnp(pipe, full.timesteps[:50], False)
        pnp_utils.register_temp_conv_injection(pipe, full.timesteps[:5])
        pnp_utils.register_out_conv_injection(pipe, full.timesteps[:5])
        pnp_utils.register_resnet_injection(pipe, full.timesteps[:5])
        masks = _masks(Fr, h, w, seed=6)
        i5 = inputs(5)
        save.update({"pnp_" + k: _np(v) for k, v in i5.items()})
        save["pnp_mask_float"] = np.stack([_np(m[0]) for m in masks])
        save["pnp_mask_bool"] = np.stack([_np(m[1]) for m in masks])
        for tag, t in (("t981", 981), ("t861", 861), ("t1", 1)):  # conv+attn / attn only / attn only (last step)
            pnp_utils.register_time_all(pipe, t, masks)
            o = ext(unet, i5["sample"], t, i5["fps"], i5["image_latents_first"], i5["image_latents"],
                    i5["image_embeddings"], i5["encoder_hidden_states"], return_dict=False)[0]
            save["pnp_out_" + tag] = _np(o)
    # the toy's weights (40 MB) are not stored: tests rebuild them with the same seeded init
    # (oracle.unet_ref.init_weights_(seed=9) + fp16 rounding) and verify this checksum first
    save["weights_abs_sum"] = np.float64(sum(float(v.double().abs().sum()) for v in unet.state_dict().values()))
    np.savez_compressed(os.path.join(OUT, "g7_unet_ext.npz"), **save)


def gen_masks(ref_utils):
    """G9: ``utils.mask_preprocess`` (reference code; cv2.threshold / PILToTensor shimmed) on the boat_surf demo
    masks: native 1280x720 -> [16,90,160], and PNGs first resized to 512x512 -> [16,64,64] (bench config)."""
    import tempfile
    from PIL import Image
    out = {}
    for name in ("boat_mask", "surf_mask"):
        src = os.path.join(REF, "demo", "boat_surf", name)
        fl, bl = ref_utils.mask_preprocess(src, "cpu", torch.float16, 1, 4, 16, downscale=8)
        out[f"{name}_90x160_float_u8"] = np.round(_np(fl[0, 0]).astype(np.float32) * 255).astype(np.uint8)
        out[f"{name}_90x160_bool"] = _np(bl[0, 0])
        with tempfile.TemporaryDirectory() as td:
            for i in range(16):
                Image.open(os.path.join(src, f"{i:05d}.png")).resize((512, 512), Image.NEAREST).save(
                    os.path.join(td, f"{i:05d}.png"))
            fl, bl = ref_utils.mask_preprocess(td, "cpu", torch.float16, 1, 4, 16, downscale=8)
        out[f"{name}_64x64_float_u8"] = np.round(_np(fl[0, 0]).astype(np.float32) * 255).astype(np.uint8)
        out[f"{name}_64x64_bool"] = _np(bl[0, 0])
    np.savez_compressed(os.path.join(OUT, "g9_boat_surf_masks.npz"), **out)


def copy_mask_pngs():
    """G9 inputs: the boat_surf demo's 2 x 16 mask PNGs (data files of the reference's demo, 1280x720 palette images,
    580 KB) so that the PRODUCT's ``mvoc_amd.utils.mask_preprocess`` can be run against G9 on machines without
    /root/reference (tests/test_host_cpu.py::test_mask_preprocess_matches_g9)"""
    import shutil
    for name in ("boat_mask", "surf_mask"):
        dst = os.path.join(OUT, "boat_surf_masks", name)
        os.makedirs(dst, exist_ok=True)
        for i in range(16):
            shutil.copyfile(os.path.join(REF, "demo", "boat_surf", name, f"{i:05d}.png"), os.path.join(dst, f"{i:05d}.png"))


# ---- G8: the three denoising loops, run from the reference's own pipeline methods --------------------------------
def fake_unet(x, t, ehs, fps, ilf, il, ie):
    """Stand-in for the UNet inside the loops: elementwise fp16 arithmetic only (bit-reproducible on any machine), a
    different function of every input so that a wrong batch / conditioning order changes the result.  The tests carry
    the same function (tests/test_oracle_golden.py); it is test scaffolding, not part of either code base."""
    s = (ehs[:, 0, 0].float() * 0.01 + ie[:, 0, 0].float() * 0.02 + fps.float() * 0.001 + float(t) * 1e-4).to(x.dtype)
    return x * 0.5 + il * 0.25 - ilf * 0.125 + s[:, None, None, None, None]


def _seeded(key, shape, scale=1.0):
    g = torch.Generator().manual_seed(int(key) % (2 ** 31))
    return (torch.randn(shape, generator=g) * scale).half()


def _loop_pipe(pipeline_mod, pnp_utils, unet, scheduler, calls, Fr, h, w, D):
    """an I2VGenXLPipeline instance without diffusers underneath: the encoders are seeded stand-ins keyed by the "image"
    (a 1-element id tensor) / prompt string; everything between them and the scheduler is the reference's code"""
    P = pipeline_mod.I2VGenXLPipeline
    pipe = object.__new__(P)
    pipe.unet, pipe.scheduler, pipe.vae_scale_factor = unet, scheduler, 8
    pipe.device = pipe._execution_device = torch.device("cpu")
    pipe.check_inputs = lambda *a, **k: None
    pipe.maybe_free_model_hooks = lambda: None

    class _Bar:
        def __enter__(self): return self
        def __exit__(self, *a): return False
        def update(self): pass
    pipe.progress_bar = lambda total=None: _Bar()

    def encode_prompt(prompt, device, n, negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None, **_):
        key = lambda s_: 7 + sum(str(s_).encode())
        pe = prompt_embeds if prompt_embeds is not None else _seeded(key(prompt), (1, 7, D))
        ne = negative_prompt_embeds if negative_prompt_embeds is not None else _seeded(1000 + key(negative_prompt), (1, 7, D))
        return pe, ne
    pipe.encode_prompt = encode_prompt
    pipe.image_processor = types.SimpleNamespace(preprocess=lambda img: img.float())
    pipe.feature_extractor = types.SimpleNamespace(crop_size={"width": 4, "height": 4})

    class _Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float16))
        def forward(self, image):
            return types.SimpleNamespace(image_embeds=_seeded(300 + int(image.reshape(-1)[0]), (1, D)))
    pipe.image_encoder = _Enc()
    pipe.vae = types.SimpleNamespace(
        config=types.SimpleNamespace(scaling_factor=0.18215),
        encode=lambda image: types.SimpleNamespace(latent_dist=types.SimpleNamespace(
            sample=lambda: _seeded(500 + int(image.reshape(-1)[0]), (1, 4, h, w)))))
    pipeline_mod._center_crop_wide = lambda img, size: img
    pipeline_mod._resize_bilinear = lambda img, size: img

    def unet_forward(sample, t, encoder_hidden_states=None, fps=None, image_latents=None, image_embeddings=None,
                     image_latents_first=None, cross_attention_kwargs=None, multi_frame_guidance=False, return_dict=True, **_):
        ilf = image_latents if image_latents_first is None else image_latents_first
        calls.append(dict(x=sample.clone(), t=int(t), ehs=encoder_hidden_states.clone(), fps=fps.clone(), ilf=ilf.clone(),
                          il=image_latents.clone(), ie=image_embeddings.clone(), mfg=bool(multi_frame_guidance),
                          hook_t=getattr(unet.up_blocks[-1].resnets[0], "t", None)))
        ie = image_embeddings if image_embeddings.dim() == 3 else image_embeddings[:, None]
        return (fake_unet(sample, t, encoder_hidden_states, fps, ilf, image_latents, ie),)
    unet.forward = unet_forward
    return pipe


def gen_loops(pnp_utils, pipeline_mod):
    """G8: ``invert`` (a1), ``__call__`` (a3) and ``sample_with_pnp_...`` (a2) of the reference, with its own
    ``prepare_image_latents`` / ``_encode_image`` / ``prepare_latents`` / batch assembly / fusion / CFG / permutes and the
    oracle's scheduler restatement (diffusers' is absent); the UNet is ``fake_unet``.  Recorded: everything the UNet
    was called with at every step, the hook state pushed by ``register_time_all`` before each call, the final latents
    and the written ``ddim_latents_{t}.pt`` files."""
    import tempfile
    from oracle.sched_ref import DDIMInverseSchedulerRef
    Fr, h, w, D = 3, 4, 4, 64
    cfg = U.UNetConfig.small4()
    save = {"frames": Fr, "h": h, "w": w, "dim": D}
    img = lambda i: torch.tensor([float(i)])

    def dump(tag, calls):
        save[f"{tag}_ncalls"] = len(calls)
        for k in ("x", "ehs", "fps", "ilf", "il", "ie"):
            save[f"{tag}_{k}"] = np.stack([_np(c[k]) for c in calls])
        save[f"{tag}_t"] = np.array([c["t"] for c in calls])
        save[f"{tag}_mfg"] = np.array([c["mfg"] for c in calls])
        save[f"{tag}_hook_t"] = np.array([-1 if c["hook_t"] is None else int(c["hook_t"]) for c in calls])

    with torch.no_grad(), tempfile.TemporaryDirectory() as td:
        # ---- a1: invert, cfg 1.0 (inverse.py's setting) and cfg 7.5 ------------------------------------------------
        for tag, gs in (("inv_cfg1", 1.0), ("inv_cfg75", 7.5)):
            unet = U.I2VGenXLUNet(cfg)
            calls = []
            pipe = _loop_pipe(pipeline_mod, pnp_utils, unet, DDIMInverseSchedulerRef(), calls, Fr, h, w, D)
            out_dir = os.path.join(td, tag)
            x0 = _seeded(11, (1, 4, Fr, h, w))
            seq = pipe.invert(prompt="a boat", image=img(3), height=h * 8, width=w * 8, target_fps=8, num_frames=Fr,
                              num_inference_steps=4, guidance_scale=gs, negative_prompt="bad", latents=x0.clone(),
                              return_dict=False, output_dir=out_dir)
            seq = seq[0] if isinstance(seq, (tuple, list)) else seq
            dump(tag, calls)
            save[f"{tag}_x0"], save[f"{tag}_out"] = _np(x0), _np(seq)
            files = sorted(os.listdir(out_dir))
            save[f"{tag}_files"] = np.array(files)
            save[f"{tag}_file_latents"] = np.stack([_np(torch.load(os.path.join(out_dir, f))) for f in files])
        # ---- a3: __call__ from a stored latent, cfg 9.0, ddim_init_latents_t_idx 1 -------------------------------------
        unet = U.I2VGenXLUNet(cfg)
        calls = []
        pipe = _loop_pipe(pipeline_mod, pnp_utils, unet, DDIMSchedulerRef(), calls, Fr, h, w, D)
        xT = _seeded(12, (1, 4, Fr, h, w))
        res = pipe(prompt="a boat", image=img(3), height=h * 8, width=w * 8, target_fps=8, num_frames=Fr, num_inference_steps=4,
                   guidance_scale=9.0, negative_prompt="bad", latents=xT.clone(), output_type="latent",
                   ddim_init_latents_t_idx=1, decode_chunk_size=1)
        dump("call", calls)
        save["call_xT"], save["call_out"] = _np(xT), _np(res.frames)
        # ---- a2: composition, 2 objects, all hook families registered as composite.py does -----------------------------
        for tag, kw in (("comp", dict(random_noise_ratio=0.0, obj_random_noise_fusion=False, fusion_steps=(0, 1))),
                        ("comp_rnf", dict(random_noise_ratio=0.3, obj_random_noise_fusion=True, fusion_steps=(0, 2)))):
            unet = U.I2VGenXLUNet(cfg)
            calls = []
            sched = DDIMSchedulerRef()
            pipe = _loop_pipe(pipeline_mod, pnp_utils, unet, sched, calls, Fr, h, w, D)
            full = DDIMSchedulerRef()
            full.set_timesteps(5)
            holder = _Pipe(unet)
            pnp_utils.modify_diffuser_attention_forward(unet)
            pnp_utils.register_temp_attention_pnp(holder, full.timesteps[:5], False)
            pnp_utils.register_spatial_attention_pnp(holder, full.timesteps[:5], False)
            pnp_utils.register_temp_conv_injection(holder, full.timesteps[:2])
            pnp_utils.register_out_conv_injection(holder, full.timesteps[:2])
            pnp_utils.register_resnet_injection(holder, full.timesteps[:2])
            masks = _masks(Fr, h, w, seed=8)
            pipeline_mod.mask_preprocess = lambda om, device, dtype, b, c, f, downscale=8: masks[int(om)]
            dirs = {}
            for name, key in (("bg", 20), ("obj0", 30), ("obj1", 40)):
                d_ = os.path.join(td, f"{tag}_{name}")
                os.makedirs(d_)
                for t in full.timesteps:
                    torch.save(_seeded(key * 1000 + int(t), (1, 4, Fr, h, w)), os.path.join(d_, f"ddim_latents_{int(t)}.pt"))
                dirs[name] = d_
            xT = _seeded(13, (1, 4, Fr, h, w))
            res = pipe.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection(
                prompt="windsurf", main_first_image=img(1), main_image_list=[img(10 + i) for i in range(Fr)],
                background_first_image=img(2), background_image_list=[img(20 + i) for i in range(Fr)],
                objs_first_image=[img(4), img(5)], objs_image_list=[[img(40 + i) for i in range(Fr)], [img(50 + i) for i in range(Fr)]],
                height=h * 8, width=w * 8, target_fps=8, num_frames=Fr, num_inference_steps=5, guidance_scale=9.0,
                negative_prompt="chaotic", latents=xT.clone(), output_type="latent", ddim_init_latents_t_idx=1,
                ddim_inv_prompt="", obj_mask=["0", "1"], obj_width_height=[(w * 8, h * 8)] * 2,
                obj_ddim_latents_idx_offset=[0, 1], bg_inv_latents_path=dirs["bg"],
                obj_ddim_latents_path=[dirs["obj0"], dirs["obj1"]], **kw)
            dump(tag, calls)
            save[f"{tag}_xT"], save[f"{tag}_out"] = _np(xT), _np(res.frames)
            save[f"{tag}_mask_float"] = np.stack([_np(m[0]) for m in masks])
            save[f"{tag}_mask_bool"] = np.stack([_np(m[1]) for m in masks])
    np.savez_compressed(os.path.join(OUT, "g8_loops.npz"), **save)


# ---- G10: composite.init_pnp (a15): which modules get which injection schedule, for the 7 demo entries ---------------
def hooked_state(unet):
    """{module path: [schedule..] (+ inject_background)} for everything the registration functions touched"""
    out = {}
    for name, m in unet.named_modules():
        for holder, suffix in ((m, ""), (getattr(m, "processor", None), ".processor")):
            if holder is not None and hasattr(holder, "injection_schedule"):
                sch = holder.injection_schedule
                out[name + suffix] = {"schedule": [int(v) for v in sch] if sch is not None else None,
                                      "inject_background": bool(getattr(holder, "inject_background", False))}
    return out


def gen_init_pnp():
    import json
    import yaml
    import composite as ref_composite  # the reference's harness
    assert ref_composite.__file__.startswith(REF)
    tmpl = yaml.safe_load(open(os.path.join(REF, "i2vgen-xl", "configs", "group_composite", "template.yaml")))
    entries = json.load(open(os.path.join(REF, "i2vgen-xl", "configs", "group_composite", "group_config.json")))
    keys = ("n_steps", "pnp_f_t", "pnp_spatial_attn_t", "pnp_temp_attn_t", "pnp_cross_attn_t", "inject_background")
    out = []
    for e in entries:
        cfg = types.SimpleNamespace(**{k: e.get(k, tmpl[k]) for k in keys})
        unet = U.I2VGenXLUNet(U.UNetConfig.small4())
        sched = DDIMSchedulerRef()
        sched.set_timesteps(cfg.n_steps)
        ref_composite.init_pnp(_Pipe(unet), sched, cfg)
        out.append({"video_name": e["video_name"], "config": vars(cfg), "hooked": hooked_state(unet)})
    json.dump(out, open(os.path.join(OUT, "g10_init_pnp.json"), "w"), indent=0, sort_keys=True)


def write_digests():
    """SHA256SUMS beside the fixtures (sha256sum format): lets the CPU suite check the committed files without the reference"""
    import hashlib
    with open(os.path.join(OUT, "SHA256SUMS"), "w") as fh:
        for f in sorted(x for x in os.listdir(OUT) if x.endswith((".npz", ".json"))):
            fh.write(f"{hashlib.sha256(open(os.path.join(OUT, f), 'rb').read()).hexdigest()}  {f}\n")


def main():
    os.makedirs(OUT, exist_ok=True)
    if "--only-mask-pngs" in sys.argv:
        return copy_mask_pngs()
    install_stubs()
    import pnp_utils  # the reference's
    from pipelines import pipeline_i2vgen_xl  # the reference's
    import utils as ref_utils  # the reference's
    assert pnp_utils.__file__.startswith(REF) and ref_utils.__file__.startswith(REF)
    torch.set_grad_enabled(False)
    gen_processors(pnp_utils)
    gen_feature_injection(pnp_utils)
    gen_transformer_forwards(pnp_utils)
    gen_unet_ext(pnp_utils, pipeline_i2vgen_xl)
    gen_masks(ref_utils)
    copy_mask_pngs()
    gen_loops(pnp_utils, pipeline_i2vgen_xl)
    gen_init_pnp()
    write_digests()
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
