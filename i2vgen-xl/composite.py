#!/usr/bin/env python3
"""Stage 2 of MVOC on MI355X: PnP composition sampling for every active entry of a group config.  Same CLI, config
keys, hook registration order and output naming as the reference's ``i2vgen-xl/composite.py``.

    PYTHONPATH=.. python composite.py --template_config configs/group_composite/template.yaml \
                                      --configs_json configs/group_composite/group_config.json [--synthetic] [--shard i/n]
                                      [--dedup_sources]

``--dedup_sources``: roles (background, objects) that are the same source share one UNet chunk.
An entry with ``variants: [{...}, ...]`` composes K prompts / seeds / guidance scales over its sources in one loop
(``merge_variants``; files under ``.../variant_00/``, ``variant_01/`` ...); a variant's ``pnp: {...}`` gives it injection
thresholds of its own.  An entry's ``obj_offset: [[dx, dy], ...]`` (one item per object: a pair, or one pair per frame; image
pixels in multiples of 8) places the objects at composition time (``placement_kwargs``; shared by the entry's variants).
A variant's ``placement: [[dx, dy], ...]`` (the format of ``obj_offset``) places the objects for that variant alone
(``variant_placement_kwargs``); a variant without the key takes the entry's ``obj_offset``, or none.
An entry's ``obj_transform: [{offset, scale, flip, anchor, rotate}, ...]`` (one dict per object, every key optional) scales,
mirrors, turns (``rotate``: degrees counter-clockwise or one angle per frame, not in a variant's ``transform``) and places the objects at composition time (``transform_kwargs``; shared by the entry's variants, not with ``obj_offset`` or a
variant's ``placement``).  A variant's ``transform: [{...}, ...]`` (the format of ``obj_transform``) transforms the objects for
that variant alone; a variant without the key takes the entry's ``obj_transform``, or none.
An entry's ``compose_main: true`` has the call build the main conditioning frames from the background and object
frames under the entry's own placement (``compose_main_kwargs``): ``edited_first_frame_path`` and
``edited_contorl_frame_path_main`` are not loaded, and the composed frames are written as ``main_00000.png`` ... beside each output.
An entry's ``obj_mask_edit: {grow, feather}`` or ``[{grow, feather}, null, ...]`` (latent pixels, ``grow`` in [-8, 8],
``feather`` in [0, 8]) grows or shrinks and feathers the objects' masks at composition time (``mask_edit_kwargs``; shared by the
entry's variants: a variant that sets it is refused).
"""
import argparse
import json
import logging
import os
from functools import partial
from pathlib import Path

import torch
from PIL import Image

from common import PRETRAINED_MODEL_PATH
from mvoc_amd.config import OmegaConf
from mvoc_amd.launch import my_entries, pick_device
from mvoc_amd.schedulers import DDIMScheduler
from pipelines.pipeline_i2vgen_xl import I2VGenXLPipeline, I2VGenXLUnetExtension
from pnp_utils import (modify_diffuser_attention_forward, register_out_conv_injection, register_resnet_injection,
                       register_spatial_attention_pnp, register_temp_attention_pnp, register_temp_conv_injection,
                       register_variant_schedules)
from utils import export_to_gif, load_image, seed_everything

logger = logging.getLogger(__name__)


def _schedule_prefixes(scheduler, config):
    n = config.n_steps
    conv_t, spa_t, tmp_t = int(n * config.pnp_f_t), int(n * config.pnp_spatial_attn_t), int(n * config.pnp_temp_attn_t)
    conv_ts = scheduler.timesteps[:conv_t] if conv_t >= 0 else []
    spa_ts = scheduler.timesteps[:spa_t] if spa_t >= 0 else []
    tmp_ts = scheduler.timesteps[:tmp_t] if tmp_t >= 0 else []
    return (conv_t, spa_t, tmp_t), (conv_ts, spa_ts, tmp_ts)


def init_pnp(pipe, scheduler, config, variants=None):
    """injection schedules are prefixes of the FULL timestep list (``composite.py:38-60``), registered in the
    reference's order: forward patch, temporal attn, spatial attn, temporal conv, conv_out, resnet.  ``variants``: the merged
    configs of the entry's variants (``merge_variants``); when one of them carries thresholds of its own (``pnp``) every
    variant's prefixes are registered on top (``register_variant_schedules``), by the same ``int(n * t)`` rule."""
    (conv_t, spa_t, tmp_t), (conv_ts, spa_ts, tmp_ts) = _schedule_prefixes(scheduler, config)
    modify_diffuser_attention_forward(pipe.unet)
    register_temp_attention_pnp(pipe, tmp_ts, config.inject_background)
    register_spatial_attention_pnp(pipe, spa_ts, config.inject_background)
    register_temp_conv_injection(pipe, conv_ts)
    register_out_conv_injection(pipe, conv_ts)
    register_resnet_injection(pipe, conv_ts)
    logger.debug(f"conv/spatial/temporal injection steps: {conv_t}/{spa_t}/{tmp_t}")
    if variants is not None and any("pnp" in c for c in variants):
        per = [_schedule_prefixes(scheduler, c) for c in variants]
        register_variant_schedules(pipe, conv=[p[1][0] for p in per], spatial=[p[1][1] for p in per],
                                   temporal=[p[1][2] for p in per])
        logger.debug(f"per-variant conv/spatial/temporal injection steps: {[p[0] for p in per]}")


def _frames(folder, n, size):
    out = []
    for i in range(n):
        out.append(load_image(os.path.join(folder, f"{i:0>5d}.png")).resize(tuple(size), resample=Image.Resampling.LANCZOS))
    return out


def output_suffix(config):
    return ("ddim_init_latents_t_idx_" + str(config.ddim_init_latents_t_idx) + "_nsteps_" + str(config.n_steps) + "_cfg_"
            + str(config.cfg) + "_pnpf" + str(config.pnp_f_t) + "_pnps" + str(config.pnp_spatial_attn_t) + "_pnpt"
            + str(config.pnp_temp_attn_t) + "_ratio" + str(config.random_noise_ratio) + "noise_fusion_step"
            + f"{config.fusion_step[0]}-{config.fusion_step[1]}")


# what one variant of an entry may override; every other key is shared by the variants of a call (sources, masks, the entry's
# schedules, fusion settings: the source chunks are computed once for all of them).  "pnp" is a dict of injection thresholds
# of the variant's own (any of PNP_KEYS) -- the flat threshold keys stay the entry's.  "placement" is the variant's
# own object placement in the format of the entry's ``obj_offset`` -- ``obj_offset`` itself stays the entry's;
# "transform" the variant's own scale / mirror / offset in the format of the entry's ``obj_transform``
VARIANT_KEYS = ("editing_prompt", "editing_negative_prompt", "seed", "cfg", "edited_first_frame_path",
                "edited_contorl_frame_path_main", "pnp", "placement", "transform")
PNP_KEYS = ("pnp_f_t", "pnp_spatial_attn_t", "pnp_temp_attn_t")
MAX_VARIANTS = 8


def resolve_config(template_config, entry):
    """template + entry, paths resolved against ``data_dir`` (``composite.py:88-110``)"""
    config = OmegaConf.merge(template_config, OmegaConf.create(entry))
    d = config.data_dir
    config.video_path = os.path.join(config.video_dir, config.video_name + ".mp4")
    config.video_frames_path = os.path.join(config.video_dir, config.video_name)
    config.edited_first_frame_path = os.path.join(d, config.edited_first_frame_path)
    config.obj_mask_path = [os.path.join(d, p) for p in config.obj_mask_path]
    config.obj_ddim_latents_path = [os.path.join(d, p) for p in config.obj_ddim_latents_path]
    config.bg_ddim_latents_path = os.path.join(d, config.bg_ddim_latents_path)
    config.edited_contorl_frame_path_main = os.path.join(d, config.edited_contorl_frame_path_main)
    config.edited_contorl_frame_path_background = os.path.join(d, config.edited_contorl_frame_path_background)
    config.edited_contorl_frame_path = [os.path.join(d, p) for p in config.edited_contorl_frame_path]
    return config


def merge_variants(template_config, entry):
    """An entry may carry ``variants: [{...}, ...]``: K compositions over the entry's sources in one loop, each dict overriding
    any of ``VARIANT_KEYS`` (``pnp``: a dict over ``PNP_KEYS``, the variant's own injection thresholds).  -> (config, None)
    for an entry without the key -- exactly the single composition -- else (the entry's own config, [merged config of
    variant k]).  Overriding a shared key is an error that names it."""
    entry = dict(entry)
    variants = entry.pop("variants", None)
    config = resolve_config(template_config, entry)
    if variants is None:
        return config, None
    if not 1 <= len(variants) <= MAX_VARIANTS:
        raise ValueError(f"variants: {len(variants)} entries, 1 to {MAX_VARIANTS} share one set of sources")
    merged = []
    for k, v in enumerate(variants):
        for key in v:
            if key not in VARIANT_KEYS:
                raise ValueError(f"variants[{k}] overrides '{key}', which all variants of an entry share; a variant may set "
                                 f"{', '.join(VARIANT_KEYS)}")
        pnp = dict(v.get("pnp") or {})
        for key in pnp:
            if key not in PNP_KEYS:
                raise ValueError(f"variants[{k}].pnp sets '{key}'; the per-variant injection thresholds are {', '.join(PNP_KEYS)}")
        # the thresholds land on the variant's merged config: output_suffix / variant_output_dir show the variant's own
        merged.append(resolve_config(template_config, {**entry, **dict(v), **pnp}))
    return config, merged


def placement_kwargs(config):
    """the entry's optional ``obj_offset`` -> keyword arguments of the sampling call: none when the key is absent (the call is
    then exactly today's), else ``obj_offsets`` = one item per object, ``[dx, dy]`` or one such pair per frame, in image pixels
    (the call checks and normalises them).  Shared by the variants of an entry: not one of ``VARIANT_KEYS``."""
    if "obj_offset" not in config or config.obj_offset is None:
        return {}
    plain = lambda v: [plain(x) for x in v] if hasattr(v, "__iter__") and not isinstance(v, (str, bytes)) else v
    return {"obj_offsets": plain(config.obj_offset)}


def variant_placement_kwargs(config, variants):
    """keyword arguments of the sampling call for the placements of an entry and its variants (``merge_variants``): when no
    variant sets ``placement`` exactly ``placement_kwargs(config)``; else ``variant_obj_offsets`` = one item per variant -- the
    variant's ``placement``, or the entry's ``obj_offset`` (None without one) for a variant that does not set the key."""
    if variants is None or not any("placement" in c and c.placement is not None for c in variants):
        return placement_kwargs(config)
    plain = lambda v: [plain(x) for x in v] if hasattr(v, "__iter__") and not isinstance(v, (str, bytes)) else v
    shared = placement_kwargs(config).get("obj_offsets")
    return {"variant_obj_offsets": [plain(c.placement) if "placement" in c and c.placement is not None else shared
                                    for c in variants]}


def _filter_kwargs(config):
    """the entry's optional ``obj_transform_filter`` ("nearest" or "bilinear"; next to ``obj_transform``) -> the
    sampling call's keyword of that name; absent or None: no keyword (exactly today's call).  Any other value is refused here,
    whatever else the entry sets"""
    if "obj_transform_filter" not in config or config.obj_transform_filter is None:
        return {}
    value = config.obj_transform_filter
    if value not in ("nearest", "bilinear"):
        raise ValueError(f"obj_transform_filter {value!r} is not one of 'nearest', 'bilinear'")
    return {"obj_transform_filter": str(value)}


def transform_kwargs(config, variants=None):
    """the entry's optional ``obj_transform`` (one dict per object: ``offset``, ``scale``, ``flip``, ``anchor``, ``rotate``)
    with the placements of ``variant_placement_kwargs``: none of the keys -> {} (exactly today's call); ``obj_transform`` alone
    -> ``obj_transforms`` as plain dicts and lists (the call checks and normalises them; shared by the entry's variants: not one
    of ``VARIANT_KEYS``); together with ``obj_offset`` or any variant's ``placement`` it is an error -- a transform carries its
    own offset.  ``obj_width_height`` stays ignored, as in the reference.
    ``obj_transform_filter`` ("nearest" / "bilinear") goes with ``obj_transform`` to the call as it is; "bilinear"
    without ``obj_transform`` or next to a variant's ``transform`` is an error, and so is any other value.
    A variant's ``transform`` (the format of ``obj_transform``) transforms the objects for that variant alone:
    ``variant_obj_transforms`` = one item per variant -- the variant's ``transform``, or the entry's ``obj_transform`` (None
    without one) for a variant that does not set the key; not with the entry's ``obj_offset`` or any variant's ``placement``."""
    def plain(v):
        if hasattr(v, "keys"):
            return {str(k): plain(v[k]) for k in v.keys()}
        return [plain(x) for x in v] if hasattr(v, "__iter__") and not isinstance(v, (str, bytes)) else v

    bilinear = _filter_kwargs(config).get("obj_transform_filter") == "bilinear"  # (a misspelt value is refused in every case)
    if variants is not None and any("transform" in c and c.transform is not None for c in variants):
        if bilinear:
            raise ValueError("obj_transform_filter is 'bilinear' and a variant sets 'transform': the filter samples the objects of "
                             "obj_transform, one filter for all variants (per-variant warps are not built)")
        if "obj_offset" in config and config.obj_offset is not None:
            raise ValueError("a variant sets 'transform' and the entry sets obj_offset: put the offset into the transform ('offset')")
        if any("placement" in c and c.placement is not None for c in variants):
            raise ValueError("a variant sets 'transform' and a variant sets 'placement': put the offset into the transform "
                             "('offset')")
        shared = plain(config.obj_transform) if "obj_transform" in config and config.obj_transform is not None else None
        return {"variant_obj_transforms": [plain(c.transform) if "transform" in c and c.transform is not None else shared
                                           for c in variants]}
    if "obj_transform" not in config or config.obj_transform is None:
        if bilinear:
            raise ValueError("obj_transform_filter is 'bilinear' without obj_transform: the filter samples the entry's transformed "
                             "objects")
        return variant_placement_kwargs(config, variants)
    if "obj_offset" in config and config.obj_offset is not None:
        raise ValueError("obj_transform and obj_offset are both set: put the offset into the transform ('offset')")
    if variants is not None and any("placement" in c and c.placement is not None for c in variants):
        raise ValueError("obj_transform is set and a variant sets 'placement': one transform serves all variants of an entry")
    return {"obj_transforms": plain(config.obj_transform), **_filter_kwargs(config)}


def compose_main_kwargs(config, variants=None):
    """the entry's optional ``compose_main: true`` -> keyword arguments of the sampling call: none without the key
    (exactly today's call), else ``compose_main_images=True`` -- the call builds the main conditioning frames from the background
    and object frames under the entry's own placement, and ``edited_first_frame_path`` / ``edited_contorl_frame_path_main`` are
    not loaded (they may be empty).  A variant that overrides either of the two next to the key is an error: there is nothing
    of the variant's to show, its frames are composed under its own ``placement`` / ``transform``."""
    if "compose_main" not in config or not config.compose_main:
        return {}
    if config.compose_main is not True:
        raise ValueError(f"compose_main {config.compose_main!r} is not true or false")
    for k, c in enumerate(variants or ()):
        for key in ("edited_first_frame_path", "edited_contorl_frame_path_main"):
            if getattr(c, key) != getattr(config, key):
                raise ValueError(f"variants[{k}] overrides '{key}' and the entry sets compose_main: the main frames are composed "
                                 "from the sources, under the variant's own placement or transform")
    return {"compose_main_images": True}


def mask_edit_kwargs(config):
    """the entry's optional ``obj_mask_edit`` -> keyword arguments of the sampling call: none without the key
    (exactly today's call), else ``obj_mask_edit`` as plain dicts and lists -- one ``{grow, feather}`` for all objects or one item
    per object, each None or such a dict, in latent pixels.  Checked here, before anything is loaded
    (``normalize_obj_mask_edit``).  The masks are shared by the variants of an entry: not one of ``VARIANT_KEYS``, so a variant
    that sets the key is refused by ``merge_variants``."""
    if "obj_mask_edit" not in config or config.obj_mask_edit is None:
        return {}
    from mvoc_amd.pipeline import normalize_obj_mask_edit

    def plain(v):
        if hasattr(v, "keys"):
            return {str(k): plain(v[k]) for k in v.keys()}
        return [plain(x) for x in v] if hasattr(v, "__iter__") and not isinstance(v, (str, bytes)) else v
    value = plain(config.obj_mask_edit)
    normalize_obj_mask_edit(value, len(config.obj_ddim_latents_path))
    return {"obj_mask_edit": value}


def _write_main_frames(frames, output_dir):
    """what the model was conditioned on, beside the output: ``main_00000.png`` ..."""
    for i, f in enumerate(frames):
        f.save(os.path.join(output_dir, f"main_{i:05d}.png"))


def variant_output_dir(config, k):
    """``<output_dir>/<output_suffix of the variant's merged config>/variant_{k:02d}``"""
    return os.path.join(config.output_dir, output_suffix(config), f"variant_{k:02d}")


def _write_video(video, config, output_dir):
    video = [f.resize(tuple(config.image_size), resample=Image.LANCZOS) for f in video]
    export_to_gif(video, os.path.join(output_dir, "video.gif"))
    for i, f in enumerate(video):
        f.save(os.path.join(output_dir, f"video_{i:05d}.png"))


def main(template_config, configs_list, device, synthetic=False, dedup_sources=False):
    from inverse import build_pipeline
    pipe = build_pipeline(device, synthetic)
    if dedup_sources:
        pipe.dedup_sources = True
    ddim_scheduler = DDIMScheduler.from_pretrained(PRETRAINED_MODEL_PATH, subfolder="scheduler")
    for entry in configs_list:
        if not entry["active"]:
            continue
        config, variants = merge_variants(template_config, entry)
        logger.info(f"config: {OmegaConf.to_yaml(config)}")
        size = tuple(config.image_size)
        first = lambda c: load_image(c.edited_first_frame_path).resize(size, resample=Image.Resampling.LANCZOS)
        compose = compose_main_kwargs(config, variants)  # compose_main: the call builds the main frames, none is loaded
        mask_edit = mask_edit_kwargs(config)  # obj_mask_edit: refused here, before anything is loaded
        main_1st = None if compose else first(config)
        main_frames = None if compose else _frames(config.edited_contorl_frame_path_main, config.n_frames, config.image_size)
        obj_frames = [_frames(p, config.n_frames, config.image_size) for p in config.edited_contorl_frame_path]
        bg_frames = _frames(config.edited_contorl_frame_path_background, config.n_frames, config.image_size)
        ddim_scheduler.set_timesteps(config.n_steps)
        init_pnp(pipe, ddim_scheduler, config, variants)
        pipe.register_modules(scheduler=ddim_scheduler)
        pipe.unet.forward = partial(I2VGenXLUnetExtension.forward, pipe.unet)
        out_type = "pil"
        kw = dict(prompt=config.editing_prompt, main_first_image=main_1st, main_image_list=main_frames,
                  background_first_image=bg_frames[0], background_image_list=bg_frames,
                  objs_first_image=[f[0] for f in obj_frames], objs_image_list=obj_frames, height=config.image_size[1],
                  width=config.image_size[0], num_frames=config.n_frames, num_inference_steps=config.n_steps,
                  guidance_scale=config.cfg, negative_prompt=config.editing_negative_prompt, target_fps=config.target_fps,
                  generator=torch.Generator().manual_seed(config.seed), return_dict=True,
                  ddim_init_latents_t_idx=config.ddim_init_latents_t_idx, ddim_inv_prompt=config.ddim_inv_prompt,
                  obj_mask=config.obj_mask_path, obj_width_height=config.obj_width_height,
                  random_noise_ratio=config.random_noise_ratio, bg_inv_latents_path=config.bg_ddim_latents_path,
                  obj_ddim_latents_path=config.obj_ddim_latents_path,
                  obj_ddim_latents_idx_offset=config.obj_ddim_latents_idx_offset,
                  obj_random_noise_fusion=config.obj_random_noise_fusion, fusion_steps=config.fusion_step,
                  **transform_kwargs(config, variants), **mask_edit)
        if variants is None:
            output_dirs, configs = [os.path.join(config.output_dir, output_suffix(config))], [config]
        else:  # K variants in one loop: per-variant prompt / negative prompt / seed / cfg / main image, everything else shared
            output_dirs, configs = [variant_output_dir(c, k) for k, c in enumerate(variants)], variants
            # (a variant that keeps the entry's main image passes the SAME object: one VAE draw, one vision-tower pass)
            same_1st = lambda c: c.edited_first_frame_path == config.edited_first_frame_path
            same_main = lambda c: c.edited_contorl_frame_path_main == config.edited_contorl_frame_path_main
            kw.update(prompt=[c.editing_prompt for c in variants], negative_prompt=[c.editing_negative_prompt for c in variants],
                      guidance_scale=[c.cfg for c in variants],
                      generator=[torch.Generator().manual_seed(c.seed) for c in variants],
                      main_first_image=[main_1st if same_1st(c) else first(c) for c in variants],
                      main_image_list=[main_frames if same_main(c) else
                                       _frames(c.edited_contorl_frame_path_main, c.n_frames, c.image_size) for c in variants])
        if compose:
            kw.update(main_first_image=None, main_image_list=None, **compose)
        for od in output_dirs:
            os.makedirs(od, exist_ok=True)

        def sample(output_type):
            res = pipe.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection(output_type=output_type, **kw)
            if res.main_frames is not None:
                for k, od in enumerate(output_dirs):
                    _write_main_frames(res.main_frames[k], od)
            return res.frames
        try:
            videos = sample(out_type)
        except NotImplementedError as e:  # no VAE decoder on this path: keep the composed latents
            logger.warning(f"composition decoded to latents only ({e})")
            lat = sample("latent")
            if variants is None:
                torch.save(lat.cpu(), os.path.join(output_dirs[0], "video_latents.pt"))
            else:
                for k, od in enumerate(output_dirs):
                    torch.save(lat[k:k + 1].cpu(), os.path.join(od, "video_latents.pt"))
            continue
        for k, od in enumerate(output_dirs):
            _write_video(videos[k], configs[k], od)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--template_config", type=str, default="configs/group_composite/template.yaml")
    ap.add_argument("--configs_json", type=str, default="configs/group_composite/group_config.json")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--shard", type=str, default=None)
    ap.add_argument("--dedup_sources", action="store_true", help="share one UNet chunk between roles that are the same source")
    args = ap.parse_args()
    template_config = OmegaConf.load(args.template_config)
    logging.basicConfig(level=logging.DEBUG if template_config.debug else logging.INFO,
                        format="%(asctime)s - %(levelname)s - [%(funcName)s] - %(message)s")
    assert Path(args.configs_json).exists()
    with open(args.configs_json) as f:
        configs_list = json.load(f)
    device = pick_device(template_config.device, args.shard)
    torch.set_grad_enabled(False)
    seed_everything(template_config.seed)
    main(template_config, my_entries(configs_list, args.shard), device, args.synthetic, args.dedup_sources)
