#!/usr/bin/env python3
"""End-to-end wall-clock of the boat_surf-shaped job through the drop-in drivers (GPU box): what BASELINE.json's
north_star states its ">= 8x end-to-end" target on (reference call sites: i2vgen-xl/inverse.py:111-227 for the three source
clips, i2vgen-xl/composite.py:72-224 for the composition).

A synthetic data tree of the demo's shape is written to a scratch directory (3 source clips of 16 frames at 512x512 as PNGs,
2 x 16 object masks, an edited first frame), then this repo's `i2vgen-xl/inverse.py` main() runs the three 50-step inversions
and `i2vgen-xl/composite.py` main() the 50-step composition -- seeded synthetic UNet / VAE / CLIP weights of the real
architectures (MVOC_SYNTHETIC_VAE=1, MVOC_SYNTHETIC_CLIP=1), files written exactly as the reference writes them
(ddim_latents_{t}.pt per step, video.gif + video_{i:05d}.png).  Shares of the wall-clock are measured by wrapping the VAE /
CLIP / file entry points with synchronising timers (IO excluded from the metric and reported separately).

Used by `bench.py --workload demo`; prints one JSON object.  usage: python tools/demo_job.py [--frames 16] [--size 512] [--steps 50]

--variants K (opt-in): K prompts and seeds over the job's three sources in ONE composition loop (an entry with `variants`,
DESIGN.md 6i); the JSON line holds the composition-stage time and the mean device time of a step of each kind.
--variant-thresholds a,b,.. gives variant k its own pnp_spatial_attn_t (the variants' `pnp` key); --sequential
also runs the K compositions one by one in the same process and reports the ratio.

--place "dx,dy;dx,dy" (opt-in): the entry's `obj_offset` -- one pair per object, image pixels in multiples of 8;
the composition then places the objects that far from where they sit in their clips.  Reported like --variants (K = 1 unless
--variants is given too).
--transform "scale=3/2,flip=h,offset=64,0;scale=1/2" (opt-in): the entry's `obj_transform` (`rotate=30` turns an object, 6q) -- one item per object:
scale (s or sx,sy; ints or p/q), flip (h, v, hv), offset (dx,dy) and anchor (ax,ay); nearest-neighbour scale and mirror about the
anchor, then the offset.  Reported like --place.
--variant-place "dx,dy;dx,dy|dx,dy;dx,dy|.." (opt-in, needs --variants K): K placements separated by `|`, each in the format of
--place -- the variants' `placement` key: every variant composes the objects at its own offsets over the one set
of source chunks.  With --sequential the K single jobs each take their variant's placement as `obj_offset`.
--variant-transform "scale=3/2,flip=h;scale=1/2||offset=64,0;" (opt-in, needs --variants K): K transforms separated by `|`, each
in the format of --transform -- the variants' `transform` key; an empty item leaves that variant untransformed.
With --sequential the K single jobs each take their variant's transform as `obj_transform`.
--transform-filter bilinear (opt-in, needs --transform): the entry's `obj_transform_filter` -- scaled, mirrored and
turned objects are sampled bilinearly; the result line then names the filter (`obj_transform_filter`).  Not with --variant-transform.
--compose-main (opt-in): the entry's `compose_main` -- the sampling call composes the main conditioning frames from
the background and object frames under the entry's own placement instead of loading the edited first frame and the main control
frames; the result line then holds `compose_main`: the collage stage's own wall-clock, its launches and the bytes of its tap tables.
--mask-edit "grow=1,feather=2;grow=-1" (opt-in): the entry's `obj_mask_edit` -- one item per object, latent pixels:
grow in [-8, 8] (negative shrinks the mask), feather in [0, 8]; an empty item leaves that object's masks as they are.  Parsed and
refused before any work; the result line then holds `obj_mask_edit` and `mask_edit`: the stage's launches and wall-clock.

--shared-source (opt-in): the shape of MVOC's own demo entries, where the background and both objects point at ONE inversion
directory and the same control frames.  One clip is inverted, then the composition runs with source de-duplication off and then
on (composite.py --dedup_sources), in this process; the JSON line holds both composition-stage times (the sampling call without
the VAE decode, graph capture included), the speedup and the rel-L2 between the two final latents -- informational: with
de-duplication the roles also share their VAE draws.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Shares:
    """accumulates synchronised wall-clock per category; nested calls are charged to the innermost category only"""

    def __init__(self):
        self.t = {}
        self.stack = []

    def wrap(self, obj, name, cat):
        fn = getattr(obj, name)
        shares = self

        def timed(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            shares.stack.append(0.0)
            try:
                return fn(*a, **kw)
            finally:
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                inner = shares.stack.pop()
                shares.t[cat] = shares.t.get(cat, 0.0) + dt - inner
                if shares.stack:
                    shares.stack[-1] += dt

        setattr(obj, name, timed)


def write_tree(root, frames, size):
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:size, 0:size]
    for ci, name in enumerate(("bg_clip", "obj1_clip", "obj2_clip")):
        d = os.path.join(root, "demo", name, name)
        os.makedirs(d)
        for i in range(frames):
            img = np.stack([(xx * (1 + ci) + 7 * i) % 256, (yy * 2 + 13 * i) % 256, ((xx + yy) // 2 + 31 * ci) % 256], -1).astype(np.uint8)
            img = (img // 2 + rng.integers(0, 128, img.shape, dtype=np.uint8))
            Image.fromarray(img).save(os.path.join(d, f"{i:05d}.png"))
    ef = os.path.join(root, "demo", "bg_clip", "edited_first_frame")
    os.makedirs(ef)
    Image.fromarray(rng.integers(0, 255, (size, size, 3), dtype=np.uint8)).save(os.path.join(ef, "00000.png"))
    for mi, mname in enumerate(("m1", "m2")):
        md = os.path.join(root, "demo", "bg_clip", mname)
        os.makedirs(md)
        for i in range(frames):
            m = np.zeros((size, size), np.uint8)
            y0, x0 = size // 8 + 4 * i + mi * size // 3, size // 4 + 2 * i
            m[y0:y0 + size // 3, x0:x0 + size // 3] = 255
            Image.fromarray(m).save(os.path.join(md, f"{i:05d}.png"))


def _import_drivers():
    os.environ["MVOC_SYNTHETIC_VAE"] = os.environ["MVOC_SYNTHETIC_CLIP"] = "1"
    sys.path[:0] = [os.path.join(REPO, "i2vgen-xl"), REPO]
    for m in ("utils", "pnp_utils", "inverse", "composite", "pipelines", "pipelines.pipeline_i2vgen_xl"):
        sys.modules.pop(m, None)
    import composite
    import inverse
    import utils as ref_utils
    return composite, inverse, ref_utils


def run(frames=16, size=512, steps=50, keep=False):
    composite, inverse, ref_utils = _import_drivers()
    from mvoc_amd.config import OmegaConf
    from mvoc_amd import latent_cache, pipeline as pl
    root = tempfile.mkdtemp(prefix="mvoc_demo_")
    t_tree = time.perf_counter()
    write_tree(root, frames, size)
    t_tree = time.perf_counter() - t_tree
    dev = torch.device("cuda:0")
    sh = Shares()
    # file IO: frame / mask decoding + resize, latent files, result files
    for mod, names in ((inverse, ("load_video_frames", "export_to_gif")), (composite, ("_frames", "load_image", "export_to_gif")),
                       (ref_utils, ("load_ddim_latents_at_t",))):
        for n in names:
            if hasattr(mod, n):
                sh.wrap(mod, n, "file_io")
    sh.wrap(latent_cache.LatentCache, "flush", "file_io")
    sh.wrap(pl.SyntheticConditioner, "encode_video", "vae")
    sh.wrap(pl.SyntheticConditioner, "decode", "vae")
    sh.wrap(pl.SyntheticConditioner, "image_latents", "vae")
    sh.wrap(pl.SyntheticConditioner, "encode_images", "clip")
    sh.wrap(pl.SyntheticConditioner, "encode_image", "clip")
    sh.wrap(pl.SyntheticConditioner, "encode_prompt", "clip")
    sh.wrap(pl.I2VGenXLPipeline, "synthetic", "model_build")
    sh.wrap(inverse, "build_pipeline", "model_build")

    it = OmegaConf.load(os.path.join(REPO, "tests", "data", "inversion_template.yaml"))
    it.data_dir = root
    it.image_size = [size, size]
    it.n_frames = frames
    it.inverse_config.n_steps = steps
    entries = [{"active": True, "force_recompute_latents": True, "video_name": n, "video_dir": os.path.join(root, "demo", n),
                "recon_config": {"enable_recon": False}} for n in ("bg_clip", "obj1_clip", "obj2_clip")]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inverse.main(it, entries, dev, synthetic=True)
    torch.cuda.synchronize()
    t_inv = time.perf_counter() - t0
    inv_shares, sh.t = dict(sh.t), {}

    ct = OmegaConf.load(os.path.join(REPO, "tests", "data", "composite_template.yaml"))
    ct.data_dir = root
    ct.image_size = [size, size]
    ct.n_frames = frames
    ct.n_steps = steps
    lat = "inversions/i2vgen-xl/{}/ddim_latents"
    centry = {"active": True, "task_name": "demo", "video_name": "bg_clip", "editing_prompt": "windsurf,sailboat,sky,ocean",
              "editing_negative_prompt": "Chaotic, chaotic colors", "edited_video_name": "out",
              "edited_first_frame_path": "demo/bg_clip/edited_first_frame/00000.png",
              "ddim_init_latents_t_idx": 0, "pnp_f_t": 0.1, "pnp_spatial_attn_t": 1.0, "pnp_temp_attn_t": 1.0, "random_noise_ratio": 0.0,
              "fusion_step": [0, 1], "obj_mask_path": ["demo/bg_clip/m1", "demo/bg_clip/m2"], "obj_width_height": [[size, size], [size, size]],
              "obj_ddim_latents_path": [lat.format("obj1_clip"), lat.format("obj2_clip")], "bg_ddim_latents_path": lat.format("bg_clip"),
              "edited_contorl_frame_path_main": "demo/bg_clip/bg_clip", "edited_contorl_frame_path_background": "demo/bg_clip/bg_clip",
              "edited_contorl_frame_path": ["demo/obj1_clip/obj1_clip", "demo/obj2_clip/obj2_clip"]}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    composite.main(ct, [centry], dev, synthetic=True)
    torch.cuda.synchronize()
    t_comp = time.perf_counter() - t0
    comp_shares = dict(sh.t)
    out_root = os.path.join(root, "Results", "demo", "i2vgen-xl", "bg_clip", "out")
    files = sorted(os.listdir(os.path.join(out_root, os.listdir(out_root)[0])))
    n_lat = sum(len(os.listdir(os.path.join(root, lat.format(n)))) for n in ("bg_clip", "obj1_clip", "obj2_clip"))
    if not keep:
        shutil.rmtree(root, ignore_errors=True)

    def stage(total, shares):
        other = sum(shares.values())
        d = {k: round(v, 3) for k, v in sorted(shares.items())}
        d["denoising_loops_and_host"] = round(total - other, 3)
        return d

    build = inv_shares.get("model_build", 0.0) + comp_shares.get("model_build", 0.0)
    return {
        "job": f"3 x {steps}-step DDIM inversion ({frames} frames, {size}x{size}) + 1 x {steps}-step PnP composition (bg + 2 objects), "
               f"drop-in drivers i2vgen-xl/inverse.py + composite.py, seeded synthetic UNet / VAE / CLIP weights",
        "wall_s": round(t_inv + t_comp, 3),
        "wall_s_without_model_build": round(t_inv + t_comp - build, 3),
        "inverse_py_s": round(t_inv, 3), "composite_py_s": round(t_comp, 3),
        "inverse_py_shares_s": stage(t_inv, inv_shares), "composite_py_shares_s": stage(t_comp, comp_shares),
        "files": {"ddim_latents_pt": n_lat, "result_files": files[:3] + (["..."] if len(files) > 3 else []), "n_result_files": len(files)},
        "synthetic_input_tree_s": round(t_tree, 3),
    }


def run_shared_source(frames=16, size=512, steps=50, keep=False):
    """one inverted clip behind the background and both objects: the composition with source de-duplication off, then on"""
    composite, inverse, _ = _import_drivers()
    from mvoc_amd.config import OmegaConf
    from mvoc_amd import pipeline as pl
    root = tempfile.mkdtemp(prefix="mvoc_demo_shared_")
    write_tree(root, frames, size)
    dev = torch.device("cuda:0")
    it = OmegaConf.load(os.path.join(REPO, "tests", "data", "inversion_template.yaml"))
    it.data_dir = root
    it.image_size = [size, size]
    it.n_frames = frames
    it.inverse_config.n_steps = steps
    inverse.main(it, [{"active": True, "force_recompute_latents": True, "video_name": "bg_clip",
                       "video_dir": os.path.join(root, "demo", "bg_clip"), "recon_config": {"enable_recon": False}}], dev, synthetic=True)
    torch.cuda.synchronize()

    # the sampling call's wall-clock without the VAE decode, and the final latents it decodes
    rec = {"sample_s": 0.0, "decode_s": 0.0, "latents": None}
    sample_name = "sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection"
    sample_fn, to_video = getattr(pl.I2VGenXLPipeline, sample_name), pl.I2VGenXLPipeline._to_video

    def timed_sample(self, *a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            return sample_fn(self, *a, **kw)
        finally:
            torch.cuda.synchronize()
            rec["sample_s"] += time.perf_counter() - t0

    def timed_decode(self, latents, output_type):
        rec["latents"] = latents.float().clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            return to_video(self, latents, output_type)
        finally:
            torch.cuda.synchronize()
            rec["decode_s"] += time.perf_counter() - t0

    ct = OmegaConf.load(os.path.join(REPO, "tests", "data", "composite_template.yaml"))
    ct.data_dir = root
    ct.image_size = [size, size]
    ct.n_frames = frames
    ct.n_steps = steps
    lat = "inversions/i2vgen-xl/bg_clip/ddim_latents"
    clip = "demo/bg_clip/bg_clip"
    centry = {"active": True, "task_name": "demo", "video_name": "bg_clip", "editing_prompt": "windsurf,sailboat,sky,ocean",
              "editing_negative_prompt": "Chaotic, chaotic colors", "edited_video_name": "out",
              "edited_first_frame_path": "demo/bg_clip/edited_first_frame/00000.png",
              "ddim_init_latents_t_idx": 0, "pnp_f_t": 0.1, "pnp_spatial_attn_t": 1.0, "pnp_temp_attn_t": 1.0, "random_noise_ratio": 0.0,
              "fusion_step": [0, 1], "obj_mask_path": ["demo/bg_clip/m1", "demo/bg_clip/m2"], "obj_width_height": [[size, size], [size, size]],
              "obj_ddim_latents_path": [lat, lat], "bg_ddim_latents_path": lat,
              "edited_contorl_frame_path_main": clip, "edited_contorl_frame_path_background": clip,
              "edited_contorl_frame_path": [clip, clip]}
    res = {}
    setattr(pl.I2VGenXLPipeline, sample_name, timed_sample)
    pl.I2VGenXLPipeline._to_video = timed_decode
    try:
        for name, dedup in (("off", False), ("on", True)):
            rec.update(sample_s=0.0, decode_s=0.0, latents=None)
            composite.main(ct, [centry], dev, synthetic=True, dedup_sources=dedup)
            res[name] = (rec["sample_s"] - rec["decode_s"], rec["latents"])
    finally:
        setattr(pl.I2VGenXLPipeline, sample_name, sample_fn)
        pl.I2VGenXLPipeline._to_video = to_video
    if not keep:
        shutil.rmtree(root, ignore_errors=True)
    (t_off, l_off), (t_on, l_on) = res["off"], res["on"]
    return {
        "job": f"1 x {steps}-step DDIM inversion ({frames} frames, {size}x{size}) + 2 x {steps}-step PnP composition (bg + 2 objects, "
               f"all three roles on that one source), composite.py without and with --dedup_sources, seeded synthetic weights",
        "composition_s_dedup_off": round(t_off, 3), "composition_s_dedup_on": round(t_on, 3),
        "speedup": round(t_off / t_on, 3),
        "final_latents_rel_l2": float((l_on - l_off).norm() / l_off.norm()),
        "note": "composition stage = the sampling call without the VAE decode (conditioning encoders, graph capture and the "
                "denoising loop); the rel-L2 is informational: with de-duplication the roles also share their VAE draws",
    }


VARIANT_PROMPTS = ("windsurf,sailboat,sky,ocean", "kayak,paddle,lake,mist", "sailboat,sunset,orange sky", "surfer,wave,storm clouds",
                   "rowing boat,river,reeds", "catamaran,lagoon,noon", "canoe,fjord,snow", "raft,rapids,canyon")


def boat_surf_entry(size):
    """the boat_surf-shaped composition entry over the three clips of ``write_tree`` (three distinct sources)"""
    lat = "inversions/i2vgen-xl/{}/ddim_latents"
    return {"active": True, "task_name": "demo", "video_name": "bg_clip", "editing_prompt": VARIANT_PROMPTS[0],
            "editing_negative_prompt": "Chaotic, chaotic colors", "edited_video_name": "out",
            "edited_first_frame_path": "demo/bg_clip/edited_first_frame/00000.png",
            "ddim_init_latents_t_idx": 0, "pnp_f_t": 0.1, "pnp_spatial_attn_t": 1.0, "pnp_temp_attn_t": 1.0, "random_noise_ratio": 0.0,
            "fusion_step": [0, 1], "obj_mask_path": ["demo/bg_clip/m1", "demo/bg_clip/m2"], "obj_width_height": [[size, size], [size, size]],
            "obj_ddim_latents_path": [lat.format("obj1_clip"), lat.format("obj2_clip")], "bg_ddim_latents_path": lat.format("bg_clip"),
            "edited_contorl_frame_path_main": "demo/bg_clip/bg_clip", "edited_contorl_frame_path_background": "demo/bg_clip/bg_clip",
            "edited_contorl_frame_path": ["demo/obj1_clip/obj1_clip", "demo/obj2_clip/obj2_clip"]}


class StageTimer:
    """the sampling call's wall-clock without the VAE decode (as --shared-source reports it), and the device time of every
    composition step by kind (CUDA events around ``composition_step``; the first step of a kind, which warms up and captures
    its graph, is left out of the mean)"""

    NAME = "sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection"

    def __init__(self, pl):
        self.pl, self.sample_s, self.decode_s, self.steps = pl, 0.0, 0.0, []
        self.collage_info = None  # what the sampling call reports about its collage stage (--compose-main)
        self.mask_edit_info = None  # ... and about its mask-edit stage (--mask-edit)
        self._orig = (getattr(pl.I2VGenXLPipeline, self.NAME), pl.I2VGenXLPipeline._to_video, pl.I2VGenXLPipeline.composition_step)

    def __enter__(self):
        sample_fn, to_video, step_fn = self._orig
        timer = self

        def timed_sample(self, *a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                out = sample_fn(self, *a, **kw)
                timer.collage_info = getattr(out, "collage_info", None)
                timer.mask_edit_info = getattr(out, "mask_edit_info", None)
                return out
            finally:
                torch.cuda.synchronize()
                timer.sample_s += time.perf_counter() - t0

        def timed_decode(self, latents, output_type):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                return to_video(self, latents, output_type)
            finally:
                torch.cuda.synchronize()
                timer.decode_s += time.perf_counter() - t0

        def timed_step(self, *a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = step_fn(self, *a, **kw)
            e1.record()
            kind = "conv_out_injection" if self.unet.conv_out.injecting() else "qk"
            proc = self.unet.up_blocks[1].attentions[1].transformer_blocks[0].attn1.processor
            if proc.variant_schedules is not None:  # per-variant thresholds: how many variants still inject spatial Q/K
                k = len(proc.variant_schedules)
                kind += f"_spatial_{bin(proc.injecting_mask(k)).count('1')}of{k}"
            timer.steps.append((kind, e0, e1))
            return out

        P = self.pl.I2VGenXLPipeline
        setattr(P, self.NAME, timed_sample)
        P._to_video, P.composition_step = timed_decode, timed_step
        return self

    def __exit__(self, *exc):
        P = self.pl.I2VGenXLPipeline
        setattr(P, self.NAME, self._orig[0])
        P._to_video, P.composition_step = self._orig[1], self._orig[2]

    def result(self):
        torch.cuda.synchronize()
        by, seen = {}, set()
        for kind, e0, e1 in self.steps:
            if kind not in seen:  # warm-up + capture
                seen.add(kind)
                continue
            by.setdefault(kind, []).append(e0.elapsed_time(e1))
        return {"composition_s": round(self.sample_s - self.decode_s, 3),
                "mean_step_ms": {k: round(sum(v) / len(v), 3) for k, v in sorted(by.items())},
                "steps_timed": {k: len(v) for k, v in sorted(by.items())}}


def parse_place(text):
    """"dx,dy;dx,dy" -> [[dx, dy], [dx, dy]] (one pair per object)"""
    try:
        out = [[int(v) for v in item.split(",")] for item in text.split(";")]
    except ValueError:
        raise SystemExit(f"--place {text!r}: expected integers as dx,dy;dx,dy")
    if any(len(p) != 2 for p in out):
        raise SystemExit(f"--place {text!r}: every object needs dx,dy")
    return out


def parse_transform(text):
    """"scale=3/2,flip=h,offset=64,0;scale=1/2" -> one dict per object (`;` separates the objects): the entry's `obj_transform`.
    scale = s or sx,sy (ints or p/q); flip = h, v or hv; offset = dx,dy; anchor = ax,ay; rotate = degrees (an int, a decimal or
    p/q; counter-clockwise) or one angle per frame; an empty item is the identity"""
    out = []
    for j, item in enumerate(text.split(";")):
        fields = []
        for tok in (t.strip() for t in item.split(",") if t.strip()):
            if "=" in tok:
                k, _, v = tok.partition("=")
                fields.append([k.strip(), [v.strip()]])
            elif fields:
                fields[-1][1].append(tok)
            else:
                raise SystemExit(f"--transform, object {j}: {tok!r} has no key (scale=, flip=, offset=, anchor=, rotate=)")
        d = {}
        for k, vals in fields:
            try:
                if k == "scale" and len(vals) in (1, 2):
                    sc = [int(v) if v.lstrip("-").isdigit() else v for v in vals]
                    d[k] = sc[0] if len(sc) == 1 else sc
                elif k == "flip" and len(vals) == 1:
                    d[k] = vals[0]
                elif k in ("offset", "anchor") and len(vals) == 2:
                    d[k] = [int(v) for v in vals]
                elif k == "rotate" and vals:
                    deg = [int(v) if v.lstrip("+-").isdigit() else v if "/" in v else float(v) for v in vals]
                    d[k] = deg[0] if len(deg) == 1 else deg
                else:
                    raise ValueError
            except ValueError:
                raise SystemExit(f"--transform, object {j}: cannot read {k}={','.join(vals)}")
        out.append(d)
    return out


def parse_mask_edit(text):
    """"grow=1,feather=2;grow=-1" -> one item per object (`;` separates the objects): the entry's `obj_mask_edit`.
    grow = latent pixels in [-8, 8] (negative shrinks), feather = latent pixels in [0, 8]; an empty item is None: not edited"""
    limits = {"grow": (-8, 8), "feather": (0, 8)}
    out = []
    for j, item in enumerate(text.split(";")):
        if not item.strip():
            out.append(None)
            continue
        d = {}
        for tok in (t.strip() for t in item.split(",")):
            k, eq, v = (s.strip() for s in tok.partition("="))
            if not eq or k not in limits:
                raise SystemExit(f"--mask-edit, object {j}: {tok!r} is not grow=N or feather=N")
            if k in d:
                raise SystemExit(f"--mask-edit, object {j}: {k} is given twice")
            try:
                d[k] = int(v)
            except ValueError:
                raise SystemExit(f"--mask-edit, object {j}: cannot read {k}={v} (an integer, latent pixels)")
            lo, hi = limits[k]
            if not lo <= d[k] <= hi:
                raise SystemExit(f"--mask-edit, object {j}: {k}={d[k]} is not in [{lo}, {hi}] latent pixels")
        out.append(d)
    return out


def parse_variant_place(text, variants):
    """"dx,dy;dx,dy|dx,dy;dx,dy" -> K placements, each as ``parse_place`` returns it (`|` separates the variants)"""
    if not variants:
        raise SystemExit("--variant-place needs --variants K (one placement per variant)")
    items = text.split("|")
    if len(items) != variants:
        raise SystemExit(f"--variant-place {text!r}: {len(items)} placements for {variants} variants")
    out = []
    for k, item in enumerate(items):
        try:
            out.append(parse_place(item))
        except SystemExit as e:
            raise SystemExit(f"--variant-place, variant {k}: {e}")
    if len({len(p) for p in out}) != 1:
        raise SystemExit(f"--variant-place {text!r}: every variant needs one dx,dy per object")
    return out


def parse_variant_transform(text, variants):
    """"scale=3/2,flip=h;scale=1/2||offset=64,0;" -> K transforms, each as ``parse_transform`` returns it (`|` separates the
    variants); an empty item is None: that variant is not transformed"""
    if not variants:
        raise SystemExit("--variant-transform needs --variants K (one transform per variant)")
    items = text.split("|")
    if len(items) != variants:
        raise SystemExit(f"--variant-transform {text!r}: {len(items)} transforms for {variants} variants")
    out = []
    for k, item in enumerate(items):
        try:
            out.append(parse_transform(item) if item.strip() else None)
        except SystemExit as e:
            raise SystemExit(f"--variant-transform, variant {k}: {e}")
    if len({len(t) for t in out if t is not None}) > 1:
        raise SystemExit(f"--variant-transform {text!r}: every transformed variant needs one item per object")
    return out


def run_variants(frames=16, size=512, steps=50, keep=False, variants=2, thresholds=None, sequential=False, place=None,
                 variant_place=None, transform=None, variant_transform=None, transform_filter=None, compose_main=False,
                 mask_edit=None):
    """K prompts and seeds over the boat_surf-shaped job (three distinct sources), one composition loop (composite.py `variants`).
    ``thresholds``: K values of pnp_spatial_attn_t, one per variant (the variants' `pnp` key); ``sequential``: after
    the one loop, the same K compositions one by one (single entries with the flat threshold) for the comparison."""
    if transform_filter is not None:  # refused before any work is done
        if transform is None:
            raise SystemExit("--transform-filter needs --transform (the filter samples the entry's transformed objects)")
        if variant_transform is not None and transform_filter == "bilinear":
            raise SystemExit("--transform-filter bilinear does not combine with --variant-transform: one filter samples the objects "
                             "of --transform for all variants")
    if mask_edit is not None and len(mask_edit) != 2:  # (the job has two objects) refused before any work is done
        raise SystemExit(f"--mask-edit: {len(mask_edit)} items for 2 objects (separate the objects with ;)")
    composite, inverse, _ = _import_drivers()
    from mvoc_amd.config import OmegaConf
    from mvoc_amd import pipeline as pl
    if not 1 <= variants <= len(VARIANT_PROMPTS):
        raise SystemExit(f"--variants {variants}: 1 to {len(VARIANT_PROMPTS)}")
    root = tempfile.mkdtemp(prefix="mvoc_demo_variants_")
    write_tree(root, frames, size)
    dev = torch.device("cuda:0")
    it = OmegaConf.load(os.path.join(REPO, "tests", "data", "inversion_template.yaml"))
    it.data_dir = root
    it.image_size = [size, size]
    it.n_frames = frames
    it.inverse_config.n_steps = steps
    entries = [{"active": True, "force_recompute_latents": True, "video_name": n, "video_dir": os.path.join(root, "demo", n),
                "recon_config": {"enable_recon": False}} for n in ("bg_clip", "obj1_clip", "obj2_clip")]
    inverse.main(it, entries, dev, synthetic=True)
    torch.cuda.synchronize()
    ct = OmegaConf.load(os.path.join(REPO, "tests", "data", "composite_template.yaml"))
    ct.data_dir = root
    ct.image_size = [size, size]
    ct.n_frames = frames
    ct.n_steps = steps
    if thresholds is not None and len(thresholds) != variants:
        raise SystemExit(f"--variant-thresholds: {len(thresholds)} values for {variants} variants")
    var = [{"editing_prompt": VARIANT_PROMPTS[k], "seed": 6 + k} for k in range(variants)]
    if thresholds is not None:
        for v, th in zip(var, thresholds):
            v["pnp"] = {"pnp_spatial_attn_t": float(th)}
    if variant_place is not None:  # the variants' own placements
        if len(variant_place) != variants:
            raise SystemExit(f"--variant-place: {len(variant_place)} placements for {variants} variants")
        for v, p in zip(var, variant_place):
            v["placement"] = [list(q) for q in p]
    if variant_transform is not None:  # the variants' own transforms; None: that variant is not transformed
        if len(variant_transform) != variants:
            raise SystemExit(f"--variant-transform: {len(variant_transform)} transforms for {variants} variants")
        for v, t in zip(var, variant_transform):
            if t is not None:
                v["transform"] = [dict(o) for o in t]
    centry = dict(boat_surf_entry(size), variants=var)
    if place is not None:  # shared by the variants: an entry key
        centry["obj_offset"] = [list(p) for p in place]
    if transform is not None:  # scale / mirror / offset per object: an entry key, shared by the variants
        centry["obj_transform"] = [dict(t) for t in transform]
    if transform_filter is not None:  # how the transformed objects are sampled: an entry key next to obj_transform
        centry["obj_transform_filter"] = transform_filter
    if compose_main:  # the main conditioning frames composed by the call: an entry key, the edited frames are not loaded
        centry["compose_main"] = True
    if mask_edit is not None:  # grow / shrink / feather the objects' masks: an entry key, shared by the variants
        centry["obj_mask_edit"] = [None if e is None else dict(e) for e in mask_edit]
    with StageTimer(pl) as timer:
        composite.main(ct, [centry], dev, synthetic=True)
    res = timer.result()
    if compose_main:  # the collage stage alone (frames to the device, tap tables, kernel, frames back as images), as the call reports it
        info = dict(timer.collage_info)
        res["compose_main"] = dict(info, collage_s=round(info.pop("seconds"), 3))
    if mask_edit is not None:  # the mask-edit stage alone, as the call reports it (without the option the line is the one of a run before it existed)
        res["obj_mask_edit"] = [None if e is None else dict(e) for e in mask_edit]
        res["mask_edit"] = {"launches": timer.mask_edit_info["launches"], "mask_edit_s": round(timer.mask_edit_info["seconds"], 6)}
    out_root = os.path.join(root, "Results", "demo", "i2vgen-xl", "bg_clip", "out")
    suffixes = sorted(os.listdir(out_root))  # (per-variant thresholds: every variant under the suffix of its own thresholds)
    files, where = {}, {}
    for sfx in suffixes:
        for d in sorted(os.listdir(os.path.join(out_root, sfx))):
            files[d], where[d] = sorted(os.listdir(os.path.join(out_root, sfx, d))), sfx
    dirs = sorted(files)
    if place is not None:
        res["obj_offset"] = [list(p) for p in place]
    if variant_place is not None:
        res["variant_placement"] = [[list(q) for q in p] for p in variant_place]
    if transform is not None:
        res["obj_transform"] = [dict(t) for t in transform]
        if transform_filter is not None:  # (without the option the result line is the one of a run before the option existed)
            res["obj_transform_filter"] = transform_filter
    if variant_transform is not None:
        res["variant_transform"] = [None if t is None else [dict(o) for o in t] for t in variant_transform]
    if thresholds is not None:
        res["variant_thresholds"] = [float(t) for t in thresholds]
        res["output_suffix_of"] = {d: where[d] for d in dirs}
    if sequential:  # the K compositions one by one: single entries, the flat threshold key, the same prompts and seeds
        seq = []
        for k in range(variants):
            e = dict(boat_surf_entry(size), edited_video_name=f"seq{k}",
                     **{kk: vv for kk, vv in var[k].items() if kk not in ("pnp", "placement", "transform")})
            if place is not None:
                e["obj_offset"] = [list(p) for p in place]
            if variant_place is not None:  # the single job of variant k: its placement as the entry's
                e["obj_offset"] = [list(q) for q in variant_place[k]]
            if transform is not None:
                e["obj_transform"] = [dict(t) for t in transform]
                if transform_filter is not None:
                    e["obj_transform_filter"] = transform_filter
            if variant_transform is not None and variant_transform[k] is not None:  # the single job of variant k: its transform as the entry's
                e["obj_transform"] = [dict(o) for o in variant_transform[k]]
            if thresholds is not None:
                e["pnp_spatial_attn_t"] = float(thresholds[k])
            if compose_main:
                e["compose_main"] = True
            if mask_edit is not None:
                e["obj_mask_edit"] = [None if m is None else dict(m) for m in mask_edit]
            with StageTimer(pl) as t1:
                composite.main(ct, [e], dev, synthetic=True)
            seq.append(t1.result())
        res["sequential"] = seq
        res["sequential_composition_s"] = round(sum(r["composition_s"] for r in seq), 3)
        res["ratio_vs_sequential"] = round(res["composition_s"] / res["sequential_composition_s"], 3)
    if not keep:
        shutil.rmtree(root, ignore_errors=True)
    n_obj = 2
    return dict(res, job=f"3 x {steps}-step DDIM inversion ({frames} frames, {size}x{size}) + ONE {steps}-step PnP composition loop of "
                         f"{variants} variants (prompts, seeds) over bg + 2 objects, composite.py `variants`, seeded synthetic weights",
                variants=variants, unet_batch={"qk": n_obj + 1 + 2 * variants, "conv_out_injection": n_obj + 1},
                chunk_count_expectation_vs_sequential={"qk": round((n_obj + 1 + 2 * variants) / (variants * (n_obj + 3)), 3),
                                                       "conv_out_injection": round(1 / variants, 3)},
                output_dirs=dirs, n_result_files={d: len(f) for d, f in files.items()}, result_files=files[dirs[0]][:3],
                note="composition stage = the sampling call without the VAE decode (conditioning encoders, graph capture and the "
                     "denoising loop); mean_step_ms = device time of composition_step by kind, the capturing step of each kind left out")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--shared-source", action="store_true",
                    help="one source behind every role: the composition without and with source de-duplication")
    ap.add_argument("--variants", type=int, default=0, metavar="K",
                    help="K prompts and seeds over the job's three sources in one composition loop (composite.py `variants`)")
    ap.add_argument("--variant-thresholds", type=str, default=None, metavar="a,b,..",
                    help="with --variants K: K values of pnp_spatial_attn_t, one per variant (the variants' `pnp` key)")
    ap.add_argument("--sequential", action="store_true",
                    help="with --variants K: also run the K compositions one by one and report the ratio")
    ap.add_argument("--place", type=str, default=None, metavar="dx,dy;dx,dy",
                    help="place the objects at composition time: one dx,dy per object, image pixels in multiples of 8 (`obj_offset`)")
    ap.add_argument("--variant-place", type=str, default=None, metavar="dx,dy;dx,dy|..",
                    help="with --variants K: K placements separated by |, each in the format of --place (the variants' `placement` key)")
    ap.add_argument("--transform", type=str, default=None, metavar="scale=p/q,flip=h,offset=dx,dy,rotate=deg;..",
                    help="scale / mirror / turn / place the objects at composition time: one item per object separated by ; (`obj_transform`)")
    ap.add_argument("--variant-transform", type=str, default=None, metavar="scale=p/q,flip=h;..|..",
                    help="with --variants K: K transforms separated by |, each in the format of --transform (the variants' "
                         "`transform` key); an empty item leaves that variant untransformed")
    ap.add_argument("--transform-filter", type=str, default=None, choices=("nearest", "bilinear"),
                    help="with --transform: how the transformed objects are sampled (`obj_transform_filter`; default nearest)")
    ap.add_argument("--compose-main", action="store_true",
                    help="compose the main conditioning frames from the sources under the entry's placement (`compose_main`)")
    ap.add_argument("--mask-edit", type=str, default=None, metavar="grow=N,feather=N;..",
                    help="grow (negative: shrink) and feather the objects' masks at composition time, latent pixels: one item per "
                         "object separated by ; (`obj_mask_edit`); an empty item leaves that object's masks as they are")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    mask_edit = None if a.mask_edit is None else parse_mask_edit(a.mask_edit)  # parsed and refused before any work
    if a.mask_edit and not a.variants:  # the option alone reaches run_variants as well (K = 1)
        a.variants = 1
    if a.compose_main and not a.variants:  # the option alone reaches run_variants as well (K = 1)
        a.variants = 1
    if a.variants or a.place or a.variant_place or a.transform or a.variant_transform or a.transform_filter:
        th = None if a.variant_thresholds is None else [float(x) for x in a.variant_thresholds.split(",")]
        place = None if a.place is None else parse_place(a.place)
        vplace = None if a.variant_place is None else parse_variant_place(a.variant_place, a.variants)
        transform = None if a.transform is None else parse_transform(a.transform)
        vtransform = None if a.variant_transform is None else parse_variant_transform(a.variant_transform, a.variants)
        print(json.dumps(run_variants(a.frames, a.size, a.steps, a.keep, a.variants or 1, th, a.sequential, place, vplace, transform,
                                      vtransform, a.transform_filter, a.compose_main, mask_edit)), flush=True)
    else:
        fn = run_shared_source if a.shared_source else run
        print(json.dumps(fn(a.frames, a.size, a.steps, a.keep)), flush=True)
