"""MVOC's three denoising loops on the MI355X engine, behind the reference pipeline's method names.

Reference (``i2vgen-xl/pipelines/pipeline_i2vgen_xl.py``):
  * ``I2VGenXLPipeline.invert``                       ``:1752-2018``  (loop body ``:1940-2000``)
  * ``I2VGenXLPipeline.__call__``                     ``:980-1216``   (loop body ``:1167-1202``)
  * ``I2VGenXLPipeline.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection``
                                                      ``:1220-1748``  (loop body ``:1636-1734``)

Scope: the per-step work -- UNet forward, PnP injections, latent fusion, CFG, DDIM update,
latent cache hand-off.  The once-per-clip encoders either side of the loops (CLIP text/vision, VAE) are "next"
rows: they enter through a ``conditioner`` object (``encode_prompt / encode_image / image_latents /
encode_video / decode``); ``SyntheticConditioner`` supplies tensors of the right shapes where no checkpoint
exists.  Everything inside a loop iteration runs on the GPU through libmvoc_hip; with ``use_graphs`` the whole
iteration is one captured hipGraph replay (~2000 kernel launches otherwise).
"""
import hashlib
import logging
import math
import os
import weakref
from copy import deepcopy
from fractions import Fraction

import torch

from . import ops
from .latent_cache import LatentCache
from .pnp_utils import register_time_all
from .schedulers import DDIMScheduler
from .unet import PLACEMENT_MODES, frame_shard_refusal

logger = logging.getLogger(__name__)
H16 = torch.float16


class PipelineOutput:
    def __init__(self, frames=None, inverted_latents=None, main_frames=None, collage_info=None, mask_edit_info=None):
        self.frames = frames
        self.inverted_latents = inverted_latents
        self.main_frames = main_frames  # compose_main_images: per variant the composed conditioning frames
        self.collage_info = collage_info  # ... and what composing them took (``compose_main_frames``)
        self.mask_edit_info = mask_edit_info  # obj_mask_edit: launches and seconds of the mask-edit stage


class SyntheticConditioner:
    """Deterministic stand-in for CLIP text/vision + VAE (SURVEY section 8d synthetic inputs): embeddings are
    N(0,1) draws seeded by a hash of the prompt / image bytes; image latents are frame 0 = 0.18215*N(0,1)
    followed by the frame-position ramp k/(F-1) exactly as ``prepare_image_latents`` (``:860-890``) builds it."""

    cross_attention_dim = 1024
    vae_scale_factor = 8

    def __init__(self, device, cross_attention_dim=1024, vae=None, clip=None):
        """``vae``: a ``mvoc_amd.vae.VaeCodec`` -- video / image latents and decoding then go through the HIP VAE
         instead of the seeded stand-ins; ``clip``: a ``mvoc_amd.clip.ClipCodec`` -- image / prompt embeddings
        then come from the HIP CLIP towers"""
        self.device = torch.device(device)
        self.cross_attention_dim = cross_attention_dim
        self.vae = vae
        self.clip = clip

    def _gen(self, *keys):
        h = hashlib.sha256("|".join(str(k) for k in keys).encode()).digest()
        return torch.Generator().manual_seed(int.from_bytes(h[:7], "little"))

    @staticmethod
    def _image_key(image):
        if image is None:
            return "none"
        if hasattr(image, "tobytes"):
            return hashlib.sha256(image.tobytes()).hexdigest()
        return str(image)

    def encode_prompt(self, prompt, negative_prompt=None):
        c = self.clip
        if c is not None and c.text is not None and (c.tokenizer is not None or torch.is_tensor(prompt)):
            return c.encode_prompt(prompt, negative_prompt)
        pe = torch.randn(1, 77, self.cross_attention_dim, generator=self._gen("p", prompt)).to(self.device, H16)
        ne = torch.randn(1, 77, self.cross_attention_dim, generator=self._gen("p", negative_prompt or "")).to(self.device, H16)
        return pe, ne

    def encode_image(self, image):
        return self.encode_images([image])

    def encode_images(self, images):
        """-> [n, 1, 1024]: every image of the list in one batched pass of the vision tower (the reference loops
        ``_encode_image`` per frame, ``pipeline_i2vgen_xl.py:1417-1427, 1501-1541``)"""
        if self.clip is not None and self.clip.vision is not None and all(hasattr(im, "convert") for im in images):
            return self.clip.encode_images(images)
        return torch.cat([torch.randn(1, 1, self.cross_attention_dim, generator=self._gen("i", self._image_key(im))).to(self.device, H16)
                          for im in images])

    def image_latents(self, image, num_frames, height, width):
        if self.vae is not None and hasattr(image, "convert"):
            return self.vae.image_latents(image, num_frames, height, width)
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        first = 0.18215 * torch.randn(1, 4, 1, h, w, generator=self._gen("l", self._image_key(image), h, w))
        if num_frames > 1:
            ramp = torch.cat([torch.full((1, 4, 1, h, w), (k + 1) / (num_frames - 1)) for k in range(num_frames - 1)], 2)
            first = torch.cat([first, ramp], 2)
        return first.to(self.device, H16)

    def encode_video(self, frames, height, width):
        if self.vae is not None and all(hasattr(f, "convert") for f in frames):
            return self.vae.encode_video(frames, height, width)
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        lat = [0.18215 * 4 * torch.randn(4, h, w, generator=self._gen("v", self._image_key(f), h, w)) for f in frames]
        return torch.stack(lat, 1)[None].to(self.device, H16)

    def decode(self, latents):
        """-> video [B,3,F,H,W] float32 in about [-1,1] (``decode_latents``, ``pipeline_i2vgen_xl.py:771-791``)"""
        if self.vae is None:
            raise NotImplementedError("this conditioner has no VAE (SyntheticConditioner(vae=VaeCodec(...))): pass output_type='latent'")
        return self.vae.decode(latents)


SOURCE_COND_KEYS = ("encoder_hidden_states", "image_embeddings", "image_latents_first", "image_latents", "fps")


def source_classes(cond, n_obj):
    """Static partition of a composition batch's source roles (0 = background, j = object j) for source de-duplication:
    role r joins the class of the first earlier role whose conditioning rows (``SOURCE_COND_KEYS``) equal its own bit for bit,
    else starts its own.  -> tuple of class ids (the class's first role), one per role."""
    classes = []
    for r in range(n_obj + 1):
        c = r
        for q in range(r):
            if classes[q] == q and all(torch.equal(cond[k][q], cond[k][r]) for k in SOURCE_COND_KEYS):
                c = q
                break
        classes.append(c)
    return tuple(classes)


def plan_source_map(classes, latents):
    """Per-step source map: roles of one class (``source_classes``) share a UNet chunk when they were handed the SAME latents
    tensor object (``LatentCache.get`` returns one tensor per directory and t).  ``latents``: one object per role, background
    first.  -> None when every role keeps its own chunk (the positional batch), else (nsrc, obj_chunks): chunks numbered in
    the order of their first role, so the background is always chunk 0 and object j reads chunk obj_chunks[j]."""
    if classes is None:
        return None
    if len(classes) != len(latents):
        raise ValueError(f"plan_source_map: {len(classes)} roles classified, {len(latents)} latents")
    firsts, chunk_of = [], []  # first role of each chunk
    for r, lat in enumerate(latents):
        for i, q in enumerate(firsts):
            if classes[q] == classes[r] and latents[q] is lat:
                chunk_of.append(i)
                break
        else:
            chunk_of.append(len(firsts))
            firsts.append(r)
    if len(firsts) == len(latents):
        return None
    return len(firsts), tuple(chunk_of[1:])


def source_rows(smap, n_obj):
    """roles whose latents / conditioning rows fill the source chunks of ``smap`` (the first role of each chunk)"""
    if smap is None:
        return list(range(n_obj + 1))
    nsrc, chunks = smap
    return [0] + [1 + chunks.index(c) for c in range(1, nsrc)]


MAX_VARIANTS = 8


def variant_layout(n_obj, nvar=1, do_cfg=True, smap=None):
    """Chunk indices of a composition batch of ``nvar`` = K variants over one set of sources:
    [s_0..s_{nsrc-1}, u_1..u_K, c_1..c_K] with guidance, [s_0..s_{nsrc-1}, c_1..c_K] without.  ``smap``: the source map of
    ``plan_source_map`` (None: every role its own chunk).  Blocks rather than interleaved pairs: the paired attention serves
    the K pairs in one launch (the c block sits at a constant offset behind the u block) and the u / c noise predictions are
    each contiguous for the DDIM update.  K = 1 is the positional layout.
    -> dict(nsrc, nb, src = chunk of every source role (background first), obj_chunks, u = [K] or None, c = [K], ndst)"""
    if not 1 <= int(nvar) <= MAX_VARIANTS:
        raise ValueError(f"variants: {nvar} not in [1, {MAX_VARIANTS}]")
    if not 1 <= n_obj <= 4:
        raise ValueError(f"variants: {n_obj} objects not in [1, 4]")
    if smap is None:
        nsrc, chunks = n_obj + 1, tuple(range(1, n_obj + 1))
    else:
        nsrc, chunks = int(smap[0]), tuple(int(c) for c in smap[1])
        if len(chunks) != n_obj or not 1 <= nsrc <= n_obj + 1 or any(not 0 <= c < nsrc for c in chunks):
            raise ValueError(f"variants: source map {smap} does not fit {n_obj} objects")
    ndst = 2 if do_cfg else 1
    u = [nsrc + k for k in range(nvar)] if do_cfg else None
    c = [nsrc + (ndst - 1) * nvar + k for k in range(nvar)]
    return dict(nsrc=nsrc, nb=nsrc + ndst * nvar, src=[0] + list(chunks), obj_chunks=chunks, u=u, c=c, ndst=ndst)


def normalize_obj_offsets(obj_offsets, n_obj, num_frames, factor=8):
    """``obj_offsets`` of the sampling call -> the placement the engine takes, or None.  One entry per object:
    ``(dx, dy)`` for every frame, or a list of ``num_frames`` pairs (a path), in image pixels; each a multiple of the VAE
    factor (the latent grid is 1 / ``factor`` of the image).  -> None when there is nothing to move (no argument, or all
    zeros: the call is then exactly a call without it), else a hashable tuple, per object a tuple of ``num_frames`` pairs
    ``(dy, dx)`` on the latent grid.  Anything else is a ValueError that names the object."""
    if obj_offsets is None:
        return None
    objs = list(obj_offsets)
    if len(objs) != n_obj:
        raise ValueError(f"obj_offsets: {len(objs)} entries for {n_obj} objects (one per object)")
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    out = []
    for j, entry in enumerate(objs):
        entry = list(entry) if isinstance(entry, (list, tuple)) else entry
        if isinstance(entry, list) and len(entry) == 2 and all(is_int(v) for v in entry):
            pairs = [entry] * num_frames
        elif isinstance(entry, list) and all(isinstance(q, (list, tuple)) and len(q) == 2 and all(is_int(v) for v in q) for q in entry):
            if len(entry) != num_frames:
                raise ValueError(f"obj_offsets: object {j} has {len(entry)} per-frame offsets, the clip {num_frames} frames")
            pairs = entry
        else:
            raise ValueError(f"obj_offsets: object {j} needs (dx, dy) or {num_frames} (dx, dy) pairs of integers, got {entry!r}")
        for f, (dx, dy) in enumerate(pairs):
            if dx % factor or dy % factor:
                raise ValueError(f"obj_offsets: object {j}, frame {f}: ({dx}, {dy}) is not a multiple of {factor} image pixels "
                                 "(placements are integer translations on the latent grid)")
        out.append(tuple((int(dy) // factor, int(dx) // factor) for dx, dy in pairs))
    if all(v == 0 for obj in out for pair in obj for v in pair):
        return None
    return tuple(out)


MASK_EDIT_KEYS = {"grow": (-ops.MASK_EDIT_MAX, ops.MASK_EDIT_MAX), "feather": (0, ops.MASK_EDIT_MAX)}  # key -> the range it takes


def normalize_obj_mask_edit(value, n_obj):
    """``obj_mask_edit`` of the sampling call -> None or a hashable tuple, per object ``(grow, feather)`` in latent
    pixels: ``grow`` an int in [-8, 8] (negative: shrink), ``feather`` an int in [0, 8].  ``value``: None, one dict for all
    objects, or a list of ``n_obj`` items each None or a dict with the optional keys ``grow`` and ``feather``.  Nothing to edit
    (no argument, or all zeros: the call is then exactly a call without it) -> None.  Anything else is a ValueError that names
    the object."""
    if value is None:
        return None
    if hasattr(value, "keys"):
        items = [value] * n_obj
    elif isinstance(value, (list, tuple)):
        items = list(value)
        if len(items) != n_obj:
            raise ValueError(f"obj_mask_edit: {len(items)} entries for {n_obj} objects (one per object, or one dict for all)")
    else:
        raise ValueError(f"obj_mask_edit: needs None, one dict for all objects or a list of {n_obj} items, got {type(value).__name__}")
    out = []
    for j, item in enumerate(items):
        if item is None:
            out.append((0, 0))
            continue
        if not hasattr(item, "keys"):
            raise ValueError(f"obj_mask_edit: object {j} needs None or a dict with the keys grow, feather, got {item!r}")
        edit = {"grow": 0, "feather": 0}
        for key in item.keys():
            if key not in MASK_EDIT_KEYS:
                raise ValueError(f"obj_mask_edit: object {j} has the unknown key {key!r} (the keys are grow, feather)")
            v, (lo, hi) = item[key], MASK_EDIT_KEYS[key]
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"obj_mask_edit: object {j}: {key} = {v!r} is not an int (latent pixels)")
            if not lo <= v <= hi:
                raise ValueError(f"obj_mask_edit: object {j}: {key} = {v} is not in [{lo}, {hi}] latent pixels")
            edit[key] = int(v)
        out.append((edit["grow"], edit["feather"]))
    if all(v == 0 for e in out for v in e):
        return None
    return tuple(out)


def mask_edit_launches(edit, hard=True):
    """the kernel launches of ``edit`` (``normalize_obj_mask_edit``) at one site: per object the passes of the soft planes, and with
    ``hard`` those of the hard mask (the grow passes alone)"""
    return sum(len(ops.edit_passes(g, f)) + (len(ops.edit_passes(g, 0)) if hard else 0) for g, f in edit or ())


def edit_obj_masks(masks, edit):
    """the masks of the sampling call, per object (soft fp16, hard bool) in the object's SOURCE coordinates and on the device,
    under ``edit`` (``normalize_obj_mask_edit``; None: ``masks`` as they are) -> per object (soft, hard) in the shapes and dtypes
    they came in.  The soft mask is grown or shrunk and then feathered; the hard mask is taken as fp16 0 / 1, takes
    the grow passes alone and comes back as bool; an object at (0, 0) keeps its very tensors."""
    if edit is None:
        return masks
    if len(edit) != len(masks):
        raise ValueError(f"edit_obj_masks: {len(edit)} edits for {len(masks)} objects")
    out = []
    for (soft, hard), (grow, feather) in zip(masks, edit):
        if grow == 0 and feather == 0:
            out.append((soft, hard))
            continue
        if soft.dtype != H16 or hard.dtype != torch.bool or soft.dim() < 2 or hard.shape != soft.shape:
            raise ValueError(f"edit_obj_masks: an object's masks are (fp16, bool) [..., h, w] of one shape, got {soft.dtype} "
                             f"{tuple(soft.shape)} and {hard.dtype} {tuple(hard.shape)}")
        new_soft = ops.edit_planes(soft.contiguous(), grow, feather)
        new_hard = hard if grow == 0 else ops.edit_planes(hard.to(H16).contiguous(), grow, 0) != 0
        out.append((new_soft, new_hard))
    return out


def resolve_variant_obj_offsets(variant_obj_offsets, nvar, n_obj, num_frames, factor=8):
    """``variant_obj_offsets`` of the sampling call: K = ``nvar`` items, each None or a value ``obj_offsets``
    accepts, normalised per variant by ``normalize_obj_offsets`` -> (shared placement or None, per-variant placements or None):
      (None, None)     nothing to move (no argument, or every item None / all zeros): exactly a call without the argument
      (placement, None) every variant resolves to the same placement: exactly the shared ``obj_offsets`` call
      (None, (p_0..p_{K-1})) placements differ: per-variant placement; a variant that is not placed carries all-zero offsets
    Anything else is a ValueError that names the variant (and, from ``normalize_obj_offsets``, the object)."""
    if variant_obj_offsets is None:
        return None, None
    if not isinstance(variant_obj_offsets, (list, tuple)):
        raise ValueError(f"variant_obj_offsets: needs a list of {nvar} items (one per variant), got {variant_obj_offsets!r}")
    items = list(variant_obj_offsets)
    if len(items) != nvar:
        raise ValueError(f"variant_obj_offsets: {len(items)} entries for {nvar} variants (one per variant)")
    pls = []
    for k, item in enumerate(items):
        try:
            pls.append(normalize_obj_offsets(item, n_obj, num_frames, factor))
        except ValueError as e:
            raise ValueError(f"variant_obj_offsets: variant {k}: {e}") from None
    if all(p is None for p in pls):
        return None, None
    if all(p == pls[0] for p in pls):
        return pls[0], None
    zero = tuple(((0, 0),) * num_frames for _ in range(n_obj))
    return None, tuple(zero if p is None else p for p in pls)


MAX_SCALE_TERM = 64  # numerator and denominator of a reduced scale factor (obj_transforms)


def _scale_fraction(v, what):
    """one scale value of ``obj_transforms`` -> (p, q) reduced: an int, a "p/q" (or "p") string, or a float read by its
    shortest decimal form (``Fraction(str(v))``: 1.5 -> 3/2, never the binary expansion)"""
    try:
        if isinstance(v, bool):
            raise ValueError
        if isinstance(v, int):
            fr = Fraction(v)
        elif isinstance(v, str):
            num, _, den = v.partition("/")
            fr = Fraction(int(num.strip()), int(den.strip()) if den else 1)
        elif isinstance(v, float):
            fr = Fraction(str(v))
        else:
            raise ValueError
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"{what}: scale {v!r} is not an int, a 'p/q' string or a float") from None
    p, q = fr.numerator, fr.denominator
    if not (1 <= p <= MAX_SCALE_TERM and 1 <= q <= MAX_SCALE_TERM):
        raise ValueError(f"{what}: scale {v!r} = {p}/{q} needs 1 <= p, q <= {MAX_SCALE_TERM} after reduction")
    return p, q


def normalize_obj_transforms(obj_transforms, n_obj, num_frames, lat_h, lat_w, factor=8):
    """``obj_transforms`` of the sampling call -> (placement or None, transform or None).  One dict per object
    with the optional keys ``offset`` (what an ``obj_offsets`` item accepts), ``scale`` (s or [sx, sy]; each an int, a "p/q"
    string or a float), ``flip`` (None, "h", "v", "hv": "h" mirrors left-right) and ``anchor`` ([ax, ay], image pixels in
    multiples of ``factor`` / 2; default the frame centre) -- the object is scaled and mirrored about the anchor, then moved.
      (None, None)       no argument, or every object at identity: exactly a call without the argument
      (placement, None)  every object at scale 1 without a flip: the placement ``normalize_obj_offsets`` returns
      (None, transform)  else: per object (py, qy, px, qx, flip_y, flip_x, ay2, ax2, ((dy, dx) per frame)) on the
                         ``lat_h`` x ``lat_w`` latent grid (ay2 / ax2 = twice the anchor), hashable
    Anything else is a ValueError that names the object."""
    if obj_transforms is None:
        return None, None
    return _downgrade_obj_transforms(_full_obj_transforms(obj_transforms, n_obj, num_frames, lat_h, lat_w, factor), num_frames)


def _downgrade_obj_transforms(out, num_frames):
    """full transform tuples -> (placement or None, transform or None) as ``normalize_obj_transforms`` documents"""
    zero = ((0, 0),) * num_frames
    plain = [t[0] == t[1] and t[2] == t[3] and not t[4] and not t[5] for t in out]
    if all(plain):
        if all(t[8] == zero for t in out):
            return None, None
        return tuple(t[8] for t in out), None
    return None, tuple(out)


def _full_obj_transforms(obj_transforms, n_obj, num_frames, lat_h, lat_w, factor=8, rotations=None):
    """the items of ``obj_transforms`` checked and normalised -> per object the full tuple (py, qy, px, qx, flip_y, flip_x, ay2,
    ax2, ((dy, dx) per frame)), identity and translation-only objects included.  ``rotations``: a list -- the key ``rotate`` is
    taken as well (``resolve_obj_transforms``) and per object its per-frame (C, S) of ``_rotation`` is appended to the list"""
    if not isinstance(obj_transforms, (list, tuple)):
        raise ValueError(f"obj_transforms: needs a list of {n_obj} dicts (one per object), got {obj_transforms!r}")
    items = list(obj_transforms)
    if len(items) != n_obj:
        raise ValueError(f"obj_transforms: {len(items)} entries for {n_obj} objects (one per object)")
    zero = ((0, 0),) * num_frames
    out = []
    for j, item in enumerate(items):
        what = f"obj_transforms: object {j}"
        item = {} if item is None else item
        if not hasattr(item, "keys"):
            raise ValueError(f"{what} needs a dict with any of offset, scale, flip, anchor, got {item!r}")
        item = {k: item[k] for k in item.keys()}
        unknown = sorted(set(item) - {"offset", "scale", "flip", "anchor"} - ({"rotate"} if rotations is not None else set()))
        if unknown:
            raise ValueError(f"{what} has the unknown key(s) {', '.join(map(repr, unknown))}; the keys are offset, scale, flip, anchor")
        offs = zero
        if item.get("offset") is not None:
            try:
                offs = normalize_obj_offsets([item["offset"]], 1, num_frames, factor)
            except ValueError as e:
                raise ValueError(f"{what}: offset: {str(e).replace('obj_offsets: object 0', '').strip(' ,:')}") from None
            offs = zero if offs is None else offs[0]
        scale = item.get("scale")
        scale = 1 if scale is None else scale
        if isinstance(scale, (list, tuple)):
            if len(scale) != 2:
                raise ValueError(f"{what}: scale {scale!r} needs one value or [sx, sy]")
            sx, sy = scale
        else:
            sx = sy = scale
        (px, qx), (py, qy) = _scale_fraction(sx, what), _scale_fraction(sy, what)
        flip = item.get("flip")
        if flip not in (None, "h", "v", "hv"):
            raise ValueError(f"{what}: flip {flip!r} is not one of None, 'h', 'v', 'hv'")
        flip_x, flip_y = flip in ("h", "hv"), flip in ("v", "hv")
        anchor = item.get("anchor")
        if anchor is None:
            ax2, ay2 = int(lat_w), int(lat_h)
        else:
            anchor = list(anchor) if isinstance(anchor, (list, tuple)) else anchor
            if not (isinstance(anchor, list) and len(anchor) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in anchor)):
                raise ValueError(f"{what}: anchor {anchor!r} needs [ax, ay] as integers (image pixels)")
            if any((2 * v) % factor for v in anchor):
                raise ValueError(f"{what}: anchor {tuple(anchor)} is not a multiple of {factor // 2} image pixels "
                                 "(anchors sit on half latent pixels)")
            ax2, ay2 = 2 * anchor[0] // factor, 2 * anchor[1] // factor
        out.append((py, qy, px, qx, flip_y, flip_x, ay2, ax2, tuple(offs)))
        if rotations is not None:
            rot = item.get("rotate")
            rot = 0 if rot is None else rot
            if isinstance(rot, (list, tuple)):
                if len(rot) != num_frames:
                    raise ValueError(f"{what}: rotate has {len(rot)} per-frame angles, the clip {num_frames} frames")
                rotations.append(tuple(_rotation(v, what) for v in rot))
            else:
                rotations.append((_rotation(rot, what),) * num_frames)
    return tuple(out)


WARP_DEN = 65536  # D: cos and sin of ``rotate`` are rounded to multiples of 1 / D


def _rotation(v, what):
    """one angle of ``rotate`` (degrees: an int, a float read by its shortest decimal form or a "p/q" string; positive = counter-
    clockwise on screen) -> (C, S) = (round(cos * D), round(sin * D)), D = ``WARP_DEN``.  Multiples of 90 degrees, taken after
    the angle mod 360, give the exact (+-D, 0) / (0, +-D)"""
    try:
        if isinstance(v, bool):
            raise ValueError
        if isinstance(v, int):
            fr = Fraction(v)
        elif isinstance(v, str):
            num, _, den = v.partition("/")
            fr = Fraction(int(num.strip()), int(den.strip()) if den else 1)
        elif isinstance(v, float):
            fr = Fraction(str(v))
        else:
            raise ValueError
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"{what}: rotate {v!r} is not an int, a float or a 'p/q' string of degrees") from None
    fr = fr % 360
    if fr % 90 == 0:
        return ((WARP_DEN, 0), (0, WARP_DEN), (-WARP_DEN, 0), (0, -WARP_DEN))[int(fr // 90)]
    rad = math.radians(float(fr))
    return round(math.cos(rad) * WARP_DEN), round(math.sin(rad) * WARP_DEN)


def _warp_of(full, rotation):
    """one object's full transform tuple and per-frame (C, S) -> its entry of the engine's ``warp``: (ay2, ax2, ((myy, myx, mxy,
    mxx, den, dy, dx) per frame)).  The object is scaled and mirrored about its anchor, then rotated about it, then moved, so the
    INVERSE matrix is diag(sy * qy / py, sx * qx / px) . [[C, S], [-S, C]] / D in (y, x) order, over the common denominator
    py * px * D and reduced by the gcd"""
    py, qy, px, qx, flip_y, flip_x, ay2, ax2, offs = full
    gy, gx = (-1 if flip_y else 1) * qy * px, (-1 if flip_x else 1) * qx * py
    frames = []
    for (c, s), (dy, dx) in zip(rotation, offs):
        m = (gy * c, gy * s, -gx * s, gx * c, py * px * WARP_DEN)
        g = math.gcd(*m)
        frames.append(tuple(v // g for v in m) + (dy, dx))
    return ay2, ax2, tuple(frames)


TRANSFORM_FILTERS = (None, "nearest", "bilinear")  # obj_transform_filter: None and "nearest" are the same call


def _transform_filter(value):
    """``obj_transform_filter`` -> None (nearest: today's call) or "bilinear"; anything else is a ValueError"""
    if value not in TRANSFORM_FILTERS:
        raise ValueError(f"obj_transform_filter {value!r} is not one of None, 'nearest', 'bilinear'")
    return None if value in (None, "nearest") else value


def resolve_obj_transforms(obj_transforms, n_obj, num_frames, lat_h, lat_w, factor=8, interp="nearest"):
    """``obj_transforms`` of the sampling call with the key ``rotate``: degrees, or ``num_frames`` of them (an
    object may turn along its path) -> (placement, transform, warp), at most one of them not None:
      every frame's matrix diagonal   what ``normalize_obj_transforms`` returns for the call without ``rotate``, exactly -- 0 and
                                      360 degrees drop out, 180 degrees toggles both flips (the ``flip: "hv"`` call)
      else                            warp: per object (ay2, ax2, ((myy, myx, mxy, mxx, den, dy, dx) per frame)), hashable; an
                                      object that does not turn carries its diagonal matrix
    ``interp`` = "bilinear" (``obj_transform_filter``): identity still resolves to no mode and translation only to
    the placement (an integer shift of the latent grid is exact under either filter); EVERYTHING else is a warp for all objects,
    axis-aligned scale and mirror included -- the filter is a property of the warp mode.
    Anything else is a ValueError that names the object."""
    if interp not in ("nearest", "bilinear"):
        raise ValueError(f"resolve_obj_transforms: interp {interp!r} is not 'nearest' or 'bilinear'")
    if obj_transforms is None:
        return None, None, None
    rotations = []
    fulls = _full_obj_transforms(obj_transforms, n_obj, num_frames, lat_h, lat_w, factor, rotations)
    if all(s == 0 and c == rot[0][0] for rot in rotations for c, s in rot):
        folded = tuple(t if rot[0][0] > 0 else t[:4] + (not t[4], not t[5]) + t[6:] for t, rot in zip(fulls, rotations))
        down = _downgrade_obj_transforms(folded, num_frames)
        if interp == "nearest" or down[1] is None:
            return down + (None,)
    return None, None, tuple(_warp_of(t, rot) for t, rot in zip(fulls, rotations))


def resolve_variant_obj_transforms(variant_obj_transforms, nvar, n_obj, num_frames, lat_h, lat_w, factor=8):
    """``variant_obj_transforms`` of the sampling call: K = ``nvar`` items, each None or a value ``obj_transforms``
    accepts, normalised per variant by ``normalize_obj_transforms``' rules -> (placement, variant_placements, transform,
    variant_transforms), at most one of them not None, resolved in this order:
      all None                    every variant at identity: exactly a call without the argument
      placement or transform      all variants equal: exactly the shared ``obj_transforms`` call (``obj_offsets`` when it only
                                  translates)
      variant_placements          every variant at scale 1 without a flip: exactly the ``variant_obj_offsets`` call
      variant_transforms          else: K full transform tuples, identity and translation-only variants included
    Anything else is a ValueError that names the variant (and, from ``normalize_obj_transforms``, the object)."""
    if variant_obj_transforms is None:
        return None, None, None, None
    if not isinstance(variant_obj_transforms, (list, tuple)):
        raise ValueError(f"variant_obj_transforms: needs a list of {nvar} items (one per variant), got {variant_obj_transforms!r}")
    items = list(variant_obj_transforms)
    if len(items) != nvar:
        raise ValueError(f"variant_obj_transforms: {len(items)} entries for {nvar} variants (one per variant)")
    fulls = []
    for k, item in enumerate(items):
        for j, obj in enumerate(item if isinstance(item, (list, tuple)) else ()):
            if hasattr(obj, "keys") and "rotate" in obj.keys():
                raise ValueError(f"variant_obj_transforms: variant {k}: object {j}: rotate: per-variant rotation is not built -- one "
                                 "warp serves all variants of a call (obj_transforms takes rotate)")
        try:
            fulls.append(_full_obj_transforms([None] * n_obj if item is None else item, n_obj, num_frames, lat_h, lat_w, factor))
        except ValueError as e:
            raise ValueError(f"variant_obj_transforms: variant {k}: {e}") from None
    downs = [_downgrade_obj_transforms(f, num_frames) for f in fulls]
    if all(d == (None, None) for d in downs):
        return None, None, None, None
    if all(f == fulls[0] for f in fulls):
        return downs[0][0], None, downs[0][1], None
    if all(tr is None for _, tr in downs):
        zero = tuple(((0, 0),) * num_frames for _ in range(n_obj))
        return None, tuple(zero if pl is None else pl for pl, _ in downs), None, None
    return None, None, None, tuple(fulls)


def collage_warps(placed, nvar, n_obj, num_frames, lat_h, lat_w):
    """what the resolvers of the sampling call returned (``placed``: placement / variant_placements / transform /
    variant_transforms / warp, at most one not None) -> the warps the main conditioning frames are composed under:
    a list of ONE warp for a mode shared by the variants (or none), of K = ``nvar`` for a per-variant mode; each a value
    ``ops.collage_taps`` takes, per object (ay2, ax2, ((myy, myx, mxy, mxx, den, dy, dx) per frame)) on the ``lat_h`` x ``lat_w``
    grid.  A placement is the identity matrix with its (dy, dx); a transform goes through ``_warp_of`` with the zero rotation; a
    warp is itself; no mode is the identity."""
    identity = lambda offs: (int(lat_h), int(lat_w), tuple((1, 0, 0, 1, 1, int(dy), int(dx)) for dy, dx in offs))
    of_placement = lambda pl: tuple(identity(offs) for offs in pl)
    of_transform = lambda tr: tuple(_warp_of(full, ((WARP_DEN, 0),) * num_frames) for full in tr)
    get = lambda key: placed.get(key) if placed else None
    if get("warp") is not None:
        return [tuple(placed["warp"])]
    if get("variant_transforms") is not None:
        warps = [of_transform(tr) for tr in placed["variant_transforms"]]
    elif get("transform") is not None:
        return [of_transform(placed["transform"])]
    elif get("variant_placements") is not None:
        warps = [of_placement(pl) for pl in placed["variant_placements"]]
    elif get("placement") is not None:
        return [of_placement(placed["placement"])]
    else:
        return [tuple(identity(((0, 0),) * num_frames) for _ in range(n_obj))]
    if len(warps) != nvar:
        raise ValueError(f"collage_warps: {len(warps)} per-variant values for {nvar} variants")
    return warps


def _frames_rgb_u8(frames, num_frames, height, width, what):
    """a list of ``num_frames`` images -> uint8 [F, height, width, 3] (RGB); a frame of another size is a ValueError: the call
    does not resize"""
    import numpy as np
    frames = list(frames)
    if len(frames) != num_frames:
        raise ValueError(f"compose_main_images: {what} has {len(frames)} frames, the clip {num_frames}")
    out = []
    for i, im in enumerate(frames):
        if not hasattr(im, "convert"):
            raise ValueError(f"compose_main_images: {what}, frame {i} is not an image ({type(im).__name__})")
        if tuple(im.size) != (width, height):
            raise ValueError(f"compose_main_images: {what}, frame {i} is {im.size[0]} x {im.size[1]}, the call {width} x {height} "
                             "(width x height; the call does not resize)")
        out.append(np.asarray(im.convert("RGB"), dtype=np.uint8))
    return torch.from_numpy(np.stack(out))


def crosses_gemm_offset_line(nb, frames, h, w, width0):
    """the eight-phase GEMM tiles address their operands with 32-bit byte offsets (gemm.hip g8_ok): the widest level-0 tensor
    of a forward, the feed-forward's [nb * F * h * w, 4 * width0] fp16, must stay under 2 GB for them to be chosen"""
    return nb * frames * h * w * 4 * width0 * 2 >= 2 ** 31


def _per_variant(value, n_prompts, m, what, is_scalar):
    """a scalar (shared by every variant) or a list -- one entry per prompt (each repeated m times) or one per variant"""
    if is_scalar(value):
        return [value] * (n_prompts * m)
    value = list(value)
    if len(value) == n_prompts * m:
        return value
    if len(value) == n_prompts:
        return [v for v in value for _ in range(m)]
    raise ValueError(f"{what}: {len(value)} entries for {n_prompts} prompts x {m} videos per prompt")


class CompositionState(dict):
    """the composition loop's state: a dict that can be referred to weakly.  The closures the state itself holds (``build_map``,
    the iteration bodies of its batches, which its captured graphs keep) reach it through a weak reference, so a dropped state is
    freed at once, by reference count, with its captured graphs.  As a reference cycle it would wait for the cyclic collector,
    and a collection that falls into a LATER state's graph capture destroys the graphs there: HIP refuses that ("operation not
    permitted when stream is capturing") and the process ends."""
    __slots__ = ("__weakref__",)


def _state_mode(st):
    """the entry of ``PLACEMENT_MODES`` a composition state was made with (``make_composition_state`` sets at most one of the
    five values), None for a state that places nothing"""
    return next((m for m in PLACEMENT_MODES if st.get(m.attr) is not None), None)


class GraphedStep:
    """Capture one loop iteration (a python callable working on static device buffers) into a hipGraph."""

    def __init__(self, fn, warmup=2, preserve=()):
        """``preserve``: tensors the iteration updates in place; they are restored after the eager warm-up runs"""
        self.fn = fn
        saved = [t.clone() for t in preserve]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            fn()
        for t, s in zip(preserve, saved):
            t.copy_(s)

    def __call__(self):
        self.graph.replay()


class I2VGenXLPipeline:
    """Drop-in surface of the reference pipeline for the denoising path."""

    def __init__(self, unet, scheduler=None, conditioner=None, use_graphs=True):
        self.unet = unet
        self.scheduler = scheduler or DDIMScheduler()
        self.conditioner = conditioner or SyntheticConditioner(unet.device, unet.config.cross_attention_dim)
        self.use_graphs = use_graphs
        self.vae_scale_factor = 8
        self._guidance_scale = 1.0
        self._graphs = {}
        self.max_cached_graphs = 4
        self._concurrent_states = {}  # invert_concurrent: one captured iteration per concurrent clip
        self._streams = []
        # composition loop: the UNet's source chunks are never read behind the last injection site (unet.prune_source_tail)
        self.prune_source_tail = os.environ.get("MVOC_PRUNE_SOURCE_TAIL", "1") != "0"  # (=0: A/B)
        # ... and on a step where only Q/K sites registered with inject_background=False inject, nothing reads the background chunk
        # either: the UNet runs without it (unet.prune_background)
        self.prune_background = os.environ.get("MVOC_PRUNE_BACKGROUND", "1") != "0"  # (=0: A/B)
        # ... and its unconditional / conditional chunks are one computation up to the first cross-attention (unet.shared_prefix_chunks)
        self.share_cfg_prefix = os.environ.get("MVOC_SHARE_CFG_PREFIX", "1") != "0"  # (=0: A/B)
        # ... and source roles that are the same source (same conditioning, same inversion latents) share one chunk: the batch
        # [s_0..s_{k-1}, uncond, cond] (plan_source_map, unet.source_chunks).  Opt-in: MVOC_DEDUP_SOURCES=1 or composite.py
        # --dedup_sources; the VAE draws of identical conditioning images are then shared too
        self.dedup_sources = os.environ.get("MVOC_DEDUP_SOURCES", "0") != "0"
        self.latent_cache = LatentCache(unet.device)

    # ---- reference plumbing ------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path, torch_dtype=H16, variant="fp16", device="cuda:0", **kw):
        """``I2VGenXLPipeline.from_pretrained(PRETRAINED_MODEL_PATH, torch_dtype=fp16, variant="fp16")`` of the reference drivers
        (``inverse.py:113-118``, ``composite.py:76-85``): the UNet from ``<path>/unet/config.json`` (the I2VGen-XL default when the file
        is absent) + ``<path>/unet/diffusion_pytorch_model[.fp16].safetensors`` (diffusers layout).  The checkpoint's VAE and CLIP
        towers are attached by the drivers (``mvoc_amd.vae.attach_vae`` / ``mvoc_amd.clip.attach_clip``)."""
        import json
        from safetensors.torch import load_file
        from .unet import I2VGenXLUNet
        from .unet_spec import UNetConfig
        cfg = None
        cf = os.path.join(path, "unet", "config.json")
        if os.path.exists(cf):
            with open(cf) as fh:
                cfg = UNetConfig.from_diffusers(json.load(fh))
        for name in (f"diffusion_pytorch_model.{variant}.safetensors", "diffusion_pytorch_model.safetensors"):
            f = os.path.join(path, "unet", name)
            if os.path.exists(f):
                unet = I2VGenXLUNet(cfg, device=device).load_state_dict(load_file(f))
                return cls(unet, **kw)
        raise FileNotFoundError(f"no UNet weights under {path}/unet (expected diffusers safetensors); for synthetic "
                                "weights use mvoc_amd.pipeline.I2VGenXLPipeline.synthetic()")

    @classmethod
    def synthetic(cls, config=None, device="cuda:0", seed=8888, **kw):
        from .unet import I2VGenXLUNet
        return cls(I2VGenXLUNet(config, device=device).init_random(seed), **kw)

    def to(self, device):
        return self

    def register_modules(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def _execution_device(self):
        return self.unet.device

    @property
    def device(self):
        return self.unet.device

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1

    def encode_vae_video(self, video, device=None, height=576, width=1024):
        return self.conditioner.encode_video(video, height, width)

    def prepare_latents(self, batch, channels, num_frames, height, width, dtype, device, generator, latents=None):
        shape = (batch, channels, num_frames, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is None:
            g = generator if isinstance(generator, torch.Generator) and generator.device.type == "cpu" else None
            latents = torch.randn(shape, generator=g, dtype=torch.float32).to(dtype)
        return (latents.to(device, dtype) * self.scheduler.init_noise_sigma).contiguous()

    # ---- conditioning ---------------------------------------------------------------------------------
    def _stock_conditioning(self, prompt, negative_prompt, image, num_frames, height, width, target_fps, prompt_embeds,
                            negative_prompt_embeds, image_embeddings, image_latents):
        c = self.conditioner
        if prompt_embeds is None:
            prompt_embeds, negative_prompt_embeds = c.encode_prompt(prompt, negative_prompt)
        if image_embeddings is None:
            if getattr(c, "clip", None) is not None and hasattr(image, "convert"):
                from .vae import center_crop_wide
                # :1116-1120 -- the stock entry crops before the CLIP resize (the composition entries resize the uncropped frame)
                image_embeddings = c.encode_image(center_crop_wide(image, (width, width)))
            else:
                image_embeddings = c.encode_image(image)
        if image_latents is None:
            image_latents = c.image_latents(image, num_frames, height, width)
        if self.do_classifier_free_guidance:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])
            image_embeddings = torch.cat([torch.zeros_like(image_embeddings), image_embeddings])  # :766
            image_latents = torch.cat([image_latents] * 2)
        nb = prompt_embeds.shape[0]
        fps = torch.full((nb,), float(target_fps), dtype=torch.float32, device=self.device)
        return dict(encoder_hidden_states=prompt_embeds.to(self.device, H16).contiguous(),
                    image_embeddings=image_embeddings.to(self.device, H16).contiguous(),
                    image_latents=image_latents.to(self.device, H16).contiguous(), fps=fps)

    def enable_frame_shard(self, shard):
        """Frame-shard the UNet of this pipeline over the ranks of ``shard`` (``mvoc_amd.frame_shard.FrameShard``; BASELINE
        configs[3]: one long clip on the 8 GPUs of a node).  Every rank runs the same loop on the same full latents (the
        scheduler update is replicated, 4 channels); the UNet computes F/world frames per rank.  Loop iterations run
        eagerly (torch.distributed issues the RCCL exchanges between the library's launches); rank 0 alone writes
        ``ddim_latents_{t}.pt`` files."""
        self.unet.set_frame_shard(shard)
        self.use_graphs = False
        self._graphs = {}
        self._concurrent_states = {}
        self.latent_cache.write_files = shard.rank == 0
        return self

    # ---- one loop iteration each (static buffers so that they can be graph-captured) -------------------
    def _make_stock_step(self, key, latents, cond, guidance_scale):
        """iteration of invert / __call__: [cat x2] -> UNet -> CFG + (inverse-)DDIM update, in place on `state`.
        The conditioning lives in buffers owned by the state (``load_cond`` refreshes them), so one captured iteration
        serves every later call of the same shape."""
        st = {"latents": latents.clone(), "t": torch.zeros(1, dtype=torch.float32, device=self.device),
              "coef": torch.zeros(5, dtype=torch.float32, device=self.device),
              "cond": {k: v.clone() for k, v in cond.items()}}
        do_cfg = guidance_scale > 1
        own = st["cond"]
        # loop-invariant conditioning (context tokens, cross-attention K/V, image-latent stem): once per loop, not per step
        shape = (latents.shape[0] * (2 if do_cfg else 1),) + tuple(latents.shape[1:])

        def prepare():
            return self.unet.prepare_conditioning(shape, own["fps"], own["image_latents"], own["image_latents"],
                                                  own["image_embeddings"], own["encoder_hidden_states"], False)

        prepared = prepare()

        def load_cond(new):
            """new conditioning of the same shapes -> the state's static buffers (no re-capture)"""
            for k, v in new.items():
                own[k].copy_(v)
            prepared.copy_from(prepare())

        def body():
            x = st["latents"]
            inp = torch.cat([x, x]) if do_cfg else x
            noise = self.unet.forward(inp, st["t"], own["fps"], image_latents=own["image_latents"],
                                      image_embeddings=own["image_embeddings"],
                                      encoder_hidden_states=own["encoder_hidden_states"], conditioning=prepared)[0]
            if do_cfg:
                ops.ddim_step(x, noise[1:2].contiguous(), st["coef"], v_uncond=noise[0:1].contiguous(), out=x)
            else:
                ops.ddim_step(x, noise, st["coef"], out=x)

        st["load_cond"] = load_cond
        st["run"] = GraphedStep(body, preserve=(st["latents"],)) if self.use_graphs else body
        return st

    def _run_stock_loop(self, latents, cond, num_inference_steps, guidance_scale, first_idx=0, on_step=None):
        sched = self.scheduler
        sched.set_timesteps(num_inference_steps, device=self.device)
        sched.timesteps = sched.timesteps[first_idx:]
        table, index = sched.coef_table(self.device, guidance_scale)
        # keyed by what the captured iteration bakes in (shapes, CFG layout, frame shard, graphs on/off) -- NOT by the
        # conditioning tensors' addresses: those change with every invert() / __call__()
        flags = self.unet.injection_flags()
        if any(flags):  # eager mode raises on the batch layout; a cached graph would silently replay a clean iteration
            raise RuntimeError("stock loop with PnP hooks armed: call register_time_all(pipe, None, None) first")
        key = ("stock", tuple(latents.shape), guidance_scale > 1, getattr(self.unet, "shard_generation", 0) if self.unet.shard is not None else 0,
               bool(self.use_graphs), flags, tuple((k, tuple(v.shape)) for k, v in sorted(cond.items())))
        st = self._graphs.pop(key, None)
        if st is None:
            if len(self._graphs) >= self.max_cached_graphs:  # each entry pins a UNet graph + its private activation pool
                self._graphs.pop(next(iter(self._graphs)))     # least recently used (hits are re-inserted at the end)
            st = self._make_stock_step(key, latents, cond, guidance_scale)
        else:
            st["load_cond"](cond)
        self._graphs[key] = st
        st["latents"].copy_(latents)
        for i, t in enumerate(sched.timesteps):
            st["t"].fill_(float(t))
            st["coef"].copy_(table[index[int(t)]])
            st["run"]()
            if on_step is not None:
                on_step(i, int(t), st["latents"])
        return st["latents"].clone()

    # ---- reference methods -----------------------------------------------------------------------------
    @torch.no_grad()
    def invert(self, prompt=None, image=None, height=704, width=1280, target_fps=16, num_frames=16,
               num_inference_steps=50, guidance_scale=9.0, negative_prompt=None, eta=0.0, num_videos_per_prompt=1,
               decode_chunk_size=1, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
               output_type="pil", return_dict=True, cross_attention_kwargs=None, clip_skip=1, output_dir=None,
               image_embeddings=None, image_latents=None):
        """DDIM inversion; writes ``ddim_latents_{t}.pt`` per step and returns ``[1, steps, 4, F, h, w]`` noisiest first."""
        self._guidance_scale = guidance_scale
        cond = self._stock_conditioning(prompt, negative_prompt, image, num_frames, height, width, target_fps, prompt_embeds,
                                        negative_prompt_embeds, image_embeddings, image_latents)
        latents = self.prepare_latents(1, 4, num_frames, height, width, H16, self.device, generator, latents)
        seq = []

        def on_step(i, t, lat):
            snap = lat.clone()
            seq.append(snap)
            self.latent_cache.put(output_dir, t, snap)  # device-resident hand-off + async torch.save

        self._run_stock_loop(latents, cond, num_inference_steps, guidance_scale, on_step=on_step)
        self.latent_cache.flush()
        inverted = torch.stack(list(reversed(seq)), 1)
        if not return_dict:
            return inverted
        return PipelineOutput(inverted_latents=inverted)

    @torch.no_grad()
    def invert_many(self, prompts, images, latents, output_dirs, height=704, width=1280, target_fps=16, num_frames=16,
                    num_inference_steps=50, guidance_scale=1.0, negative_prompt=None):
        """DDIM-invert several source clips of the same shape in ONE batched loop: the per-object inversions of a
        composition job (background + N objects) are independent (``inverse.py:136-190`` runs them one after another),
        so on one GPU they can share every weight read -- UNet batch n instead of n passes at batch 1.  Same files, same
        return value per clip as ``invert``; guidance 1.0 only (the setting of ``group_inversion/template.yaml``)."""
        if guidance_scale > 1:
            raise NotImplementedError("invert_many batches the cfg = 1.0 inversions of inverse.py; use invert() for CFG")
        n = len(prompts)
        if not (len(images) == len(latents) == len(output_dirs) == n and n > 0):
            raise ValueError("invert_many: prompts, images, latents and output_dirs must have the same length")
        self._guidance_scale = guidance_scale
        conds = [self._stock_conditioning(p, negative_prompt, im, num_frames, height, width, target_fps, None, None, None, None)
                 for p, im in zip(prompts, images)]
        cond = {k: torch.cat([c[k] for c in conds]).contiguous() for k in conds[0]}
        lat = torch.cat([self.prepare_latents(1, 4, num_frames, height, width, H16, self.device, None, l) for l in latents])
        seqs = [[] for _ in range(n)]

        def on_step(i, t, cur):
            for j in range(n):
                snap = cur[j:j + 1].clone()
                seqs[j].append(snap)
                self.latent_cache.put(output_dirs[j], t, snap)

        self._run_stock_loop(lat, cond, num_inference_steps, guidance_scale, on_step=on_step)
        self.latent_cache.flush()
        return [torch.stack(list(reversed(s_)), 1) for s_ in seqs]

    @torch.no_grad()
    def invert_concurrent(self, prompts, images, latents, output_dirs, height=704, width=1280, target_fps=16, num_frames=16,
                          num_inference_steps=50, guidance_scale=1.0, negative_prompt=None, concurrency_hint=True):
        """DDIM-invert several source clips AT THE SAME TIME, each in its own batch-1 loop on its own HIP stream.  The
        per-object inversions of a composition job are independent (``inverse.py:136-190`` runs them one after another; on a
        node they shard one per GPU): on one GPU their kernels interleave, and wherever a batch-1 launch cannot fill the chip --
        the 16x16 / 8x8 levels run 80-240 workgroups on 256 CUs, the small norm / statistics kernels are latency-bound -- another
        clip's kernels take the idle CUs (32.5 -> 26.7 ms per clip-step at three clips, profiles/r4).  Same return value per clip
        as ``invert``.

        ``concurrency_hint``: the value every GEMM of the captured iterations carries in ``mvoc_gemm_desc.concurrency``.
        ``False`` / ``1``: every clip runs exactly the launches of ``invert`` -- latents and ``ddim_latents_{t}.pt`` files are
        BIT-IDENTICAL to the one-by-one pass (asserted at production width in tests/test_fullwidth_gpu.py).  ``True`` (default):
        the hint is the number of clips of this call; an ``int`` fixes it whatever the group size (the driver passes its
        ``--concurrent_entries`` so that a clip's files do not depend on how many other clips happened to be pending).  With a hint
        > 1 the GEMMs whose batch-1 grid cannot fill the chip keep their K in one piece (no split-K slabs / reduce pass: the other
        clips fill the idle CUs; 25.5 ms per clip-step) and therefore sum in another order than under ``invert``: the latents then
        differ from the one-by-one pass by fp16 rounding of another summation order (rel-L2 5e-5 after a step on the 1.42 B
        network; same test), inside the per-step tolerance but NOT bit-identical."""
        n = len(prompts)
        if not (len(images) == len(latents) == len(output_dirs) == n and n > 0):
            raise ValueError("invert_concurrent: prompts, images, latents and output_dirs must have the same length")
        if self.unet.shard is not None:
            raise NotImplementedError("invert_concurrent: frame-sharded clips run one at a time")
        self._guidance_scale = guidance_scale
        sched = self.scheduler
        sched.set_timesteps(num_inference_steps, device=self.device)
        table, index = sched.coef_table(self.device, guidance_scale)
        if any(self.unet.injection_flags()):
            raise RuntimeError("stock loop with PnP hooks armed: call register_time_all(pipe, None, None) first")
        states, seqs = [], [[] for _ in range(n)]
        for j in range(n):
            cond = self._stock_conditioning(prompts[j], negative_prompt, images[j], num_frames, height, width, target_fps, None, None,
                                            None, None)
            lat = self.prepare_latents(1, 4, num_frames, height, width, H16, self.device, None, latents[j])
            hint = (n if concurrency_hint is True else max(1, int(concurrency_hint)))
            key = ("stock-concurrent", j, hint, tuple(lat.shape), guidance_scale > 1, bool(self.use_graphs),
                   tuple((k, tuple(v.shape)) for k, v in sorted(cond.items())))
            st = self._concurrent_states.pop(key, None)
            if st is None:
                with ops.gemm_concurrency(hint):  # (baked into the captured iteration: tile / split-K choices)
                    st = self._make_stock_step(key, lat, cond, guidance_scale)
            else:
                st["load_cond"](cond)
            self._concurrent_states[key] = st  # (re-)inserted at the end: least recently used first
            st["latents"].copy_(lat)
            states.append(st)
        # each entry pins a UNet graph and its private activation pool: keep this call's states plus at most as many older ones
        # as `_graphs` may hold (a job that alternates two shapes keeps both, a long multi-shape job does not grow without bound)
        while len(self._concurrent_states) > n + self.max_cached_graphs:
            self._concurrent_states.pop(next(iter(self._concurrent_states)))
        while len(self._streams) < n:
            self._streams.append(torch.cuda.Stream(device=self.device))
        cur = torch.cuda.current_stream()
        for s_ in self._streams[:n]:
            s_.wait_stream(cur)
        for t in sched.timesteps:
            row = table[index[int(t)]]
            for j, (st, s_) in enumerate(zip(states, self._streams)):
                with torch.cuda.stream(s_):  # everything of clip j -- the two small fills, the replay, the snapshot -- on stream j
                    st["t"].fill_(float(t))
                    st["coef"].copy_(row)
                    st["run"]()
                    snap = st["latents"].clone()
                    seqs[j].append(snap)
                    self.latent_cache.put(output_dirs[j], int(t), snap)
        for s_ in self._streams[:n]:
            cur.wait_stream(s_)
        self.latent_cache.flush()
        return [torch.stack(list(reversed(q)), 1) for q in seqs]

    @torch.no_grad()
    def __call__(self, prompt=None, image=None, height=704, width=1280, target_fps=16, num_frames=16,
                 num_inference_steps=50, guidance_scale=9.0, negative_prompt=None, eta=0.0, num_videos_per_prompt=1,
                 decode_chunk_size=1, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                 output_type="pil", return_dict=True, cross_attention_kwargs=None, clip_skip=1, ddim_init_latents_t_idx=0,
                 image_embeddings=None, image_latents=None):
        self._guidance_scale = guidance_scale
        cond = self._stock_conditioning(prompt, negative_prompt, image, num_frames, height, width, target_fps, prompt_embeds,
                                        negative_prompt_embeds, image_embeddings, image_latents)
        latents = self.prepare_latents(1, 4, num_frames, height, width, H16, self.device, generator, latents)
        latents = self._run_stock_loop(latents, cond, num_inference_steps, guidance_scale, first_idx=ddim_init_latents_t_idx)
        frames = latents if output_type == "latent" else self._to_video(latents, output_type)
        return PipelineOutput(frames=frames) if return_dict else (frames,)

    def _to_video(self, latents, output_type):
        """``decode_latents`` + ``tensor2vid`` (``pipeline_i2vgen_xl.py:1207-1208``): per batch entry a list of PIL frames"""
        from .vae import tensor2vid
        return tensor2vid(self.conditioner.decode(latents), output_type)

    # ---- composition --------------------------------------------------------------------------------------
    def _move_masks(self, masks, table, mover, soft=None):
        """per object the soft and the hard mask moved by ``mover`` (``ops.shift_planes`` / ``gather_planes`` / ``warp_planes``, zero fill) with
        row j of the latent-grid ``table`` -> (masks in the form they came in, the table).  ``soft`` = (table, mover): the soft
        masks go through these instead (interpolated, while the hard masks stay nearest)"""
        dev = self.device
        soft_table, soft_mover = (table, mover) if soft is None else soft
        moved = []
        for j, (s_m, h_m) in enumerate(masks):
            s16 = soft_mover(s_m.to(dev, H16).contiguous(), soft_table[j])
            h16 = mover(h_m.to(dev, H16).contiguous(), table[j])
            moved.append((s16.to(s_m.dtype), h16.to(h_m.dtype)))
        return moved, table

    def place_masks(self, masks, placement):
        """the call's masks moved to destination coordinates: per object the soft and the hard mask shifted by
        the object's per-frame offsets with zero fill (``ops.shift_planes``) -> (masks in the form they came in, the device
        table int32 [nobj, F, 2] of the latent-grid offsets)"""
        if len(placement) != len(masks):
            raise ValueError(f"placement: offsets for {len(placement)} objects, {len(masks)} masks")
        frames = masks[0][0].shape[-3]
        if any(len(obj) != frames for obj in placement):
            raise ValueError(f"placement: every object needs {frames} per-frame offsets")
        return self._move_masks(masks, torch.tensor(placement, dtype=torch.int32).to(self.device).contiguous(), ops.shift_planes)

    def transform_masks(self, masks, transform):
        """the call's masks moved to destination coordinates under a transform: per object the soft and the hard
        mask gathered through the object's per-frame index maps of the latent grid itself (``ops.level_axis_map`` with size ==
        mask size), zero where the object is absent (``ops.gather_planes``) -> (masks in the form they came in, the device table
        int32 [nobj, F, h + w] of those maps)"""
        if len(transform) != len(masks):
            raise ValueError(f"transform: {len(transform)} objects, {len(masks)} masks")
        frames, h, w = masks[0][0].shape[-3:]
        if any(len(t[8]) != frames for t in transform):
            raise ValueError(f"transform: every object needs {frames} per-frame offsets")
        return self._move_masks(masks, ops.resample_table(transform, h, w, h, w, self.device), ops.gather_planes)

    def warp_masks(self, masks, warp):
        """the call's masks moved to destination coordinates under a warp: per object the soft and the hard mask
        gathered through the object's per-frame 2-D index maps of the latent grid itself (``ops.level_warp_map`` with size == mask
        size), zero where the object is absent (``ops.warp_planes``) -> (masks in the form they came in, the device table int32
        [nobj, F, h * w] of those maps)"""
        h, w = self._warp_mask_grid(masks, warp)
        return self._move_masks(masks, ops.warp_table(warp, h, w, h, w, self.device), ops.warp_planes)

    @staticmethod
    def _warp_mask_grid(masks, warp):
        """a warp against the call's masks: one entry per object, one matrix per frame -> the latent grid (h, w)"""
        if len(warp) != len(masks):
            raise ValueError(f"warp: {len(warp)} objects, {len(masks)} masks")
        frames, h, w = masks[0][0].shape[-3:]
        if any(len(o[2]) != frames for o in warp):
            raise ValueError(f"warp: every object needs {frames} per-frame matrices")
        return h, w

    def warp_masks_bilinear(self, masks, warp):
        """``warp_masks`` under ``obj_transform_filter`` = "bilinear" (DESIGN.md 6r): the SOFT masks are interpolated through the
        taps of the latent grid itself (``ops.warp_planes_bilinear``), the HARD masks gathered through the nearest maps as ever, so
        they stay 0 / 1 -> (masks in the form they came in, the nearest table int32 [nobj, F, h * w], the tap table int32
        [nobj, F, h * w, 2])"""
        h, w = self._warp_mask_grid(masks, warp)
        taps = ops.warp_tap_table(warp, h, w, h, w, self.device)
        moved, table = self._move_masks(masks, ops.warp_table(warp, h, w, h, w, self.device), ops.warp_planes,
                                        soft=(taps, ops.warp_planes_bilinear))
        return moved, table, taps

    def _move_variant_masks(self, masks, values, move, tables_key):
        """the call's masks moved once per variant by ``move`` (``place_masks`` / ``transform_masks``) with each of ``values`` ->
        dict(``tables_key`` = per variant the device table of its move on the latent grid,
             masks = (soft, hard) fp16 [K, nobj, F, h, w] stacks for the engine (``unet.variant_masks``),
             fusion_masks = per variant the soft masks [nobj, 1, 4, F, h, w] fp16 of the fusion steps)"""
        moved = [move(masks, v) for v in values]
        first = lambda t: t.reshape(-1, *t.shape[-3:])[0].to(self.device, H16)  # as the engine forms its device masks
        return {tables_key: [tab for _, tab in moved],
                "masks": tuple(torch.stack([torch.stack([first(m[i]) for m in mk]) for mk, _ in moved]).contiguous() for i in (0, 1)),
                "fusion_masks": [torch.stack([m[0].to(self.device, H16) for m in mk]).contiguous() for mk, _ in moved]}

    def place_variant_masks(self, masks, variant_placements):
        """``_move_variant_masks`` under per-variant placement: ``place_dev`` = int32 [nobj, F, 2] offsets"""
        return self._move_variant_masks(masks, variant_placements, self.place_masks, "place_dev")

    def transform_variant_masks(self, masks, variant_transforms):
        """``_move_variant_masks`` under per-variant transforms: ``resample_dev`` = int32 [nobj, F, h + w] maps"""
        return self._move_variant_masks(masks, variant_transforms, self.transform_masks, "resample_dev")

    def make_composition_state(self, latents, cond, masks, guidance_scale, dedup_sources=None, variants=1, placement=None,
                               variant_placements=None, transform=None, variant_transforms=None, warp=None,
                               obj_transform_filter=None):
        """static buffers + the captured iteration variants of the composition loop.
        cond: dict(encoder_hidden_states [n,77,D], image_embeddings [n,F,D], image_latents_first, image_latents, fps).
        The state keeps its OWN copy of ``cond``: the hoisted conditioning (``prepare_conditioning``) and the shared-CFG-prefix
        decision below are taken once from these values, so a caller that later rewrites its tensors in place cannot make the
        captured iterations disagree with them -- new conditioning = a new state.
        ``dedup_sources`` (None: ``self.dedup_sources``): classify the source roles once (``source_classes``); every step then
        runs the batch its source map (``plan_source_map``) lays out, each map with its own buffers, built on first use.
        ``variants`` = K > 1: ``latents`` is [K, 4, F, h, w], ``cond`` rows follow ``variant_layout`` ([bg, obj.., u_1..u_K,
        c_1..c_K]), ``guidance_scale`` is a float or K floats (all > 1 or none), a step's coefficient rows are [K, 5].
        ``placement`` (``normalize_obj_offsets``; None: objects stay where they are): ``masks`` come in the objects' source
        coordinates and are moved ONCE, here, to destination coordinates -- the state's masks everywhere (hooks, fusion).
        ``variant_placements`` (``resolve_variant_obj_offsets``; not with ``placement``): K placements, one per
        variant.  Each variant's masks are moved once, here; the engine takes them as (soft, hard) [K, nobj, F, h, w] stacks,
        the fusion steps each variant's own.  The hooks keep ``masks`` as they came (shape checks and the mask key).
        ``transform`` (``normalize_obj_transforms``; not with ``placement`` / ``variant_placements``): scale, mirror
        and translation per object, one transform for all variants.  ``masks`` come in source coordinates and are gathered ONCE,
        here, to destination coordinates (``transform_masks``); the fusion steps gather the objects' latents the same way.
        ``variant_transforms`` (``resolve_variant_obj_transforms``; not with any of the three above): K transforms,
        one per variant.  Each variant's masks are gathered once, here; the engine takes them as (soft, hard) [K, nobj, F, h, w]
        stacks, the fusion steps each variant's own.  The hooks keep ``masks`` as they came (shape checks and the mask key).
        ``warp`` (``resolve_obj_transforms``; not with any of the four above): rotation with scale, mirror and
        translation per object and frame, one warp for all variants.  ``masks`` come in source coordinates and are gathered ONCE,
        here, through the 2-D maps of the latent grid (``warp_masks``); the fusion steps gather the objects' latents the same way.
        ``obj_transform_filter``: None / "nearest" = the call without it; "bilinear" (with ``warp`` only): the sites
        interpolate the objects through tap tables (``unet.warp_filter``), the soft masks and the fusion steps' object latents are
        interpolated the same way at the latent grid (``warp_masks_bilinear``), the hard masks stay nearest."""
        warp_filter = _transform_filter(obj_transform_filter)
        if warp_filter is not None and warp is None:
            raise ValueError("obj_transform_filter = 'bilinear' needs a warp: the filter is a property of the warp mode "
                             "(resolve_obj_transforms(..., interp='bilinear') returns one for everything but a translation)")
        cond = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in cond.items()}
        given = {"placement": placement, "variant_placements": variant_placements, "transform": transform,
                 "variant_transforms": variant_transforms, "warp": warp}
        # the state's keys of the five modes: each mode's value, the shared modes' latent-grid table (place_dev / resample_dev)
        # and the per-variant modes' ``_move_variant_masks`` dict (vplace / vresample); all None but the active mode's
        placed = dict.fromkeys(("placement", "place_dev", "variant_placements", "vplace", "transform", "resample_dev",
                                "variant_transforms", "vresample", "warp", "warp_dev"))
        if warp_filter is not None:
            placed.update(warp_filter=warp_filter, warp_taps_dev=None)
        on = [m for m in PLACEMENT_MODES if given[m.attr] is not None]
        if on:
            m = on[0]
            value = given[m.attr]
            if len(on) > 1:
                raise ValueError(m.mix.format(set="given"))
            if self.unet.shard is not None:
                raise RuntimeError(frame_shard_refusal(m.subject, m.mover))
            if m.per_variant and len(value) != int(variants):
                raise ValueError(f"{m.attr}: {len(value)} {m.items} for {int(variants)} variants")
            move = {"resample": self.transform_masks, "place": self.place_masks, "warp": self.warp_masks}[m.kw]
            if m.per_variant:
                value = tuple(tuple(v) for v in value)
                placed["v" + m.kw] = self._move_variant_masks(masks, value, move, m.kw + "_dev")
            elif warp_filter is not None:
                value = tuple(value)
                masks, placed["warp_dev"], placed["warp_taps_dev"] = self.warp_masks_bilinear(masks, value)
            else:
                value = tuple(value)
                masks, placed[m.kw + "_dev"] = move(masks, value)
            placed[m.attr] = value
        n_obj = len(masks)
        nvar = int(variants)
        scales = [float(g) for g in guidance_scale] if isinstance(guidance_scale, (list, tuple)) else [float(guidance_scale)]
        do_cfg = scales[0] > 1  # off: batch [bg, objs.., cond], one destination chunk for the injections
        if any((g > 1) != do_cfg for g in scales):
            raise ValueError("variants: guidance is on (scale > 1) for all variants of a call or off for all")
        lay = variant_layout(n_obj, nvar, do_cfg)
        nb = lay["nb"]
        if latents.shape[0] != nvar:
            raise ValueError(f"composition state: {nvar} variants need latents [{nvar}, 4, F, h, w], got {tuple(latents.shape)}")
        if nvar > 1 and self.unet.shard is not None:
            raise RuntimeError("variants > 1 do not combine with the frame shard: run one composition per call")
        dev = self.device
        dedup = self.dedup_sources if dedup_sources is None else bool(dedup_sources)
        st = CompositionState()
        st.update({"latents": latents.clone(), "inp": torch.empty((nb,) + tuple(latents.shape[1:]), dtype=H16, device=dev),
              "t": torch.zeros(1, dtype=torch.float32, device=dev),
              "coef": torch.zeros(5 if nvar == 1 else (nvar, 5), dtype=torch.float32, device=dev),
              "masks": masks, "variants": {}, "cond": cond, "n_obj": n_obj, "nvar": nvar,
              "fusion_masks": torch.stack([m[0].to(dev, H16) for m in masks]).contiguous(),
              "fusion_objs": torch.empty((n_obj, 1) + tuple(latents.shape[1:]), dtype=H16, device=dev), "maps": {},
              "place_tables": [], **placed})
        weak = weakref.ref(st)  # (the caller holds the state for as long as it steps it)
        st["build_map"] = lambda smap: self._composition_batch(weak(), smap, do_cfg)
        st["maps"][None] = st["build_map"](None)

        # classifier-free guidance: the unconditional and the conditional chunk receive the same latent (below); when their image
        # latents and fps are equal too -- the reference builds both from the main image, pipeline_i2vgen_xl.py:1676-1690 -- they
        # differ only in what the cross-attentions see, and the UNet shares their common prefix (unet.shared_prefix_chunks)
        # (K variants: off -- the prefix would save the network up to the first cross-attention only)
        share = bool(self.share_cfg_prefix and do_cfg and nvar == 1 and
                     all(torch.equal(cond[k][nb - 2], cond[k][nb - 1]) for k in ("image_latents_first", "image_latents", "fps")))
        st["share_cfg_prefix"] = share
        # (a frame-sharded clip runs the full layout: no de-duplication)
        st["classes"] = source_classes(cond, n_obj) if dedup and self.unet.shard is None else None
        st["body"] = st["maps"][None]["body"]
        st["nb"] = nb
        return st

    def _composition_batch(self, st, smap, do_cfg):
        """the UNet batch of one source map (None: the positional [bg, obj_1..obj_n, (uncond,) cond]): its input buffer, its
        rows of the conditioning, the hoisted conditioning and the iteration body"""
        n_obj, cond, nvar = st["n_obj"], st["cond"], st["nvar"]
        if smap is None:
            inp, mcond = st["inp"], cond
        else:
            nb_full = n_obj + 1 + (2 if do_cfg else 1) * nvar
            rows = torch.tensor(source_rows(smap, n_obj) + list(range(n_obj + 1, nb_full)), device=self.device)
            mcond = {k: v.index_select(0, rows.to(v.device)).contiguous() for k, v in cond.items()}
            inp = torch.empty((len(rows),) + tuple(st["latents"].shape[1:]), dtype=H16, device=self.device)
        nb = inp.shape[0]
        prepared = self.unet.prepare_conditioning(tuple(inp.shape), mcond["fps"], mcond["image_latents_first"],
                                                  mcond["image_latents"], mcond["image_embeddings"],
                                                  mcond["encoder_hidden_states"], False)

        weak = weakref.ref(st)  # the state holds this body (and its captured graph): no cycle back to it, see CompositionState
        del st

        def body():
            st = weak()
            x = st["latents"]  # [K, 4, F, h, w]: every variant's latent into its u_k and c_k chunk
            if do_cfg:
                inp[nb - 2 * nvar:nb - nvar].copy_(x)
            inp[nb - nvar:].copy_(x)
            u = self.unet
            mode = _state_mode(st)
            vstate = st["v" + mode.kw] if mode is not None and mode.per_variant else None
            with u.scoped(prune_source_tail=bool(self.prune_source_tail),  # this loop reads the destination chunks only
                          prune_background=bool(self.prune_background),  # ... and never the background's output
                          shared_prefix_chunks=2 if st["share_cfg_prefix"] else 0, source_chunks=smap, variants=nvar,
                          placement=st["placement"], variant_placements=st["variant_placements"], transform=st["transform"],
                          variant_transforms=st["variant_transforms"], warp=st["warp"], variant_masks=None if vstate is None else vstate["masks"],
                          **({"warp_filter": st["warp_filter"]} if st.get("warp_filter") else {})):
                noise = u.forward_ext(inp, st["t"], mcond["fps"], mcond["image_latents_first"], mcond["image_latents"],
                                      mcond["image_embeddings"], mcond["encoder_hidden_states"], multi_frame_guidance=False,
                                      conditioning=prepared)[0]
            # the engine's per-level tables of this state's mode are read by its captured graphs: they live as long as the state,
            # also after the engine drops them for another value of the mode
            # (under the bilinear filter the sites read the engine's tap tables, which have a cache of their own)
            tables = u._tap_tables[1] if st.get("warp_filter") else None if mode is None else u._level_tables[mode.attr][1]
            if tables is not None and not any(d is tables for d in st["place_tables"]):
                st["place_tables"].append(tables)
            ops.ddim_step(x, noise[nb - nvar:nb].contiguous(), st["coef"],
                          v_uncond=noise[nb - 2 * nvar:nb - nvar].contiguous() if do_cfg else None, out=x)

        return {"inp": inp, "cond": mcond, "prepared": prepared, "body": body, "nb": nb}

    def background_dead(self, smap):
        """whether the UNet drops the background chunk on the step the CURRENT hook state describes, run on the batch of source
        map ``smap`` (``unet.background_dead`` as the iteration body will see it: the body sets both attributes)"""
        with self.unet.scoped(prune_background=bool(self.prune_background), source_chunks=smap) as u:
            return bool(u.background_dead())

    def composition_variant_key(self, st, smap):
        """what a captured composition iteration bakes in, as the key of ``st["variants"]`` (see ``composition_step``).  A run
        alternates steps that drop the background chunk and steps that need it: each kind has its own graph"""
        u, mode = self.unet, _state_mode(st)
        return (u.injection_masks(st["nvar"]), u.mask_key(st["masks"]), bool(u.pair_destinations), bool(u.prune_dead_chunks),
                bool(self.prune_source_tail), bool(st.get("share_cfg_prefix")), smap, st["nvar"]) + \
            (() if mode is None else (mode.attr, st[mode.attr])) + \
            ((st["warp_filter"],) if st.get("warp_filter") else ()) + \
            (("no_background",) if self.background_dead(smap) else ())

    def composition_step(self, st, t, bg_latents, obj_latents, table_row, fuse=None):
        """one iteration of ``:1636-1734`` on device-resident latents; ``fuse`` = (mix_ratio, obj_random_noise_fusion,
        fusion object latents) on fusion steps.  With source de-duplication the roles handed the same latents tensor (and of
        one conditioning class) share a chunk: the step's source map picks the batch."""
        if fuse is not None:
            mix, rnf, fobjs = fuse
            # the object's inverted latents move with it, by the state's mode: shifted or gathered with the latent-grid table that
            # moved the fusion masks (zero fill), or copied as they are
            mode = _state_mode(st)
            mover = None if mode is None else getattr(ops, mode.mover + "_planes")
            moved_by = None if mode is None else mode.kw + "_dev"
            if st.get("warp_filter"):  # bilinear: the latents are interpolated through the taps that moved the soft masks
                mover, moved_by = ops.warp_planes_bilinear, "warp_taps_dev"
            if mode is not None and mode.per_variant:
                # K times nobj launches of the shift (the gather) and one of the single-variant fusion entry on the variant's
                # slice of the latents -- its object latents moved by ITS offsets (maps), fused with ITS (moved) masks
                vstate = st["v" + mode.kw]
                objs16 = [o.to(self.device, H16).contiguous() for o in fobjs]
                for k in range(st["nvar"]):
                    for j, o in enumerate(objs16):
                        mover(o, vstate[mode.kw + "_dev"][k][j], out=st["fusion_objs"][j])
                    lat = st["latents"][k:k + 1]
                    ops.latent_fusion(lat, bg_latents, st["fusion_objs"], vstate["fusion_masks"][k], mix, rnf, out=lat)
            else:
                for j, o in enumerate(fobjs):
                    if mode is None:
                        st["fusion_objs"][j].copy_(o)
                    else:
                        mover(o.to(self.device, H16).contiguous(), st[moved_by][j], out=st["fusion_objs"][j])
                ops.latent_fusion(st["latents"], bg_latents, st["fusion_objs"], st["fusion_masks"], mix, rnf, out=st["latents"],
                                  nvar=st["nvar"])
            obj_latents = fobjs
        smap = plan_source_map(st.get("classes"), [bg_latents] + list(obj_latents))
        b = st["maps"].get(smap)
        if b is None:
            b = st["maps"][smap] = st["build_map"](smap)
        src = [bg_latents] + list(obj_latents)
        for c, r in enumerate(source_rows(smap, st["n_obj"])):
            b["inp"][c].copy_(src[r][0])
        st["t"].fill_(float(t))
        st["coef"].copy_(table_row)
        register_time_all(self, int(t), st["masks"])
        if not self.use_graphs:
            b["body"]()
            return
        # a captured iteration bakes in EVERY site's injecting decision (the reference allows a schedule per site; with
        # per-variant schedules, DESIGN.md 6j, a site's decision is the bitmask of its injecting variants -- 0 or all bits
        # without them), the device copies of the masks and the batch's source map: all are part of the variant key
        vkey = self.composition_variant_key(st, smap)
        g = st["variants"].get(vkey)
        if g is None:
            g = st["variants"][vkey] = GraphedStep(b["body"], preserve=(st["latents"],))
        g()

    @torch.no_grad()
    def compose_main_frames(self, placed, nvar, n_obj, num_frames, height, width, background_image_list, objs_image_list,
                            obj_mask=None, obj_alpha=None, warp_filter=None, mask_edit=None):
        """the main conditioning frames of the sampling call, composed on the device: the background frames with
        every object's frames alpha-blended over them (later objects in front) under the warps ``collage_warps`` makes of
        ``placed``, at the site (height, width) under the latent grid, sampled by ``warp_filter`` (None: nearest) -> (per variant
        a list of ``num_frames`` RGB images, info).  One kernel launch per DISTINCT warp; variants that share a warp share the
        very same image objects.  ``info``: launches, table_bytes (device bytes of the tap tables), table_rows_host (the
        distinct rows built on the host and uploaded) and seconds (the stage's synchronised wall-clock).
        ``mask_edit`` (``normalize_obj_mask_edit``; None: the call without it): the stacked alphas are edited on the
        device before the collage, in the objects' source coordinates, with the radii times ``vae_scale_factor``; ``info`` then
        carries mask_edit_launches and mask_edit_seconds (inside seconds)."""
        import time
        import numpy as np
        from PIL import Image
        from .utils import mask_alpha_frames
        if not 1 <= n_obj <= ops.COLLAGE_MAX_OBJECTS:
            raise ValueError(f"compose_main_images: {n_obj} objects, the collage takes 1 to {ops.COLLAGE_MAX_OBJECTS}")
        if len(objs_image_list) != n_obj:
            raise ValueError(f"compose_main_images: objs_image_list holds {len(objs_image_list)} clips for {n_obj} objects")
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        bg = _frames_rgb_u8(background_image_list, num_frames, height, width, "background_image_list")
        objs = torch.stack([_frames_rgb_u8(fr, num_frames, height, width, f"objs_image_list[{j}]") for j, fr in enumerate(objs_image_list)])
        if obj_alpha is not None:
            if len(obj_alpha) != n_obj:
                raise ValueError(f"compose_main_images: obj_alpha holds {len(obj_alpha)} arrays for {n_obj} objects")
            alphas = [a.cpu() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)) for a in obj_alpha]
        elif obj_mask is not None:
            alphas = [torch.from_numpy(mask_alpha_frames(p, num_frames)) for p in obj_mask]
        else:
            raise ValueError("compose_main_images=True needs the objects' image-size masks: obj_mask paths or obj_alpha "
                             "(obj_masks_tensors are at latent size)")
        for j, a in enumerate(alphas):
            if a.dtype != torch.uint8 or tuple(a.shape) != (num_frames, height, width):
                raise ValueError(f"compose_main_images: the alpha of object {j} is {a.dtype} {tuple(a.shape)}, the call needs uint8 "
                                 f"[F = {num_frames}, height = {height}, width = {width}]")
        lat_h, lat_w = height // self.vae_scale_factor, width // self.vae_scale_factor
        warps = collage_warps(placed, nvar, n_obj, num_frames, lat_h, lat_w)
        dev = self.device
        bg, objs, alpha = bg.to(dev), objs.contiguous().to(dev), torch.stack(alphas).contiguous().to(dev)
        built, info = {}, {"launches": 0, "table_bytes": 0, "table_rows_host": 0}
        if mask_edit is not None:
            if len(mask_edit) != n_obj:
                raise ValueError(f"compose_main_images: mask_edit holds {len(mask_edit)} edits for {n_obj} objects")
            torch.cuda.synchronize(self.device)
            t1 = time.perf_counter()
            alpha = torch.stack([ops.edit_planes(alpha[j], g, f, self.vae_scale_factor) for j, (g, f) in enumerate(mask_edit)])
            torch.cuda.synchronize(self.device)
            info.update(mask_edit_launches=mask_edit_launches(mask_edit, hard=False), mask_edit_seconds=time.perf_counter() - t1)
        for warp in warps:
            if warp in built:
                continue
            taps = ops.collage_tap_table(warp, height, width, lat_h, lat_w, warp_filter, dev)
            out = ops.collage(bg, objs, alpha, taps).cpu().numpy()
            built[warp] = [Image.fromarray(fr) for fr in out]
            info["launches"] += 1
            info["table_bytes"] += taps.numel() * 4
            info["table_rows_host"] += sum(len(set(tuple(fr) for fr in obj[2])) for obj in warp)
        frames = [built[w] for w in warps]
        info["seconds"] = time.perf_counter() - t0  # (the frames came back through synchronising copies)
        return (frames * nvar if len(frames) == 1 else frames), info

    @torch.no_grad()
    def sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection(
            self, prompt=None, main_first_image=None, main_image_list=None, background_first_image=None,
            background_image_list=None, objs_first_image=None, objs_image_list=None, height=704, width=1280, target_fps=16,
            num_frames=16, num_inference_steps=50, guidance_scale=9.0, negative_prompt=None, eta=0.0,
            num_videos_per_prompt=1, decode_chunk_size=1, generator=None, latents=None, prompt_embeds=None,
            negative_prompt_embeds=None, output_type="pil", return_dict=True, cross_attention_kwargs=None, clip_skip=1,
            fusion_steps=(0, 3), ddim_init_latents_t_idx=1, ddim_inv_prompt=None, obj_mask=None, obj_width_height=None,
            obj_ddim_latents_idx_offset=None, obj_random_noise_fusion=False, random_noise_ratio=0.0,
            bg_inv_latents_path=None, obj_ddim_latents_path=None, obj_masks_tensors=None, obj_offsets=None,
            variant_obj_offsets=None, obj_transforms=None, variant_obj_transforms=None, obj_transform_filter=None,
            obj_mask_edit=None, compose_main_images=False, obj_alpha=None):
        """PnP composition sampling.  ``obj_mask``: list of mask paths (preprocessed by ``mvoc_amd.utils.mask_preprocess``)
        or pass ``obj_masks_tensors`` = list of (float [1,4,F,h,w], bool [1,4,F,h,w]) directly.

        K variants over one set of sources: ``prompt`` / ``negative_prompt`` may be lists, ``generator`` a list
        (one per video; a single generator is drawn K times), ``latents`` [K, 4, F, h, w], ``guidance_scale`` a float or a
        list, ``main_first_image`` a list of images and ``main_image_list`` a list of frame lists; ``num_videos_per_prompt`` =
        m repeats each prompt m times (K = len(prompt) * m).  The sources, masks, schedules and fusion settings are shared; the
        call returns K videos (``frames[k]``).  Scalars mean what they mean in a single composition.

        ``obj_offsets``: one entry per object, ``(dx, dy)`` or ``num_frames`` such pairs (a path), image pixels
        in multiples of 8 -- the object is composed that far from where it sits in its source clip (``normalize_obj_offsets``;
        translation only, shared by the variants, not with a frame shard).  None or all zeros: exactly a call without it.

        ``variant_obj_offsets`` (not together with ``obj_offsets``): a list of K items, one per variant, each None
        or a value ``obj_offsets`` accepts -- variant k composes the objects at ITS offsets over the one set of source chunks.
        All items None / zero: exactly a call without it; all items equal: exactly the ``obj_offsets`` call.

        ``obj_transforms`` (not together with ``obj_offsets`` / ``variant_obj_offsets``): one dict per object with
        the optional keys ``offset`` (an ``obj_offsets`` item), ``scale`` (s or [sx, sy]: int, "p/q" or float; p, q <= 64),
        ``flip`` (None, "h", "v", "hv") and ``anchor`` ([ax, ay], image pixels in multiples of 4; default the frame centre) --
        the object is scaled and mirrored about the anchor (nearest neighbour, exact) and then moved, without re-inverting
        anything (``normalize_obj_transforms``; shared by the variants, not with a frame shard).  ``rotate``: degrees
        counter-clockwise on screen (int, float or "p/q"), or ``num_frames`` of them -- the object is scaled and mirrored about
        its anchor, then turned about it, then moved (nearest, ``resolve_obj_transforms``); 0 / 360 are the call without the key,
        180 the ``flip: "hv"`` call.  Not inside ``variant_obj_transforms``.  Every object at identity:
        exactly a call without it; translation only: exactly the ``obj_offsets`` call.  ``obj_width_height`` stays ignored.

        ``variant_obj_transforms`` (not together with any of the three above): a list of K items, one per variant,
        each None or a value ``obj_transforms`` accepts -- variant k composes the objects under ITS transform over the one set
        of source chunks (``resolve_variant_obj_transforms``).  All items identity: exactly a call without it; all items equal:
        exactly the ``obj_transforms`` call; translations only: exactly the ``variant_obj_offsets`` call.

        ``obj_transform_filter``: None or "nearest" -- exactly the call without it; "bilinear" (with
        ``obj_transforms`` only) -- scaled, mirrored and turned objects are sampled bilinearly (fixed-point weights, an exact fp16
        chain) at every injection site, in the soft masks and in the fusion steps; a translation-only call stays the
        ``obj_offsets`` call, an identity call the call without the argument.

        ``compose_main_images``: True -- ``main_first_image`` and ``main_image_list`` stay None and the call
        builds them on the device: the background frames with the object frames alpha-blended over them under the call's own
        placement (``compose_main_frames``; per variant under ``variant_obj_offsets`` / ``variant_obj_transforms``), sampled by
        ``obj_transform_filter``.  The alphas are the image-size masks behind the ``obj_mask`` paths or ``obj_alpha``, a list of
        uint8 [F, height, width] arrays (for callers that pass ``obj_masks_tensors``).  The frames must be ``width`` x ``height``
        already; not with a frame shard.  The composed frames come back as ``.main_frames`` (per variant a list of images).
        False: exactly the call without the argument.

        ``obj_mask_edit`` (a keyword in front of the two above, whose place at the end is pinned): one dict for all
        objects or one item per object, each None or a dict with the optional keys ``grow`` (an int in [-8, 8] latent pixels,
        negative shrinks) and ``feather`` (an int in [0, 8]) -- the object's masks are grown or shrunk and then feathered
        ONCE, in the object's source coordinates and before any placement moves them (``normalize_obj_mask_edit``,
        ``edit_obj_masks``), so the hooks, the fusion steps, every placement mode and the per-variant stacks see the edited
        masks; under ``compose_main_images`` the alphas are edited the same way with the radii times the VAE factor.  One
        static edit per object, shared by the frames and the variants.  What the stage took comes back as ``.mask_edit_info``
        (launches, seconds).  None or all zeros: exactly the call without the argument."""
        from .utils import mask_preprocess
        n_obj_given = len(obj_ddim_latents_path) if obj_ddim_latents_path is not None else 0
        mask_edit = normalize_obj_mask_edit(obj_mask_edit, n_obj_given)  # refused before any work
        if compose_main_images:
            for name, value in (("main_first_image", main_first_image), ("main_image_list", main_image_list)):
                if value is not None:
                    raise ValueError(f"compose_main_images=True builds {name} from the sources: pass None, not {type(value).__name__}")
            if obj_mask is None and obj_alpha is None:
                raise ValueError("compose_main_images=True needs the objects' image-size masks: obj_mask paths or obj_alpha "
                                 "(obj_masks_tensors are at latent size)")
        # ---- the variants of this call (one with scalar arguments: the batch, kernels and launches of a single composition)
        m_rep = int(num_videos_per_prompt)
        if m_rep < 1:
            raise ValueError(f"num_videos_per_prompt = {num_videos_per_prompt}")
        if prompt_embeds is not None:
            n_prompts = prompt_embeds.shape[0]
            prompts = [None] * (n_prompts * m_rep)
        else:
            plist = list(prompt) if isinstance(prompt, (list, tuple)) else [prompt]
            n_prompts = len(plist)
            prompts = [p for p in plist for _ in range(m_rep)]
        nvar = len(prompts)
        if not 1 <= nvar <= MAX_VARIANTS:
            raise ValueError(f"{nvar} variants (prompts x num_videos_per_prompt): 1 to {MAX_VARIANTS} share one set of sources")
        scalar = lambda v: not isinstance(v, (list, tuple))
        negs = _per_variant(negative_prompt, n_prompts, m_rep, "negative_prompt", scalar)
        scales = [float(g) for g in _per_variant(guidance_scale, n_prompts, m_rep, "guidance_scale", scalar)]
        # (per-variant images come as a LIST of images / of frame lists; anything else is one image / one frame list for all)
        mains_first = _per_variant(main_first_image, n_prompts, m_rep, "main_first_image", lambda v: not isinstance(v, list))
        mains_list = _per_variant(main_image_list, n_prompts, m_rep, "main_image_list",
                                  lambda v: not (isinstance(v, list) and len(v) and isinstance(v[0], list)))
        if isinstance(generator, (list, tuple)):
            if len(generator) != nvar:
                raise ValueError(f"generator: {len(generator)} generators for {nvar} videos")
            gens = list(generator)
        else:
            gens = [generator] * nvar  # one generator: drawn once per video, variant 0 first
        if latents is not None and latents.shape[0] != nvar:
            raise ValueError(f"latents: batch {latents.shape[0]} for {nvar} videos")
        guidance_scale = scales[0]
        if any((g > 1) != (guidance_scale > 1) for g in scales):
            raise ValueError("guidance_scale: guidance is on (> 1) for all variants of a call or off for all")
        self._guidance_scale = guidance_scale
        # guidance_scale <= 1: classifier-free guidance off.  The reference's hooks hard-code the batch of 5
        # (pnp_utils.py:592,747,784,972,1061,1115: `// 5`) and cannot run this; here the batch is [bg, objs.., cond], the
        # injections write the single trailing chunk and the DDIM update takes the conditional prediction as it is
        do_cfg = guidance_scale > 1
        c = self.conditioner
        n_obj = len(obj_ddim_latents_path)
        assert obj_mask is None or len(obj_mask) == n_obj
        if obj_offsets is not None and variant_obj_offsets is not None:
            raise ValueError("obj_offsets and variant_obj_offsets are both given: a call places its objects once for all "
                             "variants or per variant")
        if obj_transforms is not None and (obj_offsets is not None or variant_obj_offsets is not None):
            raise ValueError("obj_transforms is given together with obj_offsets / variant_obj_offsets: a transform carries its "
                             "own offset, and one transform serves all variants")
        if variant_obj_transforms is not None and (obj_transforms is not None or obj_offsets is not None
                                                   or variant_obj_offsets is not None):
            raise ValueError("variant_obj_transforms is given together with obj_transforms / obj_offsets / variant_obj_offsets: "
                             "every variant's transform carries its own offset, and a call transforms per variant or once")
        warp_filter = _transform_filter(obj_transform_filter)
        if warp_filter is not None:
            if obj_offsets is not None or variant_obj_offsets is not None or variant_obj_transforms is not None:
                raise ValueError("obj_transform_filter = 'bilinear' is given together with obj_offsets / variant_obj_offsets / "
                                 "variant_obj_transforms: the filter samples the objects of obj_transforms, one filter for all variants")
            if obj_transforms is None:
                raise ValueError("obj_transform_filter = 'bilinear' is given without obj_transforms: there is nothing to sample")
        placement = normalize_obj_offsets(obj_offsets, n_obj, num_frames, self.vae_scale_factor)
        variant_placements = None
        if variant_obj_offsets is not None:
            placement, variant_placements = resolve_variant_obj_offsets(variant_obj_offsets, nvar, n_obj, num_frames,
                                                                        self.vae_scale_factor)
        transform = warp = None
        if obj_transforms is not None:
            placement, transform, warp = resolve_obj_transforms(obj_transforms, n_obj, num_frames, height // self.vae_scale_factor,
                                                                width // self.vae_scale_factor, self.vae_scale_factor,
                                                                **({} if warp_filter is None else {"interp": warp_filter}))
        variant_transforms = None
        if variant_obj_transforms is not None:
            placement, variant_placements, transform, variant_transforms = resolve_variant_obj_transforms(
                variant_obj_transforms, nvar, n_obj, num_frames, height // self.vae_scale_factor, width // self.vae_scale_factor,
                self.vae_scale_factor)
        placed = {"placement": placement, "variant_placements": variant_placements, "transform": transform,
                  "variant_transforms": variant_transforms, "warp": warp}  # (at most one is not None: each resolver returns one)
        for m in PLACEMENT_MODES:
            if placed[m.attr] is not None and self.unet.shard is not None:
                raise RuntimeError(frame_shard_refusal(m.arg + " do", m.mover))
        main_frames = collage_info = None
        if compose_main_images:
            if self.unet.shard is not None:
                raise RuntimeError(frame_shard_refusal("compose_main_images does", "collage"))
            main_frames, collage_info = self.compose_main_frames(
                placed, nvar, n_obj, num_frames, height, width, background_image_list, objs_image_list, obj_mask, obj_alpha, warp_filter,
                **({} if mask_edit is None else {"mask_edit": mask_edit}))
            # (variants that share a warp hold the SAME objects: one VAE draw and one vision-tower pass below)
            mains_first, mains_list = [fr[0] for fr in main_frames], list(main_frames)
        # source de-duplication: roles showing the same image share ONE draw of the VAE posterior (prepare_image_latents samples
        # per role, :860-890) and one vision-tower pass -- else identical frames would give every role its own image latents and
        # no two roles could share a chunk (make_composition_state)
        dedup = bool(self.dedup_sources)
        memo = {}

        def image_latents(image):
            if not dedup:
                return c.image_latents(image, num_frames, height, width)
            k = SyntheticConditioner._image_key(image)
            if k not in memo:
                memo[k] = c.image_latents(image, num_frames, height, width)
            return memo[k]

        def encode_frames(frames):
            # (a conditioner without the batched entry -- the documented interface is encode_image -- is called per frame)
            return c.encode_images(frames) if hasattr(c, "encode_images") else torch.cat([c.encode_image(f) for f in frames])
        # conditioning, assembled in the reference's batch order [bg, obj_1.., uncond, cond] (:1387, 1476, 1498, 1540)
        # (variants: the sources and variant 0 draw in the order of a single composition, the other variants after)
        if prompt_embeds is not None:
            pes = list(prompt_embeds.repeat_interleave(m_rep, 0).split(1))
            nes = list(negative_prompt_embeds.repeat_interleave(m_rep, 0).split(1)) if negative_prompt_embeds is not None else [None] * nvar
            pe, ne = pes[0], nes[0]
        else:
            pe, ne = c.encode_prompt(prompts[0], negs[0])
            pes, nes = [pe], [ne]
        inv_pe, _ = c.encode_prompt(ddim_inv_prompt, negs[0])
        main_first_image, main_image_list = mains_first[0], mains_list[0]
        main_lat = image_latents(main_first_image)
        bg_lat = image_latents(background_first_image)
        obj_first = [image_latents(im) for im in objs_first_image]
        obj_lat = [image_latents(frames[0]) for frames in objs_image_list]
        bg_lat2 = image_latents(background_image_list[0])

        # every conditioning frame of the job (background, objects, main: 4 x 16 in the demo) through the vision tower at once
        lists = [background_image_list] + list(objs_image_list) + [main_image_list]
        allf = [f for fr in lists for f in fr]
        if dedup:  # each distinct frame once, then gathered back into every list that shows it
            keys = [SyntheticConditioner._image_key(f) for f in allf]
            uniq = {}
            for k, f in zip(keys, allf):
                uniq.setdefault(k, f)
            pos = {k: i for i, k in enumerate(uniq)}
            uflat = encode_frames(list(uniq.values()))
            flat = uflat[torch.tensor([pos[k] for k in keys], device=uflat.device)]
        else:
            flat = encode_frames(allf)  # [sum F, 1, 1024]
        embs, o = [], 0
        for fr in lists:
            embs.append(flat[o:o + len(fr)].transpose(0, 1))  # [1, F, 1024]
            o += len(fr)
        main_emb = embs[-1]
        main_lats, main_embs = [main_lat], [main_emb]
        for k in range(1, nvar):  # a variant that shows variant 0's main image shares its draw and its vision-tower pass
            if prompt_embeds is None:
                pk, nk = c.encode_prompt(prompts[k], negs[k])
                pes.append(pk), nes.append(nk)
            main_lats.append(main_lat if mains_first[k] is main_first_image else image_latents(mains_first[k]))
            main_embs.append(main_emb if mains_list[k] is main_image_list
                             else encode_frames(list(mains_list[k])).transpose(0, 1))
        ndst = 2 if do_cfg else 1
        # batch order [bg, obj_1.., u_1..u_K, c_1..c_K] (variant_layout; K = 1: the reference's [bg, obj_1.., uncond, cond])
        ehs = torch.cat([inv_pe.repeat(n_obj + 1, 1, 1)] + (nes if do_cfg else []) + pes)
        first_all = torch.cat([bg_lat] + obj_first + main_lats * ndst)
        lat_all = torch.cat([bg_lat2] + obj_lat + main_lats * ndst)
        emb_all = torch.cat(embs[:-1] + ([torch.zeros_like(e) for e in main_embs] if do_cfg else []) + main_embs)
        fps = torch.full((n_obj + 1 + ndst * nvar,), float(target_fps), dtype=torch.float32, device=self.device)
        cond = dict(encoder_hidden_states=ehs.to(self.device, H16).contiguous(), image_embeddings=emb_all.to(self.device, H16).contiguous(),
                    image_latents_first=first_all.to(self.device, H16).contiguous(), image_latents=lat_all.to(self.device, H16).contiguous(), fps=fps)

        sched = self.scheduler
        sched.set_timesteps(num_inference_steps, device=self.device)
        full = deepcopy(sched)
        sched.timesteps = sched.timesteps[ddim_init_latents_t_idx:]
        offs = obj_ddim_latents_idx_offset or [0] * n_obj
        fusion_ts = [[int(full.timesteps[offs[j]:][k]) for k in range(*fusion_steps)] for j in range(n_obj)]
        latents = torch.cat([self.prepare_latents(1, 4, num_frames, height, width, H16, self.device, gens[k],
                                                  None if latents is None else latents[k:k + 1]) for k in range(nvar)])
        if obj_masks_tensors is None:
            obj_masks_tensors = [mask_preprocess(m, self.device, H16, 1, 4, num_frames, downscale=8) for m in obj_mask]
        mask_edit_info = {"launches": 0, "seconds": 0.0}
        if mask_edit is not None:  # once, in source coordinates: everything downstream sees the edited masks
            import time
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            obj_masks_tensors = edit_obj_masks([(s.to(self.device), h.to(self.device)) for s, h in obj_masks_tensors], mask_edit)
            torch.cuda.synchronize(self.device)
            extra = collage_info or {}
            mask_edit_info = {"launches": mask_edit_launches(mask_edit) + extra.get("mask_edit_launches", 0),
                              "seconds": time.perf_counter() - t0 + extra.get("mask_edit_seconds", 0.0)}
        self.unet.check_variant_schedules(nvar)  # per-variant injection schedules are hook state (pnp_utils): one entry per variant
        st = self.make_composition_state(latents, cond, obj_masks_tensors, scales if nvar > 1 else guidance_scale, variants=nvar,
                                         **{attr: value for attr, value in placed.items() if value is not None},
                                         **({"obj_transform_filter": warp_filter} if warp_filter is not None and warp is not None else {}))
        table, index = sched.coef_table(self.device, guidance_scale)
        if nvar > 1:  # [steps, K, 5]: a step's coefficient rows are one view, whatever K is
            table = torch.stack([sched.coef_table(self.device, g)[0] for g in scales], 1).contiguous()
            nb = st["nb"]
            if crosses_gemm_offset_line(nb, num_frames, latents.shape[-2], latents.shape[-1], self.unet.config.block_out_channels[0]) \
                    and not getattr(self, "_warned_gemm_line", False):
                self._warned_gemm_line = True
                logger.warning("composition of %d variants: UNet batch %d puts the widest level-0 tensor at 2 GB or more; the "
                               "eight-phase GEMM tiles (32-bit offsets) step aside for the general tiles there (DESIGN.md 6i)",
                               nvar, nb)
        cache = self.latent_cache
        fusion_counter = 0  # never incremented in the reference (:1634, 1649)
        for i, t in enumerate(sched.timesteps):
            t = int(t)
            bg = cache.get(bg_inv_latents_path, t)
            fuse = None
            if fusion_steps[0] <= i < fusion_steps[1]:
                fobjs = [cache.get(obj_ddim_latents_path[j], fusion_ts[j][fusion_counter]) for j in range(n_obj)]
                fuse = (random_noise_ratio, obj_random_noise_fusion, fobjs)
                objs = fobjs
            else:
                objs = [cache.get(obj_ddim_latents_path[j], t) for j in range(n_obj)]
            self.composition_step(st, t, bg, objs, table[index[t]], fuse)
        latents = st["latents"].clone()
        frames = latents if output_type == "latent" else self._to_video(latents, output_type)
        return PipelineOutput(frames=frames, main_frames=main_frames, collage_info=collage_info,
                              mask_edit_info=mask_edit_info) if return_dict else (frames,)
