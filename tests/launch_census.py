"""Launch census of the headline step and of the stages around it: VAE, CLIP towers, mask path (helper module, not collected by pytest).

Three parts:
  * ``Recorder``: installed as ``lib`` of ``mvoc_amd.ops`` (and of the other modules that hold the library) for the duration of a recording.  It copies the descriptor (or the scalar and
    pointer arguments) of every call of the entry points in ``DESC_ENTRIES`` / ``ARG_ENTRIES``, counts every other ``mvoc_*`` call
    by name, and calls through.  It does no device work and no synchronisation, so it can sit inside a hipGraph capture.
  * ``build_*``: a replay of one recorded call on fresh buffers that the test allocates and fills itself.  Every operand is sized
    from the descriptor's own extents and placed at the recorded address mod 256; every pointer field is rewritten, and a pointer
    field the builder does not know fails on the host before anything is launched.  Weights are drawn in their logical form and
    packed by the product's own packers, so a packing bug is caught with the kernel.
  * ``*_ref``: float64 restatements of the contracts in include/mvoc_hip.h.  They work on tensors (CPU or GPU) and take the
    LOGICAL weights, never the packed ones.
"""
import ctypes as C
import math
from collections import Counter

import torch

from mvoc_amd import _ffi
from mvoc_amd._ffi import (A_CONV3X3, A_PLAIN, A_TEMPORAL3, ACT_GEGLU, ACT_GELU, ACT_NONE, ACT_SILU, AttnDesc, GemmDesc, GnDesc,
                           TAttnDesc, TFusedDesc, XsDesc)

H16, F32, F64 = torch.float16, torch.float32, torch.float64

# entry points whose calls are recorded and replayed: name -> descriptor type
DESC_ENTRIES = {
    "mvoc_gemm_f16": GemmDesc,
    "mvoc_xs_linear_f16": XsDesc,
    "mvoc_flash_attn_f16": AttnDesc,
    "mvoc_temporal_qkv_attn_f16": TFusedDesc,
    "mvoc_temporal_attn_f16": TAttnDesc,
    "mvoc_groupnorm_f16": GnDesc,
    "mvoc_groupnorm_fold_xs_f16": GnDesc,
}
# entry points with plain arguments: name -> argument names after the descriptor (fold) or all of them (stream excluded)
ARG_ENTRIES = {
    "mvoc_groupnorm_fold_xs_f16": ("w", "bias", "n", "k", "wp_sets"),
    "mvoc_row_stats_f16": ("x", "stats", "rows", "c", "eps"),
    "mvoc_row_stats_from_moments_f32": ("moments", "rows", "ld", "n", "tile_w", "eps", "out"),
    "mvoc_layernorm_f16": ("x", "gamma", "beta", "out", "rows", "c", "eps"),
    # stem.hip / norm.hip entries of the VAE, the CLIP towers and the mask path (argument names of include/mvoc_hip.h)
    "mvoc_conv3x3_small_f16": ("x", "w", "bias", "out", "nimg", "h", "wd", "cin", "cout", "stride", "silu"),
    "mvoc_conv1x1_small_f16": ("x", "w", "bias", "out", "rows", "cin", "cout"),
    "mvoc_softmax_rows_f16": ("x", "rows", "cols"),
    "mvoc_image_to_tokens_f16": ("x", "out", "n", "c", "hw"),
    "mvoc_tokens_to_image_f16": ("x", "out", "n", "c", "hw", "ld"),
    "mvoc_gaussian_sample_f16": ("mean", "logvar", "noise", "out", "n"),
    "mvoc_scale_f16": ("x", "out", "n", "scale"),
    "mvoc_clip_patches_f16": ("pixels", "out", "nimg", "size", "patch", "kpad"),
    "mvoc_clip_embed_f16": ("table", "ids", "cls", "pos", "out", "rows", "t", "c"),
    "mvoc_mask_resize_u8": ("in", "tmp", "out", "n", "H", "W", "h", "w", "bounds_h", "kk_h", "ksize_h", "bounds_v", "kk_v", "ksize_v"),
    "mvoc_mask_finish": ("v", "float_mask", "bool_mask", "n"),
}
STEM_ENTRIES = ("mvoc_conv3x3_small_f16", "mvoc_conv1x1_small_f16", "mvoc_softmax_rows_f16", "mvoc_image_to_tokens_f16",
                "mvoc_tokens_to_image_f16", "mvoc_gaussian_sample_f16", "mvoc_scale_f16", "mvoc_clip_patches_f16", "mvoc_clip_embed_f16",
                "mvoc_mask_resize_u8", "mvoc_mask_finish")
RECORDED = tuple(DESC_ENTRIES) + tuple(n for n in ARG_ENTRIES if n not in DESC_ENTRIES)
FAMILY = {"mvoc_gemm_f16": "gemm", "mvoc_xs_linear_f16": "xs_linear", "mvoc_flash_attn_f16": "flash_attn",
          "mvoc_temporal_qkv_attn_f16": "tfused", "mvoc_temporal_attn_f16": "temporal_attn", "mvoc_groupnorm_f16": "groupnorm",
          "mvoc_groupnorm_fold_xs_f16": "groupnorm_fold_xs", "mvoc_row_stats_f16": "row_stats",
          "mvoc_row_stats_from_moments_f32": "row_stats_from_moments", "mvoc_layernorm_f16": "layernorm"}
FAMILY.update({n: n[len("mvoc_"):].replace("_f16", "") for n in STEM_ENTRIES})
# the modules that hold a reference to the library of their own (`from ._ffi import lib`): the recorder stands in for each of them
LIB_HOLDERS = ("mvoc_amd.ops", "mvoc_amd.vae", "mvoc_amd.clip", "mvoc_amd._ffi")

# the bounds of the families that are not bit-exact: (rel-L2, max abs) against fp64, those of the per-op tests in test_ops_gpu.py
FLASH_BOUND = (2e-3, 1e-2)      # test_flash_attn
GN_BOUND = (2e-3, 1.5e-2)       # test_groupnorm
LN_BOUND = (1e-3, 1e-2)         # test_layernorm


def _is_ptr_type(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def _arg_is_ptr(name, i):
    """argument i (0-based, descriptor excluded for the descriptor entries) of entry `name` is a pointer"""
    argtypes = _ffi.SIGNATURES[name][1]
    off = 1 if name in DESC_ENTRIES else 0
    return _is_ptr_type(argtypes[off + i])


def ptr_key(v):
    """what the auto dispatch can see of a pointer: whether it is NULL, and its alignment"""
    v = int(v or 0)
    return (v != 0, v % 256)


def desc_key(d):
    """every scalar field, and (is set, address mod 256) of every pointer field"""
    return tuple((name, ptr_key(getattr(d, name)) if _is_ptr_type(typ) else getattr(d, name)) for name, typ in d._fields_)


def copy_desc(d):
    dd = type(d)()
    C.memmove(C.byref(dd), C.byref(d), C.sizeof(d))
    return dd


class Launch:
    """one recorded call: the entry's name, a copy of its descriptor (or None) and its plain arguments by name"""

    def __init__(self, name, desc, args):
        self.name, self.desc, self.args = name, desc, args

    @property
    def key(self):
        ak = tuple((k, ptr_key(v) if isinstance(v, _Ptr) else v) for k, v in self.args.items())
        return (self.name, desc_key(self.desc) if self.desc is not None else (), ak)


class _Ptr(int):
    """a recorded pointer argument (an address: only its alignment is ever used)"""


class _Proxy:
    def __init__(self, rec, lib):
        self._rec, self._lib = rec, lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mvoc_"):
            return fn
        rec = self._rec

        def call(*args):
            rec.note(name, args)
            if rec.dry and name in RECORDED:
                return 0  # descriptor taken, nothing launched
            return fn(*args)
        return call


class Recorder:
    """``rec.install()`` puts the proxy in place of ``lib`` in ``mvoc_amd.ops`` and in the other modules that hold the library
    (LIB_HOLDERS); ``rec.uninstall()`` (always, in a ``finally``) restores them.  ``dry``: the recorded entries are noted and
    return 0 without launching (descriptors of extents the caller does not want to run on uninitialised buffers)."""

    def __init__(self, dry=False):
        self.calls = Counter()      # every mvoc_* call by name
        self.launches = {}          # key -> [Launch, count]
        self.dry = dry
        self._orig = None

    def install(self):
        import importlib
        from mvoc_amd import ops
        assert self._orig is None and not isinstance(ops.lib, _Proxy), "a recorder is already installed"
        self._orig = {}
        for name in LIB_HOLDERS:
            mod = importlib.import_module(name)
            self._orig[name] = (mod, mod.lib)
            mod.lib = _Proxy(self, mod.lib)

    def uninstall(self):
        if self._orig is not None:
            for mod, lib in self._orig.values():
                mod.lib = lib
            self._orig = None

    def note(self, name, args):
        self.calls[name] += 1
        if name not in RECORDED:
            return
        desc, rest = None, args
        if name in DESC_ENTRIES:
            p = args[0]
            obj = getattr(p, "_obj", None)  # C.byref(desc)
            if obj is None:
                obj = C.cast(p, C.POINTER(DESC_ENTRIES[name])).contents
            desc, rest = copy_desc(obj), args[1:]
        names = ARG_ENTRIES.get(name, ())
        vals = {}
        for i, an in enumerate(names):
            v = rest[i]
            vals[an] = _Ptr(int(v or 0)) if _arg_is_ptr(name, i) else (float(v) if isinstance(v, float) else int(v))
        ln = Launch(name, desc, vals)
        k = ln.key
        if k in self.launches:
            self.launches[k][1] += 1
        else:
            self.launches[k] = [ln, 1]

    def by_family(self):
        out = {}
        for ln, cnt in self.launches.values():
            out.setdefault(FAMILY[ln.name], []).append((ln, cnt))
        return out


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
SLACK_BYTES = 64 << 10  # past every operand's extent: a kernel that strays a little reads zeros and its stray writes are seen


def alloc(numel, dtype, addr_mod, device, fill=0.0):
    """a 1-D view of `numel` elements whose address is `addr_mod` mod 256, in a larger allocation (slack after it)"""
    es = torch.empty((), dtype=dtype).element_size()
    if addr_mod % es:
        raise ValueError(f"address mod 256 = {addr_mod} is not aligned to the {es}-byte element")
    base = torch.full((int(numel) + (256 + SLACK_BYTES) // es,), fill, dtype=dtype, device=device)
    off = ((addr_mod - base.data_ptr() % 256) % 256) // es
    v = base[off:off + int(numel)]
    assert v.data_ptr() % 256 == addr_mod
    v.base_alloc = base
    return v


def rewrite(d, bufs):
    """set every pointer field of `d` from `bufs` (name -> tensor); a field recorded non-NULL that `bufs` lacks is an error, raised
    before any launch: a replay never launches with a recorded address"""
    for name, typ in d._fields_:
        if not _is_ptr_type(typ):
            continue
        was = getattr(d, name)
        if name in bufs and bufs[name] is not None:
            if not was:
                raise RuntimeError(f"replay builder supplies `{name}`, which the recorded call left NULL")
            setattr(d, name, bufs[name].data_ptr())
        elif was:
            raise RuntimeError(f"replay builder has no buffer for the recorded pointer field `{name}` ({type(d).__name__})")
    return d


def _ints(shape, gen, device, lo=-1, hi=1, dtype=H16):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=device, dtype=torch.int16).to(dtype)


def _ints_sparse(shape, gen, device):
    """integers in [-1, 1] with about half of them zero (keeps every |sum| far inside the fp16-exact range)"""
    w = _ints(shape, gen, device)
    keep = torch.rand(tuple(shape), generator=gen, device=device) < 0.5
    return w * keep.to(w.dtype)


def r16(x):
    """one fp16 rounding point of the eager chain (the kernels round fp32 -> fp16 with RNE; exact values round identically)"""
    return x.to(H16).to(x.dtype)


def ulp16(x):
    """one fp16 ulp at |x| (subnormal spacing 2^-24 below 2^-14)"""
    a = x.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def silu64(x):
    return x / (1.0 + torch.exp(-x))


# Bound of an fp32 activation against its fp64 value.  The kernels evaluate GELU with Abramowitz-Stegun 7.1.26 (|erf error| <= 1.5e-7)
# in fp32 (common.h: gelu_fast_f): |gelu32(x) - gelu(x)| <= 0.5 |x| (1.5e-7 + three fp32 roundings of values <= 1, 6e-8 each) plus the
# rounding of the product (2^-24 of a result <= |x|) = 2.8e-7 |x| < 2^-21 |x| (test_launch_census_cpu: test_activation_bound_derivation
# measures 2.65e-7 |x| at most).  Where gelu(x) is tiny (x <= -4) that absolute error is many fp16 ulps of the result, so it is a term of
# its own.  SiLU (v_exp + v_rcp, relative error a few fp32 ulps, no cancellation) needs no such term: its rounding flip is one ulp.
GELU_ABS = 2.0 ** -21


def act_bound(x, act):
    """|act32(x) - act64(x)| beyond the rounding flip (which the caller's ulp terms cover)"""
    return GELU_ABS * x.abs() if act == ACT_GELU else torch.zeros_like(x)


# ---- GEMM: extents, replay, reference -----------------------------------------------------------------------------------------------
def gemm_out_cols(d):
    return d.n // 2 if d.act == ACT_GEGLU else (d.n_store if d.n_store else d.n)


def gemm_rows_a(d):
    return d.nimg * d.hsrc * d.wsrc if d.a_mode == A_CONV3X3 else d.m


def gemm_w_rows(d):
    return 4 * d.n if (d.a_mode == A_CONV3X3 and d.upsample == 2) else d.n


def gemm_extents(d):
    """element counts of every operand the descriptor reaches (the `need` of tools/gemm_shapes_pmc.py, for every pointer field):
    name -> (numel, dtype)"""
    rows_a = gemm_rows_a(d)
    cols = gemm_out_cols(d)
    ext = {
        "a": (rows_a * max(d.lda, 1), H16),
        "a2": (rows_a * max(d.lda2, 1), H16),
        "w": (gemm_w_rows(d) * d.k, H16),
        "out": (d.m * d.ldo, H16),
        "bias": (d.n, H16),
        "rowadd": (-(-d.m // max(d.rowadd_div, 1)) * max(d.ld_rowadd, 1), H16),
        "resid": (d.m * max(d.ldr, 1), H16),
        "workspace": (d.workspace_bytes // 4, F32),
        "ln_rowsum": (d.n, F32),
        "ln_bias": (d.n, F32),
        "ln_stats": (d.m * 2, F32),
        "chan_sums": ((d.m // 256) * cols * 2, F32),
        "row_moments": (d.m * max(d.row_moments_ld, 1) * 2, F32),
    }
    return ext


def chunk_major_ref(w, ntaps):
    """the k_order = 1 permutation written out (include/mvoc_hip.h): k = (c / 64) * ntaps * 64 + tap * 64 + c % 64"""
    n, k = w.shape
    cin = k // ntaps
    out = torch.empty_like(w)
    for c0 in range(0, cin, 64):
        for t in range(ntaps):
            out[:, (c0 // 64) * ntaps * 64 + t * 64:(c0 // 64) * ntaps * 64 + (t + 1) * 64] = w[:, t * cin + c0:t * cin + c0 + 64]
    return out


def gemm_logical_weights(d, gen, device):
    """logical weights of the descriptor's operation (ints in [-1, 1], about half zero), their packed form through the product's
    packers, and the logical bias / LayerNorm vectors.  Returns (packed tensors by field, logical dict)."""
    from mvoc_amd import ops
    from mvoc_amd.unet import pack_conv3x3, pack_conv3x3_subpixel, pack_geglu, pack_tconv
    L, P = {}, {}
    n = d.n
    if d.act == ACT_GEGLU and (d.a_mode != A_PLAIN or d.rowadd):
        raise RuntimeError("GEGLU replay is written for plain launches without a row-add")
    if d.a_mode == A_PLAIN:
        wl = _ints_sparse((n, d.k), gen, device)
        L["w"] = wl
    elif d.a_mode == A_CONV3X3:
        wl = _ints_sparse((n, d.cin, 3, 3), gen, device)
        L["w"] = wl
        if d.upsample == 2:
            wp = pack_conv3x3_subpixel(wl)
        else:
            wp = pack_conv3x3(wl)
            if d.k_order == 1:
                cm = ops.chunk_major_weights(wp, 9)
                if not torch.equal(cm, chunk_major_ref(wp, 9)):
                    raise AssertionError("ops.chunk_major_weights differs from the k_order = 1 permutation of include/mvoc_hip.h")
                wp = cm
    elif d.a_mode == A_TEMPORAL3:
        wl = _ints_sparse((n, d.cin, 3, 1, 1), gen, device)
        L["w"] = wl
        wp = pack_tconv(wl)
        if d.k_order == 1:
            cm = ops.chunk_major_weights(wp, 3)
            if not torch.equal(cm, chunk_major_ref(wp, 3)):
                raise AssertionError("ops.chunk_major_weights differs from the k_order = 1 permutation of include/mvoc_hip.h")
            wp = cm
    else:
        raise RuntimeError(f"unknown a_mode {d.a_mode}")
    L["bias"] = _ints((n,), gen, device, -4, 4)
    if d.ln_rowsum:
        L["ln_rowsum"] = (wl.reshape(n, -1).double().sum(1)).to(F32)  # a contract input: any fp32 vector; the weights' sums here
        L["ln_bias"] = _ints((n,), gen, device, -4, 4, F32)
    if d.a_mode == A_PLAIN:
        if d.act == ACT_GEGLU:
            wp, bp = pack_geglu(wl, L["bias"])
            P["bias"] = bp
            if d.ln_rowsum:
                P["ln_rowsum"] = pack_geglu(wl, L["ln_rowsum"])[1]
                P["ln_bias"] = pack_geglu(wl, L["ln_bias"])[1]
        else:
            wp = wl
    P.setdefault("bias", L["bias"])
    if d.ln_rowsum:
        P.setdefault("ln_rowsum", L["ln_rowsum"])
        P.setdefault("ln_bias", L["ln_bias"])
    P["w"] = wp.contiguous()
    if tuple(P["w"].shape) != (gemm_w_rows(d), d.k):
        raise RuntimeError(f"packed weights {tuple(P['w'].shape)} do not match the descriptor's [{gemm_w_rows(d)}, {d.k}]")
    return P, L


OUT_SENTINEL = 0x7E5A  # an fp16 NaN no kernel produces: untouched output bytes keep it


def build_gemm(d0, device, seed, workspace_bytes_fn=None):
    """a replay of a recorded mvoc_gemm_f16 descriptor: (descriptor with rewritten pointers, buffers by field, logical operands)"""
    d = copy_desc(d0)
    gen = torch.Generator(device=device).manual_seed(seed)
    ext = gemm_extents(d)
    bufs = {}
    for name, (numel, dt) in ext.items():
        v = getattr(d, name)
        if not v:
            continue
        bufs[name] = alloc(numel, dt, int(v) % 256, device)
    P, L = gemm_logical_weights(d, gen, device)
    for name in ("a", "a2", "rowadd", "resid"):
        if name in bufs:
            bufs[name].copy_(_ints(bufs[name].shape, gen, device, *((-1, 1) if name in ("a", "a2") else (-4, 4))))
    for name in ("w", "bias", "ln_rowsum", "ln_bias"):
        if name in bufs:
            src = P[name].reshape(-1)
            if src.numel() != bufs[name].numel():
                raise RuntimeError(f"`{name}`: packed {src.numel()} elements, the descriptor reaches {bufs[name].numel()}")
            bufs[name].copy_(src)
    if "ln_stats" in bufs:  # test-supplied {mean, rstd}: dyadic, so the folded epilogue is exact in fp32
        mean = _ints((d.m,), gen, device, -2, 2, F32) * 0.5
        rstd = torch.exp2(-_ints((d.m,), gen, device, 0, 2, F32))
        bufs["ln_stats"].copy_(torch.stack([mean, rstd], 1).reshape(-1))
    if "workspace" in bufs:
        # the workspace ops._gemm attaches when the recorded call had one
        from mvoc_amd._ffi import lib
        nb = (workspace_bytes_fn or lib.mvoc_gemm_workspace_bytes)(d.m, d.n, d.k)
        if nb != d.workspace_bytes:
            raise RuntimeError(f"recorded workspace_bytes {d.workspace_bytes} != mvoc_gemm_workspace_bytes {nb}")
    if "out" in bufs:
        bufs["out"].base_alloc.view(torch.int16).fill_(OUT_SENTINEL)
    rewrite(d, bufs)
    return d, bufs, L


def apply_image_multipliers(d, bufs, L, mult):
    """the large-extent pattern: image i of the activation := image 0 times the integer mult[i]; bias (and the logical bias) zero, so
    that the output of image i is mult[i] times image 0's, exactly (fp32 sums of small integers)"""
    nimg = len(mult)
    if d.a2 or d.resid or d.rowadd or d.ln_rowsum or d.act != ACT_NONE or gemm_rows_a(d) % nimg or d.m % nimg:
        raise RuntimeError("the multiplier pattern is written for single-source launches with a plain epilogue")
    a = bufs["a"].reshape(nimg, -1)
    m = torch.tensor(mult, dtype=H16, device=a.device)[:, None]
    step = 4
    if mult[0] != 1:
        raise RuntimeError("image 0 is the unscaled one")
    for i0 in range(1, nimg, step):
        a[i0:i0 + step] = a[0:1] * m[i0:i0 + step]
    if "bias" in bufs:
        bufs["bias"].zero_()
    L["bias"] = torch.zeros_like(L["bias"])


IMAGE_MULT = (1, -1, 2, -2)  # exact in fp16 and in every fp32 sum; neighbouring images differ, so does every pair less than 4 apart


def image_multipliers(nimg):
    return [IMAGE_MULT[i % 4] for i in range(nimg)]


def nearest_index(n_out, n_in, device):
    """F.interpolate(mode='nearest', size=...) source index: floor(dst * (in / out)) in fp32, clamped"""
    s = torch.tensor(n_in / n_out, dtype=F32)
    return (torch.arange(n_out, dtype=F32) * s).floor().long().clamp(max=n_in - 1).to(device)


def gemm_row_unit(d):
    if d.a_mode == A_CONV3X3:
        return d.hout * d.wout
    if d.a_mode == A_TEMPORAL3:
        return d.frames * d.hw
    return 1


def gemm_blocks(d, budget=1 << 26):
    """output row blocks [r0, r1) for the reference, whole images / videos, each a few hundred MB of fp64 at most"""
    unit = gemm_row_unit(d)
    width = max(d.cin * (9 if d.a_mode == A_CONV3X3 else 3 if d.a_mode == A_TEMPORAL3 else 1), d.k, d.n)
    if d.a_mode == A_CONV3X3:
        width = max(width, d.cin * (d.hup + 2) * (d.wup + 2) // max(d.hout * d.wout, 1) * 2)
    per = max(unit, (budget // width) // unit * unit)
    return [(r0, min(d.m, r0 + per)) for r0 in range(0, d.m, per)]


def gemm_acc(d, T, L, r0, r1):
    """fp64 sum_k A(m, k) W(n, k) for output rows [r0, r1), logical weights, all n rows"""
    dev = T["a"].device
    if d.a_mode == A_PLAIN:
        return _a_rows_range(d, T, r0, r1) @ L["w"].to(F64).t()
    wl = L["w"].to(F64)
    if d.a_mode == A_TEMPORAL3:
        per = d.frames * d.hw
        v0, v1 = r0 // per, r1 // per
        x = _a_rows_range(d, T, v0 * per, v1 * per).reshape(v1 - v0, d.frames, d.hw, d.cin)
        xp = torch.nn.functional.pad(x, (0, 0, 0, 0, 1, 1))
        acc = 0
        for t in range(3):
            acc = acc + xp[:, t:t + d.frames].reshape(-1, d.cin) @ wl[:, :, t, 0, 0].t()
        return acc
    # conv3x3: gather the (upsampled) source of whole images, pad, nine shifted slabs
    per_o = d.hout * d.wout
    i0, i1 = r0 // per_o, r1 // per_o
    per_s = d.hsrc * d.wsrc
    x = _a_rows_range(d, T, i0 * per_s, i1 * per_s).reshape(i1 - i0, d.hsrc, d.wsrc, d.cin)
    if d.upsample:
        x = x.index_select(1, nearest_index(d.hup, d.hsrc, dev)).index_select(2, nearest_index(d.wup, d.wsrc, dev))
    hu, wu = x.shape[1], x.shape[2]
    if d.pad_mode == 0:
        xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    else:
        xp = torch.nn.functional.pad(x, (0, 0, 0, 1, 0, 1))
    s = max(d.stride, 1)
    acc = 0
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, ky:ky + s * (d.hout - 1) + 1:s, kx:kx + s * (d.wout - 1) + 1:s]
            assert sl.shape[1] == d.hout and sl.shape[2] == d.wout, (sl.shape, hu, wu)
            acc = acc + sl.reshape(-1, d.cin) @ wl[:, :, ky, kx].t()
    return acc


def _a_rows_range(d, T, s0, s1):
    a = T["a"].reshape(-1)
    parts = [a[s0 * d.lda:s1 * d.lda].reshape(s1 - s0, d.lda)[:, :d.c1]]
    cin = d.cin if d.a_mode != A_PLAIN else d.k
    if cin > d.c1:
        parts.append(T["a2"].reshape(-1)[s0 * d.lda2:s1 * d.lda2].reshape(s1 - s0, d.lda2)[:, :cin - d.c1])
    return torch.cat([p.to(F64) for p in parts], 1)


def gemm_epilogue(d, acc, T, L, r0, r1):
    """the eager chain's rounding points on the fp64 accumulator: returns (stored values [rows, cols], bound [rows, cols] of the
    kernel's deviation: 0 where every step is exact)"""
    rows = r1 - r0
    n = d.n
    if d.ln_rowsum:
        st = T["ln_stats"].reshape(-1)[2 * r0:2 * r1].reshape(rows, 2).to(F64)
        y = st[:, 1:2] * (acc - st[:, 0:1] * L["ln_rowsum"].to(F64)[None, :]) + L["ln_bias"].to(F64)[None, :]
    else:
        y = acc + (L["bias"].to(F64)[None, :] if d.bias else 0)
    if d.act == ACT_GEGLU:
        inner = n // 2
        hv, gv = r16(y[:, :inner]), r16(y[:, inner:])
        g64 = gelu64(gv)
        gl = r16(g64)
        out = r16(hv * gl)
        # the kernel's r16(gelu32(gv)) may sit one fp16 ulp of gl away (rounding flip) plus the fp32 evaluation error (GELU_ABS)
        bound = ulp16(out) + hv.abs() * (ulp16(gl) + GELU_ABS * gv.abs())
        if d.resid:
            rr = T["resid"].reshape(-1)[r0 * d.ldr:r1 * d.ldr].reshape(rows, d.ldr)[:, :inner].to(F64)
            out = r16(out + rr)
            bound = bound + ulp16(out)
        return out, bound
    v = r16(y)
    if d.rowadd:
        ridx = torch.arange(r0, r1, device=acc.device) // d.rowadd_div
        cr = min(n, d.ld_rowadd)  # (the columns past the row-add's width are never stored)
        ra = T["rowadd"].reshape(-1).reshape(-1, d.ld_rowadd)[:, :cr].index_select(0, ridx).to(F64)
        v = v.clone()
        v[:, :cr] = r16(v[:, :cr] + ra)
    bound = torch.zeros_like(v)
    if d.act in (ACT_SILU, ACT_GELU):
        a64 = silu64(v) if d.act == ACT_SILU else gelu64(v)
        bound = ulp16(a64) + act_bound(v, d.act)
        v = r16(a64)
    cols = gemm_out_cols(d)
    v, bound = v[:, :cols], bound[:, :cols]
    if d.resid:
        rr = T["resid"].reshape(-1)[r0 * d.ldr:r1 * d.ldr].reshape(rows, d.ldr)[:, :cols].to(F64)
        v = r16(v + rr)
        if d.act != ACT_NONE:
            bound = bound + ulp16(v)
    return v, bound


def gemm_ref(d, T, L, r0=0, r1=None):
    """fp64 restatement of mvoc_gemm_f16 for output rows [r0, r1): (stored values, deviation bound)"""
    r1 = d.m if r1 is None else r1
    return gemm_epilogue(d, gemm_acc(d, T, L, r0, r1), T, L, r0, r1)


def stored_rows(d, bufs, r0, r1):
    cols = gemm_out_cols(d)
    return bufs["out"].reshape(-1)[r0 * d.ldo:r1 * d.ldo].reshape(r1 - r0, d.ldo)[:, :cols]


# ---- xs_linear ----------------------------------------------------------------------------------------------------------------------
def xs_extents(d):
    nsets = d.m // d.wp_set_rows if d.wp_set_rows else 1
    cols = d.n // 2 if d.act == ACT_GEGLU else (d.n_store or d.n)
    return {"x": (d.m * d.k, H16), "wp": (nsets * (d.n // 32) * (d.k // 16 + 1) * 512, H16),
            "out": (d.m * d.ldo, H16), "resid": (d.m * max(d.ldr, 1), H16)}, cols


def build_xs(d0, device, seed):
    from mvoc_amd.unet import pack_geglu, pack_xs_weights
    d = copy_desc(d0)
    gen = torch.Generator(device=device).manual_seed(seed)
    ext, cols = xs_extents(d)
    bufs = {name: alloc(numel, dt, int(getattr(d, name)) % 256, device) for name, (numel, dt) in ext.items() if getattr(d, name)}
    nsets = d.m // d.wp_set_rows if d.wp_set_rows else 1
    Ws, Cs, packs = [], [], []
    for _ in range(nsets):
        w = _ints_sparse((d.n, d.k), gen, device)
        c = _ints((d.n,), gen, device, -4, 4, F32)
        Ws.append(w)
        Cs.append(c)
        if d.act == ACT_GEGLU:
            wp_, cp_ = pack_geglu(w, c)
            packs.append(pack_xs_weights(wp_, cp_))
        else:
            packs.append(pack_xs_weights(w, c))
    wp = torch.stack(packs).reshape(-1)
    if wp.numel() != bufs["wp"].numel():
        raise RuntimeError("packed xs weights do not match the descriptor's extent")
    bufs["wp"].copy_(wp)
    if d.normalize:
        # rows mu + (+-v), half of each sign: mean and variance exact in fp32, the normalised values round to exactly +-1 in fp16
        # (distance to the rounding boundary ~ 2^-11, against an fp32 rsqrt error of ~ 2^-23)
        mu = _ints((d.m, 1), gen, device, -2, 2, F32)
        v = _ints((d.m, 1), gen, device, 1, 3, F32)
        sign = torch.ones((d.m, d.k), device=device)
        sign[:, d.k // 2:] = -1
        perm = torch.argsort(torch.rand((d.m, d.k), generator=gen, device=device), 1)
        x = mu + v * torch.gather(sign, 1, perm)
        bufs["x"].copy_(x.to(H16).reshape(-1))
    else:
        bufs["x"].copy_(_ints((d.m * d.k,), gen, device))
    if "resid" in bufs:
        bufs["resid"].copy_(_ints(bufs["resid"].shape, gen, device, -4, 4))
    bufs["out"].base_alloc.view(torch.int16).fill_(OUT_SENTINEL)
    rewrite(d, bufs)
    return d, bufs, {"W": Ws, "c": Cs}


def xs_ref(d, T, L, r0=0, r1=None):
    """fp64 restatement of mvoc_xs_linear_f16 for rows [r0, r1) (within one weight set): (stored values, bound)"""
    r1 = d.m if r1 is None else r1
    s = (r0 // d.wp_set_rows) if d.wp_set_rows else 0
    if d.wp_set_rows:
        assert (r1 - 1) // d.wp_set_rows == s
    x = T["x"].reshape(-1)[r0 * d.k:r1 * d.k].reshape(r1 - r0, d.k).to(F64)
    if d.normalize:
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        x = r16((x - mean) / torch.sqrt(var + d.ln_eps))
    y = x @ L["W"][s].to(F64).t() + L["c"][s].to(F64)[None, :]
    fake = GemmDesc()
    fake.n, fake.act, fake.n_store, fake.m = d.n, d.act, d.n_store, d.m
    fake.ldr = d.ldr
    fake.resid = 1 if d.resid else None
    Tr = {"resid": T.get("resid")}
    fake.bias = None
    return gemm_epilogue(fake, y, Tr, {}, r0, r1)


def xs_blocks(d, budget=1 << 26):
    per = max(256, budget // max(d.n, d.k))
    if d.wp_set_rows:
        per = min(per, d.wp_set_rows)
        while d.wp_set_rows % per:
            per -= 256 if per > 256 else 1
    return [(r0, min(d.m, r0 + per)) for r0 in range(0, d.m, per)]


# ---- attention -----------------------------------------------------------------------------------------------------------------------
def attn_hd(d):
    return d.head_dim or 64


def attn_scale(d):
    return d.scale if d.scale else 1.0 / math.sqrt(64.0) if attn_hd(d) == 64 else 1.0 / math.sqrt(attn_hd(d))


def attn_extents(d):
    hd = attn_hd(d)
    nkv = (d.nbatch - 1) // max(d.kv_bdiv, 1) + 1
    e = lambda nb, bs, t, ts: (nb - 1) * bs + (t - 1) * ts + d.heads * hd
    ext = {"q": e(d.nbatch, d.q_bs, d.tq, d.q_ts), "k": e(nkv, d.k_bs, d.tk, d.k_ts), "v": e(nkv, d.v_bs, d.tk, d.v_ts),
           "out": e(d.nbatch, d.o_bs, d.tq, d.o_ts)}
    ext["v2"], ext["out2"] = ext["v"], ext["out"]
    return ext


def build_attn(d0, device, seed):
    d = copy_desc(d0)
    gen = torch.Generator(device=device).manual_seed(seed)
    bufs = {}
    for name, numel in attn_extents(d).items():
        if getattr(d, name):
            bufs[name] = alloc(numel, H16, int(getattr(d, name)) % 256, device)
            if name in ("q", "k", "v", "v2"):
                bufs[name].copy_(torch.randn(numel, generator=gen, device=device).to(H16))
            else:
                bufs[name].base_alloc.view(torch.int16).fill_(OUT_SENTINEL)
    rewrite(d, bufs)
    return d, bufs


def attn_view(buf, nb, bs, t, ts, heads, hd):
    return buf.as_strided((nb, t, heads, hd), (bs, ts, hd, 1), buf.storage_offset())


def attn_ref(d, T, which="out", b0=0, b1=None, q0=0, q1=None):
    """fp64 softmax(q k^T * scale) v for batches [b0, b1), queries [q0, q1): [b, q, heads, hd]"""
    hd = attn_hd(d)
    b1 = d.nbatch if b1 is None else b1
    q1 = d.tq if q1 is None else q1
    nkv = (d.nbatch - 1) // max(d.kv_bdiv, 1) + 1
    q = attn_view(T["q"], d.nbatch, d.q_bs, d.tq, d.q_ts, d.heads, hd)[b0:b1, q0:q1].to(F64)
    kidx = torch.arange(b0, b1, device=q.device) // max(d.kv_bdiv, 1)
    k = attn_view(T["k"], nkv, d.k_bs, d.tk, d.k_ts, d.heads, hd).index_select(0, kidx).to(F64)
    v = attn_view(T["v2" if which == "out2" else "v"], nkv, d.v_bs, d.tk, d.v_ts, d.heads, hd).index_select(0, kidx).to(F64)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * attn_scale(d)
    if d.causal:
        qi = torch.arange(q0, q1, device=q.device)[:, None]
        ki = torch.arange(d.tk, device=q.device)[None, :]
        s = s.masked_fill(ki > qi, float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v)


def attn_out_view(d, T, which="out"):
    bs, ts = d.o_bs, d.o_ts
    return attn_view(T[which], d.nbatch, bs, d.tq, ts, d.heads, attn_hd(d))


# ---- temporal attention --------------------------------------------------------------------------------------------------------------
def tattn_extents(d):
    e = lambda p: (d.nsample - 1) * getattr(d, p + "_bs") + (d.hw - 1) * getattr(d, p + "_ps") + (d.frames - 1) * getattr(d, p + "_ts") + d.heads * 64
    return {"q": e("q"), "k": e("k"), "v": e("v"), "out": e("o")}


def build_tattn(d0, device, seed):
    d = copy_desc(d0)
    gen = torch.Generator(device=device).manual_seed(seed)
    bufs = {}
    for name, numel in tattn_extents(d).items():
        bufs[name] = alloc(numel, H16, int(getattr(d, name)) % 256, device)
        if name != "out":
            bufs[name].copy_(torch.randn(numel, generator=gen, device=device).to(H16))
        else:
            bufs[name].base_alloc.view(torch.int16).fill_(OUT_SENTINEL)
    rewrite(d, bufs)
    return d, bufs


def tattn_view(d, buf, p):
    """[nsample, hw, frames, heads, 64] view of operand p in ('q', 'k', 'v', 'o')"""
    return buf.as_strided((d.nsample, d.hw, d.frames, d.heads, 64),
                          (getattr(d, p + "_bs"), getattr(d, p + "_ps"), getattr(d, p + "_ts"), 64, 1), buf.storage_offset())


def frame_attention64(q, k, v):
    """q/k/v [..., frames, heads, 64] fp64 -> attention over the frame axis, scale 1/8"""
    s = torch.einsum("...fhd,...ghd->...hfg", q, k) / 8.0
    return torch.einsum("...hfg,...ghd->...fhd", torch.softmax(s, -1), v)


def tattn_ref(d, T, s0=0, s1=None):
    """samples [s0, s1): [s, hw, frames, heads, 64] fp64"""
    s1 = d.nsample if s1 is None else s1
    return frame_attention64(*(tattn_view(d, T[n], p)[s0:s1].to(F64) for n, p in (("q", "q"), ("k", "k"), ("v", "v"))))


# ---- fused LayerNorm -> QKV -> temporal attention ------------------------------------------------------------------------------------
def build_tfused(d0, device, seed):
    from mvoc_amd.unet import Linear, pack_tfused_weights
    d = copy_desc(d0)
    gen = torch.Generator(device=device).manual_seed(seed)
    c, rows = d.c, d.nsample * d.frames * d.hw
    bufs = {"x": alloc(rows * c, H16, d.x % 256, device), "wp": alloc(3 * c * c, H16, d.wp % 256, device),
            "ln_rowsum": alloc(3 * c, F32, d.ln_rowsum % 256, device), "ln_bias": alloc(3 * c, F32, d.ln_bias % 256, device),
            "out": alloc(rows * c, H16, d.out % 256, device)}
    x = (torch.randn(rows, c, generator=gen, device=device) * 1.4 + 0.3).to(H16)
    w = (torch.randn(3 * c, c, generator=gen, device=device) / math.sqrt(c)).to(H16)
    gm = (1 + 0.3 * torch.randn(c, generator=gen, device=device)).to(H16)
    bt = (0.3 * torch.randn(c, generator=gen, device=device)).to(H16)
    lin = Linear(w).fold_layernorm(gm, bt, d.ln_eps)
    bufs["x"].copy_(x.reshape(-1))
    bufs["wp"].copy_(pack_tfused_weights(lin.w_ln, d.heads).reshape(-1))
    bufs["ln_rowsum"].copy_(lin.ln[0])
    bufs["ln_bias"].copy_(lin.ln[1])
    bufs["out"].base_alloc.view(torch.int16).fill_(OUT_SENTINEL)
    rewrite(d, bufs)
    return d, bufs, {"w": w, "gamma": gm, "beta": bt}


def layernorm64(x, gamma, beta, eps):
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps)
    if gamma is not None:
        y = y * gamma.to(F64) + beta.to(F64)
    return y


def tfused_ref(d, T, L, s0=0, s1=None):
    """LayerNorm (rounded to fp16) -> QKV projection (rounded to fp16) -> attention over frames, in fp64: [rows, c] of samples
    [s0, s1)"""
    c = d.c
    s1 = d.nsample if s1 is None else s1
    per = d.frames * d.hw
    rows = (s1 - s0) * per
    x = T["x"].reshape(-1, c)[s0 * per:s1 * per]
    qkv = r16(r16(layernorm64(x, L["gamma"], L["beta"], d.ln_eps)) @ L["w"].to(F64).t())

    def seq(t):
        return t.reshape(s1 - s0, d.frames, d.hw, d.heads, 64).permute(0, 2, 1, 3, 4)

    o = frame_attention64(seq(qkv[:, :c]), seq(qkv[:, c:2 * c]), seq(qkv[:, 2 * c:]))
    return o.permute(0, 2, 1, 3, 4).reshape(rows, c)


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------
def chan_sums64(x, rows_per_slab=256):
    """{sum, sum of squares} per 256-row slab and channel, fp64 -> [rows / 256, c, 2]"""
    xs = x.to(F64).reshape(-1, rows_per_slab, x.shape[-1])
    return torch.stack([xs.sum(1), (xs * xs).sum(1)], -1)


def build_gn(d0, device, seed, fold_args=None, mult=None):
    """``mult`` (the large-extent pattern): sample i := sample 0 times the integer mult[i] (exact in fp16), beta zero; L["x"] then
    holds sample 0 only"""
    d = copy_desc(d0)
    gen = torch.Generator(device=device).manual_seed(seed)
    rows = d.nsample * d.rows_per_sample
    c2 = d.c - d.c1
    bufs = {"x": alloc(rows * d.c1, H16, d.x % 256, device)}
    if mult is None:
        x = (torch.randn(rows, d.c1, generator=gen, device=device) * 2 + 0.5).to(H16)
        bufs["x"].copy_(x.reshape(-1))
    else:
        if d.x2 or fold_args is not None or len(mult) != d.nsample or mult[0] != 1:
            raise RuntimeError("the multiplier pattern is written for a single-source GroupNorm, sample 0 unscaled")
        x = (torch.randn(d.rows_per_sample, d.c1, generator=gen, device=device) * 2 + 0.5).to(H16)
        xb = bufs["x"].reshape(d.nsample, -1)
        for i, s_ in enumerate(mult):
            torch.mul(x.reshape(-1), s_, out=xb[i])
    L = {"x": x}
    if d.x2:
        bufs["x2"] = alloc(rows * c2, H16, d.x2 % 256, device)
        x2 = (torch.randn(rows, c2, generator=gen, device=device) * 3 - 0.25).to(H16)
        bufs["x2"].copy_(x2.reshape(-1))
        L["x2"] = x2
    for name, mk in (("gamma", lambda: 1 + 0.2 * torch.randn(d.c, generator=gen, device=device)),
                     ("beta", lambda: 0.2 * torch.randn(d.c, generator=gen, device=device))):
        if getattr(d, name):
            bufs[name] = alloc(d.c, H16, getattr(d, name) % 256, device)
            L[name] = mk().to(H16) if not (mult is not None and name == "beta") else torch.zeros(d.c, dtype=H16, device=device)
            bufs[name].copy_(L[name])
    if d.out:
        bufs["out"] = alloc(rows * d.c, H16, d.out % 256, device)
        bufs["out"].base_alloc.view(torch.int16).fill_(OUT_SENTINEL)
    if d.workspace:
        bufs["workspace"] = alloc(d.workspace_bytes // 4, F32, d.workspace % 256, device)
    if d.chan_sums:  # the producer's statistics, supplied from fp64 sums of the rows
        bufs["chan_sums"] = alloc(rows // 256 * d.c1 * 2, F32, d.chan_sums % 256, device)
        bufs["chan_sums"].copy_(chan_sums64(x).to(F32).reshape(-1))
    if d.chan_sums2:
        bufs["chan_sums2"] = alloc(rows // 256 * c2 * 2, F32, d.chan_sums2 % 256, device)
        bufs["chan_sums2"].copy_(chan_sums64(L["x2"]).to(F32).reshape(-1))
    rewrite(d, bufs)
    fa = None
    if fold_args is not None:
        n, k = fold_args["n"], fold_args["k"]
        w = (torch.randn(n, k, generator=gen, device=device) / math.sqrt(k)).to(H16)
        fa = dict(fold_args)
        fa["w"] = alloc(n * k, H16, fold_args["w"] % 256, device)
        fa["w"].copy_(w.reshape(-1))
        L["w"] = w
        if fold_args["bias"]:
            b = torch.randn(n, generator=gen, device=device).to(H16)
            fa["bias"] = alloc(n, H16, fold_args["bias"] % 256, device)
            fa["bias"].copy_(b)
            L["bias"] = b
        else:
            fa["bias"] = None
        fa["wp_sets"] = alloc(d.nsample * (n // 32) * (k // 16 + 1) * 512, H16, fold_args["wp_sets"] % 256, device)
    return d, bufs, L, fa


def groupnorm64(x, nsample, groups, eps, gamma, beta, silu):
    """x [nsample * rows, c] -> F.group_norm over (rows, c / groups) per sample, fp64"""
    c = x.shape[1]
    xs = x.to(F64).reshape(nsample, -1, groups, c // groups)
    mean = xs.mean((1, 3), keepdim=True)
    var = ((xs - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((xs - mean) / torch.sqrt(var + eps)).reshape(x.shape[0], c)
    if gamma is not None:
        y = y * gamma.to(F64) + beta.to(F64)
    return silu64(y) if silu else y


def gn_ref(d, L, s0=0, s1=None):
    """rows of samples [s0, s1)"""
    s1 = d.nsample if s1 is None else s1
    r0, r1 = s0 * d.rows_per_sample, s1 * d.rows_per_sample
    x = L["x"][r0:r1] if "x2" not in L else torch.cat([L["x"][r0:r1], L["x2"][r0:r1]], 1)
    return groupnorm64(x, s1 - s0, d.groups, d.eps, L.get("gamma"), L.get("beta"), bool(d.silu))


def unpack_xs_weights(wp, n, k):
    """inverse of unet.pack_xs_weights: ([n, k] fp16 weights, [n] fp32 constants)"""
    nk = k // 16
    wp = wp.reshape(n // 32, nk + 1, 512)
    w = wp[:, :nk].reshape(n // 32, nk, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(n, k)
    c = wp[:, nk, :64].contiguous().view(F32).reshape(n)
    return w, c


def gn_fold_ref(d, L, s0=0, s1=None):
    """GroupNorm(x) @ W^T + bias in fp64, samples [s0, s1): [rows, n]"""
    s1 = d.nsample if s1 is None else s1
    y = groupnorm64(L["x"][s0 * d.rows_per_sample:s1 * d.rows_per_sample], s1 - s0, d.groups, d.eps, L["gamma"], L["beta"], False)
    out = y @ L["w"].to(F64).t()
    if "bias" in L:
        out = out + L["bias"].to(F64)
    return out


# ---- row statistics / LayerNorm --------------------------------------------------------------------------------------------------
def row_stats64(x, eps):
    x = x.to(F64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + eps)


def row_moments64(x, tile_w, ld):
    """{sum, sum of squares} per row and tile_w-channel tile: [rows, ld, 2] fp64 (unused entries zero)"""
    rows, n = x.shape
    out = torch.zeros((rows, ld, 2), dtype=F64, device=x.device)
    x = x.to(F64)
    for t in range(-(-n // tile_w)):
        s = x[:, t * tile_w:min(n, (t + 1) * tile_w)]
        out[:, t, 0] = s.sum(1)
        out[:, t, 1] = (s * s).sum(1)
    return out


def row_stats_ratio(st, x, eps):
    """worst deviation of fp32 {mean, rstd} rows from fp64, in units of the bounds of
    test_gemm_row_moments_and_layernorm_statistics_from_them (mean 1e-4 + 1e-5 |mean|, rstd 2e-5 relative)"""
    mean, rstd = row_stats64(x, eps)
    st = st.to(F64)
    return max(float(((st[:, 0] - mean).abs() / (1e-4 + 1e-5 * mean.abs())).max()), float(((st[:, 1] - rstd).abs() / (2e-5 * rstd)).max()))


def rel_l2(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---- the stem entries of the VAE, the CLIP towers and the mask path ------------------------------------------------------------------
U8, I32 = torch.uint8, torch.int32
U8_SENTINEL = 0xA5  # the byte the slack around a uint8 output keeps


# Bound of the fp32 softmax (norm.hip: softmax_rows_kernel) against fp64, relative to the result p = exp(d) / sum, d = x - max <= 0.
# Only results that do not round to zero matter: p >= 2^-25 and sum >= 1 give |d| <= 25 ln 2 < 17.4 (below that one fp16 ulp, 2^-24
# absolute, dwarfs any relative error).  Terms, in units of 2^-23 = one fp32 ulp:
#   exp(d) as exp2(d * log2 e): the product's rounding and the constant's, |d| log2(e) 2^-24 each, move the result by
#     2 |d| log2(e) ln(2) 2^-24 = |d| 2^-23 relative, the exponential itself one ulp                              -> 17.4 + 1
#   the sum: the same error in a p-weighted mean (<= 17.4 + 1), cols / 64 sequential additions per lane and 6 butterfly steps of
#     half an ulp each                                                                                            -> 18.4 + (cols / 64 + 6) / 2
#   1 / sum one ulp, the product half an ulp                                                                       -> 1.5
# (test_stage_census_cpu: test_softmax_bound_derivation measures an fp32 evaluation of the same chain against this.)
def softmax_rel(cols):
    return (2 * 18.4 + (cols / 64 + 6) / 2 + 1.5) * 2.0 ** -23


# Bound of an fp32 exponential against fp64, relative, at argument h: one ulp for the library routine; where the compiler takes
# exp2(h * log2 e) instead the argument's rounding adds |h| 2^-23 as above.  (|h| + 2) 2^-23 covers both.
def exp32_rel(h):
    return (h.abs() + 2.0) * 2.0 ** -23


def stem_extents(name, a):
    """element counts of every pointer argument of a stem entry: name -> (numel, dtype); what the torch formulation touches"""
    if name == "mvoc_conv3x3_small_f16":
        ho, wo = (a["h"] - 1) // a["stride"] + 1, (a["wd"] - 1) // a["stride"] + 1
        return {"x": (a["nimg"] * a["h"] * a["wd"] * a["cin"], H16), "w": (a["cout"] * 9 * a["cin"], H16), "bias": (a["cout"], H16),
                "out": (a["nimg"] * ho * wo * a["cout"], H16)}
    if name == "mvoc_conv1x1_small_f16":
        return {"x": (a["rows"] * a["cin"], H16), "w": (a["cout"] * a["cin"], H16), "bias": (a["cout"], H16), "out": (a["rows"] * a["cout"], H16)}
    if name == "mvoc_softmax_rows_f16":
        return {"x": (a["rows"] * a["cols"], H16)}
    if name == "mvoc_image_to_tokens_f16":
        return {"x": (a["n"] * a["c"] * a["hw"], H16), "out": (a["n"] * a["hw"] * a["c"], H16)}
    if name == "mvoc_tokens_to_image_f16":
        return {"x": ((a["n"] * a["hw"] - 1) * a["ld"] + a["c"], H16), "out": (a["n"] * a["c"] * a["hw"], H16)}
    if name == "mvoc_gaussian_sample_f16":
        return {k: (a["n"], H16) for k in ("mean", "logvar", "noise", "out")}
    if name == "mvoc_scale_f16":
        return {"x": (a["n"], H16), "out": (a["n"], H16)}
    if name == "mvoc_clip_patches_f16":
        g = a["size"] // a["patch"]
        return {"pixels": (a["nimg"] * 3 * a["size"] ** 2, H16), "out": (a["nimg"] * g * g * a["kpad"], H16)}
    if name == "mvoc_clip_embed_f16":
        nb = a["rows"] // a["t"]
        return {"table": (STEM_VOCAB * a["c"] if a["ids"] else nb * (a["t"] - 1) * a["c"], H16), "ids": (a["rows"], I32), "cls": (a["c"], H16),
                "pos": (a["t"] * a["c"], H16), "out": (a["rows"] * a["c"], H16)}
    if name == "mvoc_mask_resize_u8":
        return {"in": (a["n"] * a["H"] * a["W"], U8), "tmp": (a["n"] * a["H"] * a["w"], U8), "out": (a["n"] * a["h"] * a["w"], U8),
                "bounds_h": (a["w"] * 2, I32), "kk_h": (a["w"] * a["ksize_h"], I32), "bounds_v": (a["h"] * 2, I32),
                "kk_v": (a["h"] * a["ksize_v"], I32)}
    if name == "mvoc_mask_finish":
        return {"v": (a["n"], U8), "float_mask": (a["n"], H16), "bool_mask": (a["n"], U8)}
    raise RuntimeError(f"no replay builder for {name}")


STEM_VOCAB = 997  # rows of the replay's token table (the recorded call does not tell the vocabulary's size)
STEM_OUTPUTS = {"mvoc_conv3x3_small_f16": ("out",), "mvoc_conv1x1_small_f16": ("out",), "mvoc_softmax_rows_f16": ("x",),
                "mvoc_image_to_tokens_f16": ("out",), "mvoc_tokens_to_image_f16": ("out",), "mvoc_gaussian_sample_f16": ("out",),
                "mvoc_scale_f16": ("out",), "mvoc_clip_patches_f16": ("out",), "mvoc_clip_embed_f16": ("out",),
                "mvoc_mask_resize_u8": ("tmp", "out"), "mvoc_mask_finish": ("float_mask", "bool_mask")}


def fill_sentinel(t):
    b = t.base_alloc
    if b.dtype == H16:
        b.view(torch.int16).fill_(OUT_SENTINEL)
    else:
        b.view(U8).fill_(U8_SENTINEL)


def stray_writes(t):
    """elements of the allocation around the view `t` that no longer hold the sentinel"""
    b = t.base_alloc
    off = (t.data_ptr() - b.data_ptr()) // b.element_size()
    if b.dtype == H16:
        bb, sv = b.view(torch.int16), OUT_SENTINEL
    else:
        bb, sv = b.view(U8).reshape(-1), U8_SENTINEL
        off, n = off * b.element_size(), t.numel() * b.element_size()
        return int((bb[:off] != sv).sum()) + int((bb[off + n:] != sv).sum())
    return int((bb[:off] != sv).sum()) + int((bb[off + t.numel():] != sv).sum())


def unwritten(t):
    """fp16 elements of an output that still hold the sentinel"""
    return int((t.view(torch.int16) == OUT_SENTINEL).sum())


def build_stem(ln, device, seed):
    """a replay of a recorded stem call: (positional arguments without the stream, buffers by argument name + the logical operands
    under upper-case names).  Every pointer argument gets a fresh buffer at the recorded address mod 256; an argument the builder
    does not know fails here, on the host."""
    from mvoc_amd.unet import pack_conv3x3_small
    from mvoc_amd.utils import pil_bicubic_tables
    name, a = ln.name, ln.args
    gen = torch.Generator(device=device).manual_seed(seed)
    ext = stem_extents(name, a)
    T = {}
    for k, v in a.items():
        if not isinstance(v, _Ptr):
            continue
        if k not in ext:
            raise RuntimeError(f"replay builder has no buffer for the recorded pointer argument `{k}` ({name})")
        if v:
            T[k] = alloc(ext[k][0], ext[k][1], int(v) % 256, device)
    for k in STEM_OUTPUTS[name]:
        if k not in T:
            raise RuntimeError(f"{name}: the recorded call has no `{k}`")
    if name == "mvoc_conv3x3_small_f16":
        T["x"].copy_(_ints(T["x"].shape, gen, device, -2, 2))
        T["W"] = _ints((a["cout"], a["cin"], 3, 3), gen, device, -2, 2)
        T["w"].copy_(pack_conv3x3_small(T["W"]).reshape(-1))
        if "bias" in T:
            T["bias"].copy_(_ints(T["bias"].shape, gen, device, -4, 4))
    elif name == "mvoc_conv1x1_small_f16":
        for k, r in (("x", 3), ("w", 3), ("bias", 8)):
            if k in T:
                T[k].copy_(_ints(T[k].shape, gen, device, -r, r))
    elif name == "mvoc_softmax_rows_f16":
        x = (torch.randn(a["rows"], a["cols"], generator=gen, device=device) * 3).to(H16)
        x[a["rows"] // 2, a["cols"] // 3] = 40.0  # a dominant score
        x[0] = x[0, 0]                            # a constant row
        T["X"] = x
        fill_sentinel(T["x"])  # (in place: the slack around it is what must stay)
        T["x"].copy_(x.reshape(-1))
    elif name in ("mvoc_image_to_tokens_f16", "mvoc_tokens_to_image_f16", "mvoc_clip_patches_f16"):
        k = "pixels" if name == "mvoc_clip_patches_f16" else "x"
        T[k].copy_(torch.randn(T[k].shape, generator=gen, device=device).to(H16))
    elif name == "mvoc_gaussian_sample_f16":
        for k, sc in (("mean", 1.0), ("logvar", 4.0), ("noise", 1.0)):
            T[k].copy_((torch.randn(T[k].shape, generator=gen, device=device) * sc).to(H16))
        edge = torch.tensor([-40.0, 30.0, 0.0, -30.0, 20.0, 19.98, -29.98], device=device).to(H16)[:a["n"]]
        T["logvar"][:len(edge)] = edge
    elif name == "mvoc_scale_f16":
        T["x"].copy_((torch.randn(T["x"].shape, generator=gen, device=device) * 4).to(H16))
    elif name == "mvoc_clip_embed_f16":
        for k in ("table", "cls", "pos"):
            if k in T:
                T[k].copy_(torch.randn(T[k].shape, generator=gen, device=device).to(H16))
        if "ids" in T:
            T["ids"].copy_(torch.randint(0, STEM_VOCAB, T["ids"].shape, generator=gen, device=device, dtype=torch.int32))
            T["ids"][:2] = torch.tensor([0, STEM_VOCAB - 1], dtype=I32, device=device)[:a["rows"]]
    elif name == "mvoc_mask_resize_u8":
        T["in"].copy_(torch.randint(0, 256, T["in"].shape, generator=gen, device=device, dtype=torch.int16).to(U8))
        bh, kh = pil_bicubic_tables(a["W"], a["w"])
        bv, kv = pil_bicubic_tables(a["H"], a["h"])
        if kh.shape[1] != a["ksize_h"] or kv.shape[1] != a["ksize_v"]:
            raise RuntimeError("the recorded table pitch differs from pil_bicubic_tables of the recorded sizes")
        for k, t in (("bounds_h", bh), ("kk_h", kh), ("bounds_v", bv), ("kk_v", kv)):
            T[k].copy_(torch.from_numpy(t).reshape(-1).to(device))
    elif name == "mvoc_mask_finish":
        v = torch.randint(0, 256, T["v"].shape, generator=gen, device=device, dtype=torch.int16).to(U8)
        v[:256] = torch.arange(256, device=device).to(U8)[:a["n"]]  # every value at least once
        T["v"].copy_(v)
    for k in STEM_OUTPUTS[name]:
        if k != "x":
            fill_sentinel(T[k])
    args = [T[k].data_ptr() if (isinstance(v, _Ptr) and v) else (None if isinstance(v, _Ptr) else v) for k, v in a.items()]
    return args, T


def pil_resize_u8(frames, w, h):
    """PIL's Image.resize((w, h)) of "L" images with its default filter (BICUBIC), the path tests/golden/g9_boat_surf_masks.npz was
    made by (reference utils.py: mask.resize((W // 8, H // 8))): uint8 [n, H, W] -> [n, h, w]"""
    import numpy as np
    from PIL import Image
    return torch.from_numpy(np.stack([np.asarray(Image.fromarray(f).resize((w, h))) for f in frames.cpu().numpy()]))


def conv3x3_small64(x, w, bias, stride, silu):
    """x [n, h, w, cin], logical w [cout, cin, 3, 3] -> (values [n, ho, wo, cout] fp64 after the kernel's roundings, bound)"""
    xp = torch.nn.functional.pad(x.to(F64), (0, 0, 1, 1, 1, 1))
    n, h, wd, cin = x.shape
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    acc = 0
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            acc = acc + sl.reshape(-1, cin) @ w[:, :, ky, kx].to(F64).t()
    v = r16(acc + (bias.to(F64) if bias is not None else 0))
    bound = torch.zeros_like(v)
    if silu:
        a64 = silu64(v)
        v, bound = r16(a64), ulp16(a64)
    return v.reshape(n, ho, wo, -1), bound.reshape(n, ho, wo, -1)


def softmax64(x):
    """softmax of the fp16 input in fp64, rounded once -> (values, alternatives).  The kernel rounds an fp32 value within
    softmax_rel(cols) of p: where that error reaches across an fp16 rounding boundary the neighbouring value is accepted, nothing else
    (never more than one fp16 ulp of the result plus the fp32 evaluation error, and far tighter away from the boundaries)"""
    p = torch.softmax(x.to(F64), -1)
    tol = softmax_rel(x.shape[-1]) * p
    return r16(p), (r16(p - tol), r16(p + tol))


def gaussian_sample64(mean, logvar, noise):
    """DiagonalGaussianDistribution.sample() with a rounding at each eager op (stem.hip: gaussian_sample_kernel):
    out = r16(mean + r16(r16(exp(r16(0.5 * clamp(logvar, -30, 20)))) * noise)).  Returns (values, alternatives): where the fp32
    exponential's error (exp32_rel) reaches across a rounding boundary of r16(exp(.)) the kernel may hold the neighbouring fp16
    value of the standard deviation; `alternatives` are the chain's results with that neighbour (equal to `values` elsewhere)"""
    mean, noise = mean.to(F64), noise.to(F64)
    h = r16(0.5 * logvar.to(F64).clamp(-30.0, 20.0))
    e = torch.exp(h)
    sd = r16(e)
    chain = lambda s: r16(mean + r16(s * noise))
    out = chain(sd)
    tol = exp32_rel(h) * e
    lo, hi = r16(e - tol), r16(e + tol)
    return out, (torch.where(lo != sd, chain(lo), out), torch.where(hi != sd, chain(hi), out))


def scale64(x, scale):
    """python float times an fp16 tensor: the fp32 product of float(scale) and x rounded to fp32, then to fp16"""
    s32 = torch.tensor(scale, dtype=F32).to(F64)
    return (x.to(F64) * s32).to(F32).to(H16)


def clip_patches_ref(x, patch, kpad):
    """[n, 3, size, size] -> im2col rows [n * g * g, kpad], k = (c, py, px), zero columns past 3 * patch^2"""
    n, c, size, _ = x.shape
    g = size // patch
    rows = x.reshape(n, c, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, c * patch * patch)
    return torch.nn.functional.pad(rows, (0, kpad - rows.shape[1]))


def clip_embed_ref(table, ids, cls, pos, rows, t):
    """out[row] = src(row) + pos[row % t], rounded once; src = table[ids[row]], or the class row at t == 0 and patch row
    (row / t) * (t - 1) + row % t - 1 otherwise"""
    c = pos.shape[1]
    r = torch.arange(rows, device=pos.device)
    if ids is not None:
        src = table[ids.long()]
    else:
        src = torch.cat([cls.reshape(1, 1, c).expand(rows // t, 1, c), table.reshape(rows // t, t - 1, c)], 1).reshape(rows, c)
    return (src.to(F64) + pos[r % t].to(F64)).to(H16)


def stem_ref(ln, T):
    """float64 (or exact) restatement of a stem entry on the replay's buffers: output name -> (values, bound or None = bit for bit)"""
    name, a = ln.name, ln.args
    if name == "mvoc_conv3x3_small_f16":
        v, b = conv3x3_small64(T["x"].reshape(a["nimg"], a["h"], a["wd"], a["cin"]), T["W"], T.get("bias"), a["stride"], a["silu"])
        return {"out": (v.reshape(-1), b.reshape(-1) if a["silu"] else None)}
    if name == "mvoc_conv1x1_small_f16":
        y = T["x"].reshape(a["rows"], a["cin"]).to(F64) @ T["w"].reshape(a["cout"], a["cin"]).to(F64).t()
        return {"out": (r16(y + (T["bias"].to(F64) if "bias" in T else 0)).reshape(-1), None)}
    if name == "mvoc_softmax_rows_f16":
        v, (lo, hi) = softmax64(T["X"])
        return {"x": (v.reshape(-1), (lo.reshape(-1), hi.reshape(-1)))}
    if name == "mvoc_image_to_tokens_f16":
        return {"out": (T["x"].reshape(a["n"], a["c"], a["hw"]).permute(0, 2, 1).reshape(-1), None)}
    if name == "mvoc_tokens_to_image_f16":
        x = T["x"].as_strided((a["n"], a["hw"], a["c"]), (a["hw"] * a["ld"], a["ld"], 1), T["x"].storage_offset())
        return {"out": (x.permute(0, 2, 1).reshape(-1), None)}
    if name == "mvoc_gaussian_sample_f16":
        v, alts = gaussian_sample64(T["mean"], T["logvar"], T["noise"])
        return {"out": (v, alts)}
    if name == "mvoc_scale_f16":
        return {"out": (scale64(T["x"], a["scale"]), None)}
    if name == "mvoc_clip_patches_f16":
        return {"out": (clip_patches_ref(T["pixels"].reshape(a["nimg"], 3, a["size"], a["size"]), a["patch"], a["kpad"]).reshape(-1), None)}
    if name == "mvoc_clip_embed_f16":
        c = a["c"]
        return {"out": (clip_embed_ref(T["table"].reshape(-1, c), T.get("ids"), T.get("cls"), T["pos"].reshape(-1, c), a["rows"], a["t"]).reshape(-1), None)}
    if name == "mvoc_mask_resize_u8":
        fr = T["in"].reshape(a["n"], a["H"], a["W"])
        return {"tmp": (pil_resize_u8(fr, a["w"], a["H"]).reshape(-1).to(fr.device), None),
                "out": (pil_resize_u8(fr, a["w"], a["h"]).reshape(-1).to(fr.device), None)}
    if name == "mvoc_mask_finish":
        v = T["v"]
        return {"float_mask": ((v.to(F64) / 255.0).to(F32).to(H16), None), "bool_mask": ((v > 10).to(U8), None)}
    raise RuntimeError(f"no reference for {name}")


def stem_compare(ln, T):
    """(number of wrong elements, worst deviation in units of the bound: 0 for the bit-exact outputs, number of elements that hold an
    accepted alternative) of a replayed stem call"""
    bad, worst, alt = 0, 0.0, 0
    for k, (ref, bound) in stem_ref(ln, T).items():
        got = T[k]
        if bound is None:
            bad += int((got.view(torch.int16) != ref.to(got.dtype).view(torch.int16)).sum()) if got.dtype == H16 else int((got != ref).sum())
        elif isinstance(bound, tuple):
            g = got.to(F64)
            bad += int(((g != ref) & (g != bound[0]) & (g != bound[1])).sum())
            alt += int(((g != ref) & ((g == bound[0]) | (g == bound[1]))).sum())
        else:
            dev = (got.to(F64) - ref).abs()
            bad += int((~(dev <= bound)).sum())
            worst = max(worst, float((dev / bound).nan_to_num(1e9).max()))
    return bad, worst, alt


def describe(ln):
    """one line of the fields that tell a launch apart, for failure messages"""
    d, a = ln.desc, ln.args
    if ln.name == "mvoc_gemm_f16":
        s = (f"gemm mode={d.a_mode} m={d.m} n={d.n} k={d.k} cin={d.cin} c1={d.c1} two_src={bool(d.a2)} ns={d.n_store} ldo={d.ldo} "
             f"act={d.act} ln={bool(d.ln_rowsum)} resid={bool(d.resid)} rowadd={bool(d.rowadd)}/{d.rowadd_div} ups={d.upsample} "
             f"stride={d.stride} pad={d.pad_mode} korder={d.k_order} conc={d.concurrency} ws={bool(d.workspace)} split={d.split_k} "
             f"tile={d.tile} cs={bool(d.chan_sums)} rm={bool(d.row_moments)} out%256={(d.out or 0) % 256}")
        if d.a_mode == A_CONV3X3:
            s += f" img={d.nimg}x{d.hsrc}x{d.wsrc}->{d.hout}x{d.wout}"
        if d.a_mode == A_TEMPORAL3:
            s += f" frames={d.frames} hw={d.hw}"
        return s
    if ln.name == "mvoc_xs_linear_f16":
        return f"xs m={d.m} n={d.n} k={d.k} ns={d.n_store} ldo={d.ldo} act={d.act} norm={d.normalize} resid={bool(d.resid)} sets={d.wp_set_rows}"
    if ln.name == "mvoc_flash_attn_f16":
        return (f"flash nb={d.nbatch} heads={d.heads} tq={d.tq} tk={d.tk} kvdiv={d.kv_bdiv} pair={bool(d.v2)} hd={d.head_dim} "
                f"pipelined={d.pipelined} q_ts={d.q_ts} k_ts={d.k_ts}")
    if ln.name == "mvoc_temporal_attn_f16":
        return f"tattn ns={d.nsample} hw={d.hw} heads={d.heads} frames={d.frames} q_ps={d.q_ps}"
    if ln.name == "mvoc_temporal_qkv_attn_f16":
        return f"tfused ns={d.nsample} frames={d.frames} hw={d.hw} c={d.c}"
    if ln.name in ("mvoc_groupnorm_f16", "mvoc_groupnorm_fold_xs_f16"):
        s = (f"{FAMILY[ln.name]} ns={d.nsample} rps={d.rows_per_sample} c={d.c} c1={d.c1} groups={d.groups} silu={d.silu} "
             f"cs={bool(d.chan_sums)} cs2={bool(d.chan_sums2)}")
        if a:
            s += f" n={a['n']} k={a['k']} bias={bool(a['bias'])}"
        return s
    return FAMILY[ln.name] + " " + " ".join(f"{k}={v if not isinstance(v, _Ptr) else ptr_key(v)}" for k, v in a.items())
