"""Thin tensor-level wrappers over the C ABI (include/mvoc_hip.h).

PyTorch supplies device memory and the current HIP stream; every computation is a libmvoc_hip kernel.
All activations are fp16, channels-last 2-D ``[rows, C]`` tensors (rows = B*F*H*W).
"""
import collections
import ctypes as C
import operator
import os
import threading

import torch

from . import _ffi
from ._ffi import (A_CONV3X3, A_PLAIN, A_TEMPORAL3, ACT_GEGLU, ACT_GELU, ACT_NONE, ACT_SILU, AttnDesc, GemmDesc, GnDesc,
                   PnpDesc, TAttnDesc, TFusedDesc, XsDesc, check, lib)

__all__ = ["linear", "conv3x3", "tconv3", "flash_attn", "temporal_attn", "groupnorm", "groupnorm_moments", "groupnorm_apply_moments", "layernorm", "pnp_blend_tokens",
           "pnp_blend_nchw", "level_offset", "level_offsets", "place_table", "place_table_variants", "shift_planes", "ddim_step", "latent_fusion", "timestep_embedding", "act", "add", "conv3x3_small",
           "adaptive_avgpool", "ncfhw_to_tokens", "tokens_to_ncfhw", "temporal_encoder4", "conv1x1_small", "softmax_rows", "ACT_NONE", "ACT_GEGLU",
           "ACT_SILU", "ACT_GELU"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name, dtype=torch.float16):
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"mvoc_amd.ops: `{name}` must be a device tensor (this package has no CPU path)")
    if t.dtype != dtype:
        raise RuntimeError(f"mvoc_amd.ops: `{name}` must be {dtype}, got {t.dtype}")
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rowmajor(t, name):
    if t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError(f"mvoc_amd.ops: `{name}` must be a 2-D row-major view, got {tuple(t.shape)} / {t.stride()}")
    return t.stride(0)


class _Conc(threading.local):
    n = 1


_CONCURRENCY = _Conc()
USE_ROW_MOMENTS = os.environ.get("MVOC_ROW_MOMENTS", "1") != "0"  # LayerNorm statistics from the producing GEMM's epilogue


def _gemm(d: GemmDesc, dev=None, out=None, sums=False, rowmom=False):
    # problems with few output tiles and a deep K get a scratch for deterministic split-K (see gemm.hip)
    if dev is not None and d.act != ACT_GEGLU and d.split_k != 1:
        nbytes = lib.mvoc_gemm_workspace_bytes(d.m, d.n, d.k)
        if nbytes:
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    cs = None
    if out is not None:  # statistics ride on the tensor OBJECT: whatever an earlier producer hung on a caller-supplied `out` is stale now
        for attr in ("chan_sums", "row_moments"):
            if hasattr(out, attr):
                delattr(out, attr)
    d.concurrency = _CONCURRENCY.n
    # (whether this SITE asks for the statistics does not depend on the row count: the host query below is then asked at every batch)
    want_sums = sums and out is not None and d.act == ACT_NONE and out.is_contiguous() and out.shape[1] == d.n_store
    if want_sums and d.m % 256 == 0:
        # REQUEST for the producer-epilogue GroupNorm statistics (include/mvoc_hip.h: chan_sums); honoured by the eight-phase tiles
        cs = torch.empty((d.m // 256, out.shape[1], 2), dtype=torch.float32, device=out.device)
        d.chan_sums = cs.data_ptr()
    rm = None
    if rowmom and USE_ROW_MOMENTS and out is not None and d.act != ACT_GEGLU and out.is_contiguous() and out.shape[1] == d.n:
        # REQUEST for the producer-epilogue LayerNorm statistics (include/mvoc_hip.h: row_moments); honoured by the eight-phase tiles
        ld = (d.n + 255) // 256
        rm = torch.empty((d.m, ld, 2), dtype=torch.float32, device=out.device)
        d.row_moments, d.row_moments_ld = rm.data_ptr(), ld
    check(lib.mvoc_gemm_f16(C.byref(d), _stream()), "gemm")
    if want_sums and lib.mvoc_gemm_chan_sums_written() and cs is not None:
        out.chan_sums = cs  # rides on the tensor OBJECT: a view / slice / copy of it carries no statistics
    if rm is not None:
        w_ = lib.mvoc_gemm_row_moments_written()
        if w_:
            out.row_moments = (rm, w_)  # likewise: (fp32 [m][ld][2], tile width)


class gemm_concurrency:
    """``with gemm_concurrency(n):`` -- the GEMM launches issued (or CAPTURED) inside by THIS thread run beside n - 1 independent
    launches of the same shape on other streams; passed to every call as ``mvoc_gemm_desc.concurrency`` (include/mvoc_hip.h).
    Host-side and thread-local: the library itself keeps no such state."""

    def __init__(self, n):
        self.n = max(1, int(n))

    def __enter__(self):
        self.old, _CONCURRENCY.n = _CONCURRENCY.n, self.n
        return self

    def __exit__(self, *exc):
        _CONCURRENCY.n = self.old


def chan_sums_of(x, rows_per_sample):
    """the producer's per-slab channel sums of the rows in ``x`` if the GEMM that wrote it emitted them and they fit the norm"""
    cs = getattr(x, "chan_sums", None)
    if cs is None or rows_per_sample % 256 or cs.shape[0] * 256 != x.shape[0] or cs.shape[1] != x.shape[1]:
        return None
    return cs


def _fill_common(d, x, x2, w, out, bias, rowadd, rowadd_div, resid, act, n_store, tile):
    d.a, d.a2, d.w, d.out = _ptr(x), _ptr(x2), _ptr(w), _ptr(out)
    d.bias, d.rowadd, d.resid = _ptr(bias), _ptr(rowadd), _ptr(resid)
    d.n = w.shape[0]
    d.k = w.shape[1]
    d.n_store = n_store
    d.ldo = out.stride(0)
    d.ldr = resid.stride(0) if resid is not None else 0
    d.ld_rowadd = rowadd.stride(0) if rowadd is not None else 0
    d.rowadd_div = rowadd_div
    d.lda = x.stride(0)
    d.lda2 = x2.stride(0) if x2 is not None else 0
    d.act = act
    d.tile = tile


def _out_cols(w, n_store, act):
    if act == ACT_GEGLU:
        return w.shape[0] // 2
    return n_store if n_store else w.shape[0]


def linear(x, w, bias=None, *, x2=None, act=ACT_NONE, resid=None, n_store=0, out=None, rowadd=None, rowadd_div=1, tile=0,
           split_k=0, ln=None, sums=False, rowmom=False):
    """out[M, n] = act(x @ w.T + bias) (+ resid).  ``x2``: second source of a channel concat ([x | x2] @ w.T).
    ``ln=(rowsum fp32 [n], lnbias fp32 [n], eps)``: LayerNorm(x) folded into the GEMM (w must be gamma-scaled).
    ``rowmom``: ask for the row statistics of the OUTPUT (the LayerNorm that reads it next: ``row_stats_of``)."""
    _chk(x, "x"), _chk(w, "w"), _chk(bias, "bias"), _chk(x2, "x2"), _chk(resid, "resid"), _chk(rowadd, "rowadd")
    _rowmajor(x, "x")
    m = x.shape[0]
    k1 = x.shape[1]
    k2 = x2.shape[1] if x2 is not None else 0
    if k1 + k2 != w.shape[1]:
        raise RuntimeError(f"linear: K mismatch {k1}+{k2} vs weight {tuple(w.shape)}")
    cols = _out_cols(w, n_store, act)
    if out is None:
        out = torch.empty((m, cols), dtype=torch.float16, device=x.device)
    d = GemmDesc()
    _fill_common(d, x, x2, w, out, bias, rowadd, rowadd_div, resid, act, cols if act != ACT_GEGLU else 0, tile)
    d.m = m
    d.a_mode = A_PLAIN
    d.c1 = k1
    d.cin = k1 + k2
    d.split_k = split_k
    if ln is not None:
        rowsum, lnbias, eps = ln[:3]
        _chk(rowsum, "ln rowsum", torch.float32), _chk(lnbias, "ln bias", torch.float32)
        d.ln_rowsum, d.ln_bias, d.ln_eps, d.split_k = rowsum.data_ptr(), lnbias.data_ptr(), eps, 1
        stats = ln[3] if len(ln) > 3 and ln[3] is not None else row_stats_of(x, eps)  # (the library has no in-kernel statistics any more)
        d.ln_stats = _chk(stats, "ln stats", torch.float32).data_ptr()
    _gemm(d, x.device, out, sums, rowmom)
    return out


# ---- chunk-major K order of the conv / temporal-conv weights (include/mvoc_hip.h: mvoc_gemm_desc.k_order) -----------------------------------
K_ORDER_CHUNK = os.environ.get("MVOC_KORDER", "1") != "0"
_CHUNK_CACHE = {}


def chunk_major_weights(w, ntaps):
    """tap-major conv weights [N, ntaps * cin] (k = tap * cin + c; unet.pack_conv3x3 / pack_tconv) -> chunk-major
    [N, (cin / 64) * ntaps * 64] (k = (c / 64) * ntaps * 64 + tap * 64 + c % 64).  Built once per weight tensor and kept (the weights
    of a loaded network are persistent; the cache holds a reference to the source so its address cannot be reused)."""
    key = (w.data_ptr(), tuple(w.shape), ntaps)
    hit = _CHUNK_CACHE.get(key)
    if hit is not None and hit[0] is w:
        return hit[1]
    n, k = w.shape
    cin = k // ntaps
    if k != ntaps * cin or cin % 64:
        raise RuntimeError(f"chunk_major_weights: k = {k} is not {ntaps} taps of a multiple of 64 channels")
    wc = w.view(n, ntaps, cin // 64, 64).permute(0, 2, 1, 3).reshape(n, k).contiguous()
    _CHUNK_CACHE[key] = (w, wc)
    return wc


def _g8_choice(m, n, conc, geglu=False):
    """gemm.hip's choice for an un-forced launch (the `eff` model there): 82 / 81 when the 320- / 256-wide eight-phase grid fills
    >= 55 % of the chip after quantisation and prices better, else 0 (another tile family takes the launch)"""
    def eff(bx, rate):
        nt = (n + bx - 1) // bx
        blocks = ((m + 255) // 256) * nt * conc
        return n / (nt * bx) * blocks / (((blocks + 255) // 256) * 256) * rate
    e81 = eff(256, 1.0)
    e82 = eff(320, 0.85) if (not geglu and n % 320 == 0) else 0.0
    if e81 < 0.55 and e82 < 0.55:
        return 0
    return 82 if e82 > e81 else 81


def _chunk_ok(d, x, x2, w, out, bias, resid, rowadd, ntaps, rows_a):
    """mirror of gemm.hip's g8_ok for a conv / temporal launch + the grid-fill rule: a k_order = 1 request the library cannot place on
    the eight-phase tiles is an error there (the caller holds the tap-major weights), so it is only made where it will be taken"""
    lim = 1 << 31
    al = lambda t: t is None or t.data_ptr() % 16 == 0
    return (K_ORDER_CHUNK and d.cin % 64 == 0 and d.c1 % 64 == 0 and d.k == ntaps * d.cin and d.m >= 1024 and d.tile in (0, 81, 82) and not d.upsample
            and d.split_k <= 1 and d.pad_mode == 0
            and out.stride(0) % 8 == 0 and d.n_store % 8 == 0 and al(out) and al(bias) and al(resid) and al(rowadd)
            and (resid is None or resid.stride(0) % 8 == 0) and (rowadd is None or (rowadd.stride(0) % 8 == 0 and d.rowadd_div >= 64))
            and rows_a * x.stride(0) * 2 < lim and (x2 is None or rows_a * x2.stride(0) * 2 < lim) and w.shape[0] * d.k * 2 < lim
            and d.m * out.stride(0) * 2 < lim and (resid is None or d.m * resid.stride(0) * 2 < lim)
            # Measured (profiles/r6/gemm_per_shape_pmc_korder.txt): FETCH falls 3-7 x on every conv (L2 hit rate 52 -> 85-92 %) and the
            # held clock rises; the 320-wide tile, whose activation offsets are formed at issue time anyway, gains (temporal K = 960:
            # - 7 %); the 256-wide tile paid 7-18 % for rebuilding its four offset registers EVERY K tile -- so the library has the
            # form for the 320-wide tile on an affine gather only (gemm8.hip: KO)
            and w.shape[0] % 320 == 0 and (d.tile == 82 or (d.tile == 0 and _g8_choice(d.m, w.shape[0], _CONCURRENCY.n) == 82))
            and (d.a_mode != A_CONV3X3 or (d.stride == 1 and d.hsrc == d.hout and d.wsrc == d.wout)))


SUBPIXEL_MIN_TILES = 200  # the sub-pixel form of Upsample2D + conv needs a grid that fills the chip; under it the 9-tap split-K form
#                           stays (8 -> 16 at batch 1).  Tests set 0 to put every upsampler of a small forward on the sub-pixel form.


def conv3x3(x, w, bias, *, nimg, h, wd, x2=None, stride=1, upsample_to=None, rowadd=None, rowadd_div=1, resid=None,
            n_store=0, out=None, tile=0, split_k=0, pad_mode=0, sums=False, w_subpixel=None):
    """3x3 conv, pad 1, on channels-last images x [nimg*h*wd, C1] (+ x2 [.., C2]); w [N, Kpad>=9*(C1+C2)] tap-major.
    ``upsample_to=(H2, W2)`` folds a nearest upsample of the source into the gather (Upsample2D).
    ``pad_mode=1``: zeros at the bottom / right only (``F.pad(x, (0,1,0,1))`` + ``conv2d(padding=0)``: VAE downsamplers).
    ``w_subpixel`` (``unet.pack_conv3x3_subpixel(w)``): with an exact 2x ``upsample_to`` the conv runs in its sub-pixel form -- four
    2 x 2 parity kernels on the source image, 4 taps of matrix work instead of 9 (include/mvoc_hip.h: upsample == 2)."""
    _chk(x, "x"), _chk(w, "w"), _chk(bias, "bias"), _chk(x2, "x2"), _chk(resid, "resid"), _chk(rowadd, "rowadd")
    _rowmajor(x, "x")
    c1 = x.shape[1]
    cin = c1 + (x2.shape[1] if x2 is not None else 0)
    hup, wup = (upsample_to if upsample_to is not None else (h, wd))
    pt = 2 if pad_mode == 0 else 1  # total padding per axis
    ho = (hup + pt - 3) // stride + 1
    wo = (wup + pt - 3) // stride + 1
    m = nimg * ho * wo
    cols = _out_cols(w, n_store, ACT_NONE)
    if out is None:
        out = torch.empty((m, cols), dtype=torch.float16, device=x.device)
    d = GemmDesc()
    _fill_common(d, x, x2, w, out, bias, rowadd, rowadd_div, resid, ACT_NONE, cols, tile)
    d.m = m
    d.a_mode = A_CONV3X3
    d.c1, d.cin = c1, cin
    d.nimg, d.hout, d.wout, d.hsrc, d.wsrc, d.stride = nimg, ho, wo, h, wd, stride
    d.upsample = 1 if upsample_to is not None else 0
    d.hup, d.wup = hup, wup
    d.split_k = split_k
    d.pad_mode = pad_mode
    lim = 1 << 31  # the eight-phase tiles address every operand through 32-bit MUBUF offsets (gemm.hip: g8_ok -- mirrored here,
    #               because a sub-pixel request the library cannot place on them is an error there, not a fall-back)
    if (w_subpixel is not None and upsample_to is not None and (hup, wup) == (2 * h, 2 * wd) and stride == 1 and x2 is None and
            resid is None and rowadd is None and pad_mode == 0 and (nimg * h * wd) % 256 == 0 and m >= 1024 and c1 % 64 == 0 and
            tile in (0, 81) and out.stride(0) % 8 == 0 and cols % 8 == 0 and
            w_subpixel.is_contiguous() and out.data_ptr() % 16 == 0 and (bias is None or bias.data_ptr() % 16 == 0) and
            nimg * h * wd * x.stride(0) * 2 < lim and m * out.stride(0) * 2 < lim and w.shape[0] * 4 * cin * 2 < lim and
            (tile == 81 or (m // 256) * ((w.shape[0] + 255) // 256) * _CONCURRENCY.n >= SUBPIXEL_MIN_TILES)):  # (an under-filled grid keeps the split-K form)
        _chk(w_subpixel, "w_subpixel")
        if tuple(w_subpixel.shape) != (4 * w.shape[0], 4 * cin):
            raise RuntimeError("conv3x3: w_subpixel must be pack_conv3x3_subpixel() of the same kernel")
        d.upsample, d.w, d.k, d.split_k = 2, w_subpixel.data_ptr(), 4 * cin, 1
        sums = False
    elif _chunk_ok(d, x, x2, w, out, bias, resid, rowadd, 9, nimg * h * wd):
        d.w, d.k_order, d.split_k = chunk_major_weights(w, 9).data_ptr(), 1, 1
    _gemm(d, x.device, out, sums)
    return out, ho, wo


def tconv3(x, w, bias, *, nvid, frames, hw, resid=None, out=None, tile=0, split_k=0, sums=False):
    """Conv3d (3,1,1), pad (1,0,0), on x [nvid*frames*hw, C]; w [N, 3*C] tap-major."""
    _chk(x, "x"), _chk(w, "w"), _chk(bias, "bias"), _chk(resid, "resid")
    _rowmajor(x, "x")
    m = nvid * frames * hw
    if out is None:
        out = torch.empty((m, w.shape[0]), dtype=torch.float16, device=x.device)
    d = GemmDesc()
    _fill_common(d, x, None, w, out, bias, None, 1, resid, ACT_NONE, w.shape[0], tile)
    d.m = m
    d.a_mode = A_TEMPORAL3
    d.c1 = d.cin = x.shape[1]
    d.frames, d.hw = frames, hw
    d.split_k = split_k
    if _chunk_ok(d, x, None, w, out, bias, resid, None, 3, m):
        d.w, d.k_order, d.split_k = chunk_major_weights(w, 3).data_ptr(), 1, 1
    _gemm(d, x.device, out, sums)
    return out


class _FlashMode(threading.local):
    field = 0


_FLASH_MODE = _FlashMode()


def flash_pipelined(mode):
    """kernel choice of the flash_attn calls THIS thread makes from now on (passed per call as ``mvoc_attn_desc.pipelined``; the library
    itself keeps no such state): -1 by key count (default), 0 the phase kernel always, 1 the software-pipelined kernel wherever it
    applies; same bits either way"""
    _FLASH_MODE.field = {-1: 0, 0: 1, 1: 2}[int(mode)]


def flash_attn(q, k, v, *, nbatch, heads, tq, tk, kv_bdiv=1, out=None, head_dim=64, causal=False, scale=0.0, v2=None, out2=None):
    """softmax(q k^T * scale) v.  q [nbatch*tq, >=heads*head_dim] / k, v [(nbatch/kv_bdiv)*tk, ..] row-major views.
    head_dim 64 (scale 1/8) is the UNet's; 96 + an explicit scale + ``causal`` serve the CLIP towers (clip.py).
    ``v2`` / ``out2`` (views laid out like ``v`` / ``out``): a second value tensor attending with the same q and k -- the PnP
    destination pair (include/mvoc_hip.h); the result equals two plain calls bit for bit."""
    _chk(q, "q"), _chk(k, "k"), _chk(v, "v"), _chk(v2, "v2"), _chk(out2, "out2")
    if out is None:
        out = torch.empty((nbatch * tq, heads * head_dim), dtype=torch.float16, device=q.device)
    d = AttnDesc()
    d.q, d.k, d.v, d.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    if v2 is not None:
        if out2 is None or _rowmajor(v2, "v2") != _rowmajor(v, "v") or _rowmajor(out2, "out2") != _rowmajor(out, "out"):
            raise RuntimeError("flash_attn: the paired form needs out2, and v2 / out2 laid out like v / out")
        d.v2, d.out2 = v2.data_ptr(), out2.data_ptr()
    d.q_ts, d.k_ts, d.v_ts, d.o_ts = _rowmajor(q, "q"), _rowmajor(k, "k"), _rowmajor(v, "v"), _rowmajor(out, "out")
    d.q_bs, d.k_bs, d.v_bs, d.o_bs = tq * d.q_ts, tk * d.k_ts, tk * d.v_ts, tq * d.o_ts
    d.nbatch, d.heads, d.tq, d.tk, d.kv_bdiv = nbatch, heads, tq, tk, kv_bdiv
    d.head_dim, d.causal, d.scale = head_dim, int(bool(causal)), scale
    d.pipelined = _FLASH_MODE.field
    check(lib.mvoc_flash_attn_f16(C.byref(d), _stream()), "flash_attn")
    return out


def temporal_attn(q, k, v, *, nsample, frames, hw, heads, out=None):
    """Attention over the frame axis of canonical [nsample, frames, hw, C] rows (q/k/v may be column slices)."""
    _chk(q, "q"), _chk(k, "k"), _chk(v, "v")
    if out is None:
        out = torch.empty((nsample * frames * hw, heads * 64), dtype=torch.float16, device=q.device)
    d = TAttnDesc()
    d.q, d.k, d.v, d.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    for name, t in (("q", q), ("k", k), ("v", v), ("o", out)):
        ld = _rowmajor(t, name)
        setattr(d, name + "_ps", ld)
        setattr(d, name + "_ts", hw * ld)
        setattr(d, name + "_bs", frames * hw * ld)
    d.nsample, d.hw, d.heads, d.frames = nsample, hw, heads, frames
    check(lib.mvoc_temporal_attn_f16(C.byref(d), _stream()), "temporal_attn")
    return out


XS_K = (64, 128, 320)   # activation-stationary kernels: the rows' K channels live in registers


def xs_linear(x, wp, n, *, normalize=False, eps=1e-5, act=ACT_NONE, resid=None, n_store=0, out=None, set_rows=0):
    """activation-stationary linear (include/mvoc_hip.h: mvoc_xs_linear_f16): x contiguous [m, k]; wp = unet.pack_xs_weights(W
    [n, k], constants [n]) (fragment-ordered weights + the per-channel constants); ``normalize``: LayerNorm folded (rows
    normalised in registers; W gamma-scaled, constants = beta @ W^T + bias)"""
    _chk(x, "x"), _chk(wp, "wp"), _chk(resid, "resid")
    m, k = x.shape
    nsets = m // set_rows if set_rows else 1
    if not x.is_contiguous() or k % 16 or n % 32 or wp.numel() != nsets * (n // 32) * (k // 16 + 1) * 512 or (set_rows and m % set_rows):
        raise RuntimeError("xs_linear: x must be contiguous [m, k] and wp the pack_xs_weights() image of an [n, k] matrix "
                           "(one image per set_rows rows when set_rows is given)")
    cols = n // 2 if act == ACT_GEGLU else (n_store if n_store else n)
    if out is None:
        out = torch.empty((m, cols), dtype=torch.float16, device=x.device)
    d = XsDesc()
    d.x, d.wp, d.resid, d.out = x.data_ptr(), wp.data_ptr(), _ptr(resid), out.data_ptr()
    d.m, d.n, d.k, d.n_store, d.ldo = m, n, k, cols, _rowmajor(out, "out")
    d.ldr = _rowmajor(resid, "resid") if resid is not None else 0
    d.act, d.normalize, d.ln_eps, d.wp_set_rows = act, int(bool(normalize)), eps, set_rows
    check(lib.mvoc_xs_linear_f16(C.byref(d), _stream()), "xs_linear")
    return out


TFUSED_CHANNELS = (64, 128, 320)
TFUSED_FRAMES = (8, 16, 32)


def temporal_qkv_attn(x, wp, ln, *, nsample, frames, hw, heads, out=None):
    """LayerNorm -> QKV -> attention over the frame axis in one kernel (see include/mvoc_hip.h): x raw rows
    [nsample*frames*hw, c], wp the fragment-packed gamma-scaled QKV weights, ln = (rowsum fp32 [3c], bias fp32 [3c], eps)."""
    _chk(x, "x"), _chk(wp, "wp"), _chk(ln[0], "ln rowsum", torch.float32), _chk(ln[1], "ln bias", torch.float32)
    c = heads * 64
    if not x.is_contiguous() or tuple(x.shape) != (nsample * frames * hw, c):
        raise RuntimeError(f"temporal_qkv_attn: x must be contiguous [{nsample * frames * hw}, {c}], got {tuple(x.shape)}")
    if wp.numel() != 3 * c * c or ln[0].numel() != 3 * c or ln[1].numel() != 3 * c:
        raise RuntimeError("temporal_qkv_attn: packed weights / LayerNorm vectors do not match c")
    if out is None:
        out = torch.empty_like(x)
    d = TFusedDesc()
    d.x, d.wp, d.ln_rowsum, d.ln_bias, d.out = x.data_ptr(), wp.data_ptr(), ln[0].data_ptr(), ln[1].data_ptr(), out.data_ptr()
    d.nsample, d.frames, d.hw, d.c, d.heads, d.ln_eps = nsample, frames, hw, c, heads, ln[2]
    check(lib.mvoc_temporal_qkv_attn_f16(C.byref(d), _stream()), "temporal_qkv_attn")
    return out


def _gn_desc(x, gamma, beta, x2, out, nsample, rows_per_sample, groups, eps, silu):
    _chk(x, "x"), _chk(gamma, "gamma"), _chk(beta, "beta"), _chk(x2, "x2")
    c1 = x.shape[1]
    c = c1 + (x2.shape[1] if x2 is not None else 0)
    if not x.is_contiguous() or (x2 is not None and not x2.is_contiguous()):
        raise RuntimeError("groupnorm: inputs must be contiguous")
    wsb = lib.mvoc_groupnorm_workspace_bytes(nsample, rows_per_sample, c, groups)
    ws = torch.empty((max(wsb, 4) + 3) // 4, dtype=torch.float32, device=x.device)
    d = GnDesc()
    d.x, d.x2, d.gamma, d.beta, d.out = x.data_ptr(), _ptr(x2), _ptr(gamma), _ptr(beta), _ptr(out)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    d.nsample, d.rows_per_sample, d.c, d.c1, d.groups, d.silu, d.eps = nsample, rows_per_sample, c, c1, groups, int(silu), eps
    return d, ws


USE_CHAN_SUMS = os.environ.get("MVOC_CHAN_SUMS", "1") != "0"  # MVOC_CHAN_SUMS=0: every GroupNorm reads its own statistics (A/B)


def groupnorm(x, gamma, beta, *, nsample, rows_per_sample, groups, eps, silu, x2=None, out=None):
    """GroupNorm over ``rows_per_sample`` rows x (C/groups) channels per sample, optional fused SiLU; [x | x2] concat.
    When the GEMMs that produced x (and x2) left their per-slab channel sums on the tensors (``_gemm``), the statistics pass
    over the input is skipped."""
    c = x.shape[1] + (x2.shape[1] if x2 is not None else 0)
    if out is None:
        out = torch.empty((nsample * rows_per_sample, c), dtype=torch.float16, device=x.device)
    d, ws = _gn_desc(x, gamma, beta, x2, out, nsample, rows_per_sample, groups, eps, silu)
    cs = chan_sums_of(x, rows_per_sample) if USE_CHAN_SUMS else None
    cs2 = chan_sums_of(x2, rows_per_sample) if (x2 is not None and cs is not None) else None
    if cs is not None and (x2 is None or cs2 is not None) and x.shape[1] % (c // groups) == 0:
        d.chan_sums, d.chan_sums2 = cs.data_ptr(), _ptr(cs2)
    check(lib.mvoc_groupnorm_f16(C.byref(d), _stream()), "groupnorm")
    return out


def groupnorm_fold_xs(x, gamma, beta, w, bias, *, nsample, rows_per_sample, groups, eps):
    """GroupNorm(x) folded into the linear ``w`` [n, k] (+ ``bias``) that reads it (include/mvoc_hip.h:
    mvoc_groupnorm_fold_xs_f16): the per-sample weight streams for ``xs_linear(x_raw, wp, n, set_rows=rows_per_sample)``; the
    statistics come from the producer's channel sums when x carries them"""
    _chk(w, "w"), _chk(bias, "bias")
    n, k = w.shape
    if k != x.shape[1] or n % 32 or k % 16 or not w.is_contiguous():
        raise RuntimeError("groupnorm_fold_xs: w must be contiguous [n % 32 == 0, k == channels of x]")
    d, ws = _gn_desc(x, gamma, beta, None, None, nsample, rows_per_sample, groups, eps, False)
    cs = chan_sums_of(x, rows_per_sample) if USE_CHAN_SUMS else None
    if cs is not None:
        d.chan_sums = cs.data_ptr()
    wp = torch.empty((nsample, n // 32, k // 16 + 1, 512), dtype=torch.float16, device=x.device)
    check(lib.mvoc_groupnorm_fold_xs_f16(C.byref(d), w.data_ptr(), _ptr(bias), n, k, wp.data_ptr(), _stream()), "groupnorm_fold_xs")
    return wp


def groupnorm_moments(x, *, nsample, rows_per_sample, groups):
    """This rank's {count, mean, M2} per (sample, group): fp32 [nsample, groups, 3] (first half of a sharded GroupNorm)."""
    mom = torch.empty((nsample, groups, 3), dtype=torch.float32, device=x.device)
    d, ws = _gn_desc(x, None, None, None, None, nsample, rows_per_sample, groups, 0.0, False)
    check(lib.mvoc_groupnorm_moments_f16(C.byref(d), mom.data_ptr(), _stream()), "groupnorm_moments")
    return mom


def groupnorm_apply_moments(x, parts, gamma, beta, *, nsample, rows_per_sample, groups, eps, silu, out=None):
    """Second half: ``parts`` fp32 [nparts, nsample, groups, 3] (all ranks' moments in rank order) -> normalised rows."""
    _chk(parts, "parts", torch.float32)
    if parts.dim() != 4 or tuple(parts.shape[1:]) != (nsample, groups, 3) or not parts.is_contiguous():
        raise RuntimeError(f"groupnorm_apply_moments: parts must be contiguous [nparts, {nsample}, {groups}, 3]")
    if out is None:
        out = torch.empty((nsample * rows_per_sample, x.shape[1]), dtype=torch.float16, device=x.device)
    d, ws = _gn_desc(x, gamma, beta, None, out, nsample, rows_per_sample, groups, eps, silu)
    check(lib.mvoc_groupnorm_apply_moments_f16(C.byref(d), parts.data_ptr(), parts.shape[0], _stream()), "groupnorm_apply_moments")
    return out


def row_stats(x, eps=1e-5):
    """{mean, rstd} per row, fp32 [rows, 2]"""
    _chk(x, "x")
    if not x.is_contiguous():
        raise RuntimeError("row_stats: x must be contiguous")
    out = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    check(lib.mvoc_row_stats_f16(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], eps, _stream()), "row_stats")
    return out


def row_stats_of(x, eps=1e-5):
    """{mean, rstd} per row of x: from the row moments the producing GEMM left on the tensor (``_gemm``) when there are any -- a few
    bytes per row instead of a pass over the tensor -- else ``row_stats``"""
    rm = getattr(x, "row_moments", None)
    if rm is None or not USE_ROW_MOMENTS or rm[0].shape[0] != x.shape[0]:
        return row_stats(x, eps)
    mom, tile_w = rm
    out = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    check(lib.mvoc_row_stats_from_moments_f32(mom.data_ptr(), x.shape[0], mom.shape[1], x.shape[1], tile_w, eps, out.data_ptr(), _stream()),
          "row_stats_from_moments")
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    _chk(x, "x"), _chk(gamma, "gamma"), _chk(beta, "beta")
    if not x.is_contiguous():
        raise RuntimeError("layernorm: x must be contiguous")
    if out is None:
        out = torch.empty_like(x)
    check(lib.mvoc_layernorm_f16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                 eps, _stream()), "layernorm")
    return out


def _pnp_desc(x, x2, masks, chunk_stride, f_stride, p_stride, frames, height, width, channels, base_chunk0, ndst=2):
    _chk(x, "x"), _chk(x2, "x2"), _chk(masks, "masks")
    if masks.dim() == 5 and masks.is_contiguous() and masks.shape[2] == frames:
        # per-variant placement: a [K, nobj, F, mh, mw] stack.  The descriptor has no field for K: it takes the
        # stack's pointer (variant 0 first) and one variant's dims; K and the stack's shape are checked against the 4-D table by
        # _check_table, and both blend functions refuse a stack that comes without such a table before any launch (_blend_entry)
        masks = masks[0]
    if masks.dim() != 4 or not masks.is_contiguous() or masks.shape[1] != frames:
        raise RuntimeError(f"pnp: masks must be contiguous [nobj, F, mh, mw] fp16, got {tuple(masks.shape)}")
    d = PnpDesc()
    d.x, d.x2, d.masks = x.data_ptr(), _ptr(x2), masks.data_ptr()
    d.chunk_stride, d.f_stride, d.p_stride = chunk_stride, f_stride, p_stride
    d.nobj, d.frames, d.height, d.width, d.channels = masks.shape[0], frames, height, width, channels
    d.mask_h, d.mask_w, d.base_chunk0, d.ndst = masks.shape[2], masks.shape[3], int(base_chunk0), int(ndst)
    return d


def _src_map_args(src_map, nobj):
    """``src_map`` = (nsrc, obj_chunks) of the source-de-duplicated batch [s_0..s_{nsrc-1}, destinations..] -> ctypes args"""
    nsrc, chunks = src_map
    if len(chunks) != nobj:
        raise RuntimeError(f"pnp: the source map names {len(chunks)} objects, the masks {nobj}")
    return int(nsrc), (C.c_int32 * nobj)(*[int(c) for c in chunks])


def _variant_map(src_map, nobj):
    """the ``_variants`` entries always take a map: the positional sources [bg, obj_1..obj_n] are the identity map"""
    return _src_map_args(src_map if src_map is not None else (nobj + 1, tuple(range(1, nobj + 1))), nobj)


def _check_variants(x, x2, nvar, need, what):
    """the variants kernels address chunk nsrc + ndst*nvar - 1 of each tensor: refuse a buffer that does not reach it"""
    if not 1 <= int(nvar) <= 8:
        raise RuntimeError(f"{what}: variants {nvar} not in [1, 8]")
    for t in (x, x2):
        if t is not None and t.storage_offset() + need > t.untyped_storage().nbytes() // t.element_size():
            raise RuntimeError(f"{what}: the tensor's storage ends before the last destination chunk "
                               f"(needs {need} elements from its first)")


def _active_mask(active, nvar, what):
    """``active`` (per-variant injection schedules) -> None when every variant injects (today's entries), else
    the bitmask for the ``_sel`` entries"""
    if active is None:
        return None
    active, nvar = int(active), int(nvar)
    if not 1 <= nvar <= 8:
        raise RuntimeError(f"{what}: variants {nvar} not in [1, 8]")
    if not 1 <= active < (1 << nvar):
        raise RuntimeError(f"{what}: active mask {active:#x} not in [1, 2^{nvar}): bit k set = variant k injects")
    return None if active == (1 << nvar) - 1 else active


# ---- the table forms: one row per keyword of ``pnp_blend_<layout>`` that hands the blend a device table --------------
# keyword       the argument of ``pnp_blend_tokens`` / ``pnp_blend_nchw``
# suffix        the entry is mvoc_pnp_blend_scatter_<layout><suffix>
# per_variant   a 4-D [K, nobj, F, ..] table next to a [K, nobj, F, mh, mw] mask stack is allowed: <suffix>_variants (6l, 6o)
# tail          descriptor -> the table's dims after [nobj, F] as (how a message writes it, size)
# noun          what the message about the mask stack calls a per-variant table, after its shape
# together      the refusal when a keyword of an EARLIER row is given as well (a later row outranks an earlier one)
# stack         the refusal of a mask stack that has no per-variant table of this form beside it
# no_background where ``no_background`` is refused for the keyword: None -- not by name (the positional flag's own refusal in
#               ``pnp_blend_tokens`` names a placement); "entry" -- where the entry is chosen; "first" -- before that refusal
_TableForm = collections.namedtuple("_TableForm", "keyword suffix per_variant tail noun together stack no_background")
_NO_STACK = "does not take a [K, nobj, F, mh, mw] mask stack"
_TABLE_FORMS = (
    _TableForm("place", "_placed", True, lambda d: (("2", 2),), "", None,
               "a [K, nobj, F, mh, mw] mask stack needs place= as an int32 [K, nobj, F, 2] table", None),
    _TableForm("resample", "_resampled", True, lambda d: (("H + W", d.height + d.width),), " resample",
               "resample= and place= are both given: a translation is part of the resample table",
               f"resample= {_NO_STACK}: one transform serves all variants", "entry"),
    _TableForm("warp", "_warped", False, lambda d: (("H * W", d.height * d.width),), "",
               "warp= is given together with place= / resample=: the 2-D map carries scale, mirror and translation",
               f"warp= {_NO_STACK}: one warp serves all variants", "first"),
    _TableForm("warp_taps", "_bilinear", False, lambda d: (("H * W", d.height * d.width), ("2", 2)), "",
               "warp_taps= is given together with place= / resample= / warp=: the tap table carries the whole warp",
               f"warp_taps= {_NO_STACK}: one warp serves all variants", "first"),
)


def _tail_text(tail):
    return ", ".join(label if label.isdigit() else f"{label} = {size}" for label, size in tail)


def _refuse_no_background(what, form):
    raise RuntimeError(f"{what}: {form.keyword}= with no_background: pass src_map=(nobj, range(nobj)) instead")


def _select_entry(what, tables, mask_dim, no_background, src_map, nvar, active):
    """(suffix, row, table) of the library entry mvoc_pnp_blend_scatter_<layout><suffix> that the arguments of
    ``pnp_blend_<layout>`` select: by the one table given in ``tables`` (keyword -> table or None; a 3-D table shared by the
    variants, or where the row allows it a 4-D table per variant, which goes with a 5-D [K, nobj, F, mh, mw] mask stack and the
    stack with nothing else), else by ``src_map`` / ``nvar`` / ``active``; every other combination is refused"""
    given = [f for f in _TABLE_FORMS if tables.get(f.keyword) is not None]
    form = given[-1] if given else None
    table = tables[form.keyword] if form else None
    if len(given) > 1:
        raise RuntimeError(f"{what}: {form.together}")
    per_variant = form is not None and form.per_variant and torch.is_tensor(table) and table.dim() == 4
    if mask_dim == 5 and not per_variant:
        raise RuntimeError(f"{what}: {(form or _TABLE_FORMS[0]).stack}")
    if form is None:
        if nvar == 1:
            return "" if src_map is None else "_mapped", None, None
        return "_variants" if active is None else "_variants_sel", None, None
    if no_background and form.no_background:
        _refuse_no_background(what, form)
    return form.suffix + ("_variants" if per_variant else ""), form, table


def _blend_entry(what, place, resample, mask_dim, no_background, src_map, nvar, active, warp=None, warp_taps=None):
    """the suffix ``_select_entry`` chooses, with the tables as arguments (``place`` / ``resample``: DESIGN.md 6k-6o, ``warp``: 6q,
    ``warp_taps``: 6r)"""
    tables = dict(place=place, resample=resample, warp=warp, warp_taps=warp_taps)
    return _select_entry(what, tables, mask_dim, no_background, src_map, nvar, active)[0]


def _check_table(what, name, table, masks, nvar, d):
    """the form of the table of keyword ``name`` against the descriptor: int32 [nobj, F, <the row's tail>], or where the row allows
    it per variant [K, nobj, F, ..] next to a [K, nobj, F, mh, mw] mask stack"""
    _chk(table, name, torch.int32)
    form = next(f for f in _TABLE_FORMS if f.keyword == name)
    tail = form.tail(d)
    shape, dims = (d.nobj, d.frames) + tuple(size for _, size in tail), f"nobj = {d.nobj}, F = {d.frames}"
    per_variant = form.per_variant and table.dim() == 4
    if per_variant:
        shape, dims = (int(nvar),) + shape, f"K = {int(nvar)}, " + dims
    if tuple(table.shape) != shape or not table.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be a contiguous int32 [{dims}, {_tail_text(tail)}] table"
                           f"{' with a [K, nobj, F, mh, mw] mask stack' if per_variant else ''}, got {tuple(table.shape)}")
    if per_variant and (masks.dim() != 5 or tuple(masks.shape[:3]) != shape[:3] or not masks.is_contiguous()):
        raise RuntimeError(f"{what}: a [K, nobj, F, {', '.join(label for label, _ in tail)}]{form.noun} table needs masks as a "
                           f"contiguous [{dims}, mh, mw] stack, got {tuple(masks.shape)}")


def _pnp_blend(layout, d, x, x2, masks, need, ndst, src_map, nvar, active, tables, no_background=False):
    """call the library entry mvoc_pnp_blend_scatter_<layout><suffix> that the arguments of ``pnp_blend_<layout>`` select
    (``_select_entry``) on the descriptor ``d``; ``need(nchunk)``: elements a tensor must hold from its first for a batch of
    nchunk chunks"""
    what = f"pnp_blend_{layout}"
    suffix, form, table = _select_entry(what, tables, masks.dim(), no_background, src_map, nvar, active)

    def call(*args):
        name = f"pnp_blend_scatter_{layout}{suffix}"
        check(getattr(lib, "mvoc_" + name)(C.byref(d), *args, _stream()), name)

    if suffix == "":
        return call()
    if suffix == "_mapped":
        return call(*_src_map_args(src_map, d.nobj))
    nsrc, chunks = _variant_map(src_map, d.nobj)
    _check_variants(x, x2, nvar, need(nsrc + (int(ndst) or 2) * int(nvar)), what)
    if suffix == "_variants":
        return call(nsrc, chunks, int(nvar))
    if suffix == "_variants_sel":
        return call(nsrc, chunks, int(nvar), active)
    # a table: its entries take the bitmask in every case (all bits: every variant injects)
    _check_table(what, form.keyword, table, masks, nvar, d)
    return call(nsrc, chunks, int(nvar), _all_or(active, nvar), table.data_ptr())


def pnp_blend_tokens(x, masks, *, frames, height, width, channels, chunk_stride, f_stride, p_stride, x2=None,
                     base_chunk0=False, ndst=2, src_map=None, nvar=1, active=None, place=None, no_background=False, resample=None,
                     warp=None, warp_taps=None):
    """In-place masked blend + scatter on channel-contiguous data (see include/mvoc_hip.h).  ``ndst``: trailing
    destination chunks (2 = [uncond, cond], 1 = [cond] with CFG off).  ``src_map`` = (nsrc, obj_chunks): the batch holds
    nsrc de-duplicated source chunks, object j reads chunk obj_chunks[j] (None: [bg, obj_1..obj_n], the unmapped entry).
    ``nvar`` = K > 1: K variants share the sources, the batch is [s.., u_1..u_K, c_1..c_K] ([s.., c_1..c_K] with ndst 1).
    ``active``: bit k set = variant k injects (None or all K bits: every variant, the entries of a call without it).
    ``place``: the table of ``place_table`` for this height x width: every object is read at its shifted pixel,
    ``masks`` are in destination coordinates -- the ``_placed`` entry, whatever ``nvar`` / ``src_map`` / ``active`` are.
    ``no_background``: the batch is [obj_1..obj_n, (uncond,) cond] with no background chunk in front -- the
    positional entry only: not with ``base_chunk0``, a map, variants or a placement (a map (nobj, range(nobj)) says the same
    there).
    ``resample``: the table of ``resample_table`` for this height x width: every object is read at the pixel its
    per-axis maps name (scale, mirror and translation, nearest), ``masks`` are in destination coordinates -- the ``_resampled``
    entry, whatever ``nvar`` / ``src_map`` / ``active`` are.  Not with ``place``, not with a per-variant mask stack.
    A 4-D ``resample`` (``resample_table_variants``) with a [K, nobj, F, mh, mw] mask stack: a transform and masks
    per variant -- the ``_resampled_variants`` entry.
    ``warp``: the table of ``warp_table`` for this height x width: every object is read at the pixel its 2-D map
    names (rotation with scale, mirror and translation, nearest), ``masks`` are in destination coordinates -- the ``_warped``
    entry, whatever ``nvar`` / ``src_map`` / ``active`` are.  Not with ``place`` / ``resample``, a per-variant mask stack or
    ``no_background``.
    ``warp_taps``: the table of ``warp_tap_table`` for this height x width: every object is interpolated from the
    four pixels its taps name (the same warps, bilinear on an exact fp16 chain) -- the ``_bilinear`` entry, whatever ``nvar`` /
    ``src_map`` / ``active`` are.  Not with ``place`` / ``resample`` / ``warp``, a per-variant mask stack or ``no_background``."""
    d = _pnp_desc(x, x2, masks, chunk_stride, f_stride, p_stride, frames, height, width, channels, base_chunk0, ndst)
    active = _active_mask(active, nvar, "pnp_blend_tokens")
    tables = dict(place=place, resample=resample, warp=warp, warp_taps=warp_taps)
    if no_background:
        if base_chunk0:
            raise RuntimeError("pnp_blend_tokens: no_background with base_chunk0: the base would be the chunk the batch does not hold")
        for form in _TABLE_FORMS:
            if form.no_background == "first" and tables[form.keyword] is not None:
                _refuse_no_background("pnp_blend_tokens", form)
        if src_map is not None or nvar != 1 or place is not None or active is not None:
            raise RuntimeError("pnp_blend_tokens: no_background is the positional entry's flag; with a source map, variants or a "
                               "placement pass src_map=(nobj, range(nobj)) instead")
        last = (d.nobj + (int(ndst) or 2) - 1) * chunk_stride
        _check_variants(x, x2, 1, last + (frames - 1) * f_stride + (height * width - 1) * p_stride + channels, "pnp_blend_tokens")
        d.base_chunk0 = -1  # (include/mvoc_hip.h: no background chunk, the base is the last chunk)
    reach = (frames - 1) * f_stride + (height * width - 1) * p_stride + channels  # of the last chunk's last element
    _pnp_blend("tokens", d, x, x2, masks, lambda nchunk: (nchunk - 1) * chunk_stride + reach, ndst, src_map, nvar, active, tables,
               no_background)
    return x


def pnp_blend_nchw(x, masks, *, frames, x2=None, base_chunk0=True, ndst=2, src_map=None, nvar=1, active=None, place=None,
                   resample=None, warp=None, warp_taps=None):
    """In-place on x [(nobj+1+ndst)*F, C, H, W] (reference feature-map layout); with ``src_map`` = (nsrc, obj_chunks)
    x is [(nsrc+ndst)*F, C, H, W], with ``nvar`` = K > 1 [(nsrc+ndst*K)*F, C, H, W]; ``active`` picks the variants that are
    written, ``place`` moves the objects, ``resample`` scales / mirrors / moves them, ``warp`` also turns them, ``warp_taps`` does so
    with bilinear sampling (see ``pnp_blend_tokens``)."""
    if x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError("pnp_blend_nchw: x must be contiguous [N, C, H, W]")
    d = _pnp_desc(x, x2, masks, 0, 0, 0, frames, x.shape[2], x.shape[3], x.shape[1], base_chunk0, ndst)
    active = _active_mask(active, nvar, "pnp_blend_nchw")
    _pnp_blend("nchw", d, x, x2, masks, lambda nchunk: nchunk * frames * x[0].numel(), ndst, src_map, nvar, active,
               dict(place=place, resample=resample, warp=warp, warp_taps=warp_taps))
    return x


# ---- placement: per-frame integer translation of the objects ------------------------------------------
def level_offset(d, size, mask_size):
    """the offset ``d`` (latent grid, ``mask_size`` rows or columns) on a feature grid of ``size``: round-half-up of
    d * size / mask_size in integers, floor division for negatives"""
    d, size, mask_size = int(d), int(size), int(mask_size)
    return (2 * d * size + mask_size) // (2 * mask_size)


def level_offsets(placement, height, width, mask_h, mask_w):
    """``placement`` = per object, per frame (dy, dx) on the mask_h x mask_w latent grid -> the same structure of (dfy, dfx)
    on a height x width feature grid (``level_offset`` per axis)"""
    return tuple(tuple((level_offset(dy, height, mask_h), level_offset(dx, width, mask_w)) for dy, dx in obj) for obj in placement)


def place_table(placement, height, width, mask_h, mask_w, device):
    """the device table the ``_placed`` blend entries read: int32 [nobj, F, 2] = (dfy, dfx) of ``level_offsets``.  An offset that
    does not fit int32 is refused here (the library cannot see the table's contents); every int32 value is valid to the kernels"""
    lv = level_offsets(placement, height, width, mask_h, mask_w)
    if len({len(o) for o in lv}) != 1 or not lv or not lv[0]:
        raise RuntimeError("place_table: every object needs the same number (>= 1) of per-frame offsets")
    for j, obj in enumerate(lv):
        for f, pair in enumerate(obj):
            if any(not -2 ** 31 <= v < 2 ** 31 for v in pair):
                raise RuntimeError(f"place_table: offset {pair} of object {j}, frame {f} does not fit int32")
    return torch.tensor(lv, dtype=torch.int32).to(device).contiguous()


def _per_variant(what, variants, noun, table):
    """[``table(v)`` for v in variants]; a refusal names the variant it came from"""
    if not variants:
        raise RuntimeError(f"{what}: needs at least one variant's {noun}")
    out = []
    for k, v in enumerate(variants):
        try:
            out.append(table(v))
        except RuntimeError as e:
            raise RuntimeError(f"{what}: variant {k}: {e}") from None
    return out


def place_table_variants(placements, height, width, mask_h, mask_w, device):
    """the device table the ``_placed_variants`` blend entries read: int32 [K, nobj, F, 2], row k = ``place_table`` of
    ``placements[k]`` (the same rule, ``level_offset``, and the same int32 refusal)"""
    tabs = _per_variant("place_table_variants", placements, "placement", lambda pl: place_table(pl, height, width, mask_h, mask_w, "cpu"))
    if len({tuple(t.shape) for t in tabs}) != 1:
        raise RuntimeError(f"place_table_variants: the variants' tables differ in shape: {[tuple(t.shape) for t in tabs]}")
    return torch.stack(tabs).to(device).contiguous()


def _all_or(active, nvar):
    """the ``_placed`` entries take the bitmask in every case: all bits for 'every variant injects'"""
    return (1 << int(nvar)) - 1 if active is None else active


def _move_planes(what, entry, src, table, tail, out, name):
    """what the four plane movers share: contiguous fp16 planes ``src`` [..., F, h, w] through the device table ``table`` (the
    argument ``name`` of ``what``), int32 [F, <tail(h, w)>] with the dims as (how a message writes it, size), into ``out`` (None: a new
    tensor) by the library's mvoc_<entry>_f16"""
    _chk(src, "src"), _chk(table, name, torch.int32)
    if src.dim() < 3 or not src.is_contiguous():
        raise RuntimeError(f"{what}: src must be contiguous [..., F, h, w], got {tuple(src.shape)}")
    frames, h, w = src.shape[-3:]
    dims = tail(h, w)
    if tuple(table.shape) != (frames,) + tuple(size for _, size in dims) or not table.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be a contiguous int32 [F = {frames}, {_tail_text(dims)}] table, got {tuple(table.shape)}")
    if out is None:
        out = torch.empty_like(src)
    _chk(out, "out")
    if out.shape != src.shape or not out.is_contiguous():
        raise RuntimeError(f"{what}: out must be contiguous and of src's shape")
    check(getattr(lib, f"mvoc_{entry}_f16")(src.data_ptr(), out.data_ptr(), src.numel() // (frames * h * w), frames, h, w,
                                            table.data_ptr(), _stream()), entry)
    return out


def shift_planes(src, offsets, out=None):
    """zero-filled per-frame integer translation of contiguous fp16 planes [..., F, h, w] (leading dims = planes of ONE
    object): out[.., f, y, x] = src[.., f, y - dy_f, x - dx_f] or 0.  ``offsets``: device int32 [F, 2] = (dy_f, dx_f)."""
    return _move_planes("shift_planes", "shift_planes", src, offsets, lambda h, w: (("2", 2),), out, name="offsets")


# ---- scale and mirror: nearest resampling through per-axis index maps ---------------------------------------
def level_axis_map(d, p, q, flip, a2, size, mask_size):
    """the source index of every destination index of ONE axis of a feature grid of ``size`` rows under a latent (mask) axis of
    ``mask_size`` rows -> a list of ``size`` ints, -1 where the object is absent.  The object appears ``p / q`` times its source
    size, mirrored when ``flip``, about the anchor ``a2`` / 2 (latent rows; pixel i has its centre at i + 1/2), then moved by
    ``d`` latent rows (``level_offset`` carries d to this level).  Python ints only: floor of the exact rational, which is nearest
    on pixel centres.  p == q without a flip is ``i - level_offset(d)``: the translation of DESIGN.md 6k."""
    d, p, q, a2, S, L = int(d), int(p), int(q), int(a2), int(size), int(mask_size)
    if p < 1 or q < 1 or S < 1 or L < 1:
        raise RuntimeError(f"level_axis_map: scale {p}/{q} and the sizes {S}, {L} must be positive")
    sg = -1 if flip else 1
    df = level_offset(d, S, L)
    out = []
    for i in range(S):
        num = a2 * S * p + sg * q * ((2 * (i - df) + 1) * L - a2 * S)
        s = num // (2 * p * L)
        out.append(s if 0 <= s < S else -1)
    return out


def transform_maps(transform, height, width, mask_h, mask_w):
    """``transform`` = per object (py, qy, px, qx, flip_y, flip_x, ay2, ax2, ((dy, dx) per frame)) -> nested lists
    [nobj][F][height + width]: per frame ``level_axis_map`` of the y axis, then of the x axis"""
    if not transform or len({len(t[8]) for t in transform}) != 1 or not transform[0][8]:
        raise RuntimeError("transform_maps: every object needs the same number (>= 1) of per-frame offsets")
    rows = []
    for py, qy, px, qx, fy, fx, ay2, ax2, offs in transform:
        ycache, xcache = {}, {}
        obj = []
        for dy, dx in offs:
            if dy not in ycache:
                ycache[dy] = level_axis_map(dy, py, qy, fy, ay2, height, mask_h)
            if dx not in xcache:
                xcache[dx] = level_axis_map(dx, px, qx, fx, ax2, width, mask_w)
            obj.append(ycache[dy] + xcache[dx])
        rows.append(obj)
    return rows


def resample_table(transform, height, width, mask_h, mask_w, device):
    """the device table the ``_resampled`` blend entries read: int32 [nobj, F, height + width] (``transform_maps``).  Every
    entry is in [-1, size) by construction; the kernels treat any other value as absent as well"""
    return torch.tensor(transform_maps(transform, height, width, mask_h, mask_w), dtype=torch.int32).to(device).contiguous()


def resample_table_variants(variant_transforms, height, width, mask_h, mask_w, device):
    """the device table the ``_resampled_variants`` blend entries read: int32 [K, nobj, F, height + width], row k
    = ``resample_table`` of ``variant_transforms[k]`` (the same rule, ``level_axis_map``)"""
    rows = _per_variant("resample_table_variants", variant_transforms, "transform",
                        lambda tr: transform_maps(tr, height, width, mask_h, mask_w))
    shapes = {(len(r), len(r[0])) for r in rows}
    if len(shapes) != 1:
        raise RuntimeError(f"resample_table_variants: the variants' tables differ in shape (objects, frames): {sorted(shapes)}")
    return torch.tensor(rows, dtype=torch.int32).to(device).contiguous()


def gather_planes(src, maps, out=None):
    """zero-filled per-frame gather of contiguous fp16 planes [..., F, h, w] (leading dims = planes of ONE object):
    out[.., f, y, x] = src[.., f, ymap_f[y], xmap_f[x]] or 0 where either index is outside.  ``maps``: device int32 [F, h + w]."""
    return _move_planes("gather_planes", "gather_planes", src, maps, lambda h, w: (("h + w", h + w),), out, name="maps")


# ---- rotation: nearest resampling through ONE 2-D index map --------------------------------------------------
def _warp_args(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw):
    myy, myx, mxy, mxx = (int(v) for v in m)
    dy, dx, den, ay2, ax2, H, W, Lh, Lw = (int(v) for v in (dy, dx, den, ay2, ax2, H, W, Lh, Lw))
    if den < 1 or H < 1 or W < 1 or Lh < 1 or Lw < 1:
        raise RuntimeError(f"level_warp_map: the denominator {den} and the sizes {H} x {W}, {Lh} x {Lw} must be positive")
    return dy, dx, myy, myx, mxy, mxx, den, ay2, ax2, H, W, Lh, Lw


def warp_numerator_bound(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw):
    """an upper bound, from the arguments alone, on the magnitude of every numerator, denominator and intermediate product
    ``level_warp_map`` forms: the vectorised int64 form is exact while it stays below 2^62"""
    dy, dx, myy, myx, mxy, mxx, den, ay2, ax2, H, W, Lh, Lw = _warp_args(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw)
    nyb = (2 * (H + abs(level_offset(dy, H, Lh))) + 1) * Lh + abs(ay2) * H
    nxb = (2 * (W + abs(level_offset(dx, W, Lw))) + 1) * Lw + abs(ax2) * W
    numy = abs(ay2) * den * H * W + abs(myy) * nyb * W + abs(myx) * nxb * H
    numx = abs(ax2) * den * H * W + abs(mxy) * nyb * W + abs(mxx) * nxb * H
    return max(numy, numx, 2 * den * W * Lh, 2 * den * H * Lw, H * W)


def _warp_coords_py(dy, dx, myy, myx, mxy, mxx, den, ay2, ax2, H, W, Lh, Lw):
    """the source coordinate of every destination pixel, row by row, as one exact rational per axis: (Ny, Dy, Nx, Dx), the
    coordinate Ny / Dy rows and Nx / Dx columns.  Python ints: the definition.  ``level_warp_map`` floors them, ``level_warp_taps``
    splits them into a tap and a weight"""
    dfy, dfx = level_offset(dy, H, Lh), level_offset(dx, W, Lw)
    cy, cx, Dy, Dx = ay2 * den * H * W, ax2 * den * H * W, 2 * den * W * Lh, 2 * den * H * Lw
    for iy in range(H):
        ny = (2 * (iy - dfy) + 1) * Lh - ay2 * H
        for ix in range(W):
            nx = (2 * (ix - dfx) + 1) * Lw - ax2 * W
            yield cy + myy * ny * W + myx * nx * H, Dy, cx + mxy * ny * W + mxx * nx * H, Dx


def _warp_coords_i64(dy, dx, myy, myx, mxy, mxx, den, ay2, ax2, H, W, Lh, Lw):
    """``_warp_coords_py`` on int64 tensors: (Ny [H, W], Dy, Nx [H, W], Dx) -- exact only below the bound its caller checks"""
    dfy, dfx = level_offset(dy, H, Lh), level_offset(dx, W, Lw)
    ny = ((2 * (torch.arange(H, dtype=torch.int64) - dfy) + 1) * Lh - ay2 * H)[:, None]
    nx = ((2 * (torch.arange(W, dtype=torch.int64) - dfx) + 1) * Lw - ax2 * W)[None, :]
    return (ay2 * den * H * W + myy * W * ny + myx * H * nx, 2 * den * W * Lh,
            ax2 * den * H * W + mxy * W * ny + mxx * H * nx, 2 * den * H * Lw)


def _fdiv(a, b):
    return torch.div(a, b, rounding_mode="floor")  # floor division of integers: exact


def _warp_coords(what, bound, form, term, args):
    """the coordinates of ``_warp_args`` ``args`` in the form that ``form`` (None, "py", "i64") and ``bound`` select: the int64
    tensors only while ``bound`` stays below 2^62, else (or when forced) the generator of Python ints -> (is_i64, coordinates)"""
    fits = bound < 2 ** 62
    if form == "i64" and not fits:
        raise RuntimeError(f"{what}: the int64 form is not exact for these arguments ({term} may reach 2^62)")
    if form not in (None, "py", "i64"):
        raise RuntimeError(f"{what}: form {form!r} is not one of None, 'py', 'i64'")
    i64 = fits and form != "py"
    return i64, (_warp_coords_i64 if i64 else _warp_coords_py)(*args)


def level_warp_map(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw, form=None):
    """the linear source pixel sy * W + sx of every destination pixel of an H x W feature grid under an Lh x Lw latent (mask)
    grid -> a list of H * W ints, -1 where the object is absent.  ``m`` = (myy, myx, mxy, mxx) over the positive denominator
    ``den`` is the INVERSE matrix (rows y then x): the destination pixel centre, in latent units relative to the anchor
    (``ay2`` / 2, ``ax2`` / 2) and moved back by (``dy``, ``dx``) latent pixels (``level_offset`` carries them to this level), is
    multiplied by it, carried back to this level and floored.  Python ints define the rule; the vectorised int64 form is taken
    only while ``warp_numerator_bound`` stays below 2^62 (``form`` = "py" / "i64" forces one: tests).  A diagonal matrix is the
    outer combination of ``level_axis_map`` of the two axes."""
    args = _warp_args(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw)
    H, W = args[9], args[10]
    i64, coords = _warp_coords("level_warp_map", warp_numerator_bound(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw), form, "a numerator", args)
    if i64:
        Ny, Dy, Nx, Dx = coords
        sy, sx = _fdiv(Ny, Dy), _fdiv(Nx, Dx)
        inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        return torch.where(inside, sy * W + sx, torch.full_like(sy, -1)).reshape(-1).tolist()
    out = []
    for Ny, Dy, Nx, Dx in coords:
        sy, sx = Ny // Dy, Nx // Dx
        out.append(sy * W + sx if 0 <= sy < H and 0 <= sx < W else -1)
    return out


def _check_frames(what, warp):
    if not warp or len({len(w[2]) for w in warp}) != 1 or not warp[0][2]:
        raise RuntimeError(f"{what}: every object needs the same number (>= 1) of per-frame matrices")


def _per_frame(warp, level):
    """``warp`` = per object (ay2, ax2, ((myy, myx, mxy, mxx, den, dy, dx) per frame)) -> nested lists [nobj][F] of
    ``level(dy, dx, (myy, myx, mxy, mxx), den, ay2, ax2)``, computed once per distinct frame value of an object"""
    rows = []
    for ay2, ax2, frames in warp:
        cache = {}
        obj = []
        for fr in frames:
            fr = tuple(fr)
            if fr not in cache:
                myy, myx, mxy, mxx, den, dy, dx = fr
                cache[fr] = level(dy, dx, (myy, myx, mxy, mxx), den, ay2, ax2)
            obj.append(cache[fr])
        rows.append(obj)
    return rows


def warp_maps(warp, height, width, mask_h, mask_w):
    """``warp`` = per object (ay2, ax2, ((myy, myx, mxy, mxx, den, dy, dx) per frame)) -> nested lists [nobj][F][height * width]:
    per frame ``level_warp_map``, computed once per distinct frame value of an object"""
    _check_frames("warp_maps", warp)
    return _per_frame(warp, lambda *a: level_warp_map(*a, height, width, mask_h, mask_w))


def warp_table(warp, height, width, mask_h, mask_w, device):
    """the device table the ``_warped`` blend entries read: int32 [nobj, F, height * width] (``warp_maps``).  Every entry is in
    [-1, height * width) by construction; the kernels treat any other value as absent as well"""
    if height * width >= 2 ** 31:
        raise RuntimeError(f"warp_table: {height} x {width} pixels do not fit the int32 entries")
    return torch.tensor(warp_maps(warp, height, width, mask_h, mask_w), dtype=torch.int32).to(device).contiguous()


def warp_planes(src, map, out=None):
    """zero-filled per-frame gather of contiguous fp16 planes [..., F, h, w] (leading dims = planes of ONE object) through a 2-D
    map: out[.., f, pix] = src[.., f, map_f[pix]] or 0 where the entry is outside.  ``map``: device int32 [F, h * w]."""
    return _move_planes("warp_planes", "gather_planes_warped", src, map, lambda h, w: (("h * w", h * w),), out, name="map")


# ---- bilinear sampling of warped objects: four taps and fixed-point weights per pixel ------------------------------
TAP_WEIGHT_ONE = 256  # the weights are q / 256, q an integer in [0, 256]
TAP_SITE_LIMIT = 65535  # a tap row / column + 1 is a 16-bit field and 0xffff is kept for "absent"


def warp_taps_bound(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw):
    """an upper bound on the magnitude of everything ``level_warp_taps`` forms: with B = ``warp_numerator_bound`` (>= |N| and
    >= D), |T| = |2N - D| <= 3B, |y0 * 2D| <= |T| + 2D <= 5B and 256 * (T - y0 * 2D) + D < 512D + D = 513D <= 513B -- the factor
    of 512 the weights add to the nearest rule.  The vectorised int64 form is exact while this stays below 2^62"""
    return 513 * warp_numerator_bound(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw)


def _axis_tap(N, D, fdiv=operator.floordiv):
    T = 2 * N - D                       # the source coordinate minus half a pixel, over 2D
    i0 = fdiv(T, 2 * D)                 # floor: the upper / left tap
    q = fdiv(TAP_WEIGHT_ONE * (T - i0 * 2 * D) + D, 2 * D)  # round half up: the weight of tap i0 + 1, 0..256
    return i0, q


def _level_warp_taps(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw, form):
    """``level_warp_taps`` as a list of tuples (the Python ints) or an int64 tensor [H * W, 4] (the int64 form)"""
    args = _warp_args(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw)
    i64, coords = _warp_coords("level_warp_taps", warp_taps_bound(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw), form, "a term", args)
    if i64:
        Ny, Dy, Nx, Dx = coords
        (y0, qy), (x0, qx) = _axis_tap(Ny, Dy, _fdiv), _axis_tap(Nx, Dx, _fdiv)
        return torch.stack([y0, x0, qy, qx], dim=-1).reshape(args[9] * args[10], 4)
    out = []
    for Ny, Dy, Nx, Dx in coords:
        (y0, qy), (x0, qx) = _axis_tap(Ny, Dy), _axis_tap(Nx, Dx)
        out.append((y0, x0, qy, qx))
    return out


def level_warp_taps(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw, form=None):
    """the bilinear taps of every destination pixel of an H x W feature grid under an Lh x Lw latent (mask) grid -> a list of
    H * W tuples (y0, x0, qy, qx).  The arguments and the source coordinate N / D per axis are those of ``level_warp_map`` (which
    floors it: the nearest pixel); here, per axis,
        T  = 2N - D                               the coordinate minus half a pixel, over 2D
        i0 = T // 2D                              the upper / left tap
        q  = (256 * (T - i0 * 2D) + D) // 2D      round half up: tap i0 + 1 has the weight q / 256, tap i0 the weight (256 - q) / 256
    Python ints define the rule; the vectorised int64 form is taken only while ``warp_taps_bound`` stays below 2^62 (``form`` =
    "py" / "i64" forces one: tests).  A pixel is present iff one of its four taps lies inside the plane (``tap_present``)."""
    out = _level_warp_taps(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw, form)
    return [tuple(r) for r in out.tolist()] if torch.is_tensor(out) else out


def tap_present(y0, x0, H, W):
    """at least one of the taps (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) lies inside the H x W plane; a tap of
    weight 0 counts"""
    return -1 <= y0 <= H - 1 and -1 <= x0 <= W - 1


def pack_taps(taps, H, W):
    """(y0, x0, qy, qx) per pixel -> the device form, two int32 words per pixel: word 0 = ((y0 + 1) << 16) | (x0 + 1) (as a signed
    32-bit value), or -1 where the pixel is absent; word 1 = (qy << 16) | qx"""
    if H >= TAP_SITE_LIMIT or W >= TAP_SITE_LIMIT:
        raise RuntimeError(f"pack_taps: {H} x {W}: a site of {TAP_SITE_LIMIT} rows or columns or more does not fit the 16-bit tap fields")
    out = []
    for y0, x0, qy, qx in taps:
        w0 = ((y0 + 1) << 16) | (x0 + 1) if tap_present(y0, x0, H, W) else -1
        out.append([w0 - (1 << 32) if w0 >= 1 << 31 else w0, (qy << 16) | qx])
    return out


def _level_tap_words(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw):
    """``pack_taps(level_warp_taps(...))`` as an int32 tensor [H * W, 2], without the detour through lists where the int64 form
    serves"""
    t = _level_warp_taps(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw, None)
    if not torch.is_tensor(t):
        return torch.tensor(pack_taps(t, H, W), dtype=torch.int32)
    y0, x0, qy, qx = t.unbind(-1)
    present = (y0 >= -1) & (y0 <= H - 1) & (x0 >= -1) & (x0 <= W - 1)
    w0 = torch.where(present, ((y0 + 1) << 16) | (x0 + 1), torch.full_like(y0, -1))
    w0 = torch.where(w0 >= 1 << 31, w0 - (1 << 32), w0)
    return torch.stack([w0, (qy << 16) | qx], dim=-1).to(torch.int32)


def warp_taps(warp, height, width, mask_h, mask_w):
    """``warp`` (the value of ``warp_maps``) -> an int32 tensor [nobj, F, height * width, 2] on the CPU: per frame the packed
    ``level_warp_taps``, computed once per distinct frame value of an object"""
    _check_frames("warp_taps", warp)
    if height >= TAP_SITE_LIMIT or width >= TAP_SITE_LIMIT:
        raise RuntimeError(f"warp_taps: {height} x {width}: a site of {TAP_SITE_LIMIT} rows or columns or more does not fit the "
                           "16-bit tap fields")
    rows = _per_frame(warp, lambda *a: _level_tap_words(*a, height, width, mask_h, mask_w))
    return torch.stack([torch.stack(obj) for obj in rows]).contiguous()


def warp_tap_table(warp, height, width, mask_h, mask_w, device):
    """the device table the ``_bilinear`` blend entries read: int32 [nobj, F, height * width, 2] (``warp_taps``).  The kernels
    read a tap only inside the plane: every int32 pair is safe to them"""
    return warp_taps(warp, height, width, mask_h, mask_w).to(device).contiguous()


def warp_planes_bilinear(src, taps, out=None):
    """zero-filled per-frame bilinear gather of contiguous fp16 planes [..., F, h, w] (leading dims = planes of ONE object)
    through a tap table: out[.., f, pix] = the fp16 chain of DESIGN.md 6r on the four taps of taps_f[pix], 0 where none lies
    inside.  ``taps``: device int32 [F, h * w, 2]."""
    return _move_planes("warp_planes_bilinear", "gather_planes_bilinear", src, taps, lambda h, w: (("h * w", h * w), ("2", 2)), out,
                        name="taps")


# ---- the main conditioning frames, composed from the placed objects at the image site -------------------------------
COLLAGE_FILTERS = (None, "nearest", "bilinear")  # what ``obj_transform_filter`` resolves to, and its two spellings of nearest
COLLAGE_MAX_OBJECTS = 16


def _level_nearest_words(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw):
    """the nearest form of a tap row: ``pack_taps`` of the pixel ``level_warp_map`` names as the upper-left tap with zero weights
    (-1 where the object is absent), as an int32 tensor [H * W, 2] -- without the detour through lists where the int64 form serves"""
    args = _warp_args(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw)
    i64, coords = _warp_coords("collage_taps", warp_numerator_bound(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw), None, "a numerator", args)
    if not i64:
        px = level_warp_map(dy, dx, m, den, ay2, ax2, H, W, Lh, Lw, "py")
        return torch.tensor(pack_taps([(s // W, s % W, 0, 0) if s >= 0 else (-2, -2, 0, 0) for s in px], H, W), dtype=torch.int32)
    Ny, Dy, Nx, Dx = coords
    sy, sx = _fdiv(Ny, Dy), _fdiv(Nx, Dx)
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    w0 = torch.where(inside, ((sy + 1) << 16) | (sx + 1), torch.full_like(sy, -1))
    w0 = torch.where(w0 >= 1 << 31, w0 - (1 << 32), w0).reshape(-1)
    return torch.stack([w0, torch.zeros_like(w0)], dim=-1).to(torch.int32)


def _collage_rows(warp, height, width, mask_h, mask_w, filter):
    """-> (rows, index): the DISTINCT tap rows of ``warp`` at the site, each an int32 [height * width, 2] tensor computed once, and
    per object the row of every frame as indices into them"""
    _check_frames("collage_taps", warp)
    if filter not in COLLAGE_FILTERS:
        raise RuntimeError(f"collage_taps: filter {filter!r} is not one of None, 'nearest', 'bilinear'")
    if height >= TAP_SITE_LIMIT or width >= TAP_SITE_LIMIT:
        raise RuntimeError(f"collage_taps: {height} x {width}: a site of {TAP_SITE_LIMIT} rows or columns or more does not fit the "
                           "16-bit tap fields")
    words = _level_tap_words if filter == "bilinear" else _level_nearest_words
    rows = []

    def level(*a):
        rows.append(words(*a, height, width, mask_h, mask_w))
        return len(rows) - 1
    return rows, _per_frame(warp, level)


def collage_taps(warp, H, W, mask_h, mask_w, filter=None):
    """``warp`` (the value of ``warp_maps``) -> the tap table of the collage at the image site H x W under the mask_h x mask_w latent
    grid: an int32 CPU tensor [nobj, F, H * W, 2], one computation per distinct frame value of an object.  "bilinear": ``warp_taps``
    bit for bit; None / "nearest": degenerate taps -- the upper-left tap is the pixel ``level_warp_map`` names, both weights 0.
    When no object changes along the clip the frame axis is a stride-0 view of the one row per object (no F copies)."""
    rows, index = _collage_rows(warp, H, W, mask_h, mask_w, filter)
    if all(len(set(obj)) == 1 for obj in index):
        return torch.stack([rows[obj[0]] for obj in index])[:, None].expand(len(index), len(index[0]), H * W, 2)
    return torch.stack(rows)[torch.tensor(index)].contiguous()


def collage_tap_table(warp, H, W, mask_h, mask_w, filter, device):
    """the device table ``collage`` reads: ``collage_taps`` as a contiguous int32 [nobj, F, H * W, 2].  Only the DISTINCT rows are
    built on the host and uploaded; the frames that share a row are spread on the device"""
    rows, index = _collage_rows(warp, H, W, mask_h, mask_w, filter)
    return torch.stack(rows).to(device)[torch.tensor(index, device=device)].contiguous()


def collage(bg, objs, alpha, taps, out=None):
    """the background with every object alpha-blended over it through a tap table, in integers (the rule is stated
    at mvoc_collage_rgb_u8 in include/mvoc_hip.h).  ``bg`` uint8 [F, H, W, 3], ``objs`` uint8 [nobj, F, H, W, 3], ``alpha`` uint8
    [nobj, F, H, W], ``taps`` int32 [nobj, F, H * W, 2] (``collage_tap_table``), all contiguous on the device -> uint8 [F, H, W, 3]"""
    _chk(bg, "bg", torch.uint8), _chk(objs, "objs", torch.uint8), _chk(alpha, "alpha", torch.uint8), _chk(taps, "taps", torch.int32)
    if bg.dim() != 4 or bg.shape[-1] != 3 or not bg.is_contiguous():
        raise RuntimeError(f"collage: bg must be contiguous [F, H, W, 3], got {tuple(bg.shape)}")
    frames, h, w = bg.shape[:3]
    if objs.dim() != 5 or tuple(objs.shape[1:]) != tuple(bg.shape) or not objs.is_contiguous():
        raise RuntimeError(f"collage: objs must be contiguous [nobj, F = {frames}, H = {h}, W = {w}, 3], got {tuple(objs.shape)}")
    nobj = objs.shape[0]
    if tuple(alpha.shape) != (nobj, frames, h, w) or not alpha.is_contiguous():
        raise RuntimeError(f"collage: alpha must be contiguous [nobj = {nobj}, F = {frames}, H = {h}, W = {w}], got {tuple(alpha.shape)}")
    if tuple(taps.shape) != (nobj, frames, h * w, 2) or not taps.is_contiguous():
        raise RuntimeError(f"collage: taps must be a contiguous int32 [nobj = {nobj}, F = {frames}, h * w = {h * w}, 2] table, "
                           f"got {tuple(taps.shape)}")
    if taps.data_ptr() % 8:
        raise RuntimeError(f"collage: taps must be 8-byte aligned (the kernel reads a table entry as one int2), got an address "
                           f"ending in {taps.data_ptr() % 8}")
    if out is None:
        out = torch.empty_like(bg)
    _chk(out, "out", torch.uint8)
    if out.shape != bg.shape or not out.is_contiguous():
        raise RuntimeError("collage: out must be contiguous and of bg's shape")
    lo, hi = out.data_ptr(), out.data_ptr() + out.numel()
    for name, t in (("bg", bg), ("objs", objs), ("alpha", alpha), ("taps", taps)):
        if t.data_ptr() < hi and lo < t.data_ptr() + t.numel() * t.element_size():
            raise RuntimeError(f"collage: out overlaps {name} (in place is not supported)")
    check(lib.mvoc_collage_rgb_u8(bg.data_ptr(), objs.data_ptr(), alpha.data_ptr(), out.data_ptr(), nobj, frames, h, w,
                                  taps.data_ptr(), _stream()), "collage_rgb_u8")
    return out


# ---- matte edges: grow, shrink and feather masks in the object's source coordinates ---------------------------------
MASK_OPS = {"max": 0, "min": 1, "mean": 2}
MASK_FILTER_MAX_RADIUS = 64  # what the entries take: 8 latent pixels at the image site of a vae_scale_factor of 8
MASK_EDIT_MAX = 8            # |grow| and feather of an edit, in latent pixels


def mask_filter(src, op, radius, axis, out=None):
    """one pass of the mask filter (the rule is stated at mvoc_mask_filter_f16 in include/mvoc_hip.h): every plane of the contiguous
    device tensor ``src`` [..., h, w], fp16 or uint8, filtered along ``axis`` (0: along y, 1: along x) with the window
    2 * radius + 1 and clamped taps; ``op`` "max", "min" or "mean" -> ``out`` (None: a new tensor of src's shape)"""
    if not (isinstance(src, torch.Tensor) and src.is_cuda):
        raise RuntimeError("mvoc_amd.ops: `src` must be a device tensor (this package has no CPU path)")
    if src.dtype not in (torch.float16, torch.uint8):
        raise RuntimeError(f"mask_filter: src must be torch.float16 or torch.uint8, got {src.dtype}")
    if op not in MASK_OPS:
        raise RuntimeError(f"mask_filter: op {op!r} is not one of 'max', 'min', 'mean'")
    if axis not in (0, 1):
        raise RuntimeError(f"mask_filter: axis {axis!r} is not 0 (along y) or 1 (along x)")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= MASK_FILTER_MAX_RADIUS:
        raise RuntimeError(f"mask_filter: radius {radius!r} is not an int in [0, {MASK_FILTER_MAX_RADIUS}]")
    if src.dim() < 2 or not src.is_contiguous() or src.numel() == 0:
        raise RuntimeError(f"mask_filter: src must be contiguous [..., h, w] and not empty, got {tuple(src.shape)} / {src.stride()}")
    h, w = src.shape[-2:]
    if out is None:
        out = torch.empty_like(src)
    _chk(out, "out", src.dtype)
    if out.shape != src.shape or not out.is_contiguous():
        raise RuntimeError("mask_filter: out must be contiguous and of src's shape")
    nbytes = src.numel() * src.element_size()
    if out.data_ptr() < src.data_ptr() + nbytes and src.data_ptr() < out.data_ptr() + nbytes:
        raise RuntimeError("mask_filter: out overlaps src (in place is not supported)")
    head = (src.data_ptr(), out.data_ptr(), src.numel() // (h * w), h, w, MASK_OPS[op], radius, axis)
    if src.dtype == torch.float16:
        inv = C.c_float(1.0 / (2 * radius + 1)).value  # formed in double, rounded once to float
        check(lib.mvoc_mask_filter_f16(*head, inv, _stream()), "mask_filter_f16")
    else:
        check(lib.mvoc_mask_filter_u8(*head, _stream()), "mask_filter_u8")
    return out


def edit_passes(grow, feather, scale=1):
    """the passes of an edit, in order, as (op, radius, axis): grow > 0 a max and grow < 0 a min pass along x, then along y; then
    feather a mean pass along x, then along y; radii times ``scale``; a radius of 0 is the identity and has no pass"""
    passes = []
    if grow:
        passes += [("max" if grow > 0 else "min", abs(grow) * scale, 1), ("max" if grow > 0 else "min", abs(grow) * scale, 0)]
    if feather:
        passes += [("mean", feather * scale, 1), ("mean", feather * scale, 0)]
    return passes


def edit_planes(src, grow, feather, scale=1):
    """the edit of DESIGN.md 6u on contiguous device planes [..., h, w], fp16 or uint8: ``edit_passes`` through ``mask_filter``, the
    intermediate of two passes in the planes' own type.  Returns ``src`` itself when both are 0."""
    for op, radius, axis in edit_passes(grow, feather, scale):
        src = mask_filter(src, op, radius, axis)
    return src


def ddim_step(x, v_cond, coef_dev, v_uncond=None, out=None):
    """coef_dev: fp32 device tensor {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev), guidance_scale}; a [K, 5] tensor
    with K > 1 updates K variants in one launch: x, v_cond, v_uncond, out are then [K, ...] and variant k takes row k."""
    _chk(x, "x"), _chk(v_cond, "v_cond"), _chk(v_uncond, "v_uncond"), _chk(coef_dev, "coef", torch.float32)
    if out is None:
        out = torch.empty_like(x)
    for t in (x, v_cond, v_uncond, out):
        if t is not None and not t.is_contiguous():
            raise RuntimeError("ddim_step: tensors must be contiguous")
    if coef_dev.dim() == 2 and coef_dev.shape[0] > 1:
        nvar = coef_dev.shape[0]
        if not coef_dev.is_contiguous() or coef_dev.shape[1] != 5 or x.shape[0] != nvar or any(
                t is not None and t.numel() != x.numel() for t in (v_cond, v_uncond, out)):
            raise RuntimeError(f"ddim_step: {nvar} coefficient rows need contiguous [{nvar}, 5] and [{nvar}, ...] tensors of one size")
        check(lib.mvoc_ddim_step_variants_f16(x.data_ptr(), _ptr(v_uncond), v_cond.data_ptr(), coef_dev.data_ptr(),
                                              out.data_ptr(), x.numel() // nvar, nvar, _stream()), "ddim_step_variants")
        return out
    check(lib.mvoc_ddim_step_f16(x.data_ptr(), _ptr(v_uncond), v_cond.data_ptr(), coef_dev.data_ptr(), out.data_ptr(),
                                 x.numel(), _stream()), "ddim_step")
    return out


def latent_fusion(latents, bg, objs, masks, mix_ratio, obj_random_noise_fusion=False, out=None, nvar=1):
    """objs / masks: contiguous [nobj, *latents.shape] fp16.  ``nvar`` = K > 1: latents / out are [K, ...] (K variants), bg is
    one variant's size and objs / masks are [nobj, *bg.shape], read by every variant."""
    _chk(latents, "latents"), _chk(bg, "bg"), _chk(objs, "objs"), _chk(masks, "masks")
    if out is None:
        out = torch.empty_like(latents)
    if nvar != 1:
        n = bg.numel()
        if not 1 <= nvar <= 8 or latents.numel() != n * nvar or out.numel() != n * nvar or objs.numel() != masks.numel() \
                or objs.numel() % n or not all(t.is_contiguous() for t in (latents, bg, objs, masks, out)):
            raise RuntimeError(f"latent_fusion: {nvar} variants need contiguous latents/out [{nvar}, ...bg.shape] and objs/masks "
                               "[nobj, ...bg.shape]")
        check(lib.mvoc_latent_fusion_variants_f16(latents.data_ptr(), bg.data_ptr(), objs.data_ptr(), masks.data_ptr(),
                                                  out.data_ptr(), objs.numel() // n, n, int(nvar), float(mix_ratio),
                                                  int(obj_random_noise_fusion), _stream()), "latent_fusion_variants")
        return out
    n = latents.numel()
    if objs.numel() != masks.numel() or objs.numel() % n:
        raise RuntimeError("latent_fusion: objs/masks must be [nobj, ...latents.shape]")
    check(lib.mvoc_latent_fusion_f16(latents.data_ptr(), bg.data_ptr(), objs.data_ptr(), masks.data_ptr(), out.data_ptr(),
                                     objs.numel() // n, n, float(mix_ratio), int(obj_random_noise_fusion), _stream()),
          "latent_fusion")
    return out


def timestep_embedding(t_dev, dim):
    _chk(t_dev, "t", torch.float32)
    out = torch.empty((t_dev.numel(), dim), dtype=torch.float16, device=t_dev.device)
    check(lib.mvoc_timestep_embedding_f16(t_dev.data_ptr(), t_dev.numel(), dim, out.data_ptr(), _stream()), "timestep_embedding")
    return out


def act(x, kind):
    _chk(x, "x")
    out = torch.empty_like(x)
    check(lib.mvoc_act_f16(x.data_ptr(), out.data_ptr(), x.numel(), kind, _stream()), "act")
    return out


def add(a, b):
    _chk(a, "a"), _chk(b, "b")
    out = torch.empty_like(a)
    check(lib.mvoc_add_f16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "add")
    return out


def conv3x3_small(x, w, bias, *, nimg, h, wd, cin, cout, stride=1, silu=False):
    _chk(x, "x"), _chk(w, "w"), _chk(bias, "bias")
    ho, wo = (h + 2 - 3) // stride + 1, (wd + 2 - 3) // stride + 1
    out = torch.empty((nimg * ho * wo, cout), dtype=torch.float16, device=x.device)
    check(lib.mvoc_conv3x3_small_f16(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), nimg, h, wd, cin, cout, stride,
                                     int(silu), _stream()), "conv3x3_small")
    return out, ho, wo


def adaptive_avgpool(x, *, nimg, h, w, c, oh, ow):
    _chk(x, "x")
    out = torch.empty((nimg * oh * ow, c), dtype=torch.float16, device=x.device)
    check(lib.mvoc_adaptive_avgpool_f16(x.data_ptr(), out.data_ptr(), nimg, h, w, c, oh, ow, _stream()), "adaptive_avgpool")
    return out


def ncfhw_to_tokens(x, out, coff=0):
    """x [B,C,F,h,w] -> out [B*F*h*w, ld] channels coff..coff+C"""
    _chk(x, "x"), _chk(out, "out")
    b, c, f, h, w = x.shape
    x = x.contiguous()  # (a copy, if one is made, is held until the launch is enqueued)
    check(lib.mvoc_ncfhw_to_tokens_f16(x.data_ptr(), out.data_ptr(), b, c, f, h * w, out.stride(0), coff,
                                       _stream()), "ncfhw_to_tokens")
    return out


def tokens_to_ncfhw(x, b, c, f, h, w):
    _chk(x, "x")
    out = torch.empty((b, c, f, h, w), dtype=torch.float16, device=x.device)
    check(lib.mvoc_tokens_to_ncfhw_f16(x.data_ptr(), out.data_ptr(), b, c, f, h * w, x.stride(0), _stream()), "tokens_to_ncfhw")
    return out


def temporal_encoder4(x, params, out, *, b, f, hw, coff):
    _chk(x, "x"), _chk(params, "params"), _chk(out, "out")
    check(lib.mvoc_temporal_encoder4_f16(x.data_ptr(), params.data_ptr(), out.data_ptr(), b, f, hw, out.stride(0), coff,
                                         _stream()), "temporal_encoder4")
    return out


def conv1x1_small(x, w, bias):
    """out[r, o] = sum_c x[r, c] * w[o, c] + bias[o] for a handful of channels (the VAE's quant / post_quant 1x1 convs)"""
    _chk(x, "x"), _chk(w, "w"), _chk(bias, "bias")
    if not x.is_contiguous() or x.shape[1] != w.shape[1]:
        raise RuntimeError("conv1x1_small: x must be contiguous [rows, cin] with cin == w.shape[1]")
    out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float16, device=x.device)
    w = w.contiguous()
    check(lib.mvoc_conv1x1_small_f16(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), x.shape[0], x.shape[1],
                                     w.shape[0], _stream()), "conv1x1_small")
    return out


def image_to_tokens(x):
    """[n, c, h, w] fp16 -> channels-last rows [n*h*w, c]"""
    _chk(x, "x")
    n, c, h, w = x.shape
    out = torch.empty((n * h * w, c), dtype=torch.float16, device=x.device)
    x = x.contiguous()
    check(lib.mvoc_image_to_tokens_f16(x.data_ptr(), out.data_ptr(), n, c, h * w, _stream()), "image_to_tokens")
    return out


def tokens_to_image(x, n, c, h, w):
    """channels-last rows [n*h*w, ld] (first c channels) -> [n, c, h, w]"""
    _chk(x, "x")
    out = torch.empty((n, c, h, w), dtype=torch.float16, device=x.device)
    check(lib.mvoc_tokens_to_image_f16(x.data_ptr(), out.data_ptr(), n, c, h * w, _rowmajor(x, "x"), _stream()), "tokens_to_image")
    return out


def permute_rows(x, shape4, perm):
    """x: contiguous [prod(shape4), c] rows viewed as [*shape4, c]; returns the rows of ``x.view(*shape4, c).permute(*perm, 4)``
    made contiguous ([prod, c]) -- the pack / unpack copies around the frame-shard exchanges as one HIP kernel"""
    _chk(x, "x")
    if not x.is_contiguous() or x.dim() != 2:
        raise RuntimeError("permute_rows: x must be contiguous [rows, c]")
    st = [shape4[1] * shape4[2] * shape4[3], shape4[2] * shape4[3], shape4[3], 1]
    dims = (C.c_int64 * 4)(*[shape4[p] for p in perm])
    strides = (C.c_int64 * 4)(*[st[p] for p in perm])
    out = torch.empty_like(x)
    check(lib.mvoc_permute_rows_f16(x.data_ptr(), out.data_ptr(), dims, strides, x.shape[1], _stream()), "permute_rows")
    return out


def softmax_rows(x):
    """in-place softmax over the last dim of a contiguous [rows, cols] fp16 matrix (fp32 math, one rounding)"""
    _chk(x, "x")
    if x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError("softmax_rows: x must be contiguous [rows, cols]")
    check(lib.mvoc_softmax_rows_f16(x.data_ptr(), x.shape[0], x.shape[1], _stream()), "softmax_rows")
    return x


def prof_enable(on):
    lib.mvoc_prof_enable(int(on))


def prof_reset():
    lib.mvoc_prof_reset()


def prof_collect():
    n = len(_ffi.FAMILIES)
    ms = (C.c_double * n)()
    cnt = (C.c_int64 * n)()
    work = (C.c_double * n)()
    check(lib.mvoc_prof_collect(ms, cnt, work), "prof_collect")
    return {fam: {"ms": ms[i], "launches": cnt[i], "work": work[i]} for i, fam in enumerate(_ffi.FAMILIES)}


def delay_us(us):
    check(lib.mvoc_delay_us(int(us), _stream()), "delay_us")
