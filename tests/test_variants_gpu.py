"""GPU: K variants over one set of source chunks -- the batch [s_0..s_{nsrc-1}, u_1..u_K, c_1..c_K].

* kernels: the ``_variants`` blend entries write, for every variant k, destination chunks bit-identical (``_same_bits``: int16
  views of every number, NaN where the twin has NaN) to the positional kernel run on that variant's own batch
  [bg, obj.., u_k, c_k]; sources untouched (int16 views); bad ``nvar`` / maps refused.
  The batched DDIM / fusion entries equal K single calls bit for bit.
* UNet: a forward under ``unet.variants = K`` against the ORACLE's forward of every variant's own batch (the project's forward
  tolerance) and against the engine's own single-variant forward (the batch-independence bar of
  test_source_dedup_gpu.py: another row count means other tiles).
* loop: K compositions in one loop against the oracle's loop run per variant; graph replay against eager; the UNet batch of
  every step; the loop glue bit for bit on an elementwise stand-in UNet; C-ABI calls per step independent of K.
"""
import ctypes as C
import itertools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _specials(x, g):
    flat = x.view(-1)
    n = flat.numel()
    for v in (-0.0, float("inf"), float("-inf"), float("nan")):
        idx = torch.randint(0, n, (max(1, n // 97),), generator=g)
        flat[idx.to(flat.device)] = v
    return x


def _masks(nobj, F, mh, mw, soft, g):
    u8 = torch.randint(0, 256, (nobj, F, mh, mw), generator=g)
    m = (u8.float() / 255).half() if soft else (u8 > 100).half()
    return m.cuda().contiguous()


def _maps(nobj):
    """None = the identity (positional sources), then non-identity maps"""
    out = [None, (1, (0,) * nobj)]
    if nobj >= 2:
        out += [(2, (1, 0) + (1,) * (nobj - 2)), (2, (1,) * nobj)]
    if nobj >= 3:
        out += [(3, tuple(1 + j % 2 for j in range(nobj)))]
    return out


def _i16(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    """a stricter torch.equal between two DIFFERENT kernels: the same bits wherever the value is a number (signed zeros and
    infinities included), a NaN exactly where the other has one.  The sign of a NaN is not compared: hipcc picks the
    instructions of `x*(1-m) + y*m` per kernel (packed fp16 multiplies, mixed-precision adds), and which operand's NaN an add
    of two NaNs returns -- inf * 0 gives -NaN on this hardware -- follows the operand order the compiler chose.  (torch.equal
    itself is False for any tensor that holds a NaN.)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(_i16(a)[~na], _i16(b)[~nb]))


def _src_order(smap, nobj):
    """compact chunk behind each source role [bg, obj_1..obj_n]"""
    return list(range(nobj + 1)) if smap is None else [0] + list(smap[1])


def _strides(layout, ld, F, hw):
    return (hw * ld, ld) if layout == "spatial" else (ld, F * ld)  # (f_stride, p_stride)


def _tokens_variants_direct(buf, layout, F, H, W, c, masks, base0, ndst, smap, nvar):
    """the C entry itself, whatever nvar is (ops routes nvar = 1 to the single-variant entries); returns its status"""
    from mvoc_amd import ops
    ld, hw = buf.stride(0), H * W
    fs, ps = _strides(layout, ld, F, hw)
    d = ops._pnp_desc(buf[:, :c], buf[:, c:2 * c], masks, F * hw * ld, fs, ps, F, H, W, c, base0, ndst)
    nobj = masks.shape[0]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    return ops.lib.mvoc_pnp_blend_scatter_tokens_variants(C.byref(d), nsrc, arr, nvar, ops._stream())


def _nchw_variants_direct(x, masks, F, base0, ndst, smap, nvar):
    from mvoc_amd import ops
    d = ops._pnp_desc(x, None, masks, 0, 0, 0, F, x.shape[2], x.shape[3], x.shape[1], base0, ndst)
    nobj = masks.shape[0]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    return ops.lib.mvoc_pnp_blend_scatter_nchw_variants(C.byref(d), nsrc, arr, nvar, ops._stream())


def _run_tokens(buf, layout, F, H, W, c, masks, base0, ndst, smap=None, nvar=1):
    from mvoc_amd import ops
    ld, hw = buf.stride(0), H * W
    fs, ps = _strides(layout, ld, F, hw)
    ops.pnp_blend_tokens(buf[:, :c], masks, x2=buf[:, c:2 * c], frames=F, height=H, width=W, channels=c,
                         chunk_stride=F * hw * ld, f_stride=fs, p_stride=ps, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=nvar)


KS = (1, 2, 3, 8)


@pytest.mark.parametrize("nobj", [1, 2, 3, 4])
@pytest.mark.parametrize("layout", ["spatial", "temporal"])
def test_tokens_variants_equal_the_positional_kernel_per_variant(layout, nobj):
    g = torch.Generator().manual_seed(20 * nobj + (layout == "temporal"))
    F, H, W, c = 3, 5, 6, 16
    rows = F * H * W
    n = 0
    for K, ndst, base0, (soft, mres), smap in itertools.product(KS, (1, 2), (False, True), ((False, "same"), (True, "other")),
                                                                _maps(nobj)):
        mh, mw = (H, W) if mres == "same" else (3, 9)
        masks = _masks(nobj, F, mh, mw, soft, g)
        nsrc = nobj + 1 if smap is None else smap[0]
        comp = _specials(torch.randn((nsrc + ndst * K) * rows, 3 * c, generator=g).half(), g).cuda()
        comp0 = comp.clone()
        chunk = lambda t, i: t[i * rows:(i + 1) * rows]
        what = (K, ndst, base0, soft, mres, smap)
        if K == 1:
            assert _tokens_variants_direct(comp, layout, F, H, W, c, masks, base0, ndst, smap, 1) == 0, what
            twin = comp0.clone()  # nvar = 1 is the _mapped entry (the positional one for the identity map)
            _run_tokens(twin, layout, F, H, W, c, masks, base0, ndst, smap)
            assert _same_bits(comp, twin), what
        else:
            _run_tokens(comp, layout, F, H, W, c, masks, base0, ndst, smap, nvar=K)
        for k in range(K):
            dst = [nsrc + d * K + k for d in range(ndst)]  # (u_k,) c_k
            full = torch.cat([chunk(comp0, i) for i in _src_order(smap, nobj) + dst]).contiguous()
            _run_tokens(full, layout, F, H, W, c, masks, base0, ndst)
            for d, i in enumerate(dst):
                assert _same_bits(chunk(comp, i), chunk(full, nobj + 1 + d)), (what, k, d)
        torch.cuda.synchronize()
        assert torch.equal(_i16(comp[:nsrc * rows]), _i16(comp0[:nsrc * rows])), what  # sources untouched
        assert torch.equal(_i16(comp[:, 2 * c:]), _i16(comp0[:, 2 * c:])), what  # v columns untouched
        n += 1
    assert n == len(KS) * 8 * len(_maps(nobj))


@pytest.mark.parametrize("nobj", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", [(4, 6), (3, 5)])  # hw % 8 == 0: 8 pixels per work item / else 1
def test_nchw_variants_equal_the_positional_kernel_per_variant(hw, nobj):
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(200 + nobj + hw[1])
    H, W = hw
    F, Cc = 2, 4
    for K, ndst, base0, (soft, mres), smap in itertools.product(KS, (1, 2), (False, True), ((False, "same"), (True, "other")),
                                                                _maps(nobj)):
        mh, mw = (H, W) if mres == "same" else (2 * H, W + 1)
        masks = _masks(nobj, F, mh, mw, soft, g)
        nsrc = nobj + 1 if smap is None else smap[0]
        comp = _specials(torch.randn((nsrc + ndst * K) * F, Cc, H, W, generator=g).half(), g).cuda()
        comp0 = comp.clone()
        chunk = lambda t, i: t[i * F:(i + 1) * F]
        what = (K, ndst, base0, soft, mres, smap)
        if K == 1:
            assert _nchw_variants_direct(comp, masks, F, base0, ndst, smap, 1) == 0, what
            twin = comp0.clone()
            ops.pnp_blend_nchw(twin, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap)
            assert _same_bits(comp, twin), what
        else:
            ops.pnp_blend_nchw(comp, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K)
        for k in range(K):
            dst = [nsrc + d * K + k for d in range(ndst)]
            full = torch.cat([chunk(comp0, i) for i in _src_order(smap, nobj) + dst]).contiguous()
            ops.pnp_blend_nchw(full, masks, frames=F, base_chunk0=base0, ndst=ndst)
            for d, i in enumerate(dst):
                assert _same_bits(chunk(comp, i), chunk(full, nobj + 1 + d)), (what, k, d)
        assert torch.equal(_i16(comp[:nsrc * F]), _i16(comp0[:nsrc * F])), what


def test_invalid_variant_counts_and_maps_are_refused():
    from mvoc_amd import ops
    F, H, W, c = 2, 4, 4, 8
    masks = _masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    buf = torch.zeros(11 * F * H * W, 3 * c, dtype=torch.float16, device="cuda")
    nchw = torch.zeros(11 * F, 4, H, W, dtype=torch.float16, device="cuda")
    # the C entries: status -1 and an error text
    for nvar, msg in ((0, "nvar 0"), (9, "nvar 9"), (-3, "nvar -3")):
        assert _tokens_variants_direct(buf, "spatial", F, H, W, c, masks, False, 2, None, nvar) == -1
        assert msg in ops.lib.mvoc_last_error().decode()
        assert _nchw_variants_direct(nchw, masks, F, True, 2, None, nvar) == -1
        assert msg in ops.lib.mvoc_last_error().decode()
    for smap, msg in (((0, (0, 0)), "nsrc 0"), ((4, (0, 0)), "nsrc 4"), ((2, (0, 2)), "obj_chunk[1] = 2"),
                      ((2, (-1, 0)), "obj_chunk[0] = -1")):
        assert _tokens_variants_direct(buf, "spatial", F, H, W, c, masks, False, 2, smap, 2) == -1
        assert msg in ops.lib.mvoc_last_error().decode()
        assert _nchw_variants_direct(nchw, masks, F, True, 2, smap, 2) == -1
        assert msg in ops.lib.mvoc_last_error().decode()
        with pytest.raises(RuntimeError, match="pnp mapped"):
            _run_tokens(buf, "spatial", F, H, W, c, masks, False, 2, smap, nvar=2)
        with pytest.raises(RuntimeError, match="pnp mapped"):
            ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, src_map=smap, nvar=2)
    # the Python layer: a count out of range, a map of the wrong length, a buffer that ends before the last destination chunk
    for nvar in (0, 9):
        with pytest.raises(RuntimeError, match="not in"):
            _run_tokens(buf, "spatial", F, H, W, c, masks, False, 2, None, nvar=nvar)
        with pytest.raises(RuntimeError, match="not in"):
            ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, nvar=nvar)
    with pytest.raises(RuntimeError, match="names 3 objects"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, src_map=(1, (0, 0, 0)), nvar=2)
    with pytest.raises(RuntimeError, match="storage ends"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, nvar=5)  # 3 + 10 chunks in a buffer of 11
    with pytest.raises(RuntimeError, match="storage ends"):
        _run_tokens(buf, "spatial", F, H, W, c, masks, False, 2, None, nvar=5)
    torch.cuda.synchronize()
    assert not buf.any() and not nchw.any()


def test_profiler_counts_the_variant_traffic():
    """(distinct sources read, + K bases when the base is c_k) + ndst * K chunks written, per tensor, + the mask values"""
    from mvoc_amd import ops
    F, H, W, c, K = 2, 4, 4, 8, 3
    rows = F * H * W
    masks = _masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    chunk_bytes, mask_bytes = 2.0 * rows * c, 2.0 * 2 * F * H * W
    ops.prof_enable(True)
    try:
        for base0, ndst, smap, chunks in ((True, 2, None, 3 + 2 * K), (False, 2, None, 2 + K + 2 * K), (True, 1, (2, (1, 1)), 2 + K),
                                          (False, 2, (1, (0, 0)), 1 + K + 2 * K)):
            nsrc = 3 if smap is None else smap[0]
            buf = torch.zeros((nsrc + ndst * K) * rows, 3 * c, dtype=torch.float16, device="cuda")
            ops.prof_reset()
            _run_tokens(buf, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K)
            torch.cuda.synchronize()
            got = ops.prof_collect()["pnp"]
            assert got["launches"] == 1 and got["work"] == 2 * (chunks * chunk_bytes + mask_bytes), (base0, ndst, smap, got)  # q and k
            nchw = torch.zeros((nsrc + ndst * K) * F, c, H, W, dtype=torch.float16, device="cuda")
            ops.prof_reset()
            ops.pnp_blend_nchw(nchw, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K)
            torch.cuda.synchronize()
            got = ops.prof_collect()["pnp"]
            assert got["launches"] == 1 and got["work"] == chunks * chunk_bytes + mask_bytes, (base0, ndst, smap, got)
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_ddim_step_variants_equal_single_calls(K):
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(40 + K)
    shape = (K, 4, 3, 5, 7)
    x, vu, vc = (torch.randn(shape, generator=g).half().cuda() for _ in range(3))
    coef = torch.rand(K, 5, generator=g).cuda() * torch.tensor([1.0, 1.0, 1.0, 1.0, 12.0]).cuda() + 0.05  # K different rows
    n_per = x[0].numel()
    for cfg in (True, False):
        out = torch.full_like(x, float("nan"))
        rc = ops.lib.mvoc_ddim_step_variants_f16(x.data_ptr(), vu.data_ptr() if cfg else None, vc.data_ptr(), coef.data_ptr(),
                                                 out.data_ptr(), n_per, K, ops._stream())
        assert rc == 0, ops.lib.mvoc_last_error()
        for k in range(K):
            one = ops.ddim_step(x[k:k + 1].contiguous(), vc[k:k + 1].contiguous(), coef[k],
                                v_uncond=vu[k:k + 1].contiguous() if cfg else None)
            assert torch.equal(_i16(out[k:k + 1]), _i16(one)), (K, cfg, k)
        if K > 1:  # the wrapper picks the batched entry from the [K, 5] coefficient rows; in place as the loop runs it
            y = x.clone()
            ops.ddim_step(y, vc, coef, v_uncond=vu if cfg else None, out=y)
            assert torch.equal(_i16(y), _i16(out)), (K, cfg)
    for bad in (0, 9):
        assert ops.lib.mvoc_ddim_step_variants_f16(x.data_ptr(), None, vc.data_ptr(), coef.data_ptr(), x.data_ptr(), n_per, bad,
                                                   ops._stream()) == -1


@pytest.mark.parametrize("rnf", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_latent_fusion_variants_equal_single_calls(K, rnf):
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(60 + K)
    one = (1, 4, 3, 5, 7)
    for nobj in (1, 2, 4):
        lat = torch.randn((K,) + one[1:], generator=g).half().cuda()
        bg = torch.randn(one, generator=g).half().cuda()
        objs = torch.randn((nobj,) + one, generator=g).half().cuda()
        masks = (torch.randint(0, 256, (nobj,) + one, generator=g).float() / 255).half().cuda()
        out = torch.full_like(lat, float("nan"))
        rc = ops.lib.mvoc_latent_fusion_variants_f16(lat.data_ptr(), bg.data_ptr(), objs.data_ptr(), masks.data_ptr(), out.data_ptr(),
                                                     nobj, bg.numel(), K, 0.3, int(rnf), ops._stream())
        assert rc == 0, ops.lib.mvoc_last_error()
        for k in range(K):
            ref = ops.latent_fusion(lat[k:k + 1].contiguous(), bg, objs, masks, 0.3, rnf)
            assert torch.equal(_i16(out[k:k + 1]), _i16(ref)), (K, nobj, k)
        if K > 1:
            y = lat.clone()
            ops.latent_fusion(y, bg, objs, masks, 0.3, rnf, out=y, nvar=K)
            assert torch.equal(_i16(y), _i16(out))


# ---- UNet ------------------------------------------------------------------------------------------------------------
def _toy_pair():
    from oracle import unet_ref as U
    from mvoc_amd.unet import I2VGenXLUNet
    o = U.I2VGenXLUNet(U.UNetConfig.small4())
    U.init_weights_(o, seed=9)
    for p in o.parameters():
        p.copy_(p.half().float())
    return o, I2VGenXLUNet(o.config.to_dict()).load_state_dict(o.state_dict())


def _arm(eng, steps):
    from mvoc_amd import pnp_utils
    from mvoc_amd.schedulers import DDIMScheduler
    pipe = types.SimpleNamespace(unet=eng)
    s = DDIMScheduler()
    s.set_timesteps(steps)
    pnp_utils.register_temp_attention_pnp(pipe, s.timesteps[:steps], False)
    pnp_utils.register_spatial_attention_pnp(pipe, s.timesteps[:steps], False)
    pnp_utils.register_temp_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_out_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_resnet_injection(pipe, s.timesteps[:1])
    return pipe, [int(t) for t in s.timesteps[:2]]  # (feature-injection step, Q/K-only step)


def _disarm(eng, pipe):
    from mvoc_amd import pnp_utils
    pnp_utils.register_time_all(pipe, None, None)
    for blk in eng.up_blocks:
        for m in list(blk.resnets) + list(blk.temp_convs):
            m.injection_schedule = None
        for tr in list(blk.attentions) + list(blk.temp_attentions):
            tr.transformer_blocks[0].attn1.processor.injection_schedule = None
    eng.conv_out.injection_schedule = None


def _roles(F, h, w, cd, seed, K):
    """per-role rows: 'S', 'O', 'P' three sources; 'u0'.. / 'c0'.. the destination pairs (a pair shares latents and image
    latents, as classifier-free guidance feeds them; every variant has its own)"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).half().cuda()
    nt = 7 if cd == 64 else 77
    row = lambda: dict(sample=mk(1, 4, F, h, w), il1=mk(1, 4, F, h, w) * 0.18, il=mk(1, 4, F, h, w) * 0.18, ie=mk(1, F, cd), eh=mk(1, nt, cd))
    r = {k: row() for k in ("S", "O", "P")}
    for k in range(K):
        r[f"u{k}"] = row()
        r[f"c{k}"] = dict(r[f"u{k}"], ie=mk(1, F, cd), eh=mk(1, nt, cd))
    return r


def _batch(roles, names):
    b = {k: torch.cat([roles[n][k] for n in names]).contiguous() for k in roles["S"]}
    b["fps"] = torch.full((len(names),), 8.0, device="cuda")
    return b


def _fwd(eng, x, t):
    return eng.forward_ext(x["sample"], torch.tensor([float(t)]).cuda(), x["fps"], x["il1"], x["il"], x["ie"], x["eh"])[0]


def _close(a, b, what):
    """the bar of test_source_dedup_gpu.py for the engine's forward at another batch size"""
    d = (a.float() - b.float()).abs().max() / b.float().abs().max()
    rel = (a.float() - b.float()).norm() / b.float().norm()
    print(f"{what}: vs the single-variant engine forward max-abs/max {float(d):.2e}, rel-L2 {float(rel):.2e}"
          f"{' (bit-identical)' if torch.equal(a, b) else ''}")
    assert torch.isfinite(a).all() and d < 8e-3 and rel < 5e-3, (what, float(d), float(rel))


def _close_oracle(a, ref, what):
    """the project's forward tolerance: rel-L2 <= 3e-3, max-abs <= 2e-2 * max|ref|"""
    a, ref = a.float().cpu(), ref.float()
    rel = (a - ref).norm() / ref.norm()
    d = (a - ref).abs().max() / ref.abs().max()
    print(f"{what}: vs the oracle rel-L2 {float(rel):.2e}, max-abs/max|ref| {float(d):.2e}")
    assert torch.isfinite(a).all() and rel <= 3e-3 and d <= 2e-2, (what, float(rel), float(d))


def _hook_masks(F, h, w):
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (2, F, h, w), generator=g)
    cpu = [((u8[j].float() / 255).half()[None, None].repeat(1, 4, 1, 1, 1), (u8[j] > 10)[None, None].repeat(1, 4, 1, 1, 1)) for j in range(2)]
    return cpu, [(a.cuda(), b.cuda()) for a, b in cpu]


def _variant_forward(eng, roles, t, src, smap, K, cfg, dead, tail=True):
    """the engine under ``variants = K`` on [src.., u_0..u_{K-1}, c_0..c_{K-1}] -> per variant its destination chunks"""
    names = list(src) + ([f"u{k}" for k in range(K)] if cfg else []) + [f"c{k}" for k in range(K)]
    saved = eng.prune_dead_chunks
    eng.source_chunks, eng.variants, eng.prune_source_tail, eng.prune_dead_chunks = smap, K, tail, dead
    try:
        out = _fwd(eng, _batch(roles, names), t)
    finally:
        eng.source_chunks, eng.variants, eng.prune_source_tail, eng.prune_dead_chunks = None, 1, False, saved
    assert out.shape[0] == len(names)
    ns, ndst = len(src), 2 if cfg else 1
    return [torch.cat([out[ns + d * K + k][None] for d in range(ndst)]) for k in range(K)]


def _single_forward(eng, roles, t, src, smap, k, cfg, dead, tail=True):
    names = list(src) + ([f"u{k}"] if cfg else []) + [f"c{k}"]
    saved = eng.prune_dead_chunks
    eng.source_chunks, eng.prune_source_tail, eng.prune_dead_chunks = smap, tail, dead
    try:
        out = _fwd(eng, _batch(roles, names), t)
    finally:
        eng.source_chunks, eng.prune_source_tail, eng.prune_dead_chunks = None, False, saved
    return out[len(src):]


# (kind, K, guidance, compact sources, source map, the sources expanded to [bg, obj_1, obj_2], prune_dead_chunks)
TOY_CASES = [
    ("feature", 2, True, "SOP", None, "SOP", True),
    ("feature", 2, True, "SOP", None, "SOP", False),
    ("feature", 3, True, "S", (1, (0, 0)), "SSS", True),
    ("feature", 3, False, "SOP", None, "SOP", False),
    ("feature", 2, False, "SO", (2, (1, 1)), "SOO", True),
    ("feature", 3, True, "SO", (2, (1, 0)), "SOS", False),
    ("qk", 2, True, "SOP", None, "SOP", True),
    ("qk", 3, True, "SOP", None, "SOP", False),
    ("qk", 2, False, "SOP", None, "SOP", True),
    ("qk", 3, False, "S", (1, (0, 0)), "SSS", True),
    ("qk", 2, True, "SO", (2, (0, 1)), "SSO", False),
    ("qk", 3, True, "S", (1, (0, 0)), "SSS", True),
]


@pytest.mark.parametrize("case", TOY_CASES, ids=lambda c: f"{c[0]}-K{c[1]}-{'cfg' if c[2] else 'nocfg'}-{c[3]}-{'dead' if c[6] else 'alive'}")
def test_unet_variants_against_the_oracle_and_the_single_variant_forward(case):
    from oracle.pnp_model_ref import PnPState, install_pnp
    from oracle import sched_ref
    from mvoc_amd import pnp_utils
    kind, K, cfg, src, smap, full, dead = case
    F, h, w, cd, steps = 3, 8, 8, 64, 5
    o, eng = _toy_pair()
    cpu_masks, masks = _hook_masks(F, h, w)
    roles = _roles(F, h, w, cd, 4, K)
    pipe, (t_feat, t_qk) = _arm(eng, steps)
    t = t_feat if kind == "feature" else t_qk
    rs = sched_ref.DDIMSchedulerRef()
    rs.set_timesteps(steps)
    st = PnPState(conv_schedule=rs.timesteps[:1], spatial_schedule=rs.timesteps[:steps], temporal_schedule=rs.timesteps[:steps])
    install_pnp(o, st)
    st.t, st.masks, st.ndst = t, cpu_masks, 2 if cfg else 1
    try:
        pnp_utils.register_time_all(pipe, t, masks)
        outs = _variant_forward(eng, roles, t, src, smap, K, cfg, dead)
        for k in range(K):
            what = f"{kind} step K={K} variant {k} {'cfg' if cfg else 'no cfg'} {src} {smap} prune_dead_chunks={dead}"
            names = list(full) + ([f"u{k}"] if cfg else []) + [f"c{k}"]
            b = {key: v.float().cpu() for key, v in _batch(roles, names).items()}
            ref = o.forward_ext(b["sample"], t, torch.tensor([8] * len(names)), b["il1"], b["il"], b["ie"], b["eh"])[0]
            _close_oracle(outs[k], ref[len(full):], what)
            _close(outs[k], _single_forward(eng, roles, t, src, smap, k, cfg, dead), what)
    finally:
        _disarm(eng, pipe)


def test_unet_one_variant_is_the_plain_call_and_a_wrong_batch_is_refused():
    from mvoc_amd import pnp_utils
    _, eng = _toy_pair()
    F, h, w, cd = 3, 8, 8, 64
    _, masks = _hook_masks(F, h, w)
    roles = _roles(F, h, w, cd, 1, 2)
    pipe, (t_feat, t_qk) = _arm(eng, 5)
    try:
        for t in (t_feat, t_qk):
            pnp_utils.register_time_all(pipe, t, masks)
            plain = _fwd(eng, _batch(roles, ["S", "O", "P", "u0", "c0"]), t)
            assert eng.variants == 1
            eng.variants = 1
            assert torch.equal(_fwd(eng, _batch(roles, ["S", "O", "P", "u0", "c0"]), t), plain)
        eng.variants = 2
        with pytest.raises(RuntimeError, match="UNet batch is 6"):  # (3 + 2 would be two variants with guidance off)
            _fwd(eng, _batch(roles, ["S", "O", "P", "u0", "c0", "c1"]), t_qk)
        with pytest.raises(RuntimeError, match="UNet batch is 8"):
            _fwd(eng, _batch(roles, ["S", "O", "P", "u0", "u1", "c0", "c1", "c1"]), t_qk)
        eng.variants = 9
        with pytest.raises(RuntimeError, match="1 to 8"):
            _fwd(eng, _batch(roles, ["S", "O", "P", "u0", "c0"]), t_qk)
        eng.variants, eng.shared_prefix_chunks = 2, 2
        with pytest.raises(RuntimeError, match="shared_prefix_chunks"):
            _fwd(eng, _batch(roles, ["S", "O", "P", "u0", "u1", "c0", "c1"]), t_qk)
    finally:
        eng.variants, eng.shared_prefix_chunks = 1, 0
        _disarm(eng, pipe)


def test_unet_variants_full_size():
    """one of each step kind on the 1.42 B network at 16 x 64 x 64, K = 2, against the single-variant engine forward; then a Q/K
    step at K = 5: UNet batch 13, past the 2 GB line of the eight-phase GEMM tiles (the dispatch falls back by itself)"""
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import crosses_gemm_offset_line
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cuda:0").init_random(8888)
    F, h, w, cd, K = 16, 64, 64, 1024, 2
    _, masks = _hook_masks(F, h, w)
    roles = _roles(F, h, w, cd, 4, 5)
    pipe, (t_feat, t_qk) = _arm(eng, 50)
    try:
        for kind, t in (("feature", t_feat), ("qk", t_qk)):
            pnp_utils.register_time_all(pipe, t, masks)
            outs = _variant_forward(eng, roles, t, "SOP", None, K, True, True)
            for k in range(K):
                _close(outs[k], _single_forward(eng, roles, t, "SOP", None, k, True, True), f"full size {kind} step K=2 variant {k}")
        assert crosses_gemm_offset_line(3 + 2 * 5, F, h, w, eng.config.block_out_channels[0])
        outs = _variant_forward(eng, roles, t_qk, "SOP", None, 5, True, True)
        for k in (0, 4):
            _close(outs[k], _single_forward(eng, roles, t_qk, "SOP", None, k, True, True), f"full size qk step K=5 (batch 13) variant {k}")
    finally:
        _disarm(eng, pipe)


# ---- loop ------------------------------------------------------------------------------------------------------------
GUIDANCE = (9.0, 6.0)


def _variants_job(graphs, shared=False, dedup=False, K=2, per_prompt=1, steps=5):
    """test_composition_vs_oracle's job with three distinct sources (``shared``: ONE source behind every role) and K variants:
    two prompts, two initial latents, two guidance scales, two main images.  The oracle's loop once per variant, the HIP
    pipeline once, the UNet batch of every network run."""
    from oracle import loops_ref, sched_ref
    from oracle.pnp_model_ref import PnPState, install_pnp
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    o, eng = _toy_pair()
    g = torch.Generator().manual_seed(5)
    f, h, w, cd, n = 3, 8, 8, 64, steps
    nrow = 3 + 2 * K  # rows: bg, obj_1, obj_2, then (u_k, c_k) per variant
    cond = dict(encoder_hidden_states=torch.randn(nrow, 7, cd, generator=g).half(), image_embeddings=torch.randn(nrow, f, cd, generator=g).half(),
                image_latents_first=torch.randn(nrow, 4, f, h, w, generator=g).half(), image_latents=torch.randn(nrow, 4, f, h, w, generator=g).half())
    for key in cond:
        if shared or key == "encoder_hidden_states":  # (the inversion prompt is one for all sources)
            cond[key][1] = cond[key][0]
            cond[key][2] = cond[key][0]
    for k in range(K):
        u, c = 3 + 2 * k, 4 + 2 * k
        cond["image_embeddings"][u] = 0
        cond["image_latents_first"][u] = cond["image_latents_first"][c]
        cond["image_latents"][c] = cond["image_latents_first"][c]
        cond["image_latents"][u] = cond["image_latents"][c]
    cpu_masks, _ = _hook_masks(f, h, w)
    s = DDIMScheduler()
    s.set_timesteps(n)
    dirs = ["/virtual/bg", "/virtual/bg", "/virtual/bg"] if shared else ["/virtual/bg", "/virtual/o1", "/virtual/o2"]
    src = {d: {int(t): torch.randn(1, 4, f, h, w, generator=g).half() for t in s.timesteps} for d in dict.fromkeys(dirs)}
    x0 = torch.randn(K, 4, f, h, w, generator=g).half()
    rs = sched_ref.DDIMSchedulerRef()
    rs.set_timesteps(n)
    st = PnPState(conv_schedule=rs.timesteps[:1], spatial_schedule=rs.timesteps[:3], temporal_schedule=rs.timesteps[:4])
    install_pnp(o, st)
    st.masks = cpu_masks
    kw = dict(ddim_init_latents_t_idx=0, fusion_steps=(0, 2), random_noise_ratio=0.3, obj_random_noise_fusion=True)
    refs = []
    for k in range(K if per_prompt == 1 else 0):
        rows = [0, 1, 2, 3 + 2 * k, 4 + 2 * k]

        def unet_fn(inp, t, rows=rows):
            st.t = int(t)
            return o.forward_ext(inp.float(), int(t), torch.tensor([8] * 5), cond["image_latents_first"][rows].float(),
                                 cond["image_latents"][rows].float(), cond["image_embeddings"][rows].float(),
                                 cond["encoder_hidden_states"][rows].float())[0].half()

        refs.append(loops_ref.composition_loop(unet_fn, sched_ref.DDIMSchedulerRef(), x0[k:k + 1], lambda t: src[dirs[0]][t],
                                               lambda j, t: src[dirs[1 + j]][t], [m[0] for m in cpu_masks], n,
                                               guidance_scale=GUIDANCE[k % 2], **kw))
    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=graphs)
    pipe.dedup_sources = dedup
    pnp_utils.register_temp_attention_pnp(pipe, s.timesteps[:4], False)
    pnp_utils.register_spatial_attention_pnp(pipe, s.timesteps[:3], False)
    pnp_utils.register_temp_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_out_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_resnet_injection(pipe, s.timesteps[:1])
    pipe.latent_cache.write_files = False
    for d, lat in src.items():
        for t, v in lat.items():
            pipe.latent_cache.put(d, t, v.cuda())

    class Cond:  # the reference's assembly order
        def encode_prompt(self, prompt, negative_prompt=None):
            if str(prompt).startswith("edit"):
                k = int(prompt[4:])
                return cond["encoder_hidden_states"][4 + 2 * k:5 + 2 * k].cuda(), cond["encoder_hidden_states"][3 + 2 * k:4 + 2 * k].cuda()
            return cond["encoder_hidden_states"][0:1].cuda(), None

        def image_latents(self, image, num_frames, height, width):
            idx, fr, first = image
            return cond["image_latents_first" if first else "image_latents"][idx:idx + 1].cuda()

        def encode_image(self, image):
            idx, fr, first = image
            return cond["image_embeddings"][idx:idx + 1, fr:fr + 1].cuda()

    pipe.conditioner = Cond()
    batches = []
    emb = eng._embeddings

    def recording(timestep, fps, B):  # once per run of the network, with the batch it really runs
        batches.append(B)
        return emb(timestep, fps, B)

    eng._embeddings = recording
    clips = [[(r, i, False) for i in range(f)] for r in range(3)]
    if per_prompt == 1:
        var = dict(prompt=[f"edit{k}" for k in range(K)], main_first_image=[(4 + 2 * k, 0, True) for k in range(K)],
                   main_image_list=[[(4 + 2 * k, i, False) for i in range(f)] for k in range(K)], latents=x0.cuda(),
                   guidance_scale=[GUIDANCE[k % 2] for k in range(K)], negative_prompt=["neg"] * K)
    else:  # diffusers' num_videos_per_prompt: one prompt, one generator drawn once per video
        var = dict(prompt="edit0", main_first_image=(4, 0, True), main_image_list=[(4, i, False) for i in range(f)],
                   num_videos_per_prompt=per_prompt, generator=torch.Generator().manual_seed(3), guidance_scale=9.0, negative_prompt="neg")
    out = pipe.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection(
        background_first_image=(0, 0, True), background_image_list=clips[0], objs_first_image=[(1, 0, True), (2, 0, True)],
        objs_image_list=[clips[1], clips[2]], height=h * 8, width=w * 8, num_frames=f, num_inference_steps=n,
        target_fps=8, output_type="latent", ddim_inv_prompt="", bg_inv_latents_path=dirs[0], obj_ddim_latents_path=dirs[1:],
        obj_ddim_latents_idx_offset=[0, 0], obj_masks_tensors=[(a.clone(), b.clone()) for a, b in cpu_masks], **var, **kw).frames
    eng._embeddings = emb
    return types.SimpleNamespace(out=out, refs=refs, batches=batches, pipe=pipe)


def _check_refs(job, what):
    for k, ref in enumerate(job.refs):
        d = (job.out[k:k + 1].cpu().float() - ref.float()).abs().max()
        print(f"{what}: variant {k} after {len(job.batches)} network runs vs the oracle's loop for that variant: max-abs {float(d):.2e}")
        assert d < 3e-2, (k, float(d))


def test_variants_composition_vs_oracle_and_graph_replay():
    """three distinct sources, K = 2: n + 1 + 2K = 7 chunks on the Q/K steps (and on the last, hook-free step), the n + 1 = 3
    source chunks once on the conv_out-injection step"""
    eager = _variants_job(False)
    assert eager.out.shape[0] == 2
    assert eager.batches == [3, 7, 7, 7, 7], eager.batches
    _check_refs(eager, "eager")
    graphed = _variants_job(True)
    assert set(graphed.batches) == {3, 7}, graphed.batches  # (the network runs only while a step kind is warmed up and captured)
    _check_refs(graphed, "graphed")
    assert torch.equal(graphed.out, eager.out)


def test_variants_composition_with_one_deduplicated_source():
    """dedup_sources and one source behind every role: 1 chunk on the conv_out-injection step, 1 + 2K on the Q/K steps; the
    second fusion step hands the objects latents of another t than the background (a partial map: 2 + 2K)"""
    eager = _variants_job(False, shared=True, dedup=True)
    assert eager.batches == [1, 6, 5, 5, 5], eager.batches
    _check_refs(eager, "eager, one source")
    graphed = _variants_job(True, shared=True, dedup=True)
    assert set(graphed.batches) == {1, 5, 6}, graphed.batches
    assert torch.equal(graphed.out, eager.out)


def test_num_videos_per_prompt_returns_that_many_videos():
    job = _variants_job(False, K=2, per_prompt=2, steps=4)
    assert job.out.shape[0] == 2, tuple(job.out.shape)
    assert job.batches == [3, 7, 7, 7], job.batches
    assert torch.isfinite(job.out).all() and not torch.equal(job.out[0], job.out[1])  # two draws of the one generator


# ---- loop glue bit for bit ----------------------------------------------------------------------------------------------
def _glue_pipe():
    """the toy engine (attribute tree for the hooks) with its forward replaced by the elementwise fp16 stand-in of
    tests/g8_common.py -- batch-independent by construction, so K variants must equal K single calls bit for bit"""
    from g8_common import fake_unet, seeded, prompt_key
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    _, eng = _toy_pair()
    D = 64
    calls = []

    def fwd_ext(sample, timestep, fps, image_latents_first, image_latents, image_embeddings=None, encoder_hidden_states=None, **kw):
        calls.append(sample.clone())
        return (fake_unet(sample, timestep, encoder_hidden_states, fps, image_latents_first, image_latents, image_embeddings),)

    eng.forward_ext = fwd_ext
    eng.prepare_conditioning = lambda *a, **k: None

    class Cond:
        def encode_prompt(self, prompt, negative_prompt=None):
            return seeded(prompt_key(prompt), (1, 7, D)).cuda(), seeded(1000 + prompt_key(negative_prompt), (1, 7, D)).cuda()

        def encode_image(self, image):
            return seeded(300 + int(image), (1, D))[None].cuda()

        def image_latents(self, image, num_frames, height, width):
            h, w = height // 8, width // 8
            first = (seeded(500 + int(image), (1, 4, h, w)) * 0.18215)[:, :, None]
            ramp = [torch.full((1, 4, 1, h, w), k / (num_frames - 1)).half() for k in range(1, num_frames)]
            return torch.cat([first] + ramp, 2).cuda()

    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), conditioner=Cond(), use_graphs=False)
    full = DDIMScheduler()
    full.set_timesteps(5)
    pnp_utils.register_temp_attention_pnp(pipe, full.timesteps[:5], False)
    pnp_utils.register_spatial_attention_pnp(pipe, full.timesteps[:5], False)
    pnp_utils.register_temp_conv_injection(pipe, full.timesteps[:2])
    pnp_utils.register_out_conv_injection(pipe, full.timesteps[:2])
    pnp_utils.register_resnet_injection(pipe, full.timesteps[:2])
    return pipe, calls, full


@pytest.mark.parametrize("gs", [(9.0, 7.5, 4.0), (1.0, 1.0, 1.0)])
def test_loop_glue_three_variants_equal_three_single_calls(gs):
    from g8_common import seeded
    Fr, h, w, K = 4, 6, 5, 3
    pipe, calls, full = _glue_pipe()
    pipe.latent_cache.write_files = False
    dirs = {}
    for name, key in (("bg", 20), ("obj0", 30), ("obj1", 40)):
        dirs[name] = f"/virtual/glue_{name}"
        for t in full.timesteps:
            pipe.latent_cache.put(dirs[name], int(t), seeded(key * 1000 + int(t), (1, 4, Fr, h, w)).cuda())
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (2, Fr, h, w), generator=g)
    masks = [((u8[j].float() / 255).half()[None, None].repeat(1, 4, 1, 1, 1).cuda(), (u8[j] > 10)[None, None].repeat(1, 4, 1, 1, 1).cuda())
             for j in range(2)]
    xT = torch.randn(K, 4, Fr, h, w, generator=g).half().cuda()
    prompts, negs, mains = ["windsurf", "kayak", "a red sail"], ["chaotic", "dull", "chaotic"], [1, 6, 1]
    shared = dict(background_first_image=2, background_image_list=[20 + i for i in range(Fr)], objs_first_image=[4, 5],
                  objs_image_list=[[40 + i for i in range(Fr)], [50 + i for i in range(Fr)]], height=h * 8, width=w * 8, target_fps=8,
                  num_frames=Fr, num_inference_steps=5, output_type="latent", ddim_init_latents_t_idx=1, ddim_inv_prompt="",
                  obj_mask=["0", "1"], obj_ddim_latents_idx_offset=[0, 1], bg_inv_latents_path=dirs["bg"],
                  obj_ddim_latents_path=[dirs["obj0"], dirs["obj1"]], obj_masks_tensors=masks, random_noise_ratio=0.3,
                  obj_random_noise_fusion=True, fusion_steps=(0, 2))
    run = pipe.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection
    singles = []
    for k in range(K):
        del calls[:]
        out = run(prompt=prompts[k], negative_prompt=negs[k], guidance_scale=gs[k], main_first_image=mains[k],
                  main_image_list=[10 * mains[k] + i for i in range(Fr)], latents=xT[k:k + 1], **shared).frames
        singles.append((list(calls), out))
    del calls[:]
    out = run(prompt=prompts, negative_prompt=negs, guidance_scale=list(gs), main_first_image=mains,
              main_image_list=[[10 * m + i for i in range(Fr)] for m in mains], latents=xT, **shared).frames
    assert out.shape[0] == K and len(calls) == 4
    ndst = 2 if gs[0] > 1 else 1
    for k in range(K):
        sc, so = singles[k]
        assert len(sc) == 4
        for i in range(4):  # the latents every step starts from (and the sources beside them), bit for bit
            assert calls[i].shape[0] == 3 + ndst * K and sc[i].shape[0] == 3 + ndst
            assert torch.equal(_i16(calls[i][:3]), _i16(sc[i][:3])), (k, i)
            for d in range(ndst):
                assert torch.equal(_i16(calls[i][3 + d * K + k]), _i16(sc[i][3 + d])), (k, i, d)
        assert torch.equal(_i16(out[k:k + 1]), _i16(so)), k


# ---- C-ABI calls per step -----------------------------------------------------------------------------------------------
def _count_step_calls(K):
    """every mvoc_* call of one eager fusion + conv_out-injection step and of one eager Q/K step, K variants"""
    from launch_census import Recorder
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline, variant_layout
    from mvoc_amd.schedulers import DDIMScheduler
    _, eng = _toy_pair()
    g = torch.Generator().manual_seed(8)
    f, h, w, cd, n = 4, 8, 8, 64, 5
    lay = variant_layout(2, K, True)
    nb = lay["nb"]
    mk = lambda *s: torch.randn(*s, generator=g).half().cuda()
    cond = dict(encoder_hidden_states=mk(nb, 7, cd), image_embeddings=mk(nb, f, cd), image_latents_first=mk(nb, 4, f, h, w),
                image_latents=mk(nb, 4, f, h, w), fps=torch.full((nb,), 8.0, device="cuda"))
    _, masks = _hook_masks(f, h, w)
    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False)
    s = pipe.scheduler
    s.set_timesteps(n)
    pnp_utils.register_temp_attention_pnp(pipe, s.timesteps[:4], False)
    pnp_utils.register_spatial_attention_pnp(pipe, s.timesteps[:3], False)
    pnp_utils.register_temp_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_out_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_resnet_injection(pipe, s.timesteps[:1])
    scales = [9.0, 7.0, 5.0, 3.0][:K]
    st = pipe.make_composition_state(mk(K, 4, f, h, w), cond, masks, scales if K > 1 else scales[0], variants=K)
    table = torch.stack([s.coef_table(pipe.device, gs)[0] for gs in scales], 1).contiguous()
    index = s.coef_table(pipe.device, scales[0])[1]
    lat = lambda: mk(1, 4, f, h, w)
    counts = []
    for i, fuse in ((0, True), (1, False)):
        t = int(s.timesteps[i])
        row = table[index[t]] if K > 1 else table[index[t], 0]
        objs = [lat(), lat()]
        rec = Recorder()
        rec.install()
        try:
            pipe.composition_step(st, t, lat(), objs, row, (0.3, True, objs) if fuse else None)
        finally:
            rec.uninstall()
        torch.cuda.synchronize()
        counts.append(rec.calls)
    pnp_utils.register_time_all(pipe, None, None)
    return counts


def test_c_abi_calls_per_step_do_not_depend_on_k():
    one, four = _count_step_calls(1), _count_step_calls(4)
    twins = {"mvoc_pnp_blend_scatter_tokens_variants": "mvoc_pnp_blend_scatter_tokens", "mvoc_pnp_blend_scatter_nchw_variants":
             "mvoc_pnp_blend_scatter_nchw", "mvoc_ddim_step_variants_f16": "mvoc_ddim_step_f16",
             "mvoc_latent_fusion_variants_f16": "mvoc_latent_fusion_f16"}
    for kind, a, b in zip(("fusion + conv_out-injection step", "Q/K step"), one, four):
        diff = {k: (a.get(k, 0), b.get(k, 0)) for k in sorted(set(a) | set(b)) if a.get(k, 0) != b.get(k, 0)}
        print(f"{kind}: {sum(a.values())} C-ABI calls at K = 1, {sum(b.values())} at K = 4; by name (K = 1, K = 4): {diff}")
        assert sum(a.values()) == sum(b.values()), (kind, diff)
        for v, base in twins.items():  # the _variants entries stand in for their twins, call for call
            assert a.get(v, 0) == 0 and b.get(base, 0) == 0 and b.get(v, 0) == a.get(base, 0), (kind, v)


# ---- composite.py ---------------------------------------------------------------------------------------------------------
def test_composite_py_writes_one_directory_per_variant():
    """inverse.py x 3 + composite.py on an entry with `variants` (tools/demo_job.py --variants), tiny sizes: the usual files of a
    composition under variant_00/ and variant_01/"""
    import importlib.util
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("demo_job_variants", os.path.join(repo, "tools", "demo_job.py"))
    dj = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dj)
    saved_path, saved_env = list(sys.path), {k: os.environ.get(k) for k in ("MVOC_SYNTHETIC_VAE", "MVOC_SYNTHETIC_CLIP")}
    try:
        res = dj.run_variants(frames=4, size=64, steps=5, keep=False, variants=2)
    finally:
        sys.path[:] = saved_path
        for k, v in saved_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        for m in ("utils", "pnp_utils", "inverse", "composite", "pipelines", "pipelines.pipeline_i2vgen_xl"):
            sys.modules.pop(m, None)
    assert res["output_dirs"] == ["variant_00", "variant_01"] and res["unet_batch"] == {"qk": 7, "conv_out_injection": 3}
    assert res["n_result_files"] == {"variant_00": 5, "variant_01": 5}  # video.gif + one png per frame
    assert res["result_files"][0] == "video.gif" and res["result_files"][1] == "video_00000.png"
