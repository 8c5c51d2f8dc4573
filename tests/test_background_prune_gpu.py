"""GPU: dropping the dead background chunk on Q/K-only composition steps -- the positional blend without a
background chunk bit for bit against the layout that has one, the refusals, the toy UNet with the switch on against off, the
cases that fall back to the full batch, and the composition loop alternating both kinds of step under graphs."""
import ctypes as C
import itertools

import pytest
import torch

import test_variants_gpu as tv

pytestmark = pytest.mark.gpu

H16 = torch.float16
SENTINEL = 777.0


def _i16(t):
    return t.contiguous().view(torch.int16)


# ---- the blend kernel ----------------------------------------------------------------------------------------------------
F_, H_, W_, MH, MW = 2, 5, 7, 3, 4  # (masks 3 x 4 on 5 x 7 pixels: the nearest resize is exercised)


def _blend_buffers(nobj, ndst, c, seed):
    """[guard, bg, obj_1..obj_n, dst.., guard] chunks of F*HW rows in a [rows, 3C] qkv buffer; the guards hold a sentinel"""
    g = torch.Generator().manual_seed(seed)
    per = F_ * H_ * W_
    nchunk = 1 + 1 + nobj + ndst + 1
    buf = torch.randn(nchunk * per, 3 * c, generator=g).half().cuda()
    buf[:per] = SENTINEL
    buf[(nchunk - 1) * per:] = SENTINEL
    masks = (torch.randint(0, 256, (nobj, F_, MH, MW), generator=g).float() / 255).half().cuda()
    masks[:, :, 0, 0] = 0.0
    masks[:, :, -1, -1] = 1.0
    return buf, masks, per


def _blend(buf, masks, first_chunk, per, c, both, ndst, **kw):
    from mvoc_amd import ops
    ld = buf.stride(0)
    rows = buf[first_chunk * per:]
    ops.pnp_blend_tokens(rows[:, :c], masks, x2=rows[:, c:2 * c] if both else None, frames=F_, height=H_, width=W_, channels=c,
                         chunk_stride=per * ld, f_stride=H_ * W_ * ld, p_stride=ld, ndst=ndst, **kw)


@pytest.mark.parametrize("c", [8, 24])
@pytest.mark.parametrize("both", [False, True], ids=["q", "qk"])
@pytest.mark.parametrize("nobj,ndst", list(itertools.product([1, 2, 3, 4], [1, 2])))
def test_blend_without_a_background_chunk_is_the_positional_blend(nobj, ndst, both, c):
    buf, masks, per = _blend_buffers(nobj, ndst, c, 100 * nobj + 10 * ndst + c)
    ref, got = buf.clone(), buf.clone()
    ref[per:2 * per] = float("nan")  # the positional call must not read its background chunk (base = the last chunk)
    got[per:2 * per] = SENTINEL      # ... and here that chunk is a second guard in front of the first object chunk
    ref0, got0 = ref.clone(), got.clone()
    _blend(ref, masks, 1, per, c, both, ndst)
    _blend(got, masks, 2, per, c, both, ndst, no_background=True)
    torch.cuda.synchronize()
    d0 = (2 + nobj) * per  # first destination row
    d1 = d0 + ndst * per
    assert torch.equal(_i16(got[d0:d1]), _i16(ref[d0:d1]))
    assert not torch.isnan(ref[d0:d1]).any()
    assert not torch.equal(_i16(got[d0:d1, :c]), _i16(got0[d0:d1, :c]))  # the blend wrote something
    # nothing but q (and k) of the destination chunks changed: guards, objects, v -- and k when only q is blended
    keep = c if not both else 2 * c
    for t, t0 in ((got, got0), (ref, ref0)):
        assert torch.equal(_i16(t[:d0]), _i16(t0[:d0])) and torch.equal(_i16(t[d1:]), _i16(t0[d1:]))
        assert torch.equal(_i16(t[d0:d1, keep:]), _i16(t0[d0:d1, keep:]))
    assert bool((got[:2 * per] == SENTINEL).all()) and bool((got[d1:] == SENTINEL).all())
    if ndst == 2:  # one blend, stored twice
        assert torch.equal(_i16(got[d0:d0 + per, :keep]), _i16(got[d0 + per:d1, :keep]))


def test_the_flag_is_refused_where_nothing_reads_it():
    from mvoc_amd import ops
    nobj, ndst, c = 2, 2, 8
    buf, masks, per = _blend_buffers(nobj, ndst, c, 7)
    keep = buf.clone()
    ld = buf.stride(0)
    rows = buf[2 * per:]  # [obj_1, obj_2, uncond, cond, guard]

    def desc():  # the layout travels as base_chunk0 = -1 (include/mvoc_hip.h), so it cannot meet base_chunk0 = 1 in a descriptor:
        # that combination is refused where it can be asked for, in ops (below)
        return ops._pnp_desc(rows[:, :c], rows[:, c:2 * c], masks, per * ld, H_ * W_ * ld, ld, F_, H_, W_, c, -1, ndst)

    lib, s = ops.lib, ops._stream()
    arr = (C.c_int32 * nobj)(*range(nobj))
    place = torch.zeros(nobj, F_, 2, dtype=torch.int32, device="cuda")
    calls = [("tokens_mapped", lambda d: lib.mvoc_pnp_blend_scatter_tokens_mapped(C.byref(d), nobj, arr, s)),
             ("tokens_variants", lambda d: lib.mvoc_pnp_blend_scatter_tokens_variants(C.byref(d), nobj, arr, 1, s)),
             ("tokens_variants_sel", lambda d: lib.mvoc_pnp_blend_scatter_tokens_variants_sel(C.byref(d), nobj, arr, 1, 1, s)),
             ("tokens_placed", lambda d: lib.mvoc_pnp_blend_scatter_tokens_placed(C.byref(d), nobj, arr, 1, 1, place.data_ptr(), s)),
             ("tokens_placed_variants",
              lambda d: lib.mvoc_pnp_blend_scatter_tokens_placed_variants(C.byref(d), nobj, arr, 1, 1, place.data_ptr(), s))]
    for name, call in calls:
        assert call(desc()) != 0, name
    # every _nchw entry, on a contiguous [(nobj + 1 + ndst) F, C, H, W] tensor
    x = torch.randn((nobj + 1 + ndst) * F_, 4, H_, W_).half().cuda()
    xk = x.clone()
    hard = (masks[:, :, :1, :1] > 0.5).half().expand(nobj, F_, H_, W_).contiguous()

    def ndesc():
        return ops._pnp_desc(x, None, hard, 0, 0, 0, F_, H_, W_, 4, -1, ndst)

    full = (C.c_int32 * nobj)(*range(1, nobj + 1))
    ncalls = [("nchw", lambda d: lib.mvoc_pnp_blend_scatter_nchw(C.byref(d), s)),
              ("nchw_mapped", lambda d: lib.mvoc_pnp_blend_scatter_nchw_mapped(C.byref(d), nobj + 1, full, s)),
              ("nchw_variants", lambda d: lib.mvoc_pnp_blend_scatter_nchw_variants(C.byref(d), nobj + 1, full, 1, s)),
              ("nchw_variants_sel", lambda d: lib.mvoc_pnp_blend_scatter_nchw_variants_sel(C.byref(d), nobj + 1, full, 1, 1, s)),
              ("nchw_placed", lambda d: lib.mvoc_pnp_blend_scatter_nchw_placed(C.byref(d), nobj + 1, full, 1, 1, place.data_ptr(), s)),
              ("nchw_placed_variants",
               lambda d: lib.mvoc_pnp_blend_scatter_nchw_placed_variants(C.byref(d), nobj + 1, full, 1, 1, place.data_ptr(), s))]
    for name, call in ncalls:
        assert call(ndesc()) != 0, name
    torch.cuda.synchronize()
    assert torch.equal(_i16(buf), _i16(keep)) and torch.equal(_i16(x), _i16(xk))  # nothing was written
    # the same descriptor with base_chunk0 = 0 is taken (the refusals above are the layout's)
    d = desc()
    d.base_chunk0 = 0
    assert lib.mvoc_pnp_blend_scatter_tokens_mapped(C.byref(d), nobj, arr, s) == 0
    torch.cuda.synchronize()
    buf.copy_(keep)
    # ops raises on the same combinations before it calls the library
    kw = dict(frames=F_, height=H_, width=W_, channels=c, chunk_stride=per * ld, f_stride=H_ * W_ * ld, p_stride=ld, no_background=True)
    before = buf.clone()
    for bad, what in ((dict(base_chunk0=True), "base_chunk0"), (dict(src_map=(2, (0, 1))), "positional"), (dict(nvar=2), "positional"),
                      (dict(place=place), "positional"), (dict(nvar=2, active=1), "positional")):
        with pytest.raises(RuntimeError, match=what):
            ops.pnp_blend_tokens(rows[:, :c], masks, **kw, **bad)
    small = torch.zeros((nobj + 1) * per, 3 * c, dtype=H16, device="cuda")  # [obj_1, obj_2, uncond, cond] needs four chunks
    with pytest.raises(RuntimeError, match="storage ends before"):
        ops.pnp_blend_tokens(small[:, :c], masks, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_i16(buf), _i16(before)) and not small.any()  # ... and nothing was written


# ---- toy UNet ------------------------------------------------------------------------------------------------------------
F, h, w, cd = 3, 8, 8, 64


@pytest.fixture(scope="module")
def toy():
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    return eng, masks, tv._roles(F, h, w, cd, 4, 2)


def _rows_of(rec):
    """the most rows any GEMM of the recording ran on: B * F * h * w at the first level, whatever else the step launches"""
    m = [ln.desc.m for ln, _ in rec.launches.values() if ln.name == "mvoc_gemm_f16"]
    return max(m) // (F * h * w) if m else 0


def _forward(eng, roles, names, t, *, prune, tail=True, share=False, K=1, placement=None, smap=None, record=False):
    from launch_census import Recorder
    rec = Recorder() if record else None
    eng.prune_background, eng.prune_source_tail, eng.shared_prefix_chunks = prune, tail, 2 if share else 0
    eng.variants, eng.placement, eng.source_chunks = K, placement, smap
    if rec is not None:
        rec.install()
    try:
        out = tv._fwd(eng, tv._batch(roles, names), t)
    finally:
        if rec is not None:
            rec.uninstall()
        eng.prune_background, eng.prune_source_tail, eng.shared_prefix_chunks = False, False, 0
        eng.variants, eng.placement, eng.source_chunks = 1, None, None
    assert out.shape[0] == len(names) and not eng._no_bg
    return (out, _rows_of(rec)) if record else out


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


PLACEMENT = (((1, -2), (0, 1), (-2, 0)), ((3, 2),) * F)
FORWARD_CASES = {
    "plain": (["S", "O", "P", "u0", "c0"], {}),
    "share_cfg_prefix": (["S", "O", "P", "u0", "c0"], dict(share=True)),
    "K2": (["S", "O", "P", "u0", "u1", "c0", "c1"], dict(K=2)),
    "placed": (["S", "O", "P", "u0", "c0"], dict(placement=PLACEMENT)),
    "placed_K2": (["S", "O", "P", "u0", "u1", "c0", "c1"], dict(K=2, placement=PLACEMENT)),
    "guidance_off": (["S", "O", "P", "c0"], {}),
    "dedup_objects": (["S", "O", "u0", "c0"], dict(smap=(2, (1, 1)))),
}


@pytest.mark.parametrize("case", list(FORWARD_CASES))
def test_unet_qk_step_without_the_background_chunk(toy, case):
    """Q/K-only timestep, forward_ext with the switch on against off: chunk 0 zeros, the destination chunks within the rel-L2 1e-3
    that test_fullwidth_gpu.py holds prune_source_tail to against the five-chunk forward, and with prune_source_tail off the
    object chunks too.  (The same kernels on the same rows: bit-identical unless a launch picks another tile at the smaller M.)"""
    from mvoc_amd import pnp_utils
    eng, masks, roles = toy
    names, kw = FORWARD_CASES[case]
    nsrc = sum(1 for n in names if n in "SOP")
    pipe, (_, t_qk) = tv._arm(eng, 5)
    try:
        pnp_utils.register_time_all(pipe, t_qk, masks)
        for tail in (True, False):
            off, rows_off = _forward(eng, roles, names, t_qk, prune=False, tail=tail, record=True, **kw)
            on, rows_on = _forward(eng, roles, names, t_qk, prune=True, tail=tail, record=True, **kw)
            torch.cuda.synchronize()
            assert rows_off == len(names) and rows_on == len(names) - 1, (rows_off, rows_on)
            assert not on[0].any()
            assert torch.isfinite(on).all()
            rd = _rel(on[nsrc:], off[nsrc:])
            print(f"{case}, prune_source_tail={tail}: destination chunks rel-L2 {rd:.2e} against the full batch"
                  f"{' (bit-identical)' if torch.equal(on[nsrc:], off[nsrc:]) else ''}")
            assert rd < 1e-3, (case, tail, rd)
            if tail:
                assert not on[:nsrc].any() and not off[:nsrc].any()
            elif nsrc > 1:
                ro = _rel(on[1:nsrc], off[1:nsrc])
                print(f"{case}: object chunks rel-L2 {ro:.2e}{' (bit-identical)' if torch.equal(on[1:nsrc], off[1:nsrc]) else ''}")
                assert ro < 1e-3, (case, ro)
    finally:
        tv._disarm(eng, pipe)
        for s in eng.hook_sites():
            s.inject_background = False


@pytest.mark.parametrize("case", ["inject_background", "feature_step", "object_on_chunk_0", "no_site_injects"])
def test_unet_falls_back_to_the_full_batch(toy, case):
    from mvoc_amd import pnp_utils
    from mvoc_amd.unet import Processor
    eng, masks, roles = toy
    names, kw = ["S", "O", "P", "u0", "c0"], {}
    pipe, (t_feat, t_qk) = tv._arm(eng, 5)
    t = t_qk
    try:
        if case == "inject_background":
            for s in eng.hook_sites():
                if isinstance(s, Processor):
                    s.inject_background = True
        elif case == "feature_step":
            t, kw = t_feat, {}
            saved, eng.prune_dead_chunks = eng.prune_dead_chunks, False  # (else the step runs on the source chunks only)
        elif case == "object_on_chunk_0":
            names, kw = ["S", "O", "u0", "c0"], dict(smap=(2, (0, 1)))
        pnp_utils.register_time_all(pipe, None if case == "no_site_injects" else t, None if case == "no_site_injects" else masks)
        try:
            off = _forward(eng, roles, names, t, prune=False, tail=False, **kw)
            on, rows = _forward(eng, roles, names, t, prune=True, tail=False, record=True, **kw)
        finally:
            if case == "feature_step":
                eng.prune_dead_chunks = saved
        torch.cuda.synchronize()
        assert rows == len(names), (case, rows)
        assert torch.equal(_i16(on), _i16(off)), case
        assert on[0].any()  # (prune_source_tail is off: the background chunk's own output)
    finally:
        tv._disarm(eng, pipe)
        for s in eng.hook_sites():
            s.inject_background = False


# ---- composition loop ------------------------------------------------------------------------------------------------------
def _loop(graphs, prune=True):
    """feature step -> Q/K step -> feature step -> Q/K step on the toy pipeline; per step the chunks the network ran on"""
    from launch_census import Recorder
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    _, eng = tv._toy_pair()
    g = torch.Generator().manual_seed(11)
    mk = lambda *s: torch.randn(*s, generator=g).half().cuda()
    nb = 5
    cond = dict(encoder_hidden_states=mk(nb, 7, cd), image_embeddings=mk(nb, F, cd), image_latents_first=mk(nb, 4, F, h, w) * 0.18,
                image_latents=mk(nb, 4, F, h, w) * 0.18, fps=torch.full((nb,), 8.0, device="cuda"))
    for k in ("image_latents_first", "image_latents"):
        cond[k][3] = cond[k][4]
    _, masks = tv._hook_masks(F, h, w)
    sched = DDIMScheduler()
    sched.set_timesteps(4, device="cuda")
    ts = [int(t) for t in sched.timesteps]
    pipe = I2VGenXLPipeline(eng, sched, use_graphs=graphs)
    pipe.prune_background = prune
    pnp_utils.register_temp_attention_pnp(pipe, ts, False)
    pnp_utils.register_spatial_attention_pnp(pipe, ts, False)
    feat = [ts[0], ts[2]]
    pnp_utils.register_temp_conv_injection(pipe, feat)
    pnp_utils.register_out_conv_injection(pipe, feat)
    pnp_utils.register_resnet_injection(pipe, feat)
    st = pipe.make_composition_state(mk(1, 4, F, h, w), cond, masks, 9.0)
    table, index = sched.coef_table(pipe.device, 9.0)
    src = {t: [mk(1, 4, F, h, w) for _ in range(3)] for t in ts}
    rows = []
    try:
        for t in ts:
            rec = Recorder()
            rec.install()
            try:
                pipe.composition_step(st, t, src[t][0], src[t][1:], table[index[t]])
            finally:
                rec.uninstall()
            rows.append(_rows_of(rec))
        torch.cuda.synchronize()
        assert not eng.prune_background and not eng._no_bg  # the loop restores the engine's switch
        return st["latents"].clone(), rows, len(st["variants"])
    finally:
        pnp_utils.register_time_all(pipe, None, None)


def test_composition_loop_alternates_both_kinds_of_step_under_graphs():
    eager, rows_e, _ = _loop(False)
    assert rows_e == [3, 4, 3, 4], rows_e  # feature steps: the three source chunks; Q/K steps: [obj_1, obj_2, uncond, cond]
    graphed, rows_g, ngraphs = _loop(True)
    assert rows_g[:2] == [3, 4] and rows_g[2:] == [0, 0], rows_g  # each kind is captured once (its own graph) and replayed
    assert ngraphs == 2
    assert torch.isfinite(graphed).all() and torch.equal(_i16(graphed), _i16(eager))
    full, rows_f, _ = _loop(False, prune=False)
    assert rows_f == [3, 5, 3, 5], rows_f
    print(f"latents after four steps, background chunk dropped against kept: rel-L2 {_rel(eager, full):.2e}"
          f"{' (bit-identical)' if torch.equal(eager, full) else ''}")
