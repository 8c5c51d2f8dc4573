"""GPU: per-variant injection schedules in the K-variant composition loop.

* kernels: the ``_sel`` blend entries write, for every variant whose bit is set in ``active``, the u_k / c_k chunks the
  ``_variants`` entry writes on a clone of the input (``_same_bits`` of test_variants_gpu.py); every other chunk, the sources and
  the v columns stay int16-identical to the input; bad masks refused; the profiler's chunk count.
* UNet: a forward whose variants inject at different site families, per variant against the ORACLE run with that variant's own
  schedules (the project's forward tolerance) and against the engine's own single-variant forward (the batch-independence bar);
  a partially injecting conv_out; the launches of the paired attention.
* loop: three variants with three threshold sets against the oracle's loop per variant, graph replay against eager, one captured
  graph per distinct per-site mask tuple, equal thresholds = the calls and graphs of a call without them; composite.py's ``pnp`` key.

The small helpers (operands with specials, masks, source maps, toy engine, role batches, tolerances) are those of
test_variants_gpu.py, imported from it so that both files judge by the same bars.
"""
import ctypes as C
import itertools
import types

import pytest
import torch

import test_variants_gpu as tv

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KS = (2, 3, 8)


def _actives(K):
    """one bit, alternating bits, all but one, all"""
    full = (1 << K) - 1
    return [1 << (K // 2), 0b01010101 & full, full & ~(1 << (K - 1) // 2), full]


def _two_maps(nobj):
    m = tv._maps(nobj)
    return [m[0], m[-1]]  # the identity, a non-identity map


def _tokens_sel_direct(buf, layout, F, H, W, c, masks, base0, ndst, smap, nvar, active):
    from mvoc_amd import ops
    ld, hw = buf.stride(0), H * W
    fs, ps = tv._strides(layout, ld, F, hw)
    d = ops._pnp_desc(buf[:, :c], buf[:, c:2 * c], masks, F * hw * ld, fs, ps, F, H, W, c, base0, ndst)
    nobj = masks.shape[0]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    return ops.lib.mvoc_pnp_blend_scatter_tokens_variants_sel(C.byref(d), nsrc, arr, nvar, active, ops._stream())


def _nchw_sel_direct(x, masks, F, base0, ndst, smap, nvar, active):
    from mvoc_amd import ops
    d = ops._pnp_desc(x, None, masks, 0, 0, 0, F, x.shape[2], x.shape[3], x.shape[1], base0, ndst)
    nobj = masks.shape[0]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    return ops.lib.mvoc_pnp_blend_scatter_nchw_variants_sel(C.byref(d), nsrc, arr, nvar, active, ops._stream())


def _check_selected(got, inp, twin, chunk, nsrc, ndst, K, active, what):
    """injecting variants: the chunks of ``twin`` (the _variants entry on a clone); everything else: the input, bit for bit"""
    for k in range(K):
        for d in range(ndst):
            i = nsrc + d * K + k
            if (active >> k) & 1:
                assert tv._same_bits(chunk(got, i), chunk(twin, i)), (what, "injecting", k, d)
            else:
                assert torch.equal(tv._i16(chunk(got, i)), tv._i16(chunk(inp, i))), (what, "not injecting", k, d)
    assert torch.equal(tv._i16(chunk(got, slice(0, nsrc))), tv._i16(chunk(inp, slice(0, nsrc)))), (what, "sources")


@pytest.mark.parametrize("nobj", [1, 2, 3, 4])
@pytest.mark.parametrize("layout", ["spatial", "temporal"])
def test_tokens_sel_writes_the_injecting_variants_only(layout, nobj):
    g = torch.Generator().manual_seed(700 + 20 * nobj + (layout == "temporal"))
    F, H, W, c = 3, 5, 6, 16
    rows = F * H * W
    n = 0
    for K, ndst, base0, (soft, mres), smap in itertools.product(KS, (1, 2), (False, True), ((False, "same"), (True, "other")),
                                                                _two_maps(nobj)):
        mh, mw = (H, W) if mres == "same" else (3, 9)
        masks = tv._masks(nobj, F, mh, mw, soft, g)
        nsrc = nobj + 1 if smap is None else smap[0]
        comp0 = tv._specials(torch.randn((nsrc + ndst * K) * rows, 3 * c, generator=g).half(), g).cuda()
        twin = comp0.clone()
        tv._run_tokens(twin, layout, F, H, W, c, masks, base0, ndst, smap, nvar=K)

        def chunk(t, i):
            return t[i * rows:(i + 1) * rows, :2 * c] if not isinstance(i, slice) else t[i.start * rows:i.stop * rows, :2 * c]

        for active in _actives(K):
            what = (K, ndst, base0, soft, mres, smap, bin(active))
            comp = comp0.clone()
            assert _tokens_sel_direct(comp, layout, F, H, W, c, masks, base0, ndst, smap, K, active) == 0, what
            _check_selected(comp, comp0, twin, chunk, nsrc, ndst, K, active, what)
            assert torch.equal(tv._i16(comp[:, 2 * c:]), tv._i16(comp0[:, 2 * c:])), (what, "v columns")
            n += 1
    assert n == len(KS) * 8 * 2 * 4


@pytest.mark.parametrize("nobj", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", [(4, 6), (3, 5)])  # hw % 8 == 0: 8 pixels per work item / else 1
def test_nchw_sel_writes_the_injecting_variants_only(hw, nobj):
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(900 + nobj + hw[1])
    H, W = hw
    F, Cc = 2, 4
    for K, ndst, base0, (soft, mres), smap in itertools.product(KS, (1, 2), (False, True), ((False, "same"), (True, "other")),
                                                                _two_maps(nobj)):
        mh, mw = (H, W) if mres == "same" else (2 * H, W + 1)
        masks = tv._masks(nobj, F, mh, mw, soft, g)
        nsrc = nobj + 1 if smap is None else smap[0]
        comp0 = tv._specials(torch.randn((nsrc + ndst * K) * F, Cc, H, W, generator=g).half(), g).cuda()
        twin = comp0.clone()
        ops.pnp_blend_nchw(twin, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K)

        def chunk(t, i):
            return t[i * F:(i + 1) * F] if not isinstance(i, slice) else t[i.start * F:i.stop * F]

        for active in _actives(K):
            what = (K, ndst, base0, soft, mres, smap, bin(active))
            comp = comp0.clone()
            assert _nchw_sel_direct(comp, masks, F, base0, ndst, smap, K, active) == 0, what
            _check_selected(comp, comp0, twin, chunk, nsrc, ndst, K, active, what)


def test_ops_routes_a_full_mask_to_the_variants_entries_and_a_partial_one_to_sel():
    from launch_census import Recorder
    from mvoc_amd import ops
    F, H, W, c, K = 2, 4, 4, 8, 3
    rows = F * H * W
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    buf = torch.randn((3 + 2 * K) * rows, 3 * c).half().cuda()
    nchw = torch.randn((3 + 2 * K) * F, c, H, W).half().cuda()
    one = torch.randn(5 * rows, 3 * c).half().cuda()
    one_nchw = torch.randn(5 * F, c, H, W).half().cuda()

    def tokens(b, **kw):
        ld = b.stride(0)
        ops.pnp_blend_tokens(b[:, :c], masks, x2=b[:, c:2 * c], frames=F, height=H, width=W, channels=c, chunk_stride=rows * ld,
                             f_stride=H * W * ld, p_stride=ld, **kw)

    rec = Recorder()
    rec.install()
    try:
        for active in (None, 0b111):
            tokens(buf, nvar=K, active=active)
            ops.pnp_blend_nchw(nchw, masks, frames=F, nvar=K, active=active)
        assert dict(rec.calls) == {"mvoc_pnp_blend_scatter_tokens_variants": 2, "mvoc_pnp_blend_scatter_nchw_variants": 2}
        rec.calls.clear()
        tokens(buf, nvar=K, active=0b101)
        ops.pnp_blend_nchw(nchw, masks, frames=F, nvar=K, active=0b010)
        assert dict(rec.calls) == {"mvoc_pnp_blend_scatter_tokens_variants_sel": 1, "mvoc_pnp_blend_scatter_nchw_variants_sel": 1}
        rec.calls.clear()
        for active in (None, 1):  # one variant: the positional / mapped entries of a call without the argument
            tokens(one, active=active)
            ops.pnp_blend_nchw(one_nchw, masks, frames=F, active=active, src_map=(3, (2, 1)))
        assert dict(rec.calls) == {"mvoc_pnp_blend_scatter_tokens": 2, "mvoc_pnp_blend_scatter_nchw_mapped": 2}
        rec.calls.clear()
        for bad, nvar in ((0, K), (0b1000, K), (2, 1), (0, 1)):
            with pytest.raises(RuntimeError, match="active mask"):
                tokens(buf, nvar=nvar, active=bad)
            with pytest.raises(RuntimeError, match="active mask"):
                ops.pnp_blend_nchw(nchw, masks, frames=F, nvar=nvar, active=bad)
        with pytest.raises(RuntimeError, match="storage ends"):  # the bounds check of the _variants path
            ops.pnp_blend_nchw(nchw, masks, frames=F, nvar=5, active=0b10001)
        with pytest.raises(RuntimeError, match="storage ends"):
            tokens(buf, nvar=5, active=0b10001)
        assert not rec.calls
    finally:
        rec.uninstall()
    torch.cuda.synchronize()


def test_sel_entries_refuse_a_bad_mask():
    from mvoc_amd import ops
    F, H, W, c = 2, 4, 4, 8
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    buf = torch.zeros(21 * F * H * W, 3 * c, dtype=torch.float16, device="cuda")
    nchw = torch.zeros(21 * F, 4, H, W, dtype=torch.float16, device="cuda")
    for nvar, active in ((3, 0), (3, 0b1000), (3, 0b1001), (1, 2), (8, 1 << 8), (9, 1), (0, 1), (2, 0xFFFFFFFF)):
        assert _tokens_sel_direct(buf, "spatial", F, H, W, c, masks, False, 2, None, nvar, active) == -1, (nvar, active)
        assert ops.lib.mvoc_last_error().decode().strip(), (nvar, active)
        assert "pnp variants" in ops.lib.mvoc_last_error().decode()
        assert _nchw_sel_direct(nchw, masks, F, True, 2, None, nvar, active) == -1, (nvar, active)
        assert "pnp variants" in ops.lib.mvoc_last_error().decode()
    assert _tokens_sel_direct(buf, "spatial", F, H, W, c, masks, False, 2, (2, (0, 2)), 2, 1) == -1  # the map is checked as before
    assert "obj_chunk[1] = 2" in ops.lib.mvoc_last_error().decode()
    assert _tokens_sel_direct(buf, "spatial", F, H, W, c, masks, False, 2, None, 8, 0b10000001) == 0  # 3 + 16 chunks of 21
    torch.cuda.synchronize()
    assert not buf.any() and not nchw.any()


def test_profiler_counts_the_injecting_variants_only():
    """distinct sources read (+ one base per injecting variant when the base is c_k) + ndst chunks written per injecting variant"""
    from mvoc_amd import ops
    F, H, W, c, K = 2, 4, 4, 8, 4
    rows = F * H * W
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    chunk_bytes, mask_bytes = 2.0 * rows * c, 2.0 * 2 * F * H * W
    ops.prof_enable(True)
    try:
        for base0, ndst, smap, active, chunks in ((True, 2, None, 0b0101, 3 + 2 * 2), (False, 2, None, 0b0111, 2 + 3 + 2 * 3),
                                                  (True, 1, (2, (1, 1)), 0b1000, 2 + 1), (False, 2, (1, (0, 0)), 0b0010, 1 + 1 + 2),
                                                  (False, 1, None, 0b1001, 2 + 2 + 2)):
            nsrc = 3 if smap is None else smap[0]
            buf = torch.zeros((nsrc + ndst * K) * rows, 3 * c, dtype=torch.float16, device="cuda")
            ops.prof_reset()
            ld = buf.stride(0)
            ops.pnp_blend_tokens(buf[:, :c], masks, x2=buf[:, c:2 * c], frames=F, height=H, width=W, channels=c,
                                 chunk_stride=rows * ld, f_stride=H * W * ld, p_stride=ld, base_chunk0=base0, ndst=ndst, src_map=smap,
                                 nvar=K, active=active)
            torch.cuda.synchronize()
            got = ops.prof_collect()["pnp"]
            assert got["launches"] == 1 and got["work"] == 2 * (chunks * chunk_bytes + mask_bytes), (base0, ndst, smap, active, got)
            nchw = torch.zeros((nsrc + ndst * K) * F, c, H, W, dtype=torch.float16, device="cuda")
            ops.prof_reset()
            ops.pnp_blend_nchw(nchw, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active)
            torch.cuda.synchronize()
            got = ops.prof_collect()["pnp"]
            assert got["launches"] == 1 and got["work"] == chunks * chunk_bytes + mask_bytes, (base0, ndst, smap, active, got)
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


# ---- UNet ------------------------------------------------------------------------------------------------------------
def _attn_sites(eng, temporal):
    from mvoc_amd.pnp_utils import ATTN_SITES
    for res, blocks in ATTN_SITES.items():
        for b in blocks:
            tr = (eng.up_blocks[res].temp_attentions if temporal else eng.up_blocks[res].attentions)[b]
            yield tr.transformer_blocks[0].attn1.processor


def _feature_sites(eng):
    return list(eng.up_blocks[3].resnets) + list(eng.up_blocks[3].temp_convs)


def _clear(eng, pipe):
    tv._disarm(eng, pipe)
    for s in eng.hook_sites():
        s.variant_schedules = None


def _set_uniform(eng, t, spatial, temporal, feature, conv_out):
    """one variant's schedules on every site of a family (the single-variant twin)"""
    for s in eng.hook_sites():
        s.variant_schedules = None
    for p in _attn_sites(eng, False):
        p.injection_schedule = [t] if spatial else None
    for p in _attn_sites(eng, True):
        p.injection_schedule = [t] if temporal else None
    for m in _feature_sites(eng):
        m.injection_schedule = [t] if feature else None
    eng.conv_out.injection_schedule = [t] if conv_out else None


def _set_per_variant(eng, t, K, spatial, temporal, feature, conv_out):
    """families on for the given sets of variants; the shared schedule stays None"""
    _set_uniform(eng, t, False, False, False, False)
    sched = lambda on: [[t] if k in on else [] for k in range(K)]
    for p in _attn_sites(eng, False):
        p.variant_schedules = sched(spatial)
    for p in _attn_sites(eng, True):
        p.variant_schedules = sched(temporal)
    for m in _feature_sites(eng):
        m.variant_schedules = sched(feature)
    eng.conv_out.variant_schedules = sched(conv_out)


def _full_forward(eng, roles, t, K, cfg, pair=True, dead=True, tail=True):
    names = ["S", "O", "P"] + ([f"u{k}" for k in range(K)] if cfg else []) + [f"c{k}" for k in range(K)]
    saved = eng.prune_dead_chunks, eng.pair_destinations
    eng.variants, eng.prune_source_tail, eng.prune_dead_chunks, eng.pair_destinations = K, tail, dead, pair
    try:
        out = tv._fwd(eng, tv._batch(roles, names), t)
    finally:
        eng.variants, eng.prune_source_tail = 1, False
        eng.prune_dead_chunks, eng.pair_destinations = saved
    assert out.shape[0] == len(names)
    return out


def _dest(out, K, cfg, k):
    ndst = 2 if cfg else 1
    return torch.cat([out[3 + d * K + k][None] for d in range(ndst)])


class _FlashSpy:
    """every self-attention call of ops.flash_attn: (first image, images, paired) in units of images of the batch"""

    def __init__(self):
        from mvoc_amd import ops
        self.ops, self.orig, self.calls = ops, ops.flash_attn, []

    def __enter__(self):
        def spy(q, k, v, **kw):
            if "kv_bdiv" not in kw:  # (cross-attention reads the context's K/V)
                hw = kw["tq"]
                row = lambda t: t.storage_offset() // t.stride(0)
                self.calls.append((row(q) // hw, kw["nbatch"], None if kw.get("v2") is None else row(kw["v2"]) // hw))
            return self.orig(q, k, v, **kw)
        self.ops.flash_attn = spy
        return self

    def __exit__(self, *exc):
        self.ops.flash_attn = self.orig

    def sites(self):
        """the calls of one transformer each: a site's first call starts at image 0 (the sources, or the whole batch)"""
        out = []
        for c in self.calls:
            if c[0] == 0:
                out.append([])
            out[-1].append(c)
        return out


@pytest.mark.parametrize("K,cfg", [(3, True), (2, False)], ids=["K3-cfg", "K2-nocfg"])
def test_unet_variants_inject_at_different_families(K, cfg):
    """spatial Q/K on for variants {0, 2}, temporal Q/K for {1}, resnet / temporal-conv features for {0}"""
    from oracle.pnp_model_ref import PnPState, install_pnp
    from mvoc_amd import pnp_utils
    F, h, w, cd = 3, 8, 8, 64
    on = dict(spatial={0, 2} & set(range(K)), temporal={1}, feature={0})
    o, eng = tv._toy_pair()
    cpu_masks, masks = tv._hook_masks(F, h, w)
    roles = tv._roles(F, h, w, cd, 14, K)
    pipe = types.SimpleNamespace(unet=eng)
    t = 981
    st = PnPState()
    install_pnp(o, st)
    del o.conv_out.forward  # this step's feature injection is at the resnets and temporal convs, not at conv_out
    st.masks, st.ndst = cpu_masks, 2 if cfg else 1
    try:
        _set_per_variant(eng, t, K, on["spatial"], on["temporal"], on["feature"], set())
        pnp_utils.register_time_all(pipe, t, masks)
        with _FlashSpy() as spy:
            out = _full_forward(eng, roles, t, K, cfg)
        sites = spy.sites()
        if cfg:
            # the paired attention: an injecting variant's u / c rows by a call with v2, nobody else's
            nimg, split = (3 + 2 * K) * F, [s for s in sites if len(s) > 1]
            assert len(split) == 8 and all(len(s) == 1 and s[0][:2] == (0, nimg) and s[0][2] is None for s in sites if len(s) == 1)
            for s in split:
                paired, plain = [0] * nimg, [0] * nimg
                for i0, n, i2 in s:
                    for i in range(i0, i0 + n):
                        (plain if i2 is None else paired)[i] += 1
                    if i2 is not None:
                        for i in range(i2, i2 + n):
                            paired[i] += 1
                assert all(a + b == 1 for a, b in zip(paired, plain)), s  # every image exactly once
                assert not any(paired[:3 * F])
                for k in range(K):
                    for d in range(2):
                        i = (3 + d * K + k) * F
                        assert paired[i:i + F] == [int(k in on["spatial"])] * F, (k, d, s)
            plain_out = _full_forward(eng, roles, t, K, cfg, pair=False)
            assert torch.equal(tv._i16(plain_out), tv._i16(out))  # pairing decides launches, not values
        else:
            assert all(len(s) == 1 for s in sites)
        twins = []
        for k in range(K):
            _set_uniform(eng, t, k in on["spatial"], k in on["temporal"], k in on["feature"], False)
            twins.append(tv._single_forward(eng, roles, t, "SOP", None, k, cfg, True))
        for k in range(K):
            what = f"families K={K} variant {k} {'cfg' if cfg else 'no cfg'}"
            st.t = t
            st.spatial_schedule = [t] if k in on["spatial"] else None
            st.temporal_schedule = [t] if k in on["temporal"] else None
            st.conv_schedule = [t] if k in on["feature"] else None
            names = ["S", "O", "P"] + ([f"u{k}"] if cfg else []) + [f"c{k}"]
            b = {key: v.float().cpu() for key, v in tv._batch(roles, names).items()}
            ref = o.forward_ext(b["sample"], t, torch.tensor([8] * len(names)), b["il1"], b["il"], b["ie"], b["eh"])[0]
            tv._close_oracle(_dest(out, K, cfg, k), ref[3:], what)
            tv._close(_dest(out, K, cfg, k), twins[k], what)
    finally:
        _clear(eng, pipe)


def test_unet_partial_conv_out_injection_runs_the_full_batch():
    """K = 2, conv_out injects for variant 1 only (spatial and temporal Q/K for both): the full batch runs, variant 1's
    prediction is the blend of the source predictions, variant 0's its own"""
    from oracle.pnp_model_ref import PnPState, install_pnp
    from mvoc_amd import ops, pnp_utils
    F, h, w, cd, K = 3, 8, 8, 64, 2
    o, eng = tv._toy_pair()
    cpu_masks, masks = tv._hook_masks(F, h, w)
    roles = tv._roles(F, h, w, cd, 15, K)
    pipe = types.SimpleNamespace(unet=eng)
    t = 981
    st = PnPState(spatial_schedule=[t], temporal_schedule=[t])
    install_pnp(o, st)
    st.masks, st.t = cpu_masks, t
    calls = []
    orig = eng._forward_source_chunks
    eng._forward_source_chunks = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    try:
        _set_uniform(eng, t, True, True, False, False)
        eng.conv_out.variant_schedules = [[], [t]]
        pnp_utils.register_time_all(pipe, t, masks)
        assert eng.conv_out.injecting() and eng.conv_out.injecting_mask(2) == 0b10
        out = _full_forward(eng, roles, t, K, True)
        assert not calls
        # variant 1: the conv_out blend of the source predictions, bit for bit (the _variants entry on the same rows)
        B, Cc = out.shape[0], out.shape[1]
        nchw = out.permute(0, 2, 1, 3, 4).reshape(B * F, Cc, h, w).contiguous()
        ops.pnp_blend_nchw(nchw, eng.device_masks(masks)[1], frames=F, base_chunk0=True, ndst=2, nvar=K)
        blend = nchw.reshape(B, F, Cc, h, w).permute(0, 2, 1, 3, 4)
        for i in (3 + 1, 3 + K + 1):
            assert torch.equal(tv._i16(out[i]), tv._i16(blend[i])), i
        for i in (3, 3 + K):  # variant 0 keeps its own prediction
            assert not torch.equal(out[i], blend[i])
        assert torch.equal(out[3 + 1], out[3 + K + 1])
        for k in range(K):
            what = f"partial conv_out K=2 variant {k}"
            st.conv_schedule = [t] if k == 1 else None
            names = ["S", "O", "P", f"u{k}", f"c{k}"]
            b = {key: v.float().cpu() for key, v in tv._batch(roles, names).items()}
            ref = o.forward_ext(b["sample"], t, torch.tensor([8] * 5), b["il1"], b["il"], b["ie"], b["eh"])[0]
            tv._close_oracle(_dest(out, K, True, k), ref[3:], what)
            _set_uniform(eng, t, True, True, False, k == 1)
            del calls[:]
            twin = tv._single_forward(eng, roles, t, "SOP", None, k, True, True)
            assert len(calls) == (1 if k == 1 else 0)
            tv._close(_dest(out, K, True, k), twin, what)
        # both variants inject at conv_out: the source chunks only
        _set_uniform(eng, t, True, True, False, False)
        eng.conv_out.variant_schedules = [[t], [t]]
        del calls[:]
        both = _full_forward(eng, roles, t, K, True)
        assert len(calls) == 1
        assert torch.equal(both[3], both[3 + 1]) and torch.equal(both[3], both[3 + K])
        # a list of the wrong length raises at the site and names it
        eng.conv_out.variant_schedules = [[t], [t], []]
        with pytest.raises(RuntimeError, match="conv_out.*3 schedules.*2 variants"):
            _full_forward(eng, roles, t, K, True)
    finally:
        eng._forward_source_chunks = orig
        _clear(eng, pipe)


# ---- loop ------------------------------------------------------------------------------------------------------------
GUIDANCE = (9.0, 6.0, 7.5)
SPATIAL_STEPS, FEATURE_STEPS, TEMPORAL_STEPS = (5, 2, 0), (1, 0, 1), 4  # of five steps, per variant


def _schedules_job(graphs, mode="own", oracle=False, count_calls=False):
    """test_variants_gpu.py's composition job (three distinct sources, toy engine, five steps) with K = 3 variants;
    ``mode``: "own" = every variant its own spatial / feature schedule, "equal" = per-variant schedules that all equal the
    shared ones, "none" = no per-variant schedules, "short" = a list of two schedules for the three variants."""
    from launch_census import Recorder
    from oracle import loops_ref, sched_ref
    from oracle.pnp_model_ref import PnPState, install_pnp
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    K = 3
    o, eng = tv._toy_pair()
    g = torch.Generator().manual_seed(25)
    f, h, w, cd, n = 3, 8, 8, 64, 5
    nrow = 3 + 2 * K  # rows: bg, obj_1, obj_2, then (u_k, c_k) per variant
    cond = dict(encoder_hidden_states=torch.randn(nrow, 7, cd, generator=g).half(), image_embeddings=torch.randn(nrow, f, cd, generator=g).half(),
                image_latents_first=torch.randn(nrow, 4, f, h, w, generator=g).half(), image_latents=torch.randn(nrow, 4, f, h, w, generator=g).half())
    cond["encoder_hidden_states"][1] = cond["encoder_hidden_states"][0]  # (the inversion prompt is one for all sources)
    cond["encoder_hidden_states"][2] = cond["encoder_hidden_states"][0]
    for k in range(K):
        u, c = 3 + 2 * k, 4 + 2 * k
        cond["image_embeddings"][u] = 0
        cond["image_latents_first"][u] = cond["image_latents_first"][c]
        cond["image_latents"][c] = cond["image_latents_first"][c]
        cond["image_latents"][u] = cond["image_latents"][c]
    cpu_masks, _ = tv._hook_masks(f, h, w)
    s = DDIMScheduler()
    s.set_timesteps(n)
    dirs = ["/virtual/bg", "/virtual/o1", "/virtual/o2"]
    src = {d: {int(t): torch.randn(1, 4, f, h, w, generator=g).half() for t in s.timesteps} for d in dirs}
    x0 = torch.randn(K, 4, f, h, w, generator=g).half()
    kw = dict(ddim_init_latents_t_idx=0, fusion_steps=(0, 2), random_noise_ratio=0.3, obj_random_noise_fusion=True)
    refs = []
    if oracle:
        rs = sched_ref.DDIMSchedulerRef()
        rs.set_timesteps(n)
        st = PnPState()
        install_pnp(o, st)
        st.masks = cpu_masks
        for k in range(K):
            st.conv_schedule, st.spatial_schedule = rs.timesteps[:FEATURE_STEPS[k]], rs.timesteps[:SPATIAL_STEPS[k]]
            st.temporal_schedule = rs.timesteps[:TEMPORAL_STEPS]
            rows = [0, 1, 2, 3 + 2 * k, 4 + 2 * k]

            def unet_fn(inp, t, rows=rows):
                st.t = int(t)
                return o.forward_ext(inp.float(), int(t), torch.tensor([8] * 5), cond["image_latents_first"][rows].float(),
                                     cond["image_latents"][rows].float(), cond["image_embeddings"][rows].float(),
                                     cond["encoder_hidden_states"][rows].float())[0].half()

            refs.append(loops_ref.composition_loop(unet_fn, sched_ref.DDIMSchedulerRef(), x0[k:k + 1], lambda t: src[dirs[0]][t],
                                                   lambda j, t: src[dirs[1 + j]][t], [m[0] for m in cpu_masks], n,
                                                   guidance_scale=GUIDANCE[k], **kw))
    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=graphs)
    ts = s.timesteps
    # the shared schedules: variant 0's
    pnp_utils.register_temp_attention_pnp(pipe, ts[:TEMPORAL_STEPS], False)
    pnp_utils.register_spatial_attention_pnp(pipe, ts[:SPATIAL_STEPS[0]], False)
    pnp_utils.register_temp_conv_injection(pipe, ts[:FEATURE_STEPS[0]])
    pnp_utils.register_out_conv_injection(pipe, ts[:FEATURE_STEPS[0]])
    pnp_utils.register_resnet_injection(pipe, ts[:FEATURE_STEPS[0]])
    if mode == "own":
        pnp_utils.register_variant_schedules(pipe, conv=[ts[:m] for m in FEATURE_STEPS], spatial=[None] + [ts[:m] for m in SPATIAL_STEPS[1:]])
    elif mode == "short":
        pnp_utils.register_variant_schedules(pipe, spatial=[ts[:2], None])
    elif mode == "equal":
        pnp_utils.register_variant_schedules(pipe, conv=[ts[:FEATURE_STEPS[0]]] * K, spatial=[ts[:SPATIAL_STEPS[0]], None, None],
                                             temporal=[None] * K)
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
    batches, states, step_masks, step_calls = [], [], [], []
    emb = eng._embeddings

    def recording(timestep, fps, B):  # once per run of the network, with the batch it really runs
        batches.append(B)
        return emb(timestep, fps, B)

    eng._embeddings = recording
    make, step = pipe.make_composition_state, pipe.composition_step

    def make_state(*a, **k):
        states.append(make(*a, **k))
        return states[-1]

    rec = Recorder() if count_calls else None

    def one_step(*a, **k):
        if rec is not None:
            rec.calls.clear()
        step(*a, **k)
        step_masks.append(eng.injection_masks(K))
        if rec is not None:
            step_calls.append(dict(rec.calls))

    pipe.make_composition_state, pipe.composition_step = make_state, one_step
    clips = [[(r, i, False) for i in range(f)] for r in range(3)]
    var = dict(prompt=[f"edit{k}" for k in range(K)], main_first_image=[(4 + 2 * k, 0, True) for k in range(K)],
               main_image_list=[[(4 + 2 * k, i, False) for i in range(f)] for k in range(K)], latents=x0.cuda(),
               guidance_scale=list(GUIDANCE), negative_prompt=["neg"] * K)
    if rec is not None:
        rec.install()
    try:
        out = pipe.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection(
            background_first_image=(0, 0, True), background_image_list=clips[0], objs_first_image=[(1, 0, True), (2, 0, True)],
            objs_image_list=[clips[1], clips[2]], height=h * 8, width=w * 8, num_frames=f, num_inference_steps=n,
            target_fps=8, output_type="latent", ddim_inv_prompt="", bg_inv_latents_path=dirs[0], obj_ddim_latents_path=dirs[1:],
            obj_ddim_latents_idx_offset=[0, 0], obj_masks_tensors=[(a.clone(), b.clone()) for a, b in cpu_masks], **var, **kw).frames
    finally:
        if rec is not None:
            rec.uninstall()
        eng._embeddings = emb
    torch.cuda.synchronize()
    return types.SimpleNamespace(out=out, refs=refs, batches=batches, graphs=len(states[0]["variants"]), step_masks=step_masks,
                                 step_calls=step_calls, pipe=pipe)


def test_three_threshold_sets_in_one_loop_vs_oracle_and_graph_replay():
    """spatial injection stops after 5 / 2 / 0 steps, feature injection after 1 / 0 / 1 steps: step 0 injects at conv_out for
    variants 0 and 2 only, so the full batch of 3 + 2 * 3 chunks runs at every step"""
    eager = _schedules_job(False, oracle=True, count_calls=True)
    assert eager.out.shape[0] == 3 and eager.batches == [9] * 5, eager.batches
    for k, ref in enumerate(eager.refs):
        d = (eager.out[k:k + 1].cpu().float() - ref.float()).abs().max()
        print(f"variant {k} (spatial {SPATIAL_STEPS[k]} steps, features {FEATURE_STEPS[k]}) vs the oracle's loop for that variant alone: "
              f"max-abs {float(d):.2e}")
        assert d < 3e-2, (k, float(d))
    # steps 0 / 1 / 2 = 3 / 4 differ in some site's mask: four distinct tuples
    assert len(set(eager.step_masks)) == 4 and eager.step_masks[2] == eager.step_masks[3], eager.step_masks
    assert set(eager.step_masks[0]) == {0, 0b101, 0b011, 0b111}  # features {0, 2}; spatial Q/K {0, 1}; temporal Q/K all
    assert set(eager.step_masks[1]) == {0, 0b011, 0b111} and set(eager.step_masks[2]) == {0, 0b001, 0b111}
    assert set(eager.step_masks[4]) == {0, 0b001}
    assert eager.graphs == 0
    assert any(name.endswith("_sel") for name in eager.step_calls[1]) and sum(eager.step_calls[1].values()) > 100
    graphed = _schedules_job(True)
    assert torch.equal(graphed.out, eager.out)
    assert graphed.step_masks == eager.step_masks
    assert graphed.graphs == len(set(eager.step_masks)) == 4


def test_equal_thresholds_make_the_calls_and_graphs_of_a_call_without_them():
    plain, equal = _schedules_job(False, "none", count_calls=True), _schedules_job(False, "equal", count_calls=True)
    assert len(plain.step_calls) == len(equal.step_calls) == 5
    for i, (a, b) in enumerate(zip(plain.step_calls, equal.step_calls)):
        assert a == b and sum(a.values()) > 0, (i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
        assert not any(name.endswith("_sel") for name in b)
    assert plain.batches == equal.batches == [3, 9, 9, 9, 9]  # conv_out injects for every variant at step 0: sources only
    assert torch.equal(plain.out, equal.out)
    # (shared schedules: features 1 step, spatial Q/K 5, temporal Q/K 4 -- steps 0 / 1..3 / 4 are three kinds)
    gp, ge = _schedules_job(True, "none"), _schedules_job(True, "equal")
    assert gp.graphs == ge.graphs == 3 and torch.equal(gp.out, ge.out) and torch.equal(gp.out, plain.out)


def test_a_schedule_list_of_the_wrong_length_is_refused_by_the_call():
    with pytest.raises(RuntimeError, match=r"up_blocks\.1\.attentions\.1.*2 schedules.*3 variants"):
        _schedules_job(False, "short")


# ---- composite.py ---------------------------------------------------------------------------------------------------------
def test_composite_py_writes_each_variant_under_its_own_thresholds():
    """inverse.py x 3 + composite.py on a two-variant entry whose variants differ in pnp_spatial_attn_t (tools/demo_job.py
    --variants 2 --variant-thresholds 1.0,0.4), tiny sizes"""
    import importlib.util
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("demo_job_variant_schedules", os.path.join(repo, "tools", "demo_job.py"))
    dj = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dj)
    saved_path, saved_env = list(sys.path), {k: os.environ.get(k) for k in ("MVOC_SYNTHETIC_VAE", "MVOC_SYNTHETIC_CLIP")}
    try:
        res = dj.run_variants(frames=4, size=64, steps=5, keep=False, variants=2, thresholds=[1.0, 0.4])
    finally:
        sys.path[:] = saved_path
        for k, v in saved_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        for m in ("utils", "pnp_utils", "inverse", "composite", "pipelines", "pipelines.pipeline_i2vgen_xl"):
            sys.modules.pop(m, None)
    assert res["output_dirs"] == ["variant_00", "variant_01"]
    assert res["n_result_files"] == {"variant_00": 5, "variant_01": 5}  # video.gif + one png per frame
    sfx = res["output_suffix_of"]
    assert "_pnps1.0_" in sfx["variant_00"] and "_pnps0.4_" in sfx["variant_01"] and sfx["variant_00"] != sfx["variant_01"]
    # steps by the number of variants that still inject spatial Q/K: int(5 * 0.4) = 2 steps with both, then variant 0 alone
    # (the first step of a kind warms up and is not timed; the entry's pnp_f_t gives int(5 * 0.1) = 0 feature steps)
    assert res["steps_timed"] == {"qk_spatial_1of2": 2, "qk_spatial_2of2": 1}, res["steps_timed"]
