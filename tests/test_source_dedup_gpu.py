"""GPU: source de-duplication of the composition batch (pipeline.dedup_sources).

* kernels: the mapped blend entry points on the compact batch [s_0..s_{nsrc-1}, destinations] write destination chunks
  BIT-IDENTICAL (int16 views: NaN payloads count) to the unmapped entry on the sources expanded back to nobj + 1 chunks, and
  leave the source chunks untouched; invalid maps are refused;
* UNet: forward_ext on the compact batch under ``source_chunks`` against the positional batch, within the
  batch-independence bar of test_fullsize_gpu.py (the compact batch runs at another row count, i.e. on other tiles);
* loop: the de-duplicated composition loop against the oracle's five-chunk loop, the UNet batch per step, graph replay
  against eager, one conditioner call per distinct image.
"""
import itertools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _specials(x, g):
    """sprinkle -0.0, +-inf and NaN into an fp16 tensor"""
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
    out = [(1, (0,) * nobj)]
    if nobj >= 2:
        out += [(2, (1, 0) + (1,) * (nobj - 2)), (2, (0, 1) + (0,) * (nobj - 2)), (2, (1,) * nobj)]
    if nobj >= 3:
        out += [(3, tuple(1 + j % 2 for j in range(nobj)))]
    return out


def _order(smap, ndst):
    """compact chunk of each chunk of the expanded batch [bg, obj_1..obj_n, destinations]"""
    nsrc, chunks = smap
    return [0] + list(chunks) + [nsrc + i for i in range(ndst)]


def _i16(t):
    return t.contiguous().view(torch.int16)


def _run_tokens(buf, nchunk, layout, F, H, W, c, masks, base0, ndst, smap):
    """buf: [nchunk * F * H * W, 3c] qkv rows of one batch; q = columns [0, c), k = [c, 2c)"""
    from mvoc_amd import ops
    ld, hw = buf.stride(0), H * W
    if layout == "spatial":  # [chunk, f, p]
        fs, ps = hw * ld, ld
    else:  # temporal [chunk, p, f]
        fs, ps = ld, F * ld
    ops.pnp_blend_tokens(buf[:, :c], masks, x2=buf[:, c:2 * c], frames=F, height=H, width=W, channels=c,
                         chunk_stride=F * hw * ld, f_stride=fs, p_stride=ps, base_chunk0=base0, ndst=ndst, src_map=smap)


@pytest.mark.parametrize("nobj", [1, 2, 3, 4])
@pytest.mark.parametrize("layout", ["spatial", "temporal"])
def test_tokens_mapped_equals_unmapped_on_the_expanded_batch(layout, nobj):
    g = torch.Generator().manual_seed(10 * nobj + (layout == "temporal"))
    F, H, W, c = 3, 5, 6, 16
    n = 0
    for ndst, base0, soft, mres, smap in itertools.product((1, 2), (False, True), (False, True), ("same", "other"), _maps(nobj)):
        mh, mw = (H, W) if mres == "same" else (3, 9)
        masks = _masks(nobj, F, mh, mw, soft, g)
        nsrc = smap[0]
        rows = F * H * W
        comp = _specials(torch.randn((nsrc + ndst) * rows, 3 * c, generator=g).half(), g).cuda()
        order = _order(smap, ndst)
        full = torch.cat([comp[k * rows:(k + 1) * rows] for k in order]).contiguous()
        comp0 = comp.clone()
        _run_tokens(comp, nsrc + ndst, layout, F, H, W, c, masks, base0, ndst, smap)
        _run_tokens(full, nobj + 1 + ndst, layout, F, H, W, c, masks, base0, ndst, None)
        torch.cuda.synchronize()
        what = (ndst, base0, soft, mres, smap)
        assert torch.equal(_i16(comp[:nsrc * rows]), _i16(comp0[:nsrc * rows])), what  # sources untouched
        assert torch.equal(_i16(comp[:, 2 * c:]), _i16(comp0[:, 2 * c:])), what  # v columns untouched
        assert torch.equal(_i16(comp[nsrc * rows:]), _i16(full[(nobj + 1) * rows:])), what
        n += 1
    assert n == 16 * len(_maps(nobj))


@pytest.mark.parametrize("nobj", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", [(4, 6), (3, 5)])  # VEC 8 / VEC 1
def test_nchw_mapped_equals_unmapped_on_the_expanded_batch(hw, nobj):
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(100 + nobj + hw[1])
    H, W = hw
    F, C = 2, 4
    for ndst, base0, soft, mres, smap in itertools.product((1, 2), (False, True), (False, True), ("same", "other"), _maps(nobj)):
        mh, mw = (H, W) if mres == "same" else (2 * H, W + 1)
        masks = _masks(nobj, F, mh, mw, soft, g)
        nsrc = smap[0]
        comp = _specials(torch.randn((nsrc + ndst) * F, C, H, W, generator=g).half(), g).cuda()
        order = _order(smap, ndst)
        full = torch.cat([comp[k * F:(k + 1) * F] for k in order]).contiguous()
        comp0 = comp.clone()
        ops.pnp_blend_nchw(comp, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap)
        ops.pnp_blend_nchw(full, masks, frames=F, base_chunk0=base0, ndst=ndst)
        torch.cuda.synchronize()
        what = (ndst, base0, soft, mres, smap)
        assert torch.equal(_i16(comp[:nsrc * F]), _i16(comp0[:nsrc * F])), what
        assert torch.equal(_i16(comp[nsrc * F:]), _i16(full[(nobj + 1) * F:])), what


@pytest.mark.parametrize("nobj", [1, 2, 4])
def test_identity_map_equals_the_unmapped_entry(nobj):
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(7)
    F, H, W, c = 2, 4, 4, 8
    ident = (nobj + 1, tuple(range(1, nobj + 1)))
    for ndst, base0 in itertools.product((1, 2), (False, True)):
        masks = _masks(nobj, F, H, W, True, g)
        a = _specials(torch.randn((nobj + 1 + ndst) * F * H * W, 3 * c, generator=g).half(), g).cuda()
        b = a.clone()
        _run_tokens(a, nobj + 1 + ndst, "spatial", F, H, W, c, masks, base0, ndst, ident)
        _run_tokens(b, nobj + 1 + ndst, "spatial", F, H, W, c, masks, base0, ndst, None)
        assert torch.equal(_i16(a), _i16(b)), (ndst, base0)
        x = _specials(torch.randn((nobj + 1 + ndst) * F, 4, H, W, generator=g).half(), g).cuda()
        y = x.clone()
        ops.pnp_blend_nchw(x, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=ident)
        ops.pnp_blend_nchw(y, masks, frames=F, base_chunk0=base0, ndst=ndst)
        assert torch.equal(_i16(x), _i16(y)), (ndst, base0)


def test_invalid_maps_are_refused():
    from mvoc_amd import ops
    F, H, W, c = 2, 4, 4, 8
    masks = _masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    buf = torch.zeros(5 * F * H * W, 3 * c, dtype=torch.float16, device="cuda")
    nchw = torch.zeros(5 * F, 4, H, W, dtype=torch.float16, device="cuda")
    for smap, msg in (((0, (0, 0)), "nsrc 0"), ((4, (0, 0)), "nsrc 4"), ((2, (0, 2)), r"obj_chunk\[1\] = 2"),
                      ((2, (-1, 0)), r"obj_chunk\[0\] = -1")):
        with pytest.raises(RuntimeError, match=msg):
            _run_tokens(buf, 5, "spatial", F, H, W, c, masks, False, 2, smap)
        with pytest.raises(RuntimeError, match=msg):
            ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, src_map=smap)
    with pytest.raises(RuntimeError, match="names 3 objects"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, src_map=(1, (0, 0, 0)))
    torch.cuda.synchronize()
    assert not buf.any() and not nchw.any()


# ---- UNet ------------------------------------------------------------------------------------------------------------
def _toy():
    from oracle import unet_ref as U
    from mvoc_amd.unet import I2VGenXLUNet
    o = U.I2VGenXLUNet(U.UNetConfig.small4())
    U.init_weights_(o, seed=9)
    for p in o.parameters():
        p.copy_(p.half().float())
    return I2VGenXLUNet(o.config.to_dict()).load_state_dict(o.state_dict())


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


def _roles(F, h, w, cd, seed):
    """per-role rows: 'S' the shared source, 'O' a second source, 'u' / 'c' the destinations (equal latents / image latents)"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).half().cuda()
    r = {k: dict(sample=mk(1, 4, F, h, w), il1=mk(1, 4, F, h, w) * 0.18, il=mk(1, 4, F, h, w) * 0.18, ie=mk(1, F, cd), eh=mk(1, 7 if cd == 64 else 77, cd))
         for k in ("S", "O", "u")}
    r["c"] = dict(r["u"], ie=mk(1, F, cd), eh=mk(1, 7 if cd == 64 else 77, cd))
    return r


def _batch(roles, names):
    b = {k: torch.cat([roles[n][k] for n in names]).contiguous() for k in roles["S"]}
    b["fps"] = torch.full((len(names),), 8.0, device="cuda")
    return b


def _fwd(eng, x, t):
    return eng.forward_ext(x["sample"], torch.tensor([float(t)]).cuda(), x["fps"], x["il1"], x["il"], x["ie"], x["eh"])[0]


def _close(a, b, what):
    d = (a.float() - b.float()).abs().max() / b.float().abs().max()
    rel = (a.float() - b.float()).norm() / b.float().norm()
    print(f"{what}: destination chunks max-abs/max {float(d):.2e}, rel-L2 {float(rel):.2e}"
          f"{' (bit-identical)' if torch.equal(a, b) else ''}")
    assert torch.isfinite(a).all() and d < 8e-3 and rel < 5e-3, (what, float(d), float(rel))


def _compare(eng, pipe, masks, roles, t, compact, smap, full, ndst, what, tail_prefix=False):
    from mvoc_amd import pnp_utils
    pnp_utils.register_time_all(pipe, t, masks)
    ref = _fwd(eng, _batch(roles, full), t)
    eng.source_chunks = smap
    if tail_prefix:
        eng.prune_source_tail, eng.shared_prefix_chunks = True, 2
    try:
        out = _fwd(eng, _batch(roles, compact), t)
    finally:
        eng.source_chunks = None
        eng.prune_source_tail, eng.shared_prefix_chunks = False, 0
    assert out.shape[0] == len(compact)
    _close(out[-ndst:], ref[-ndst:], what)


def _unet_cases(eng, F, h, w, cd, steps, cases):
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (2, F, h, w), generator=g)
    masks = [((u8[j].float() / 255).half()[None, None].repeat(1, 4, 1, 1, 1).cuda(), (u8[j] > 10)[None, None].repeat(1, 4, 1, 1, 1).cuda())
             for j in range(2)]
    roles = _roles(F, h, w, cd, 4)
    pipe, (t_feat, t_qk) = _arm(eng, steps)
    try:
        for kind, compact, smap, full, ndst, tp in cases:
            _compare(eng, pipe, masks, roles, t_feat if kind == "feature" else t_qk, compact, smap, full, ndst,
                     f"{kind} step {smap} {''.join(compact)}", tp)
    finally:
        _disarm(eng, pipe)


TOY_CASES = [
    # feature injection (all five hook families): _forward_source_chunks with ONE source chunk
    ("feature", "Suc", (1, (0, 0)), "SSSuc", 2, False),
    # Q/K only, with prune_source_tail and the shared CFG prefix
    ("qk", "Suc", (1, (0, 0)), "SSSuc", 2, True),
    ("qk", "Suc", (1, (0, 0)), "SSSuc", 2, False),
    # guidance off: [S, c]
    ("feature", "Sc", (1, (0, 0)), "SSSc", 1, False),
    ("qk", "Sc", (1, (0, 0)), "SSSc", 1, False),
    # partial maps (an offset fusion step): two source chunks
    ("feature", "SOuc", (2, (1, 1)), "SOOuc", 2, False),
    ("qk", "SOuc", (2, (1, 1)), "SOOuc", 2, True),
    ("feature", "SOuc", (2, (1, 0)), "SOSuc", 2, False),
    ("qk", "SOuc", (2, (0, 1)), "SSOuc", 2, False),
]


def test_unet_compact_batch_matches_the_positional_batch():
    eng = _toy()
    _unet_cases(eng, 3, 8, 8, 64, 5, TOY_CASES)


def test_unet_source_chunks_refuses_a_wrong_batch():
    from mvoc_amd import pnp_utils
    eng = _toy()
    roles = _roles(3, 8, 8, 64, 1)
    masks = [(torch.ones(1, 4, 3, 8, 8).half().cuda(), torch.ones(1, 4, 3, 8, 8, dtype=torch.bool).cuda())] * 2
    pipe, (t_feat, t_qk) = _arm(eng, 5)
    try:
        pnp_utils.register_time_all(pipe, t_qk, masks)
        eng.source_chunks = (1, (0, 0))
        with pytest.raises(RuntimeError, match="de-duplicated source"):
            _fwd(eng, _batch(roles, "SSSuc"), t_qk)
    finally:
        eng.source_chunks = None
        _disarm(eng, pipe)


def test_unet_compact_batch_full_size():
    """one of each step kind on the full-size network at 16 x 64 x 64"""
    from mvoc_amd.unet import I2VGenXLUNet
    eng = I2VGenXLUNet(device="cuda:0").init_random(8888)
    _unet_cases(eng, 16, 64, 64, 1024, 50, [("feature", "Suc", (1, (0, 0)), "SSSuc", 2, False),
                                           ("qk", "Suc", (1, (0, 0)), "SSSuc", 2, True)])


# ---- loop ------------------------------------------------------------------------------------------------------------
def _shared_job(graphs, dedup, ddim_init_latents_t_idx=1, fusion_steps=(0, 2)):
    """test_composition_vs_oracle's job with ONE source behind every role: the oracle's five-chunk loop, the HIP pipeline,
    the UNet batch of every forward_ext and the conditioner's calls per image"""
    from oracle import loops_ref, sched_ref
    from oracle import unet_ref as U
    from oracle.pnp_model_ref import PnPState, install_pnp
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    from mvoc_amd.unet import I2VGenXLUNet
    o = U.I2VGenXLUNet(U.UNetConfig.small4())
    U.init_weights_(o, seed=9)
    for p in o.parameters():
        p.copy_(p.half().float())
    eng = I2VGenXLUNet(o.config.to_dict()).load_state_dict(o.state_dict())
    g = torch.Generator().manual_seed(5)
    f, h, w, cd, n = 3, 8, 8, 64, 5
    cond = dict(encoder_hidden_states=torch.randn(5, 7, cd, generator=g).half(), image_embeddings=torch.randn(5, f, cd, generator=g).half(),
                image_latents_first=torch.randn(5, 4, f, h, w, generator=g).half(), image_latents=torch.randn(5, 4, f, h, w, generator=g).half())
    for k in cond:  # every role shows the background's conditioning
        cond[k][1] = cond[k][0]
        cond[k][2] = cond[k][0]
    cond["image_embeddings"][3] = 0
    cond["image_latents_first"][3] = cond["image_latents_first"][4]
    cond["image_latents"][4] = cond["image_latents_first"][4]
    cond["image_latents"][3] = cond["image_latents"][4]
    u8 = torch.randint(0, 256, (2, f, h, w), generator=g)
    masks = [((u8[j].float() / 255).half()[None, None].repeat(1, 4, 1, 1, 1), (u8[j] > 10)[None, None].repeat(1, 4, 1, 1, 1)) for j in range(2)]
    s = DDIMScheduler()
    s.set_timesteps(n)
    src = {int(t): torch.randn(1, 4, f, h, w, generator=g).half() for t in s.timesteps}
    x0 = torch.randn(1, 4, f, h, w, generator=g).half()
    rs = sched_ref.DDIMSchedulerRef()
    rs.set_timesteps(n)
    st = PnPState(conv_schedule=rs.timesteps[:1], spatial_schedule=rs.timesteps[:3], temporal_schedule=rs.timesteps[:4])
    install_pnp(o, st)
    st.masks = masks

    def unet_fn(inp, t):
        st.t = int(t)
        return o.forward_ext(inp.float(), int(t), torch.tensor([8] * 5), cond["image_latents_first"].float(), cond["image_latents"].float(),
                             cond["image_embeddings"].float(), cond["encoder_hidden_states"].float())[0].half()

    kw = dict(guidance_scale=9.0, ddim_init_latents_t_idx=ddim_init_latents_t_idx, fusion_steps=fusion_steps, random_noise_ratio=0.3,
              obj_random_noise_fusion=True)
    ref = loops_ref.composition_loop(unet_fn, sched_ref.DDIMSchedulerRef(), x0, lambda t: src[t], lambda j, t: src[t],
                                     [m[0] for m in masks], n, **kw)
    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=graphs)
    pipe.dedup_sources = dedup
    pnp_utils.register_temp_attention_pnp(pipe, s.timesteps[:4], False)
    pnp_utils.register_spatial_attention_pnp(pipe, s.timesteps[:3], False)
    pnp_utils.register_temp_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_out_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_resnet_injection(pipe, s.timesteps[:1])
    pipe.latent_cache.write_files = False
    for t, v in src.items():
        pipe.latent_cache.put("/virtual/shared", t, v.cuda())
    calls = {}

    class Cond:  # the reference's assembly order; counts its calls per image
        def encode_prompt(self, prompt, negative_prompt=None):
            if prompt == "edit":
                return cond["encoder_hidden_states"][4:5].cuda(), cond["encoder_hidden_states"][3:4].cuda()
            return cond["encoder_hidden_states"][0:1].cuda(), None

        def image_latents(self, image, num_frames, height, width):
            calls[("l", image)] = calls.get(("l", image), 0) + 1
            idx, fr, first = image
            return cond["image_latents_first" if first else "image_latents"][idx:idx + 1].cuda()

        def encode_image(self, image):
            calls[("e", image)] = calls.get(("e", image), 0) + 1
            idx, fr, first = image
            return cond["image_embeddings"][idx:idx + 1, fr:fr + 1].cuda()

    pipe.conditioner = Cond()
    batches = []
    fwd = eng.forward_ext

    def recording(sample, *a, **k):
        batches.append(sample.shape[0])
        return fwd(sample, *a, **k)

    eng.forward_ext = recording
    clip = [(0, k, False) for k in range(f)]
    out = pipe.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection(
        prompt="edit", main_first_image=(4, 0, True), main_image_list=[(4, k, False) for k in range(f)],
        background_first_image=(0, 0, True), background_image_list=clip, objs_first_image=[(0, 0, True), (0, 0, True)],
        objs_image_list=[clip, clip], height=h * 8, width=w * 8, num_frames=f, num_inference_steps=n, guidance_scale=9.0,
        negative_prompt="neg", target_fps=8, latents=x0.cuda(), output_type="latent", ddim_init_latents_t_idx=ddim_init_latents_t_idx,
        ddim_inv_prompt="", fusion_steps=fusion_steps, random_noise_ratio=0.3, obj_random_noise_fusion=True,
        bg_inv_latents_path="/virtual/shared", obj_ddim_latents_path=["/virtual/shared", "/virtual/shared"],
        obj_ddim_latents_idx_offset=[0, 0], obj_masks_tensors=masks).frames
    return types.SimpleNamespace(out=out, ref=ref, batches=batches, calls=calls, pipe=pipe)


@pytest.mark.parametrize("graphs", [False, True])
def test_dedup_composition_vs_oracle(graphs):
    job = _shared_job(graphs, True)
    d = (job.out.cpu().float() - job.ref.float()).abs().max()
    print(f"de-duplicated composition after 4 steps vs the oracle's five-chunk loop: max-abs {float(d):.2e}")
    assert d < 3e-2, float(d)
    if not graphs:
        # fusion steps 0 and 1 feed the objects latents of another t than the background (a partial map), steps 2 and 3 one source
        assert job.batches == [4, 4, 3, 3], job.batches
    else:  # (forward_ext runs only while a variant is warmed up and captured: two variants, B = 4 and B = 3)
        assert set(job.batches) == {3, 4}, job.batches
    # the conditioner saw every distinct image once
    assert job.calls and all(v == 1 for v in job.calls.values()), job.calls
    assert set(job.calls) == ({("l", (4, 0, True)), ("l", (0, 0, True)), ("l", (0, 0, False))} |
                              {("e", (i, k, False)) for i in (0, 4) for k in range(3)})


def test_dedup_graph_replay_equals_eager_and_one_source_per_step():
    eager = _shared_job(False, True, ddim_init_latents_t_idx=0, fusion_steps=(0, 1))
    graphed = _shared_job(True, True, ddim_init_latents_t_idx=0, fusion_steps=(0, 1))
    assert eager.batches == [3, 3, 3, 3, 3], eager.batches  # fusion objects at the background's t: one source on every step
    d = (eager.out.cpu().float() - eager.ref.float()).abs().max()
    assert d < 3e-2, float(d)
    assert torch.equal(graphed.out, eager.out)


def test_dedup_off_keeps_the_positional_batch():
    job = _shared_job(False, False)
    assert job.batches == [5, 5, 5, 5], job.batches
    assert any(v > 1 for v in job.calls.values())  # one conditioner call per role, as the reference's assembly
    d = (job.out.cpu().float() - job.ref.float()).abs().max()
    assert d < 3e-2, float(d)
