"""CPU: per-variant injection schedules in the K-variant composition loop -- the hook state
(``variant_schedules`` / ``injecting_mask``), its registration sites, the run cutting of the paired attention as a pure function,
the new entry points' declarations, and composite.py's ``pnp`` variant key.  No kernel is launched."""
import ctypes as C
import importlib
import os
import re
import sys
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_engine():
    from mvoc_amd.unet import I2VGenXLUNet
    from oracle import unet_ref as U
    o = U.I2VGenXLUNet(U.UNetConfig.small4())
    eng = I2VGenXLUNet(o.config.to_dict(), device="cpu")
    eng.load_state_dict(o.state_dict())  # packing is plain tensor plumbing and works without a GPU
    return eng


def test_sel_entry_points_are_declared_exported_and_bound():
    from mvoc_amd import _ffi
    hdr = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "mvoc_hip.h")).read())
    args = [C.POINTER(_ffi.PnpDesc), _ffi.i32, C.POINTER(_ffi.i32), _ffi.i32, C.c_uint32, _ffi.vp]
    decl = "(const mvoc_pnp_desc* d, int32_t nsrc, const int32_t* obj_chunk, int32_t nvar, uint32_t active, void* stream);"
    for name in ("mvoc_pnp_blend_scatter_tokens_variants_sel", "mvoc_pnp_blend_scatter_nchw_variants_sel"):
        assert f"int {name}{decl}" in hdr, name
        assert hasattr(_ffi.lib, name), name
        res, got = _ffi.SIGNATURES[name]
        assert res is _ffi.i32 and got == args and getattr(_ffi.lib, name).argtypes == args, name
    # the pair they stand beside keeps its signature
    assert _ffi.SIGNATURES["mvoc_pnp_blend_scatter_tokens_variants"][1] == args[:4] + [_ffi.vp]


# ---- hook state --------------------------------------------------------------------------------------------------------
def test_injecting_mask_follows_injecting_per_variant():
    from mvoc_amd.unet import Hookable
    h = Hookable()
    assert h.variant_schedules is None
    h.injection_schedule = torch.tensor([981, 961, 941])
    h.variant_schedules = [torch.tensor([981]), [981, 961], None, []]  # tensor, list, the shared schedule, never
    want = {981: 0b0111, 961: 0b0110, 941: 0b0100, 921: 0, 1000: 0b1111}  # t == 1000: every variant injects
    for t, m in want.items():
        h.t = t
        assert h.injecting_mask(4) == m, (t, bin(h.injecting_mask(4)))
        assert h.injecting() == (m != 0), t  # "any bit"
    h.t = None
    assert h.injecting_mask(4) == 0 and not h.injecting()
    # an empty tensor never injects; a set works like a list
    h.t = 961
    h.variant_schedules = [torch.tensor([], dtype=torch.long), {961}]
    assert h.injecting_mask(2) == 0b10
    # the shared schedule may itself be None
    h.injection_schedule = None
    h.variant_schedules = [None, [961]]
    assert h.injecting_mask(2) == 0b10 and h.injecting()
    h.variant_schedules = [None, None]
    assert h.injecting_mask(2) == 0 and not h.injecting()


def test_injecting_mask_refuses_a_wrong_length_and_names_the_site():
    eng = _cpu_engine()
    rn = eng.up_blocks[3].resnets[1]
    rn.t, rn.injection_schedule, rn.variant_schedules = 981, [981], [[981], []]
    assert rn.injecting_mask(2) == 0b01
    with pytest.raises(RuntimeError, match=r"up_blocks\.3\.resnets\.1.*2 schedules.*3 variants"):
        rn.injecting_mask(3)
    with pytest.raises(RuntimeError, match=r"up_blocks\.3\.resnets\.1"):
        eng.check_variant_schedules(3)
    eng.check_variant_schedules(2)
    eng.conv_out.variant_schedules = [None]
    with pytest.raises(RuntimeError, match="conv_out"):
        eng.check_variant_schedules(2)


def test_injecting_is_unchanged_without_variant_schedules():
    from mvoc_amd.unet import Hookable
    h = Hookable()
    for sched in (None, [], [981, 961], torch.tensor([981, 961]), torch.tensor([], dtype=torch.long), {961}):
        for t in (None, 981, 961, 941, 1000):
            h.injection_schedule, h.t = sched, t
            if sched is None or t is None:
                want = False
            elif t == 1000:
                want = True
            else:
                want = t in [int(v) for v in sched]
            assert h.injecting() is want, (sched, t)
            for K in (1, 3, 8):  # no per-variant schedules: no bit or every bit
                assert h.injecting_mask(K) == (((1 << K) - 1) if want else 0)


def _sites_with(eng, pred):
    out = set()
    blocks = [(f"down_blocks.{i}", b) for i, b in enumerate(eng.down_blocks)] + [("mid_block", eng.mid_block)] + \
             [(f"up_blocks.{i}", b) for i, b in enumerate(eng.up_blocks)]
    for bp, b in blocks:
        for kind in ("resnets", "temp_convs"):
            for j, m in enumerate(getattr(b, kind)):
                if pred(m):
                    out.add(f"{bp}.{kind}.{j}")
        for kind in ("attentions", "temp_attentions"):
            for j, m in enumerate(getattr(b, kind)):
                for a in ("attn1", "attn2"):
                    if pred(getattr(m.transformer_blocks[0], a).processor):
                        out.add(f"{bp}.{kind}.{j}.{a}")
    for name in ("conv_out", "conv_in"):
        if pred(getattr(eng, name)):
            out.add(name)
    for a in ("attn1", "attn2"):
        if pred(getattr(eng.transformer_in.transformer_blocks[0], a).processor):
            out.add(f"transformer_in.{a}")
    return out


def test_register_variant_schedules_touches_the_sites_of_the_register_functions():
    from mvoc_amd import pnp_utils
    fams = {"temporal": [pnp_utils.register_temp_attention_pnp], "spatial": [pnp_utils.register_spatial_attention_pnp],
            "conv": [pnp_utils.register_temp_conv_injection, pnp_utils.register_out_conv_injection,
                     pnp_utils.register_resnet_injection]}
    K = [[981], None, []]
    all_sites = set()
    for fam, fns in fams.items():
        eng = _cpu_engine()
        pipe = types.SimpleNamespace(unet=eng)
        for fn in fns:
            fn(pipe, [981, 961], False) if fam != "conv" else fn(pipe, [981, 961])
        plain = _sites_with(eng, lambda m: m.injection_schedule is not None)
        assert plain and not _sites_with(eng, lambda m: m.variant_schedules is not None)
        pnp_utils.register_variant_schedules(pipe, **{fam: K})
        got = _sites_with(eng, lambda m: m.variant_schedules is not None)
        assert got == plain, (fam, sorted(got ^ plain))
        assert not _sites_with(eng, lambda m: m.variant_schedules is not None and m.variant_schedules != K)
        assert not (all_sites & got)  # the three families are disjoint
        all_sites |= got
        # the masks follow: variant 0 its own schedule, variant 1 the shared one, variant 2 never
        pnp_utils.register_time_all(pipe, 961, None)
        assert set(eng.injection_masks(3)) == {0, 0b010}
        assert sum(m != 0 for m in eng.injection_masks(3)) == len(plain)
        pnp_utils.register_time_all(pipe, 981, None)
        assert set(eng.injection_masks(3)) == {0, 0b011}
        # a later plain registration is a plain registration
        for fn in fns:
            fn(pipe, [981], False) if fam != "conv" else fn(pipe, [981])
        assert not _sites_with(eng, lambda m: m.variant_schedules is not None)
        assert set(eng.injection_masks(3)) == {0, 0b111}
    assert len(all_sites) == 8 + 8 + 7
    # all three at once, and None leaves a family alone
    eng = _cpu_engine()
    pipe = types.SimpleNamespace(unet=eng)
    pnp_utils.register_variant_schedules(pipe, conv=K, spatial=K, temporal=K)
    assert _sites_with(eng, lambda m: m.variant_schedules is not None) == all_sites
    pnp_utils.register_spatial_attention_pnp(pipe, [981], False)
    left = _sites_with(eng, lambda m: m.variant_schedules is not None)
    assert len(left) == 15 and not any(".attentions." in s for s in left)


def test_injection_masks_select_the_steps_injection_flags_selects_without_variant_schedules():
    """the graph key of the composition loop: without per-variant schedules the masks partition the steps exactly as the
    per-site bools did"""
    from mvoc_amd import pnp_utils
    from mvoc_amd.schedulers import DDIMScheduler
    eng = _cpu_engine()
    pipe = types.SimpleNamespace(unet=eng)
    s = DDIMScheduler()
    s.set_timesteps(10)
    pnp_utils.register_temp_attention_pnp(pipe, s.timesteps[:8], False)
    pnp_utils.register_spatial_attention_pnp(pipe, s.timesteps[:5], False)
    pnp_utils.register_temp_conv_injection(pipe, s.timesteps[:2])
    pnp_utils.register_out_conv_injection(pipe, s.timesteps[:1])
    pnp_utils.register_resnet_injection(pipe, s.timesteps[:2])
    for K in (1, 4):
        by_flags, by_masks = {}, {}
        for i, t in enumerate(s.timesteps):
            pnp_utils.register_time_all(pipe, int(t), None)
            flags, masks = eng.injection_flags(), eng.injection_masks(K)
            assert masks == tuple(((1 << K) - 1) if f else 0 for f in flags)
            by_flags.setdefault(flags, []).append(i)
            by_masks.setdefault(masks, []).append(i)
        assert sorted(by_flags.values()) == sorted(by_masks.values()) and len(by_masks) == 5
    eng.variants = 3
    assert eng.injection_masks() == eng.injection_masks(3)


# ---- the run cutting of the paired attention ------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_variant_runs_partition_alternate_and_reproduce_the_mask(K):
    from mvoc_amd.unet import variant_runs
    for active in range(1, 1 << K):
        runs = variant_runs(active, K)
        assert runs[0][0] == 0 and runs[-1][1] == K, (active, runs)
        mask = 0
        for i, (k0, k1, on) in enumerate(runs):
            assert k0 < k1 and isinstance(on, bool)
            if i:
                assert k0 == runs[i - 1][1] and on != runs[i - 1][2], (active, runs)  # a partition; maximal runs alternate
            if on:
                mask |= ((1 << (k1 - k0)) - 1) << k0
        assert mask == active, (active, runs)
    assert variant_runs((1 << K) - 1, K) == [(0, K, True)]
    assert variant_runs(0, K) == [(0, K, False)]
    if K == 4:
        assert variant_runs(0b0110, 4) == [(0, 1, False), (1, 3, True), (3, 4, False)]
        assert variant_runs(0b0101, 4) == [(0, 1, True), (1, 2, False), (2, 3, True), (3, 4, False)]


def test_variant_runs_eight_variants():
    from mvoc_amd.unet import variant_runs
    assert variant_runs(0b10000001, 8) == [(0, 1, True), (1, 7, False), (7, 8, True)]


# ---- ops: the active argument without a launch ---------------------------------------------------------------------------
def test_ops_active_mask_routing():
    from mvoc_amd import ops
    assert ops._active_mask(None, 3, "x") is None
    assert ops._active_mask(0b111, 3, "x") is None  # every variant: the entries of a call without the argument
    assert ops._active_mask(1, 1, "x") is None
    assert ops._active_mask(0b101, 3, "x") == 0b101
    for active, nvar in ((0, 3), (0b1000, 3), (-1, 3), (2, 1), (0, 1), (1 << 8, 8)):
        with pytest.raises(RuntimeError, match="active mask"):
            ops._active_mask(active, nvar, "x")
    for nvar in (0, 9):
        with pytest.raises(RuntimeError, match="not in"):
            ops._active_mask(1, nvar, "x")


# ---- composite.py ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def composite():
    ref = os.path.join(REPO, "i2vgen-xl")
    sys.path.insert(0, ref)
    names = ("utils", "pnp_utils", "composite", "inverse", "pipelines", "pipelines.pipeline_i2vgen_xl", "common")
    saved = {m: sys.modules.pop(m) for m in names if m in sys.modules}
    try:
        mod = importlib.import_module("composite")
        assert mod.__file__.startswith(REPO)
        yield mod
    finally:
        sys.path.remove(ref)
        for m in names:
            sys.modules.pop(m, None)
        sys.modules.update(saved)


def _template(tmp):
    from mvoc_amd.config import OmegaConf
    ct = OmegaConf.load(os.path.join(REPO, "tests", "data", "composite_template.yaml"))
    ct.data_dir = str(tmp)
    return ct


ENTRY = dict(active=True, video_name="boat", edited_video_name="boat_surf", edited_first_frame_path="edit/first.png",
             editing_prompt="a boat and a surfer", obj_ddim_latents_path=["inv/o0", "inv/o1"], obj_mask_path=["m/0", "m/1"],
             obj_width_height=[[64, 64], [64, 64]], edited_contorl_frame_path=["f/o0", "f/o1"],
             edited_contorl_frame_path_main="f/main", edited_contorl_frame_path_background="f/bg",
             pnp_f_t=0.2, pnp_spatial_attn_t=1.0, pnp_temp_attn_t=1.0)


def test_merge_variants_applies_the_pnp_key(composite, tmp_path):
    ct = _template(tmp_path)
    assert "pnp" in composite.VARIANT_KEYS
    vs = [{}, {"pnp": {"pnp_spatial_attn_t": 0.5}}, {"seed": 3, "pnp": {"pnp_f_t": 0.4, "pnp_spatial_attn_t": 0.3, "pnp_temp_attn_t": 0.6}},
          {"pnp": {}}]
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=vs))
    assert [(v.pnp_f_t, v.pnp_spatial_attn_t, v.pnp_temp_attn_t) for v in variants] == \
        [(0.2, 1.0, 1.0), (0.2, 0.5, 1.0), (0.4, 0.3, 0.6), (0.2, 1.0, 1.0)]
    assert (config.pnp_f_t, config.pnp_spatial_attn_t, config.pnp_temp_attn_t) == (0.2, 1.0, 1.0)  # the entry's own: untouched
    assert variants[2].seed == 3 and ["pnp" in v for v in variants] == [False, True, True, True]
    # the suffix and the output directory show the variant's own thresholds
    assert "_pnpf0.2_pnps0.5_pnpt1.0_" in composite.variant_output_dir(variants[1], 1)
    assert "_pnpf0.4_pnps0.3_pnpt0.6_" in composite.variant_output_dir(variants[2], 2)
    assert composite.variant_output_dir(variants[2], 2).endswith("variant_02")
    assert composite.output_suffix(variants[0]) == composite.output_suffix(config) == composite.output_suffix(variants[3])
    for v in variants:
        assert v.n_steps == config.n_steps and v.inject_background == config.inject_background


@pytest.mark.parametrize("name", ["inject_background", "n_steps", "pnp_spatial_t", "cfg"])
def test_merge_variants_refuses_an_unknown_name_inside_pnp(composite, tmp_path, name):
    ct = _template(tmp_path)
    with pytest.raises(ValueError, match=rf"variants\[1\]\.pnp sets '{name}'"):
        composite.merge_variants(ct, dict(ENTRY, variants=[{}, {"pnp": {"pnp_f_t": 0.1, name: 1}}]))


def test_init_pnp_registers_the_variants_prefixes(composite, tmp_path):
    eng = _cpu_engine()
    pipe = types.SimpleNamespace(unet=eng)
    ct = _template(tmp_path)
    ct.n_steps = 10
    sched = types.SimpleNamespace(timesteps=torch.arange(10) * -100 + 901)  # a stub scheduler: 901, 801, .. 1
    vs = [{"pnp": {"pnp_spatial_attn_t": 0.5}}, {"pnp": {"pnp_f_t": 0.35, "pnp_temp_attn_t": 0.0}}, {}]
    config, variants = composite.merge_variants(ct, dict(ENTRY, variants=vs))
    composite.init_pnp(pipe, sched, config, variants)
    ts = [int(t) for t in sched.timesteps]
    spa = eng.up_blocks[2].attentions[0].transformer_blocks[0].attn1.processor
    tmp = eng.up_blocks[2].temp_attentions[0].transformer_blocks[0].attn1.processor
    ints = lambda lst: [[int(t) for t in s] for s in lst]
    assert [int(t) for t in spa.injection_schedule] == ts and [int(t) for t in eng.conv_out.injection_schedule] == ts[:2]
    assert ints(spa.variant_schedules) == [ts[:5], ts, ts]
    assert ints(tmp.variant_schedules) == [ts, [], ts]
    for site in (eng.conv_out, eng.up_blocks[3].resnets[0], eng.up_blocks[3].temp_convs[2]):
        assert ints(site.variant_schedules) == [ts[:2], ts[:3], ts[:2]]  # int(10 * 0.35) = 3
    assert len(_sites_with(eng, lambda m: m.variant_schedules is not None)) == 23
    eng.check_variant_schedules(3)
    # variants without any pnp key, or no variants: the registration of today
    _, plain = composite.merge_variants(ct, dict(ENTRY, variants=[{"seed": 1}, {"seed": 2}]))
    composite.init_pnp(pipe, sched, config, plain)
    assert not _sites_with(eng, lambda m: m.variant_schedules is not None)
    composite.init_pnp(pipe, sched, config, variants)
    composite.init_pnp(pipe, sched, config)
    assert not _sites_with(eng, lambda m: m.variant_schedules is not None)
