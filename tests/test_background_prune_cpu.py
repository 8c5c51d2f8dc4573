"""CPU: dropping the dead background chunk on Q/K-only composition steps -- the engine's predicate
(``background_dead``) over the hook state, the batches ``check_pnp_batch`` accepts without chunk 0, the chunk numbers the
injection sites pass, and the graph-variant key of the composition loop.  No kernel is launched."""
import types

import pytest
import torch


def _cpu_engine():
    from mvoc_amd.unet import I2VGenXLUNet
    from oracle import unet_ref as U
    o = U.I2VGenXLUNet(U.UNetConfig.small4())
    eng = I2VGenXLUNet(o.config.to_dict(), device="cpu")
    eng.load_state_dict(o.state_dict())  # packing is plain tensor plumbing and works without a GPU
    return eng


@pytest.fixture(scope="module")
def engine():
    return _cpu_engine()


def _arm(eng, t, qk=(981, 961), feat=(981,), inject_background=False):
    from mvoc_amd import pnp_utils
    pipe = types.SimpleNamespace(unet=eng)
    pnp_utils.register_temp_attention_pnp(pipe, list(qk), inject_background)
    pnp_utils.register_spatial_attention_pnp(pipe, list(qk), inject_background)
    pnp_utils.register_temp_conv_injection(pipe, list(feat))
    pnp_utils.register_out_conv_injection(pipe, list(feat))
    pnp_utils.register_resnet_injection(pipe, list(feat))
    masks = [(torch.zeros(1, 4, 3, 8, 8), torch.zeros(1, 4, 3, 8, 8, dtype=torch.bool)) for _ in range(2)]
    pnp_utils.register_time_all(pipe, t, masks)
    return pipe, masks


def _reset(eng):
    for s in eng.hook_sites():
        s.t, s.mask, s.injection_schedule, s.variant_schedules, s.inject_background = None, None, None, None, False
    eng.prune_background, eng.source_chunks, eng.variants, eng.shard, eng._pruned = False, None, 1, None, False


def test_the_predicate_truth_table(engine):
    from mvoc_amd.unet import Processor
    eng = engine
    try:
        _arm(eng, 961)  # a Q/K-only timestep
        assert not eng.background_dead()  # the switch is off by default
        eng.prune_background = True
        assert eng.background_dead()
        # a feature-injection timestep: resnet / temporal conv / conv_out blend onto chunk 0
        _arm(eng, 981)
        assert not eng.background_dead()
        # no site injects
        _arm(eng, 941)
        assert not eng.background_dead()
        _arm(eng, None)
        assert not eng.background_dead()
        # inject_background on every attention site, then on ONE site only
        _arm(eng, 961, inject_background=True)
        assert not eng.background_dead()
        _arm(eng, 961)
        assert eng.background_dead()
        procs = [s for s in eng.hook_sites() if isinstance(s, Processor) and s.injecting()]
        assert procs
        procs[-1].inject_background = True
        assert not eng.background_dead()
        procs[-1].inject_background = False
        assert eng.background_dead()
        # ... a site with inject_background that does NOT inject now reads nothing
        procs[-1].injection_schedule = [981]
        procs[-1].inject_background = True
        assert eng.background_dead()
        procs[-1].inject_background = False
        # one feature site active in one variant only
        rn = eng.up_blocks[1].resnets[0]
        rn.variant_schedules = [[], [961]]
        assert rn.injecting() and rn.injecting_mask(2) == 0b10
        assert not eng.background_dead()
        rn.variant_schedules = [[], []]
        assert eng.background_dead()
        rn.variant_schedules = None
        # one attention site injecting in one variant only, with inject_background
        procs[0].variant_schedules = [[], [961]]
        assert eng.background_dead()
        procs[0].inject_background = True
        assert not eng.background_dead()
        procs[0].inject_background, procs[0].variant_schedules = False, None
        # a de-duplicated map with an object on chunk 0 / with none there
        eng.source_chunks = (2, (0, 1))
        assert not eng.background_dead()
        eng.source_chunks = (2, (1, 1))
        assert eng.background_dead()
        eng.source_chunks = None
        # a frame shard
        eng.shard = object()
        assert not eng.background_dead()
        eng.shard = None
        # inside a conv_out-injection step's source-only forward
        eng._pruned = True
        assert not eng.background_dead()
        eng._pruned = False
        assert eng.background_dead()
    finally:
        _reset(eng)


@pytest.mark.parametrize("nobj", [1, 2, 3, 4])
@pytest.mark.parametrize("ndst", [1, 2])
@pytest.mark.parametrize("K", [1, 3])
def test_check_pnp_batch_without_the_background_chunk(nobj, ndst, K):
    from mvoc_amd.unet import I2VGenXLUNet
    chk = I2VGenXLUNet.check_pnp_batch
    masks = [None] * nobj
    good = nobj + ndst * K
    assert chk(good, masks, None, K, no_background=True) == ndst
    assert chk(good, masks, nobj, K, no_background=True) == ndst  # nsrc given: the chunks that are left
    assert chk(good + 1, masks, None, K) == ndst  # the same step with chunk 0 in place
    accepted = {nobj + K, nobj + 2 * K}
    for B in range(1, nobj + 2 * K + 3):
        if B in accepted:
            assert chk(B, masks, None, K, no_background=True) == (B - nobj) // K
            continue
        with pytest.raises(RuntimeError, match=f"UNet batch is {B}: without its background chunk"):
            chk(B, masks, None, K, no_background=True)
    with pytest.raises(RuntimeError, match="prune_background"):
        chk(good, None, None, K, no_background=True)


def test_the_sites_pass_the_flag_or_the_renumbered_map(engine):
    eng = engine
    masks = [None, None]
    try:
        assert eng.pnp_batch(5, masks) == (2, None) and eng.no_background_kw(None) == {}
        eng._no_bg = True
        assert eng.pnp_batch(4, masks) == (2, None) and eng.no_background_kw(None) == {"no_background": True}
        assert eng.pnp_batch(3, masks) == (1, None)
        with pytest.raises(RuntimeError, match="without its background chunk"):
            eng.pnp_batch(5, masks)
        eng.variants = 2
        ndst, smap = eng.pnp_batch(6, masks)
        assert (ndst, smap) == (2, (2, (0, 1))) and eng.no_background_kw(smap) == {}
        eng.variants = 1
        eng.placement = (((0, 0),) * 3,) * 2
        assert eng.pnp_batch(4, masks) == (2, (2, (0, 1)))
        eng.placement = None
        eng.source_chunks = (2, (1, 1))  # [bg, o] -> [o]
        assert eng.pnp_batch(3, masks) == (2, (1, (0, 0)))
        eng.source_chunks = (3, (2, 1))  # [bg, a, b] with the objects swapped -> [a, b]
        assert eng.pnp_batch(4, masks) == (2, (2, (1, 0)))
    finally:
        eng._no_bg, eng.variants, eng.placement, eng.source_chunks = False, 1, None, None


def test_the_descriptor_is_unchanged_and_the_layout_is_documented():
    import os
    from mvoc_amd import _ffi
    # no new field: the layout travels as base_chunk0 = -1, so a zero-initialised descriptor means what it always meant
    assert [f[0] for f in _ffi.PnpDesc._fields_][-2:] == ["base_chunk0", "ndst"] and len(_ffi.PnpDesc._fields_) == 15
    d = _ffi.PnpDesc()
    d.base_chunk0 = -1
    assert d.base_chunk0 == -1  # (a signed field)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvoc_hip.h")).read()
    body = hdr[hdr.index("typedef struct mvoc_pnp_desc"):hdr.index("} mvoc_pnp_desc;")]
    assert "-1 = NO BACKGROUND CHUNK" in body and "mvoc_pnp_blend_scatter_tokens only" in body


def _key_pipe(eng):
    from mvoc_amd.pipeline import I2VGenXLPipeline
    pipe = types.SimpleNamespace(unet=eng, prune_source_tail=True, prune_background=True)
    pipe.background_dead = types.MethodType(I2VGenXLPipeline.background_dead, pipe)
    pipe.composition_variant_key = types.MethodType(I2VGenXLPipeline.composition_variant_key, pipe)
    return pipe


def test_the_graph_variant_key_separates_eligible_and_ineligible_steps(engine):
    eng = engine
    try:
        pipe = _key_pipe(eng)
        _, masks = _arm(eng, 961)
        st = {"nvar": 1, "masks": masks, "share_cfg_prefix": False, "placement": None, "variant_placements": None}
        k_qk = pipe.composition_variant_key(st, None)
        assert k_qk[-1] == "no_background" and not eng.prune_background  # (the engine's switch is restored)
        # the same hook state with an object on chunk 0: another batch, and not eligible
        k_shared = pipe.composition_variant_key(st, (2, (0, 1)))
        assert k_shared != k_qk and "no_background" not in k_shared
        # the same injecting sites registered with inject_background: the injection masks agree, the key does not
        for s in eng.hook_sites():
            s.inject_background = True
        k_bg = pipe.composition_variant_key(st, None)
        assert k_bg != k_qk and k_bg == k_qk[:-1]
        for s in eng.hook_sites():
            s.inject_background = False
        # a feature step
        _, masks2 = _arm(eng, 981)
        st["masks"] = masks2
        assert "no_background" not in pipe.composition_variant_key(st, None)
        # the switch off: the key of the parent's loop
        _, masks3 = _arm(eng, 961)
        st["masks"] = masks3
        pipe.prune_background = False
        assert "no_background" not in pipe.composition_variant_key(st, None)
    finally:
        _reset(eng)
