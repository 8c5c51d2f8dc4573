"""CPU: source de-duplication of the composition batch (pipeline.dedup_sources) -- the two mapped blend entry points are
exported and bound, and the static partition / per-step source map planner (pure host logic) lays out the batch the
composition loop runs.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPPED = ("mvoc_pnp_blend_scatter_tokens_mapped", "mvoc_pnp_blend_scatter_nchw_mapped")


def test_mapped_entry_points_are_declared_exported_and_bound():
    from mvoc_amd import _ffi
    hdr = open(os.path.join(REPO, "include", "mvoc_hip.h")).read()
    for name in MAPPED:
        assert re.search(r"\bint %s\(const mvoc_pnp_desc\* d, int32_t nsrc, const int32_t\* obj_chunk, void\* stream\);" % name, hdr)
        assert hasattr(_ffi.lib, name), name
        res, args = _ffi.SIGNATURES[name]
        assert res is _ffi.i32 and args == [C.POINTER(_ffi.PnpDesc), _ffi.i32, C.POINTER(_ffi.i32), _ffi.vp]
        assert getattr(_ffi.lib, name).argtypes == args
    assert _ffi.lib.mvoc_version() == 100


def _latents(*names):
    """one distinct object per distinct name: what LatentCache.get hands out per (directory, t)"""
    objs = {}
    return [objs.setdefault(n, object()) for n in names]


def test_plan_all_roles_distinct_is_the_positional_batch():
    from mvoc_amd.pipeline import plan_source_map
    assert plan_source_map((0, 1, 2), _latents("a", "b", "c")) is None
    assert plan_source_map((0, 0, 0), _latents("a", "b", "c")) is None  # one class, three latents
    assert plan_source_map(None, _latents("a", "a", "a")) is None  # de-duplication off


def test_plan_all_roles_the_same_source():
    from mvoc_amd.pipeline import plan_source_map
    assert plan_source_map((0, 0, 0), _latents("a", "a", "a")) == (1, (0, 0))


def test_plan_background_distinct_objects_the_same():
    from mvoc_amd.pipeline import plan_source_map
    assert plan_source_map((0, 0, 0), _latents("bg", "o", "o")) == (2, (1, 1))
    assert plan_source_map((0, 1, 1), _latents("a", "a", "a")) == (2, (1, 1))  # split by conditioning instead
    assert plan_source_map((0, 0, 0), _latents("a", "b", "a")) == (2, (1, 0))
    assert plan_source_map((0, 0, 0), _latents("a", "a", "b")) == (2, (0, 1))


@pytest.mark.parametrize("n_obj", [1, 2, 3, 4])
def test_plan_one_to_four_objects(n_obj):
    from mvoc_amd.pipeline import plan_source_map, source_rows
    same = plan_source_map((0,) * (n_obj + 1), _latents(*["s"] * (n_obj + 1)))
    assert same == (1, (0,) * n_obj) and source_rows(same, n_obj) == [0]
    objs = plan_source_map((0,) * (n_obj + 1), _latents("bg", *["o"] * n_obj))
    if n_obj == 1:
        assert objs is None  # two roles, two chunks: the identity map is the positional batch
    else:
        assert objs == (2, (1,) * n_obj) and source_rows(objs, n_obj) == [0, 1]
    # object pairs: 0 with 1, 2 with 3 ...
    names = ["bg"] + [f"o{j // 2}" for j in range(n_obj)]
    m = plan_source_map((0,) * (n_obj + 1), _latents(*names))
    k = (n_obj + 1) // 2
    if n_obj == 1:
        assert m is None
    else:
        assert m == (1 + k, tuple(1 + j // 2 for j in range(n_obj)))
        assert source_rows(m, n_obj) == [0] + [1 + 2 * i for i in range(k)]
    assert plan_source_map(tuple(range(n_obj + 1)), _latents(*["s"] * (n_obj + 1))) is None  # every role its own class


def test_plan_offset_fusion_step_is_partial():
    """obj_ddim_latents_idx_offset != ddim_init_latents_t_idx: on a fusion step the objects read latents of another t than
    the background (one tensor per (directory, t)) -- a partial map on that step only, the full merge on the others"""
    from mvoc_amd.pipeline import plan_source_map
    cache = {}
    get = lambda d, t: cache.setdefault((d, t), object())
    classes = (0, 0, 0)
    steps = [(901, 981), (801, None), (701, None)]  # (t, fusion t of the objects)
    maps = []
    for t, tf in steps:
        objs = [get("src", tf if tf is not None else t) for _ in range(2)]
        maps.append(plan_source_map(classes, [get("src", t)] + objs))
    assert maps == [(2, (1, 1)), (1, (0, 0)), (1, (0, 0))]


def _cond(n_obj, do_cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    nb = n_obj + (3 if do_cfg else 2)
    one = lambda *s: torch.randn(1, *s, generator=g).half()
    rows = dict(encoder_hidden_states=one(7, 16), image_embeddings=one(3, 16), image_latents_first=one(4, 3, 2, 2),
                image_latents=one(4, 3, 2, 2))
    cond = {k: v.repeat(nb, *[1] * (v.dim() - 1)) for k, v in rows.items()}
    cond["fps"] = torch.full((nb,), 8.0)
    for k in cond:  # the destination rows differ from the sources (main branch)
        cond[k][n_obj + 1:] = cond[k][n_obj + 1:] + 1
    return cond


@pytest.mark.parametrize("do_cfg", [True, False])
@pytest.mark.parametrize("n_obj", [1, 2, 4])
def test_static_partition(n_obj, do_cfg):
    from mvoc_amd.pipeline import plan_source_map, source_classes
    cond = _cond(n_obj, do_cfg)
    classes = source_classes(cond, n_obj)
    assert classes == (0,) * (n_obj + 1)
    assert plan_source_map(classes, _latents(*["s"] * (n_obj + 1))) == (1, (0,) * n_obj)
    # a class split by unequal conditioning: each key on its own, the last object differs -> its own chunk
    for k in ("encoder_hidden_states", "image_embeddings", "image_latents_first", "image_latents", "fps"):
        c = {kk: v.clone() for kk, v in cond.items()}
        c[k][n_obj] = c[k][n_obj] * 2 + 1
        classes = source_classes(c, n_obj)
        assert classes == (0,) * n_obj + (n_obj,), k
        m = plan_source_map(classes, _latents(*["s"] * (n_obj + 1)))
        assert m == (None if n_obj == 1 else (2, (0,) * (n_obj - 1) + (1,))), (k, m)


def test_static_partition_never_merges_nan_rows():
    """the partition compares with torch.equal, as share_cfg_prefix does: a row holding a NaN equals no row, itself included"""
    from mvoc_amd.pipeline import source_classes
    cond = _cond(2, True)
    cond["image_latents"][2, 0, 0, 0, 0] = float("nan")
    cond["image_latents"][1, 0, 0, 0, 0] = float("nan")
    assert source_classes(cond, 2) == (0, 1, 2)
