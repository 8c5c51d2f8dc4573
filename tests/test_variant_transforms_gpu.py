"""GPU: per-variant object transforms in the K-variant composition loop.

* kernels: the ``_resampled_variants`` blend entries against the ``_resampled`` entries -- variant k's destination chunks equal
  the ``_resampled`` entry run with nvar = 1 on that variant's own batch [sources.., (u_k,) c_k] with table k and masks k; sources
  untouched, the chunks of an idle variant keep a sentinel; nvar = 1, K equal tables, translation-only tables and identity tables
  equal the existing entries; every int32 table entry is safe; a -0.0 base under an absent object becomes +0.0; bad arguments are
  refused with nothing written; the profiler's byte count is the stated formula.
* engine: a K = 3 forward of the toy UNet under ``variant_transforms`` against the single-variant ``transform`` forward of each
  variant, for each site kind.
* pipeline: a K = 3 call with ``variant_obj_transforms=[A, None, B]`` against three single-variant calls, graph replay against
  eager, with per-variant thresholds and with ``dedup_sources``; the three degenerate forms against the calls they resolve to.

Every comparison is on the raw fp16 bits (int16 views).  Helpers are imported from test_resample_gpu.py /
test_variant_placement_gpu.py so that the files judge by the same bars.
"""
import contextlib
import ctypes as C
import gc
import itertools
import types

import pytest
import torch

import test_placement_gpu as tp
import test_resample_gpu as rs
import test_variant_placement_gpu as tvp
import test_variants_gpu as tv

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_i16 = tv._i16
K3, F2 = 3, 2
SENTINEL = 77.0


@pytest.fixture(autouse=True)
def _no_dead_graphs_across_tests():
    """a finished toy job is a reference cycle that holds captured graphs (test_variant_placement_gpu.py): collected between
    tests, never inside a later job's graph capture"""
    gc.collect()
    yield
    gc.collect()


# ---- kernels: helpers ---------------------------------------------------------------------------------------------------------
def _variant_rows(nobj, F, H, W):
    """[3][nobj][F][H + W]: variant 0 scales 3/2 with a horizontal flip, variant 1 scales 1/2 about an off-centre anchor, variant
    2 is the identity moved by a per-frame offset -- the variants differ in every field; objects and frames differ as well"""
    from mvoc_amd import ops
    ax = lambda d, p, q, flip, a2, S: ops.level_axis_map(d, p, q, flip, a2, S, S)
    rows = []
    for k in range(K3):
        objs = []
        for j in range(nobj):
            fr = []
            for f in range(F):
                if k == 0:
                    y, x = ax(j - f, 3, 2, False, H, H), ax(f, 3, 2, True, W, W)
                elif k == 1:
                    y, x = ax(0, 1, 2, False, H - 1 + j, H), ax(j % 2, 1, 2, False, W + 3, W)
                else:
                    y, x = ax(1 + f - j, 1, 1, False, H, H), ax(-1 - f, 1, 1, False, W, W)
                fr.append(y + x)
            objs.append(fr)
        rows.append(objs)
    assert all(any(v >= 0 for v in r[:H]) and any(v >= 0 for v in r[H:]) for r in (rows[0][0][0], rows[1][0][0], rows[2][0][0]))
    assert len({str(r) for r in rows}) == K3
    return rows


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32).cuda().contiguous()


def _direct(kind, x, x2, masks, geo, c, strides, base0, ndst, smap, nvar, active, maps):
    """the C entry itself; returns its status"""
    from mvoc_amd import ops
    F, H, W = geo
    d = ops._pnp_desc(x, x2, masks, *strides, F, H, W, c, base0, ndst)
    nobj = masks.shape[-4]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    fn = getattr(ops.lib, f"mvoc_pnp_blend_scatter_{kind}_resampled_variants")
    return fn(C.byref(d), nsrc, arr, nvar, active, None if maps is None else maps.data_ptr(), ops._stream())


def _tokens_direct(buf, layout, F, H, W, c, masks, base0, ndst, smap, nvar, active, maps):
    ld, hw = buf.stride(0), H * W
    fs, ps = tv._strides(layout, ld, F, hw)
    return _direct("tokens", buf[:, :c], buf[:, c:2 * c], masks, (F, H, W), c, (F * hw * ld, fs, ps), base0, ndst, smap, nvar, active, maps)


def _nchw_direct(x, masks, F, base0, ndst, smap, nvar, active, maps):
    return _direct("nchw", x, None, masks, (F, x.shape[2], x.shape[3]), x.shape[1], (0, 0, 0), base0, ndst, smap, nvar, active, maps)


_dst = tvp._dst


def _cases(nobj_values=(1, 2, 3, 4)):
    """(n, nobj, ndst, base_chunk0, source map, active): every combination the issue names, active 0b111 and 0b101 in turn"""
    n = 0
    for nobj in nobj_values:
        for ndst, base0, smap in itertools.product((1, 2), (False, True), tp._maps(nobj)):
            for active in (0b111, 0b101):
                yield n, nobj, ndst, base0, smap, active
                n += 1


# ---- tokens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["spatial", "temporal"])
@pytest.mark.parametrize("geo", [(4, 6, None), (4, 6, (8, 12)), (3, 5, (5, 9))], ids=["4x6-same", "4x6-mask8x12", "3x5-mask5x9"])
def test_tokens_resampled_variants_equal_the_resampled_entry_per_variant(geo, layout):
    H, W, mres = geo
    mh, mw = mres or (H, W)
    F, K, c = F2, K3, 16
    rows = F * H * W
    g = torch.Generator().manual_seed(13 * H + W + (layout == "temporal"))
    chunk = lambda t, i: t[i * rows:(i + 1) * rows]
    count = 0
    for n, nobj, ndst, base0, smap, active in _cases():
        maps = _table(_variant_rows(nobj, F, H, W))
        masks = tvp._vmasks(K, nobj, F, mh, mw, bool((n // 2) % 2), g)
        nsrc = nobj + 1 if smap is None else smap[0]
        comp = tp._planted(torch.randn((nsrc + ndst * K) * rows, 3 * c, generator=g).half(), g).cuda()
        for k in range(K):
            if not (active >> k) & 1:
                for i in _dst(nsrc, ndst, K, k):
                    chunk(comp, i).fill_(SENTINEL)
        comp0 = comp.clone()
        what = (nobj, ndst, base0, smap, bin(active))
        rs._run_tokens(comp, layout, F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, resample=maps)
        for k in range(K):
            dst = _dst(nsrc, ndst, K, k)
            if not (active >> k) & 1:  # neither read nor written
                for i in dst:
                    assert bool((chunk(comp, i) == SENTINEL).all()), (what, k)
                continue
            own = torch.cat([comp0[:nsrc * rows]] + [chunk(comp0, i) for i in dst]).contiguous()  # [sources.., (u_k,) c_k]
            rs._run_tokens(own, layout, F, H, W, c, masks[k], base0, ndst, smap, nvar=1, active=1, resample=maps[k])
            for d, i in enumerate(dst):
                assert torch.equal(_i16(chunk(comp, i)[:, :2 * c]), _i16(chunk(own, nsrc + d)[:, :2 * c])), (what, k, d)
                assert not torch.equal(_i16(chunk(comp, i)[:, :2 * c]), _i16(chunk(comp0, i)[:, :2 * c])), (what, k, d)  # written
        assert torch.equal(_i16(comp[:nsrc * rows]), _i16(comp0[:nsrc * rows])), what  # sources untouched
        assert torch.equal(_i16(comp[:, 2 * c:]), _i16(comp0[:, 2 * c:])), what  # v columns untouched
        if base0:  # (one base: only the objects' transforms can tell the variants apart)
            a, b = _dst(nsrc, ndst, K, 0)[-1], _dst(nsrc, ndst, K, 2)[-1]
            assert not torch.equal(_i16(chunk(comp, a)[:, :2 * c]), _i16(chunk(comp, b)[:, :2 * c])), what
        count += 1
    assert count == 2 * 2 * 2 * (1 + 3 * 2)


# ---- NCHW -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 8), (3, 5)])  # hw % 8 == 0: base and destinations 8 pixels per work item / else 1
def test_nchw_resampled_variants_equal_the_resampled_entry_per_variant(hw):
    from mvoc_amd import ops
    H, W = hw
    F, K, Cc = F2, K3, 4
    g = torch.Generator().manual_seed(700 + W)
    chunk = lambda t, i: t[i * F:(i + 1) * F]
    count = 0
    for n, nobj, ndst, base0, smap, active in _cases():
        maps = _table(_variant_rows(nobj, F, H, W))
        mh, mw = (H, W) if n % 2 else (2 * H, W + 1)
        masks = tvp._vmasks(K, nobj, F, mh, mw, bool((n // 2) % 2), g)
        nsrc = nobj + 1 if smap is None else smap[0]
        comp = tp._planted(torch.randn((nsrc + ndst * K) * F, Cc, H, W, generator=g).half(), g).cuda()
        for k in range(K):
            if not (active >> k) & 1:
                for i in _dst(nsrc, ndst, K, k):
                    chunk(comp, i).fill_(SENTINEL)
        comp0 = comp.clone()
        what = (nobj, ndst, base0, smap, (mh, mw), bin(active))
        ops.pnp_blend_nchw(comp, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=maps)
        for k in range(K):
            dst = _dst(nsrc, ndst, K, k)
            if not (active >> k) & 1:
                for i in dst:
                    assert bool((chunk(comp, i) == SENTINEL).all()), (what, k)
                continue
            own = torch.cat([comp0[:nsrc * F]] + [chunk(comp0, i) for i in dst]).contiguous()
            ops.pnp_blend_nchw(own, masks[k], frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=1, active=1, resample=maps[k])
            for d, i in enumerate(dst):
                assert torch.equal(_i16(chunk(comp, i)), _i16(chunk(own, nsrc + d))), (what, k, d)
        assert torch.equal(_i16(comp[:nsrc * F]), _i16(comp0[:nsrc * F])), what
        count += 1
    assert count == 2 * 2 * 2 * (1 + 3 * 2)


# ---- reductions ---------------------------------------------------------------------------------------------------------------
def test_one_variant_is_the_resampled_entry():
    """nvar = 1 through the C entries themselves: the bits of the _resampled entry with the same table and masks"""
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(31)
    F, c = F2, 16
    for (H, W), nobj, ndst, base0 in itertools.product(((4, 8), (3, 5)), (1, 2, 4), (1, 2), (False, True)):
        for smap in tp._maps(nobj):
            maps = _table(_variant_rows(nobj, F, H, W)[:1])
            masks = tvp._vmasks(1, nobj, F, 5, 9, True, g)
            tok, nchw = tvp._both_layouts(g, nobj, 1, ndst, smap, F, H, W, c)
            tok2, nchw2 = tok.clone(), nchw.clone()
            assert _tokens_direct(tok, "temporal", F, H, W, c, masks, base0, ndst, smap, 1, 1, maps) == 0
            rs._run_tokens(tok2, "temporal", F, H, W, c, masks[0], base0, ndst, smap, nvar=1, active=1, resample=maps[0])
            assert torch.equal(_i16(tok), _i16(tok2)), (H, W, nobj, ndst, base0, smap)
            assert _nchw_direct(nchw, masks, F, base0, ndst, smap, 1, 1, maps) == 0
            ops.pnp_blend_nchw(nchw2, masks[0], frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=1, active=1, resample=maps[0])
            assert torch.equal(_i16(nchw), _i16(nchw2)), (H, W, nobj, ndst, base0, smap)


def test_equal_tables_with_equal_masks_are_the_resampled_entry_with_that_table():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(32)
    F, c = F2, 8
    for (H, W), nobj, (K, active), ndst, base0 in itertools.product(((4, 8), (3, 5)), (1, 3), ((2, 0b11), (3, 0b101), (8, 0xff)), (1, 2),
                                                                    (False, True)):
        for smap in tp._maps(nobj):
            one = _variant_rows(nobj, F, H, W)[0]
            masks = tv._masks(nobj, F, 5, 9, True, g)
            tok, nchw = tvp._both_layouts(g, nobj, K, ndst, smap, F, H, W, c)
            tok2, nchw2 = tok.clone(), nchw.clone()
            maps, vmasks = _table([one] * K), torch.stack([masks] * K).contiguous()
            rs._run_tokens(tok, "spatial", F, H, W, c, vmasks, base0, ndst, smap, nvar=K, active=active, resample=maps)
            rs._run_tokens(tok2, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, resample=_table(one))
            assert torch.equal(_i16(tok), _i16(tok2)), (H, W, nobj, K, ndst, base0, smap)
            ops.pnp_blend_nchw(nchw, vmasks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=maps)
            ops.pnp_blend_nchw(nchw2, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=_table(one))
            assert torch.equal(_i16(nchw), _i16(nchw2)), (H, W, nobj, K, ndst, base0, smap)


def test_translation_only_tables_return_the_bits_of_the_placed_variants_entries():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(33)
    F, c = F2, 16
    for (H, W), nobj, (K, active), ndst, base0 in itertools.product(((4, 8), (3, 5)), (1, 4), ((3, 0b111), (3, 0b101), (8, 0xb5)), (1, 2),
                                                                    (False, True)):
        offs = tvp._variant_offsets(K, nobj, F, H, W)
        place, maps = tvp._vtable(offs), _table([rs._shift_rows(o, H, W) for o in offs])
        for smap in tp._maps(nobj):
            masks = tvp._vmasks(K, nobj, F, 5, 9, True, g)
            tok, nchw = tvp._both_layouts(g, nobj, K, ndst, smap, F, H, W, c)
            tok2, nchw2 = tok.clone(), nchw.clone()
            rs._run_tokens(tok, "temporal", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, resample=maps)
            rs._run_tokens(tok2, "temporal", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, place=place)
            assert torch.equal(_i16(tok), _i16(tok2)), (H, W, nobj, K, active, ndst, base0, smap)
            ops.pnp_blend_nchw(nchw, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=maps)
            ops.pnp_blend_nchw(nchw2, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=place)
            assert torch.equal(_i16(nchw), _i16(nchw2)), (H, W, nobj, K, active, ndst, base0, smap)


def test_identity_tables_return_the_bits_of_the_variants_sel_entries():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(34)
    F, c = F2, 16
    for (H, W), nobj, (K, active), ndst, base0 in itertools.product(((4, 8), (3, 5)), (1, 3), ((2, None), (3, 0b101), (8, 0x5a)), (1, 2),
                                                                    (False, True)):
        ident = _table([[[list(range(H)) + list(range(W))] * F] * nobj] * K)
        for smap in tv._maps(nobj)[:3]:
            masks = tv._masks(nobj, F, 5, 9, True, g)
            tok, nchw = tvp._both_layouts(g, nobj, K, ndst, smap, F, H, W, c)
            tok2, nchw2 = tok.clone(), nchw.clone()
            vmasks = torch.stack([masks] * K).contiguous()
            rs._run_tokens(tok, "temporal", F, H, W, c, vmasks, base0, ndst, smap, nvar=K, active=active, resample=ident)
            rs._run_tokens(tok2, "temporal", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active)  # _variants / _variants_sel
            assert torch.equal(_i16(tok), _i16(tok2)), (H, W, nobj, K, active, ndst, base0, smap)
            ops.pnp_blend_nchw(nchw, vmasks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=ident)
            ops.pnp_blend_nchw(nchw2, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active)
            assert torch.equal(_i16(nchw), _i16(nchw2)), (H, W, nobj, K, active, ndst, base0, smap)


# ---- safety -------------------------------------------------------------------------------------------------------------
def _poisoned(shape, pad_rows, g):
    """a finite tensor of ``shape`` inside an allocation whose rows before and after it are NaN -> (tensor view, whole)"""
    whole = torch.full((shape[0] + 2 * pad_rows,) + tuple(shape[1:]), float("nan"), dtype=torch.float16, device="cuda")
    x = whole[pad_rows:pad_rows + shape[0]]
    x.copy_(tp._planted(torch.randn(*shape, generator=g).half(), g).cuda())
    return x, whole


def test_every_int32_entry_in_one_variants_table_is_safe_and_means_absent():
    """INT32_MIN, -1, H (W) and INT32_MAX in variant 1's table: its objects are absent -- the base blended with zero objects under
    zero masks -- no NaN of the poisoned allocation reaches a result, and variants 0 and 2 are what they are without it"""
    from mvoc_amd import ops
    F, K, c, nobj = F2, K3, 16, 2
    g = torch.Generator().manual_seed(41)
    lo, hi = -(2 ** 31), 2 ** 31 - 1
    for (H, W), base0 in itertools.product(((3, 5), (4, 8)), (True, False)):
        rows_v = _variant_rows(nobj, F, H, W)
        bad_y, bad_x = ([lo, -1, H, hi] * 2)[:H], ([hi, W, -1, lo] * 2)[:W]
        rows_v[1] = [[bad_y + list(range(W)), list(range(H)) + bad_x], [bad_y + bad_x, [hi] * H + [lo] * W]]
        maps = _table(rows_v)
        masks = tvp._vmasks(K, nobj, F, H, W, False, g)
        nrow = F * H * W
        nsrc, ndst = nobj + 1, 2
        # tokens
        comp, whole = _poisoned(((nsrc + ndst * K) * nrow, 3 * c), 2 * nrow, g)
        comp0 = comp.clone()
        rs._run_tokens(comp, "spatial", F, H, W, c, masks, base0, ndst, None, nvar=K, active=0b111, resample=maps)
        chunk = lambda t, i: t[i * nrow:(i + 1) * nrow]
        assert not torch.isnan(comp).any() and torch.isnan(whole[:2 * nrow]).all() and torch.isnan(whole[-2 * nrow:]).all(), (H, W, base0)
        assert torch.equal(_i16(comp[:nsrc * nrow]), _i16(comp0[:nsrc * nrow]))
        for k in range(K):
            dst = _dst(nsrc, ndst, K, k)
            own = torch.cat([comp0[:nsrc * nrow]] + [chunk(comp0, i) for i in dst]).contiguous()
            if k == 1:  # absent everywhere: zero objects under zero masks, the positional kernel
                own[nrow:nsrc * nrow] = 0.0
                rs._run_tokens(own, "spatial", F, H, W, c, torch.zeros_like(masks[k]), base0, ndst)
            else:
                rs._run_tokens(own, "spatial", F, H, W, c, masks[k], base0, ndst, nvar=1, active=1, resample=maps[k])
            for d, i in enumerate(dst):
                assert torch.equal(_i16(chunk(comp, i)[:, :2 * c]), _i16(chunk(own, nsrc + d)[:, :2 * c])), (H, W, base0, k, d)
        # NCHW
        x, xwhole = _poisoned(((nsrc + ndst * K) * F, 4, H, W), 2 * F, g)
        x0 = x.clone()
        ops.pnp_blend_nchw(x, masks, frames=F, base_chunk0=base0, ndst=ndst, nvar=K, active=0b111, resample=maps)
        fchunk = lambda t, i: t[i * F:(i + 1) * F]
        assert not torch.isnan(x).any() and torch.isnan(xwhole[:2 * F]).all() and torch.isnan(xwhole[-2 * F:]).all(), (H, W, base0)
        assert torch.equal(_i16(x[:nsrc * F]), _i16(x0[:nsrc * F]))
        for k in range(K):
            dst = _dst(nsrc, ndst, K, k)
            own = torch.cat([x0[:nsrc * F]] + [fchunk(x0, i) for i in dst]).contiguous()
            if k == 1:
                own[F:nsrc * F] = 0.0
                ops.pnp_blend_nchw(own, torch.zeros_like(masks[k]), frames=F, base_chunk0=base0, ndst=ndst)
            else:
                ops.pnp_blend_nchw(own, masks[k], frames=F, base_chunk0=base0, ndst=ndst, nvar=1, active=1, resample=maps[k])
            for d, i in enumerate(dst):
                assert torch.equal(_i16(fchunk(x, i)), _i16(fchunk(own, nsrc + d))), (H, W, base0, k, d)


def test_a_negative_zero_base_becomes_positive_zero_in_a_later_variant():
    """variant 2's object is absent everywhere (variant 0's is not): value 0 and mask 0 enter blend16_h, -0.0 * 1 + 0 * 0 = +0.0"""
    from mvoc_amd import ops
    F, H, W, c, K = F2, 4, 6, 16, K3
    nrow = F * H * W
    ident = [list(range(H)) + list(range(W))] * F
    absent = [[-1] * H + list(range(W)), list(range(H)) + [-1] * W]  # one axis each
    maps = _table([[ident], [ident], [absent]])
    masks = torch.ones(K, 1, F, H, W, dtype=torch.float16, device="cuda")
    comp = torch.randn((2 + 2 * K) * nrow, 3 * c, generator=torch.Generator().manual_seed(2)).half().cuda()  # [bg, obj, u_0..2, c_0..2]
    comp[(2 + K) * nrow:] = -0.0  # the bases: every variant's cond chunk
    rs._run_tokens(comp, "spatial", F, H, W, c, masks, False, 2, nvar=K, active=0b111, resample=maps)
    for i in _dst(2, 2, K, 2):
        assert bool((_i16(comp[i * nrow:(i + 1) * nrow, :2 * c]) == 0).all())  # +0.0: no sign bit
    for i in _dst(2, 2, K, 0):  # (an all-ones mask under the identity: the object itself)
        assert torch.equal(_i16(comp[i * nrow:(i + 1) * nrow, :2 * c]), _i16(comp[nrow:2 * nrow, :2 * c]))
    x = torch.randn((2 + 2 * K) * F, 4, 4, 8, generator=torch.Generator().manual_seed(3)).half().cuda()
    x[(2 + K) * F:] = -0.0
    m = torch.ones(K, 1, F, 4, 8, dtype=torch.float16, device="cuda")
    idn = [list(range(4)) + list(range(8))] * F
    ops.pnp_blend_nchw(x, m, frames=F, base_chunk0=False, ndst=2, nvar=K,
                       resample=_table([[idn], [idn], [[[-1] * 4 + list(range(8)), list(range(4)) + [-1] * 8]]]))
    for i in _dst(2, 2, K, 2):
        assert bool((_i16(x[i * F:(i + 1) * F]) == 0).all())
    for i in _dst(2, 2, K, 1):
        assert torch.equal(_i16(x[i * F:(i + 1) * F]), _i16(x[F:2 * F]))


def test_resampled_variants_entries_refuse_bad_arguments_and_write_nothing():
    from mvoc_amd import ops
    F, H, W, c, K = 2, 4, 4, 8, 3
    g = torch.Generator().manual_seed(0)
    masks = tvp._vmasks(8, 2, F, H, W, False, g)  # (room for every nvar tried below)
    zbuf = torch.zeros(19 * F * H * W, 3 * c, dtype=torch.float16, device="cuda")
    znchw = torch.zeros(19 * F, 4, H, W, dtype=torch.float16, device="cuda")
    buf = torch.randn(19 * F * H * W, 3 * c, generator=g).half().cuda()
    nchw = torch.randn(19 * F, 4, H, W, generator=g).half().cuda()
    buf0, nchw0 = buf.clone(), nchw.clone()
    maps = _table((_variant_rows(2, F, H, W) * 3)[:8])
    err = lambda: ops.lib.mvoc_last_error().decode()
    cases = [  # (nvar, active, map, table, base_chunk0, text)
        (0, 1, None, maps, None, "nvar 0"), (9, 1, None, maps, None, "nvar 9"), (-1, 1, None, maps, None, "nvar -1"),
        (3, 0, None, maps, None, "active mask 0x0"), (3, 8, None, maps, None, "active mask 0x8"), (1, 2, None, maps, None, "active mask 0x2"),
        (8, 256, None, maps, None, "active mask 0x100"),
        (2, 3, (0, (0, 0)), maps, None, "nsrc 0"), (2, 3, (4, (0, 1)), maps, None, "nsrc 4"), (2, 3, (2, (0, 2)), maps, None, "obj_chunk[1] = 2"),
        (2, 3, (2, (-1, 0)), maps, None, "obj_chunk[0] = -1"),
        (2, 3, None, None, None, "null map table"),
        (1, 1, (2, (0, 1)), maps, -1, "base_chunk0 = -1"),
    ]
    for tok, img in ((zbuf, znchw), (buf, nchw)):
        for nvar, active, smap, tab, b0, text in cases:
            assert _tokens_direct(tok, "spatial", F, H, W, c, masks, False if b0 is None else b0, 2, smap, nvar, active, tab) == -1, text
            assert text in err(), (text, err())
            assert _nchw_direct(img, masks, F, True if b0 is None else b0, 2, smap, nvar, active, tab) == -1, text
            assert text in err(), (text, err())
    torch.cuda.synchronize()
    assert not zbuf.any() and not znchw.any()  # a zero buffer stays zero
    assert torch.equal(_i16(buf), _i16(buf0)) and torch.equal(_i16(nchw), _i16(nchw0))  # nothing was written
    # the Python layer: the forms of the table and of the mask stack, and the arguments a table does not combine with
    run = lambda m, t, nvar=K, **kw: rs._run_tokens(buf, "spatial", F, H, W, c, m, False, 2, None, nvar=nvar, resample=t, **kw)
    with pytest.raises(RuntimeError, match=r"int32 \[K = 3, nobj = 2, F = 2, H \+ W = 8\]"):
        run(masks[:K], maps[:2])
    with pytest.raises(RuntimeError, match=r"int32 \[K = 3, nobj = 2, F = 2, H \+ W = 8\]"):
        ops.pnp_blend_nchw(nchw, masks[:K], frames=F, ndst=2, nvar=K, resample=maps[:K, :, :, :7].contiguous())
    with pytest.raises(RuntimeError, match=r"needs masks as a contiguous \[K = 3, nobj = 2, F = 2, mh, mw\] stack"):
        run(masks[0], maps[:K])
    with pytest.raises(RuntimeError, match=r"needs masks as a contiguous \[K = 3"):
        ops.pnp_blend_nchw(nchw, masks[:2], frames=F, ndst=2, nvar=K, resample=maps[:K])
    with pytest.raises(RuntimeError, match="does not take a .* mask stack"):  # a 3-D table keeps today's error
        run(masks[:K], maps[0])
    with pytest.raises(RuntimeError, match="resample"):
        ops.pnp_blend_nchw(nchw, masks[:K], frames=F, ndst=2, nvar=K, resample=maps[:K].long())
    with pytest.raises(RuntimeError, match="resample= and place= are both given"):
        run(masks[:K], maps[:K], place=tvp._vtable(tvp._variant_offsets(K, 2, F, H, W)))
    with pytest.raises(RuntimeError, match="no_background"):
        run(masks[:K], maps[:K], no_background=True)
    with pytest.raises(RuntimeError, match="storage ends"):  # 3 + 2 * 8 chunks in a buffer of 9
        ops.pnp_blend_nchw(torch.zeros(9 * F, 4, H, W, dtype=torch.float16, device="cuda"), masks, frames=F, ndst=2, nvar=8, resample=maps)
    torch.cuda.synchronize()
    assert torch.equal(_i16(buf), _i16(buf0)) and torch.equal(_i16(nchw), _i16(nchw0))
    # a valid call with the same buffers goes through (the refusals above were about the arguments)
    assert _tokens_direct(buf, "spatial", F, H, W, c, masks, False, 2, None, 8, 0xff, maps) == 0, err()
    assert _nchw_direct(nchw, masks, F, True, 2, None, 1, 1, maps) == 0, err()
    torch.cuda.synchronize()
    assert not torch.equal(_i16(buf), _i16(buf0)) and not torch.equal(_i16(nchw), _i16(nchw0))


def test_profiler_counts_the_stated_bytes():
    """fill_placed_variants' chunk count with `on` mask sets + the table, 4 * nvar * nobj * F * (H + W) bytes"""
    from mvoc_amd import ops
    F, H, W, c, K, nobj = 2, 4, 4, 8, 3, 2
    rows = F * H * W
    masks = tvp._vmasks(K, nobj, F, H, W, False, torch.Generator().manual_seed(0))
    maps = _table(_variant_rows(nobj, F, H, W))
    chunk_bytes, table = 2.0 * rows * c, 4.0 * K * nobj * F * (H + W)
    ops.prof_enable(True)
    try:
        for base0, ndst, smap, active, nobjc in ((True, 2, None, 0b101, 2), (False, 2, None, 0b011, 2), (False, 1, (2, (1, 1)), 0b100, 1),
                                                 (True, 1, (1, (0, 0)), 0b111, 1), (True, 2, (2, (1, 0)), 0b110, 2)):
            on = bin(active).count("1")
            nsrc = 3 if smap is None else smap[0]
            want = chunk_bytes * (on * nobjc + (1 if base0 else on) + ndst * on) + 2.0 * on * nobj * F * H * W
            buf = torch.zeros((nsrc + ndst * K) * rows, 3 * c, dtype=torch.float16, device="cuda")
            nchw = torch.zeros((nsrc + ndst * K) * F, c, H, W, dtype=torch.float16, device="cuda")
            ops.prof_reset()
            rs._run_tokens(buf, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, resample=maps)
            torch.cuda.synchronize()
            t = ops.prof_collect()["pnp"]
            ops.prof_reset()
            ops.pnp_blend_nchw(nchw, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=maps)
            torch.cuda.synchronize()
            n = ops.prof_collect()["pnp"]
            assert t["launches"] == 1 and t["work"] == 2 * want + table, (base0, ndst, smap, active, t, 2 * want + table)  # q and k
            assert n["launches"] == 1 and n["work"] == want + table, (base0, ndst, smap, active, n, want + table)
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


# ---- engine -------------------------------------------------------------------------------------------------------------
F3 = 3
TR_A = rs.ENGINE_TRANSFORM  # 3/2 mirrored left-right on a path; 1/2 in y, mirrored top-bottom about an off-centre anchor
TR_0 = ((1, 1, 1, 1, False, False, 8, 8, ((0, 0),) * F3),) * 2  # the identity: what a variant that is not transformed carries
TR_B = ((1, 2, 1, 2, False, False, 6, 10, ((0, 0), (1, -1), (0, 2))), (1, 1, 1, 1, True, True, 8, 8, ((-1, 2),) * F3))


@pytest.mark.parametrize("kind", ["qk", "conv_out", "features"])
def test_unet_variant_transforms_equal_the_single_variant_transformed_forwards(kind):
    """K = 3 under variant_transforms (A, identity, B): variant k's destination chunks are those of the single-variant forward
    under transform k, for a Q/K step, a conv_out step and, with prune_dead_chunks off, the feature sites"""
    from mvoc_amd import ops, pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    F, h, w, cd, K = F3, 8, 8, 64, 3
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    vt = (TR_A, TR_0, TR_B)
    glue = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False)
    vstate = glue.transform_variant_masks(masks, vt)
    assert [t.tolist() for t in vstate["resample_dev"]] == [ops.transform_maps(tr, h, w, h, w) for tr in vt]
    assert all(tuple(m.shape) == (K, 2, F, h, w) and m.dtype == torch.float16 for m in vstate["masks"])
    roles = tv._roles(F, h, w, cd, 4, K)
    pipe, (t_feat, t_qk) = tv._arm(eng, 5)
    t = t_qk if kind == "qk" else t_feat
    saved = eng.prune_dead_chunks
    src = ["S", "O", "P"]

    def forward(names, **attrs):
        attrs = dict(attrs, prune_source_tail=True, prune_dead_chunks=kind != "features")
        old = {a: getattr(eng, a) for a in attrs}
        for a, v in attrs.items():
            setattr(eng, a, v)
        try:
            return tv._fwd(eng, tv._batch(roles, names), t)
        finally:
            for a, v in old.items():
                setattr(eng, a, v)

    try:
        pnp_utils.register_time_all(pipe, t, masks)  # the hooks carry ONE mask set: the call's, as it came
        names = src + [f"u{k}" for k in range(K)] + [f"c{k}" for k in range(K)]
        got = forward(names, variants=K, variant_transforms=vt, variant_masks=vstate["masks"])
        tables = dict(eng._level_tables["variant_transforms"][1])
        plain = forward(names, variants=K)
        refs = []
        for k, tr in enumerate(vt):
            pnp_utils.register_time_all(pipe, t, glue.transform_masks(masks, tr)[0])
            refs.append(forward(src + [f"u{k}", f"c{k}"], transform=tr))
    finally:
        eng.prune_dead_chunks = saved
        tv._disarm(eng, pipe)
    torch.cuda.synchronize()
    assert eng.variant_transforms is None and eng.variant_masks is None and eng.variants == 1
    levels = {key[:2] for key in tables}  # every site was handed the [K, nobj, F, H + W] table of its own level
    assert levels == {"qk": {(8, 8), (4, 4), (2, 2)}, "conv_out": {(8, 8)}}.get(kind, levels) and (8, 8) in levels, (kind, levels)
    for (H, W, mh, mw), tab in tables.items():
        assert (mh, mw) == (h, w) and tab.tolist() == [ops.transform_maps(tr, H, W, h, w) for tr in vt]
    for k in range(K):
        for d in range(2):
            a, b = got[3 + d * K + k], refs[k][3 + d]
            diff = float((a.float() - b.float()).abs().max())
            print(f"{kind}: variant {k} chunk {'uc'[d]}: max-abs vs the single-variant forward {diff:.3e}"
                  f"{' (bit-identical)' if torch.equal(_i16(a), _i16(b)) else ''}")
    for k in range(K):
        for d in range(2):
            assert torch.equal(_i16(got[3 + d * K + k]), _i16(refs[k][3 + d])), (kind, k, d)
    assert torch.isfinite(got[3:]).all()
    for k in (0, 2):  # the transforms moved something; the identity variant is the untransformed one
        assert not torch.equal(got[3 + K + k], plain[3 + K + k]), (kind, k)
    assert torch.equal(_i16(got[3 + K + 1]), _i16(plain[3 + K + 1])), kind


def test_unet_refuses_variant_transforms_it_cannot_run():
    from mvoc_amd import pnp_utils
    F, h, w, cd, K = F3, 8, 8, 64, 3
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    roles = tv._roles(F, h, w, cd, 4, K)
    pipe, (_, t_qk) = tv._arm(eng, 5)
    names = ["S", "O", "P"] + [f"u{k}" for k in range(K)] + [f"c{k}" for k in range(K)]
    stack = torch.zeros(K, 2, F, h, w, dtype=torch.float16, device="cuda")
    try:
        pnp_utils.register_time_all(pipe, t_qk, masks)
        eng.variants, eng.variant_masks = K, (stack, stack)
        eng.variant_transforms = (TR_A, TR_B)
        with pytest.raises(RuntimeError, match="variant_transforms holds 2 transforms, the call 3 variants"):
            tv._fwd(eng, tv._batch(roles, names), t_qk)
        eng.variant_transforms = (TR_A, TR_0, TR_B[:1])
        with pytest.raises(RuntimeError, match=r"variant_transforms\[2\] holds 1 objects, the hooks carry 2 masks"):
            tv._fwd(eng, tv._batch(roles, names), t_qk)
        eng.variant_transforms = (TR_A, TR_0, TR_B)
        for attr, val in (("placement", tvp.PL_A), ("variant_placements", (tvp.PL_A, tvp.PL_0, tvp.PL_B)), ("transform", TR_A)):
            setattr(eng, attr, val)
            with pytest.raises(RuntimeError, match="variant_transforms is set together with"):
                tv._fwd(eng, tv._batch(roles, names), t_qk)
            setattr(eng, attr, None)
        eng.variant_masks = None
        with pytest.raises(RuntimeError, match="variant_transforms is set but variant_masks is not"):
            tv._fwd(eng, tv._batch(roles, names), t_qk)
        eng.shard = types.SimpleNamespace(rank=0, world=1)
        with pytest.raises(RuntimeError, match="frame shard"):
            eng.pnp_batch(9, masks)
        with pytest.raises(RuntimeError, match="frame shard"):
            eng.place_kw(masks, 8, 8)
    finally:
        eng.variants, eng.variant_masks, eng.variant_transforms, eng.shard = 1, None, None, None
        eng.placement, eng.variant_placements, eng.transform = None, None, None
        tv._disarm(eng, pipe)
    assert eng.place_kw(masks, 8, 8) == {}


# ---- pipeline -----------------------------------------------------------------------------------------------------------
T_A = rs.TRANSFORMS  # 3/2 mirrored left-right on a path; 1/2 in y mirrored top-bottom about an off-centre anchor, moved
T_B = [{"scale": "1/2", "anchor": [16, 48]}, {"flip": "hv", "offset": [(0, -24), (16, 16), (0, -64)]}]  # object 1 leaves the frame
T_ID = [{"scale": 1.0, "flip": None, "offset": [(0, 0)] * 3, "anchor": [8, 16]}, {}]
SAMPLE = rs.SAMPLE


@contextlib.contextmanager
def _with_call_kwargs(**extra):
    """test_variant_placement_gpu.py's toy job passes the offsets arguments; here its sampling call is handed more"""
    from mvoc_amd.pipeline import I2VGenXLPipeline
    orig = getattr(I2VGenXLPipeline, SAMPLE)

    def call(self, *a, **kw):
        return orig(self, *a, **extra, **kw)

    setattr(I2VGenXLPipeline, SAMPLE, call)
    try:
        yield
    finally:
        setattr(I2VGenXLPipeline, SAMPLE, orig)


def _job(graphs, variant_transforms="none", transforms="none", **kw):
    extra = {}
    if variant_transforms != "none":
        extra["variant_obj_transforms"] = variant_transforms
    if transforms != "none":
        extra["obj_transforms"] = transforms
    with _with_call_kwargs(**extra):
        return tvp._job(graphs, **kw)


_keys = lambda job: {(k[0],) + k[2:] for k in job.state["variants"]}  # (without the mask key: the ids of each job's own tensors)


def test_three_transforms_in_one_loop_equal_three_single_calls_and_graph_replay():
    """variant_obj_transforms = [A, None, B]: the final latents of variant k are those of the single-variant call with
    obj_transforms A, none and B (two fusion steps included); graph replay equals eager"""
    from mvoc_amd import ops
    eager = _job(False, [T_A, None, T_B], count_calls=True)
    st = eager.state
    assert st["placement"] is None and st["variant_placements"] is None and st["transform"] is None and st["vplace"] is None
    vt = st["variant_transforms"]
    assert len(vt) == 3 and vt[0] == rs.TRANSFORMS_LAT and vt[1] == TR_0
    # every variant's masks gathered once, with ITS S = L maps: the engine's stacks and the fusion masks
    soft, hard = st["vresample"]["masks"]
    for k, tr in enumerate(vt):
        rows = ops.transform_maps(tr, 8, 8, 8, 8)
        assert st["vresample"]["resample_dev"][k].tolist() == rows
        for j in range(2):
            for f, r in enumerate(rows[j]):
                want = rs._gather_last2(eager.masks[j][0][0, 0, f].cuda(), r[:8], r[8:])
                assert torch.equal(soft[k, j, f], want) and torch.equal(st["vresample"]["fusion_masks"][k][j, 0, 0, f], want)
                assert torch.equal(hard[k, j, f], rs._gather_last2(eager.masks[j][1][0, 0, f].cuda().half(), r[:8], r[8:]))
    # the hooks keep the call's masks as they came; the per-level [K, nobj, F, H + W] tables stay alive with the state
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(st["masks"], eager.masks))
    assert len(st["place_tables"]) == 1 and {k[:2] for k in st["place_tables"][0]} == {(8, 8), (4, 4), (2, 2)}
    assert all(tuple(t.shape) == (3, 2, 3, k[0] + k[1]) for k, t in st["place_tables"][0].items())
    names = set().union(*eager.step_calls)
    assert {"mvoc_pnp_blend_scatter_tokens_resampled_variants", "mvoc_pnp_blend_scatter_nchw_resampled_variants",
            "mvoc_gather_planes_f16"} <= names
    assert not any(n.startswith("mvoc_pnp_blend") and not n.endswith("_resampled_variants") for n in names), names
    assert "mvoc_shift_planes_f16" not in names
    # two fusion steps: per variant the two fusion objects through the gather kernel and one single-variant fusion launch
    assert [c.get("mvoc_gather_planes_f16", 0) for c in eager.step_calls] == [6, 6, 0, 0, 0]
    assert [c.get("mvoc_latent_fusion_f16", 0) for c in eager.step_calls] == [3, 3, 0, 0, 0]
    assert not any("mvoc_latent_fusion_variants_f16" in c for c in eager.step_calls)
    singles = [_job(False, transforms=T_A, only=0), _job(False, only=1), _job(False, transforms=T_B, only=2)]
    assert singles[0].state["transform"] == vt[0] and singles[1].state["transform"] is None and singles[2].state["transform"] == vt[2]
    tvp._compare_with_singles(eager, singles, "eager")
    graphed = _job(True, [T_A, None, T_B])
    assert graphed.graphs >= 3 and torch.equal(_i16(graphed.out), _i16(eager.out)) and torch.isfinite(eager.out).all()
    assert all("variant_transforms" in k for k in graphed.state["variants"])  # part of the graph-variant key
    plain = _job(False)
    for k in (0, 2):
        assert not torch.equal(plain.out[k], eager.out[k]), k  # the transforms moved the result


def test_variant_transforms_with_per_variant_thresholds():
    job = _job(True, [T_A, None, T_B], thresholds=True)
    singles = [_job(True, transforms=T_A, only=0, thresholds=True), _job(True, only=1, thresholds=True),
               _job(True, transforms=T_B, only=2, thresholds=True)]
    tvp._compare_with_singles(job, singles, "per-variant thresholds")
    assert job.graphs == 4  # spatial Q/K injects for 3 / 1 / 5 steps: steps 0, 1..2, 3, 4 are four kinds


def test_variant_transforms_with_deduplicated_sources():
    """one source behind every role: both objects read the background's chunk, each variant through its own maps"""
    job = _job(False, [T_B, T_A, None], dedup=True)
    assert any(m is not None for m in job.state["maps"]), job.state["maps"].keys()  # a de-duplicated batch did run
    singles = [_job(False, transforms=T_B, only=0, dedup=True), _job(False, transforms=T_A, only=1, dedup=True), _job(False, only=2, dedup=True)]
    tvp._compare_with_singles(job, singles, "dedup_sources")
    graphed = _job(True, [T_B, T_A, None], dedup=True)
    assert torch.equal(_i16(graphed.out), _i16(job.out))


def test_equal_variant_transforms_make_the_calls_and_graphs_of_the_shared_transform():
    shared, equal = _job(False, transforms=T_A, count_calls=True), _job(False, [T_A] * 3, count_calls=True)
    assert equal.state["variant_transforms"] is None and equal.state["vresample"] is None
    assert equal.state["transform"] == shared.state["transform"] == rs.TRANSFORMS_LAT
    tvp._same_calls(shared, equal, lambda n: n.endswith("_resampled_variants"))
    assert any(n.endswith("_resampled") for c in equal.step_calls for n in c)
    gs, ge = _job(True, transforms=T_A), _job(True, [T_A] * 3)
    assert gs.graphs == ge.graphs >= 3 and _keys(gs) == _keys(ge)
    assert torch.equal(_i16(gs.out), _i16(ge.out)) and torch.equal(_i16(gs.out), _i16(shared.out))


def test_identity_variant_transforms_make_the_calls_and_graphs_of_a_call_without_them():
    ident = [None, T_ID, [{}, None]]
    plain, same = _job(False, count_calls=True), _job(False, ident, count_calls=True)
    st = same.state
    assert st["variant_transforms"] is None and st["transform"] is None and st["placement"] is None and st["variant_placements"] is None
    tvp._same_calls(plain, same, lambda n: "_resampled" in n or "_placed" in n or n in ("mvoc_gather_planes_f16", "mvoc_shift_planes_f16"))
    gp, gs = _job(True), _job(True, ident)
    assert gp.graphs == gs.graphs >= 3 and _keys(gp) == _keys(gs)
    assert torch.equal(_i16(gp.out), _i16(gs.out)) and torch.equal(_i16(gp.out), _i16(plain.out))


def test_translation_only_variant_transforms_make_the_calls_and_graphs_of_variant_obj_offsets():
    moves = [[{"offset": tvp.OFF_A[0]}, {"offset": tvp.OFF_A[1], "scale": "2/2"}], None,
             [{"offset": tvp.OFF_B[0]}, {"offset": tvp.OFF_B[1]}]]
    older = _job(False, variant_offsets=[tvp.OFF_A, None, tvp.OFF_B], count_calls=True)
    same = _job(False, moves, count_calls=True)
    assert same.state["variant_transforms"] is None and same.state["variant_placements"] == older.state["variant_placements"] is not None
    tvp._same_calls(older, same, lambda n: "_resampled" in n or n == "mvoc_gather_planes_f16")
    assert any(n.endswith("_placed_variants") for c in same.step_calls for n in c)
    go, gs = _job(True, variant_offsets=[tvp.OFF_A, None, tvp.OFF_B]), _job(True, moves)
    assert go.graphs == gs.graphs >= 3 and _keys(go) == _keys(gs)
    assert torch.equal(_i16(go.out), _i16(gs.out)) and torch.equal(_i16(go.out), _i16(older.out))


def test_a_frame_sharded_pipeline_refuses_variant_transforms():
    with pytest.raises(RuntimeError, match="frame shard"):
        _job(False, [T_A, None, T_B], shard=True)


def test_the_call_refuses_argument_mixes_and_a_wrong_length():
    for kw in ({"transforms": T_A}, {"offsets": tvp.OFF_A}, {"variant_offsets": [tvp.OFF_A, None, tvp.OFF_B]}):
        with pytest.raises(ValueError, match="variant_obj_transforms is given together with"):
            _job(False, [T_A, None, T_B], **kw)
    with pytest.raises(ValueError, match="2 entries for 3 variants"):
        _job(False, [T_A, T_B])
    with pytest.raises(ValueError, match=r"variant 2: obj_transforms: object 1: flip 'x'"):
        _job(False, [T_A, None, [{}, {"flip": "x"}]])
