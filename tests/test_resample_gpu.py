"""GPU: scale and mirror of objects at composition time -- nearest resampling through per-axis index maps.

* kernels: ``mvoc_gather_planes_f16`` against torch indexing with zero fill; the ``_resampled`` blend entries against the EXISTING
  unplaced entries on inputs gathered beforehand in torch (object chunks gathered with zero fill, masks nearest-resized to H x W
  and zeroed where a map entry is -1) -- destination rows bit-identical (int16 views; no NaN / inf is planted), sources untouched;
  a translation-only table equals ``_placed``, the identity table the ``_variants`` / ``_variants_sel`` entries; every int32 table
  entry is safe; bad arguments refused.  Every case asserts that its result DIFFERS from the untransformed call: on a tree
  without the feature nothing here passes.
* engine: a transformed forward of the toy UNet against the same forward with ``ops.pnp_blend_tokens`` / ``pnp_blend_nchw``
  replaced by "gather in torch, call the unplaced entry, restore the sources".
* pipeline: graph replay against eager, an identity transform against a call without the argument and a translation-only one
  against the ``obj_offsets`` call (latents, C-ABI calls, graph variants), a frame-sharded pipeline refused, K = 2 variants under
  one transform, the fusion steps on gathered latents and masks.

Structure and helpers follow test_placement_gpu.py so that the files judge by the same bars.
"""
import contextlib
import ctypes as C
import itertools
import types

import pytest
import torch

import test_placement_gpu as tp
import test_variants_gpu as tv

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_i16 = tv._i16
_planted = tp._planted

# (nvar, active): one variant; two with every bit set; two with a partial mask
VARIANTS = ((1, 0b1), (2, 0b11), (2, 0b10))


def _gather_hw(src, ymap, xmap):
    """src [H, W, ...] -> out[y, x] = src[ymap[y], xmap[x]], or 0 where either index is -1"""
    ym, xm = torch.tensor(ymap, device=src.device), torch.tensor(xmap, device=src.device)
    out = src[ym.clamp(min=0)][:, xm.clamp(min=0)]
    keep = ((ym >= 0)[:, None] & (xm >= 0)[None, :]).view(len(ymap), len(xmap), *([1] * (src.dim() - 2)))
    return torch.where(keep, out, torch.zeros_like(out))  # (+0.0 where absent, also over a -0.0 source)


def _gather_last2(src, ymap, xmap):
    """src [..., H, W]"""
    return _gather_hw(src.movedim(-2, 0).movedim(-1, 1), ymap, xmap).movedim(1, -1).movedim(0, -2).contiguous()


def _spec_maps(nobj, H, W):
    """per object, per frame (F = 2) the maps of an H x W site, [nobj][F][H + W]: scale up 3/2 (second frame moved), scale
    down 1/2 (second frame gathered entirely out of the frame), a mirror in both axes with a translation, an anchor outside the
    frame with unequal scales and one mirrored axis"""
    from mvoc_amd import ops
    ax = lambda d, p, q, flip, a2, S: ops.level_axis_map(d, p, q, flip, a2, S, S)
    specs = [
        [((0, 3, 2, False, H), (0, 3, 2, False, W)), ((1, 3, 2, False, H), (-1, 3, 2, False, W))],
        [((0, 1, 2, False, H), (0, 1, 2, False, W)), ((2 * H + 3, 1, 2, False, H), (0, 1, 2, False, W))],
        [((1, 1, 1, True, H), (-1, 1, 1, True, W)), ((0, 1, 1, True, H), (2, 1, 1, False, W))],
        [((0, 2, 3, False, -3), (0, 3, 2, False, 2 * W + 3)), ((-1, 5, 4, True, H - 1), (0, 2, 3, False, -1))],
    ]
    rows = [[ax(*y, H) + ax(*x, W) for y, x in obj] for obj in specs[:nobj]]
    for j, obj in enumerate(rows):
        for f, r in enumerate(obj):  # one object is nowhere in one of its frames; every other (object, frame) shows some pixels
            assert (all(v == -1 for v in r[:H])) == ((j, f) == (1, 1)) and any(v >= 0 for v in r[H:]), (j, f, r)
    assert any(v >= 0 for v in rows[0][0]) and rows[0][0] != list(range(H)) + list(range(W))
    return rows


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32).cuda().contiguous()


def _masks_eff(masks, rows, H, W):
    """the masks of the gathered twin: nearest-resized to H x W, zero where the object's map says absent"""
    m = torch.nn.functional.interpolate(masks, size=(H, W), mode="nearest") if tuple(masks.shape[2:]) != (H, W) else masks.clone()
    for j, obj in enumerate(rows):
        for f, r in enumerate(obj):
            ym, xm = torch.tensor(r[:H], device=m.device), torch.tensor(r[H:], device=m.device)
            m[j, f] *= ((ym >= 0)[:, None] & (xm >= 0)[None, :]).to(m.dtype)
    return m.contiguous()


def _gather_chunk_tokens(chunk, layout, F, H, W, obj_rows):
    out = torch.zeros_like(chunk)
    vi, vo = tp._chunk_frames_tokens(chunk, layout, F, H, W), tp._chunk_frames_tokens(out, layout, F, H, W)
    for f, r in enumerate(obj_rows):
        vo[f] = _gather_hw(vi[f], r[:H], r[H:])
    return out


def _gather_chunk_nchw(chunk, obj_rows):
    """chunk [F, C, H, W]"""
    H = chunk.shape[2]
    return torch.stack([_gather_last2(chunk[f], r[:H], r[H:]) for f, r in enumerate(obj_rows)]).contiguous()


def _run_tokens(buf, layout, F, H, W, c, masks, base0, ndst, smap=None, nvar=1, active=None, **kw):
    from mvoc_amd import ops
    ld, hw = buf.stride(0), H * W
    fs, ps = tv._strides(layout, ld, F, hw)
    ops.pnp_blend_tokens(buf[:, :c], masks, x2=buf[:, c:2 * c], frames=F, height=H, width=W, channels=c, chunk_stride=F * hw * ld,
                         f_stride=fs, p_stride=ps, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=nvar, active=active, **kw)


def _tokens_direct(buf, layout, F, H, W, c, masks, base0, ndst, smap, nvar, active, maps):
    """the C entry itself; returns its status"""
    from mvoc_amd import ops
    ld, hw = buf.stride(0), H * W
    fs, ps = tv._strides(layout, ld, F, hw)
    d = ops._pnp_desc(buf[:, :c], buf[:, c:2 * c], masks, F * hw * ld, fs, ps, F, H, W, c, base0, ndst)
    nobj = masks.shape[0]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    return ops.lib.mvoc_pnp_blend_scatter_tokens_resampled(C.byref(d), nsrc, arr, nvar, active, None if maps is None else maps.data_ptr(),
                                                           ops._stream())


def _nchw_direct(x, masks, F, base0, ndst, smap, nvar, active, maps):
    from mvoc_amd import ops
    d = ops._pnp_desc(x, None, masks, 0, 0, 0, F, x.shape[2], x.shape[3], x.shape[1], base0, ndst)
    nobj = masks.shape[0]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    return ops.lib.mvoc_pnp_blend_scatter_nchw_resampled(C.byref(d), nsrc, arr, nvar, active, None if maps is None else maps.data_ptr(),
                                                         ops._stream())


# ---- gather kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nplane", [1, 4])
@pytest.mark.parametrize("hw", [(5, 7), (8, 8), (12, 23)])
def test_gather_planes_against_torch_indexing(hw, nplane):
    from mvoc_amd import ops
    h, w = hw
    F = 3
    g = torch.Generator().manual_seed(10 * h + nplane)
    n = nplane * F * h * w
    pad = 67
    ax = lambda d, p, q, flip, a2, S: ops.level_axis_map(d, p, q, flip, a2, S, S)
    junk = [-(2 ** 31), 2 ** 31 - 1, h, w, -7, max(h, w) + 1]
    cases = [
        [ax(0, 3, 2, False, h, h) + ax(0, 3, 2, False, w, w), ax(1, 1, 2, False, h, h) + ax(-2, 1, 2, True, w, w), ax(0, 1, 1, True, h, h) + ax(0, 1, 1, False, w, w)],
        [list(range(h)) + list(range(w)), ax(h + 2, 1, 1, False, h, h) + ax(0, 1, 1, False, w, w), ax(0, 64, 1, False, 3, h) + ax(0, 1, 64, True, 2 * w + 1, w)],
        # entries no rule of ours writes: every int32 value means "absent" unless it is a valid index
        [[junk[i % len(junk)] if i % 3 == 0 else (i * 5) % h for i in range(h)] + [junk[(i + 2) % len(junk)] if i % 4 == 1 else (i * 3) % w for i in range(w)]] * 3,
    ]
    for rows in cases:
        src_buf = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float16)
        src_buf[pad:pad + n] = _planted(torch.randn(n, generator=g).half(), g)
        src_buf = src_buf.cuda()
        src = src_buf[pad:pad + n].view(nplane, F, h, w)
        dst_buf = torch.full((n + 2 * pad,), 777.0, dtype=torch.float16, device="cuda")
        out = dst_buf[pad:pad + n].view(nplane, F, h, w)
        clean = [[v if 0 <= v < (h if i < h else w) else -1 for i, v in enumerate(r)] for r in rows]
        want = torch.stack([torch.stack([_gather_last2(src[pl, f], clean[f][:h], clean[f][h:]) for f in range(F)]) for pl in range(nplane)])
        got = ops.gather_planes(src if nplane > 1 else src[0], _table(rows), out=out if nplane > 1 else out[0])
        torch.cuda.synchronize()
        assert torch.equal(_i16(got.reshape(want.shape)), _i16(want)), rows
        assert not torch.isnan(out).any()
        assert bool((dst_buf[:pad] == 777).all()) and bool((dst_buf[pad + n:] == 777).all())  # nothing outside the extent
        assert torch.isnan(src_buf[:pad]).all() and torch.isnan(src_buf[pad + n:]).all()


def test_gather_planes_refuses_bad_arguments_and_writes_nothing():
    from mvoc_amd import ops
    src = torch.ones(2, 2, 3, 4, dtype=torch.float16, device="cuda")
    dst = torch.zeros_like(src)
    tab = _table([list(range(3)) + list(range(4))] * 2)
    call = lambda s, d, t, dims=(2, 2, 3, 4): ops.lib.mvoc_gather_planes_f16(s, d, *dims, t, ops._stream())
    err = lambda: ops.lib.mvoc_last_error().decode()
    assert call(None, dst.data_ptr(), tab.data_ptr()) == -1 and "null" in err()
    assert call(src.data_ptr(), None, tab.data_ptr()) == -1 and "null" in err()
    assert call(src.data_ptr(), dst.data_ptr(), None) == -1 and "null" in err()
    assert call(src.data_ptr(), src.data_ptr(), tab.data_ptr()) == -1 and "in place" in err()
    for dims in ((0, 2, 3, 4), (2, 0, 3, 4), (2, 2, -1, 4), (2, 2, 3, 0)):
        assert call(src.data_ptr(), dst.data_ptr(), tab.data_ptr(), dims) == -1 and "dims" in err()
    with pytest.raises(RuntimeError, match="maps must be"):
        ops.gather_planes(src, tab[:1])
    with pytest.raises(RuntimeError, match="maps must be"):
        ops.gather_planes(src, _table([list(range(3)) + list(range(3))] * 2))
    with pytest.raises(RuntimeError, match="maps"):
        ops.gather_planes(src, tab.float())
    with pytest.raises(RuntimeError, match="out must be"):
        ops.gather_planes(src, tab, out=dst[:1])
    torch.cuda.synchronize()
    assert not dst.any() and bool((src == 1).all())
    assert call(src.data_ptr(), dst.data_ptr(), tab.data_ptr()) == 0 and torch.equal(dst, src)


# ---- tokens -------------------------------------------------------------------------------------------------------------
def _expect_tokens(comp0, layout, F, H, W, c, masks, base0, ndst, smap, K, active, rows):
    """chunk index -> the rows the resampled entry must leave there: per injecting variant the POSITIONAL entry on that variant's
    own batch [bg, gathered obj_1.., (u_k,) c_k]; an idle variant's chunks as they were"""
    nobj, nrow = masks.shape[0], F * H * W
    nsrc = nobj + 1 if smap is None else smap[0]
    order = tv._src_order(smap, nobj)
    chunk = lambda t, i: t[i * nrow:(i + 1) * nrow]
    meff = _masks_eff(masks, rows, H, W)
    exp = {}
    for k in range(K):
        dst = [nsrc + d * K + k for d in range(ndst)]
        if not (active >> k) & 1:
            exp.update({i: chunk(comp0, i) for i in dst})
            continue
        parts = [chunk(comp0, order[0])] + [_gather_chunk_tokens(chunk(comp0, order[1 + j]).contiguous(), layout, F, H, W, rows[j])
                                            for j in range(nobj)] + [chunk(comp0, i) for i in dst]
        full = torch.cat(parts).contiguous()
        tv._run_tokens(full, layout, F, H, W, c, meff, base0, ndst)
        exp.update({i: chunk(full, nobj + 1 + d).clone() for d, i in enumerate(dst)})
    return exp


@pytest.mark.parametrize("layout", ["spatial", "temporal"])
@pytest.mark.parametrize("geo", [(4, 6, None), (4, 6, (8, 12)), (3, 5, (5, 9))], ids=["4x6-same", "4x6-mask8x12", "3x5-mask5x9"])
def test_tokens_resampled_equal_the_existing_entries_on_gathered_inputs(geo, layout):
    H, W, mres = geo
    mh, mw = mres or (H, W)
    F, c = 2, 16
    nrow = F * H * W
    g = torch.Generator().manual_seed(11 * H + W + (layout == "temporal"))
    n = 0
    for nobj in (1, 2, 3, 4):
        rows = _spec_maps(nobj, H, W)
        maps = _table(rows)
        for ndst, base0, (K, active), smap in itertools.product((1, 2), (False, True), VARIANTS, tp._maps(nobj)):
            masks = tv._masks(nobj, F, mh, mw, soft=bool(n % 2), g=g)
            nsrc = nobj + 1 if smap is None else smap[0]
            comp = _planted(torch.randn((nsrc + ndst * K) * nrow, 3 * c, generator=g).half(), g).cuda()
            comp0 = comp.clone()
            what = (nobj, ndst, base0, K, bin(active), smap)
            exp = _expect_tokens(comp0, layout, F, H, W, c, masks, base0, ndst, smap, K, active, rows)
            _run_tokens(comp, layout, F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, resample=maps)
            chunk = lambda t, i: t[i * nrow:(i + 1) * nrow]
            for i, want in exp.items():
                assert torch.equal(_i16(chunk(comp, i)[:, :2 * c]), _i16(want[:, :2 * c])), (what, i)
            assert torch.equal(_i16(comp[:nsrc * nrow]), _i16(comp0[:nsrc * nrow])), what  # sources untouched
            assert torch.equal(_i16(comp[:, 2 * c:]), _i16(comp0[:, 2 * c:])), what  # v columns untouched
            # the untransformed call on the same inputs writes something else: the maps matter
            plain = comp0.clone()
            _run_tokens(plain, layout, F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active)
            assert not torch.equal(_i16(plain[nsrc * nrow:]), _i16(comp[nsrc * nrow:])), what
            n += 1
    assert n == (1 + 3 * 2) * 2 * 2 * len(VARIANTS)


# ---- NCHW -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 8), (3, 5)])  # hw % 8 == 0: 8 pixels per work item / else 1
def test_nchw_resampled_equal_the_existing_entries_on_gathered_inputs(hw):
    from mvoc_amd import ops
    H, W = hw
    F, Cc = 2, 4
    g = torch.Generator().manual_seed(500 + W)
    n = 0
    for nobj in (1, 2, 3, 4):
        rows = _spec_maps(nobj, H, W)
        maps = _table(rows)
        for ndst, base0, (K, active), smap, mres in itertools.product((1, 2), (False, True), VARIANTS, tp._maps(nobj), ("same", "other")):
            mh, mw = (H, W) if mres == "same" else (2 * H, W + 1)
            masks = tv._masks(nobj, F, mh, mw, soft=bool(n % 2), g=g)
            meff = _masks_eff(masks, rows, H, W)
            nsrc = nobj + 1 if smap is None else smap[0]
            order = tv._src_order(smap, nobj)
            comp = _planted(torch.randn((nsrc + ndst * K) * F, Cc, H, W, generator=g).half(), g).cuda()
            comp0 = comp.clone()
            chunk = lambda t, i: t[i * F:(i + 1) * F]
            what = (nobj, ndst, base0, K, bin(active), smap, mres)
            ops.pnp_blend_nchw(comp, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=maps)
            for k in range(K):
                dst = [nsrc + d * K + k for d in range(ndst)]
                if not (active >> k) & 1:
                    for i in dst:
                        assert torch.equal(_i16(chunk(comp, i)), _i16(chunk(comp0, i))), (what, k)
                    continue
                parts = [chunk(comp0, order[0])] + [_gather_chunk_nchw(chunk(comp0, order[1 + j]), rows[j]) for j in range(nobj)]
                full = torch.cat(parts + [chunk(comp0, i) for i in dst]).contiguous()
                ops.pnp_blend_nchw(full, meff, frames=F, base_chunk0=base0, ndst=ndst)
                for d, i in enumerate(dst):
                    assert torch.equal(_i16(chunk(comp, i)), _i16(chunk(full, nobj + 1 + d))), (what, k, d)
            assert torch.equal(_i16(comp[:nsrc * F]), _i16(comp0[:nsrc * F])), what
            plain = comp0.clone()
            ops.pnp_blend_nchw(plain, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active)
            assert not torch.equal(_i16(plain[nsrc * F:]), _i16(comp[nsrc * F:])), what
            n += 1
    assert n == (1 + 3 * 2) * 2 * 2 * len(VARIANTS) * 2


# ---- equivalences -----------------------------------------------------------------------------------------------------------
def _shift_rows(offs, H, W):
    """the maps that say what an offset table says: ymap[y] = y - dfy, xmap[x] = x - dfx, -1 outside"""
    ax = lambda d, S: [i - d if 0 <= i - d < S else -1 for i in range(S)]
    return [[ax(dy, H) + ax(dx, W) for dy, dx in obj] for obj in offs]


def test_a_translation_only_table_returns_the_bits_of_the_placed_entries():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(21)
    F, c = 2, 16
    for (H, W), nobj, ndst, base0, (K, active) in itertools.product(((4, 8), (3, 5)), (1, 4), (1, 2), (False, True), VARIANTS):
        nrow = F * H * W
        offs = tp._offsets(nobj, H, W)
        place, maps = tp._table(offs), _table(_shift_rows(offs, H, W))
        for smap in tp._maps(nobj):
            masks = tv._masks(nobj, F, 5, 9, True, g)
            nsrc = nobj + 1 if smap is None else smap[0]
            what = (H, W, nobj, ndst, base0, K, active, smap)
            comp = _planted(torch.randn((nsrc + ndst * K) * nrow, 3 * c, generator=g).half(), g).cuda()
            twin = comp.clone()
            _run_tokens(comp, "temporal", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, resample=maps)
            _run_tokens(twin, "temporal", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, place=place)
            assert torch.equal(_i16(comp), _i16(twin)), what
            x = _planted(torch.randn((nsrc + ndst * K) * F, 4, H, W, generator=g).half(), g).cuda()
            y = x.clone()
            ops.pnp_blend_nchw(x, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=maps)
            ops.pnp_blend_nchw(y, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=place)
            assert torch.equal(_i16(x), _i16(y)), what


def test_the_identity_table_returns_the_bits_of_the_variants_entries():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(22)
    F, H, W, c = 2, 3, 5, 16
    nrow = F * H * W
    for nobj, ndst, base0, (K, active) in itertools.product((1, 3), (1, 2), (False, True), VARIANTS):
        ident = _table([[list(range(H)) + list(range(W))] * F] * nobj)
        for smap in tv._maps(nobj)[:3]:
            masks = tv._masks(nobj, F, 5, 9, True, g)
            nsrc = nobj + 1 if smap is None else smap[0]
            comp = _planted(torch.randn((nsrc + ndst * K) * nrow, 3 * c, generator=g).half(), g).cuda()
            twin = comp.clone()
            _run_tokens(comp, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, resample=ident)
            _run_tokens(twin, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active)
            assert torch.equal(_i16(comp), _i16(twin)), (nobj, ndst, base0, K, active, smap)
            for hw in ((4, 8), (3, 5)):
                idt = _table([[list(range(hw[0])) + list(range(hw[1]))] * F] * nobj)
                x = _planted(torch.randn((nsrc + ndst * K) * F, 4, *hw, generator=g).half(), g).cuda()
                y = x.clone()
                ops.pnp_blend_nchw(x, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, resample=idt)
                ops.pnp_blend_nchw(y, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active)
                assert torch.equal(_i16(x), _i16(y)), (nobj, ndst, base0, K, active, smap, hw)


# ---- safety -------------------------------------------------------------------------------------------------------------
def test_every_int32_table_entry_is_safe_and_means_absent():
    """entries the rule never writes (INT32_MIN, INT32_MAX, H, W, -7): the objects are absent there, the result is the base blended
    with zero objects under zero masks; with one valid axis the other axis alone decides"""
    from mvoc_amd import ops
    F, H, W, c = 2, 3, 5, 16
    nrow = F * H * W
    g = torch.Generator().manual_seed(4)
    masks = tv._masks(2, F, H, W, False, g)
    lo, hi = -(2 ** 31), 2 ** 31 - 1
    bad_y, bad_x = [lo, hi, H], [W, -7, hi, lo, W + 1]
    rows = [[bad_y + list(range(W)), list(range(H)) + bad_x], [bad_y + bad_x, [hi] * H + [lo] * W]]
    maps = _table(rows)
    comp = _planted(torch.randn(5 * nrow, 3 * c, generator=g).half(), g).cuda()
    comp0, twin = comp.clone(), comp.clone()
    _run_tokens(comp, "spatial", F, H, W, c, masks, True, 2, resample=maps)
    twin[nrow:3 * nrow] = 0.0
    _run_tokens(twin, "spatial", F, H, W, c, torch.zeros_like(masks), True, 2)
    assert torch.equal(_i16(comp[3 * nrow:]), _i16(twin[3 * nrow:]))
    assert torch.equal(_i16(comp[:3 * nrow]), _i16(comp0[:3 * nrow]))
    for hw in ((4, 8), (3, 5)):
        h, w = hw
        by, bx = [lo, hi, h, -7][:h] + [h] * max(0, h - 4), ([w, -7, hi, lo] * 2)[:w]
        nmaps = _table([[by + list(range(w)), list(range(h)) + bx], [by + bx, [hi] * h + [lo] * w]])
        m2 = tv._masks(2, F, h, w, True, g)
        x = _planted(torch.randn(5 * F, 4, h, w, generator=g).half(), g).cuda()
        x0, y = x.clone(), x.clone()
        ops.pnp_blend_nchw(x, m2, frames=F, base_chunk0=True, ndst=2, resample=nmaps)
        y[F:3 * F] = 0.0
        ops.pnp_blend_nchw(y, torch.zeros_like(m2), frames=F, base_chunk0=True, ndst=2)
        assert torch.equal(_i16(x[3 * F:]), _i16(y[3 * F:])) and torch.equal(_i16(x[:3 * F]), _i16(x0[:3 * F])), hw


def test_a_negative_zero_base_becomes_positive_zero_where_the_object_is_absent():
    """value 0 and mask 0 enter blend16: -0.0 * 1 + 0 * 0 = +0.0, as under the positional kernel with a zero object and mask"""
    from mvoc_amd import ops
    F, H, W, c = 2, 4, 6, 16
    nrow = F * H * W
    masks = torch.ones(1, F, H, W, dtype=torch.float16, device="cuda")
    comp = torch.randn(4 * nrow, 3 * c, generator=torch.Generator().manual_seed(2)).half().cuda()  # [bg, obj, u, c]
    comp[3 * nrow:] = -0.0  # the base (the last chunk)
    twin = comp.clone()
    rows = [[[-1] * H + list(range(W)), list(range(H)) + [-1] * W]]  # absent in both frames: one axis each
    _run_tokens(comp, "spatial", F, H, W, c, masks, False, 2, resample=_table(rows))
    for i in (2, 3):
        assert bool((_i16(comp[i * nrow:(i + 1) * nrow, :2 * c]) == 0).all())  # +0.0: no sign bit
    twin[nrow:2 * nrow] = 0.0  # the absent object
    _run_tokens(twin, "spatial", F, H, W, c, torch.zeros_like(masks), False, 2)
    assert torch.equal(_i16(twin[2 * nrow:]), _i16(comp[2 * nrow:]))
    x = torch.randn(4 * F, 4, 4, 8, generator=torch.Generator().manual_seed(3)).half().cuda()
    x[3 * F:] = -0.0
    m = torch.ones(1, F, 4, 8, dtype=torch.float16, device="cuda")
    ops.pnp_blend_nchw(x, m, frames=F, base_chunk0=False, ndst=2, resample=_table([[[-1] * 4 + list(range(8)), list(range(4)) + [-1] * 8]]))
    assert bool((_i16(x[2 * F:]) == 0).all())


def test_resampled_entries_refuse_bad_arguments_and_write_nothing():
    from mvoc_amd import ops
    F, H, W, c = 2, 4, 4, 8
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    buf = torch.zeros(9 * F * H * W, 3 * c, dtype=torch.float16, device="cuda")
    nchw = torch.zeros(9 * F, 4, H, W, dtype=torch.float16, device="cuda")
    maps = _table(_spec_maps(2, H, W))
    err = lambda: ops.lib.mvoc_last_error().decode()
    cases = [  # (nvar, active, map, table, base_chunk0, text)
        (0, 1, None, maps, None, "nvar 0"), (9, 1, None, maps, None, "nvar 9"),
        (3, 0, None, maps, None, "active mask 0x0"), (3, 8, None, maps, None, "active mask 0x8"), (1, 2, None, maps, None, "active mask 0x2"),
        (2, 3, (0, (0, 0)), maps, None, "nsrc 0"), (2, 3, (2, (0, 2)), maps, None, "obj_chunk[1] = 2"),
        (2, 3, (2, (-1, 0)), maps, None, "obj_chunk[0] = -1"),
        (2, 3, None, None, None, "null map table"),
        (1, 1, (2, (0, 1)), maps, -1, "base_chunk0 = -1"),
    ]
    for nvar, active, smap, tab, b0, text in cases:
        assert _tokens_direct(buf, "spatial", F, H, W, c, masks, False if b0 is None else b0, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
        assert _nchw_direct(nchw, masks, F, True if b0 is None else b0, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
    # a valid call with the same buffers goes through (the refusals above were about the arguments)
    assert _tokens_direct(buf, "spatial", F, H, W, c, masks, False, 2, None, 3, 0b111, maps) == 0, err()
    assert _nchw_direct(nchw, masks, F, True, 2, None, 1, 1, maps) == 0, err()
    # the Python layer: the table's form, and the arguments a resample table does not combine with
    with pytest.raises(RuntimeError, match=r"int32 \[nobj = 2, F = 2, H \+ W = 8\]"):
        _run_tokens(buf, "spatial", F, H, W, c, masks, False, 2, nvar=2, resample=maps[:1])
    with pytest.raises(RuntimeError, match=r"int32 \[nobj = 2, F = 2, H \+ W = 8\]"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, resample=maps[:, :, :7].contiguous())
    with pytest.raises(RuntimeError, match="resample"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, nvar=2, resample=maps.long())
    place = tp._table([[(1, 1), (0, -1)], [(2, 0), (0, 0)]])
    with pytest.raises(RuntimeError, match="resample= and place= are both given"):
        _run_tokens(buf, "spatial", F, H, W, c, masks, False, 2, resample=maps, place=place)
    with pytest.raises(RuntimeError, match="resample= and place= are both given"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, resample=maps, place=place)
    stack = torch.stack([masks, masks]).contiguous()
    with pytest.raises(RuntimeError, match="does not take a .* mask stack"):
        _run_tokens(buf, "spatial", F, H, W, c, stack, False, 2, nvar=2, resample=maps)
    with pytest.raises(RuntimeError, match="does not take a .* mask stack"):
        ops.pnp_blend_nchw(nchw, stack, frames=F, ndst=2, nvar=2, resample=maps)
    with pytest.raises(RuntimeError, match="no_background"):
        _run_tokens(buf, "spatial", F, H, W, c, masks, False, 2, resample=maps, no_background=True)
    with pytest.raises(RuntimeError, match="storage ends"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, nvar=4, resample=maps)  # 3 + 8 chunks in a buffer of 9
    torch.cuda.synchronize()
    assert not buf.any() and not nchw.any()  # zeros blended with zeros: nothing but zeros was ever written


def test_profiler_counts_the_placed_bytes_and_the_table():
    from mvoc_amd import ops
    F, H, W, c, K = 2, 4, 4, 8, 3
    nrow = F * H * W
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    place = tp._table([[(1, 0), (0, 1)], [(0, 0), (-1, -1)]])
    maps = _table(_spec_maps(2, H, W))
    ops.prof_enable(True)
    try:
        for base0, ndst, smap, active in ((True, 2, None, 0b101), (False, 1, (2, (1, 1)), 0b100)):
            nsrc = 3 if smap is None else smap[0]
            work = []
            for kw in ({"place": place}, {"resample": maps}):
                buf = torch.zeros((nsrc + ndst * K) * nrow, 3 * c, dtype=torch.float16, device="cuda")
                nchw = torch.zeros((nsrc + ndst * K) * F, c, H, W, dtype=torch.float16, device="cuda")
                ops.prof_reset()
                _run_tokens(buf, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, **kw)
                torch.cuda.synchronize()
                t = ops.prof_collect()["pnp"]
                ops.prof_reset()
                ops.pnp_blend_nchw(nchw, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, **kw)
                torch.cuda.synchronize()
                n = ops.prof_collect()["pnp"]
                assert t["launches"] == 1 and n["launches"] == 1
                work.append((t["work"], n["work"]))
            table_bytes = 4 * 2 * F * (H + W)
            assert work[1][0] == work[0][0] + table_bytes and work[1][1] == work[0][1] + table_bytes, (base0, ndst, smap, active, work)
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


# ---- engine -------------------------------------------------------------------------------------------------------------
class _PreGather:
    """``ops.pnp_blend_tokens`` / ``pnp_blend_nchw`` replaced by: gather the object chunks in torch (zero fill), call the unplaced
    entry with the masks resized and zeroed where the map says absent, restore the source chunks"""

    def __init__(self):
        from mvoc_amd import ops
        self.ops, self.orig, self.calls = ops, (ops.pnp_blend_tokens, ops.pnp_blend_nchw), []

    def __enter__(self):
        self.ops.pnp_blend_tokens, self.ops.pnp_blend_nchw = self.tokens, self.nchw
        return self

    def __exit__(self, *exc):
        self.ops.pnp_blend_tokens, self.ops.pnp_blend_nchw = self.orig

    def tokens(self, x, masks, **kw):
        maps = kw.pop("resample")
        rows = maps.cpu().tolist()
        F, H, W, c = kw["frames"], kw["height"], kw["width"], kw["channels"]
        nobj = masks.shape[0]
        assert kw.get("src_map") is None and "place" not in kw and tuple(maps.shape) == (nobj, F, H + W)
        nchunk = nobj + 1 + kw["ndst"] * kw.get("nvar", 1)
        self.calls.append(("tokens", H, W, rows))
        saved = []
        for t in (x, kw.get("x2")):
            if t is None:
                continue
            v = torch.as_strided(t, (nchunk, F, H, W, c), (kw["chunk_stride"], kw["f_stride"], kw["p_stride"] * W, kw["p_stride"], 1),
                                 t.storage_offset())
            keep = v[1:nobj + 1].clone()
            saved.append((v, keep))
            for j in range(nobj):
                for f, r in enumerate(rows[j]):
                    v[1 + j, f] = _gather_hw(keep[j, f], r[:H], r[H:])
        out = self.orig[0](x, _masks_eff(masks, rows, H, W), **kw)
        for v, keep in saved:
            v[1:nobj + 1] = keep
        return out

    def nchw(self, x, masks, **kw):
        maps = kw.pop("resample")
        rows = maps.cpu().tolist()
        F, (H, W), nobj = kw["frames"], x.shape[2:], masks.shape[0]
        assert kw.get("src_map") is None and kw.get("x2") is None and "place" not in kw
        self.calls.append(("nchw", H, W, rows))
        keep = x[F:(nobj + 1) * F].clone()
        for j in range(nobj):
            x[(1 + j) * F:(2 + j) * F] = _gather_chunk_nchw(keep[j * F:(j + 1) * F], rows[j])
        out = self.orig[1](x, _masks_eff(masks, rows, H, W), **kw)
        x[F:(nobj + 1) * F] = keep
        return out


# scale 3/2 mirrored left-right on a per-frame path; scale 1/2 in y only, mirrored top-bottom about an off-centre anchor
ENGINE_TRANSFORM = ((3, 2, 3, 2, False, True, 8, 8, ((1, -2), (0, 1), (-2, 0))), (1, 2, 1, 1, True, False, 6, 10, ((1, 0),) * 3))


@pytest.mark.parametrize("kind", ["qk", "conv_out", "features"])
def test_unet_transformed_forward_equals_the_pregathered_unplaced_forward(kind):
    """one Q/K step (spatial + temporal sites, the source tail pruned), one conv_out step (prune_dead_chunks: the NCHW blend on
    the source chunks' outputs) and, with prune_dead_chunks off, the same step through the resnet / temporal-conv feature sites"""
    from mvoc_amd import ops, pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    F, h, w, cd = 3, 8, 8, 64
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    tr = ENGINE_TRANSFORM
    moved, table = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False).transform_masks(masks, tr)
    lat_rows = ops.transform_maps(tr, h, w, h, w)
    assert table.tolist() == lat_rows and table.dtype == torch.int32
    for j in range(2):  # the masks in destination coordinates: both forms, every channel, types kept
        for a, b in zip(moved[j], masks[j]):
            assert a.dtype == b.dtype and a.shape == b.shape
            for f, r in enumerate(lat_rows[j]):
                assert torch.equal(a[0, :, f], _gather_last2(b[0, :, f], r[:h], r[h:]))
        assert not torch.equal(moved[j][0], masks[j][0])
    roles = tv._roles(F, h, w, cd, 4, 1)
    pipe, (t_feat, t_qk) = tv._arm(eng, 5)
    t = t_qk if kind == "qk" else t_feat
    names = ["S", "O", "P", "u0", "c0"]
    saved = eng.prune_dead_chunks

    def forward(transform):
        eng.transform, eng.prune_source_tail, eng.prune_dead_chunks = transform, True, kind != "features"
        try:
            return tv._fwd(eng, tv._batch(roles, names), t)
        finally:
            eng.transform, eng.prune_source_tail, eng.prune_dead_chunks = None, False, saved

    try:
        pnp_utils.register_time_all(pipe, t, moved)
        got = forward(tr)
        with _PreGather() as pre:
            ref = forward(tr)
        plain = forward(None)
    finally:
        tv._disarm(eng, pipe)
    torch.cuda.synchronize()
    sites = {c[:3] for c in pre.calls}
    if kind == "qk":
        assert {s[0] for s in sites} == {"tokens"} and {s[1:] for s in sites} == {(8, 8), (4, 4), (2, 2)}, sites
    elif kind == "conv_out":
        assert sites == {("nchw", 8, 8)} and len(pre.calls) == 1, sites
    else:
        assert ("nchw", 8, 8) in sites and ("tokens", 8, 8) in sites, sites
    for c in pre.calls:  # every site was handed the maps of its own level
        assert c[3] == ops.transform_maps(tr, c[1], c[2], h, w), c[:3]
    assert torch.equal(_i16(got[3:]), _i16(ref[3:])), kind
    assert torch.isfinite(got[3:]).all() and not torch.equal(got[3:], plain[3:]), kind  # the transform moved something
    assert eng.transform is None and len(eng._level_tables["transform"][1]) == len({c[1:3] for c in pre.calls})


def test_unet_refuses_a_transform_with_a_shard_a_placement_or_a_wrong_object_count():
    F, h, w = 3, 8, 8
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    eng.transform = ENGINE_TRANSFORM
    try:
        eng.shard = types.SimpleNamespace(rank=0, world=1)
        with pytest.raises(RuntimeError, match="frame shard"):
            eng.pnp_batch(5, masks)
        with pytest.raises(RuntimeError, match="frame shard"):
            eng.place_kw(masks, 8, 8)
        eng.shard = None
        eng.placement = (((1, 0),) * F, ((0, 1),) * F)
        with pytest.raises(RuntimeError, match="together with placement"):
            eng.place_kw(masks, 8, 8)
        eng.placement = None
        with pytest.raises(RuntimeError, match="transform holds 2 objects, the hooks carry 1 masks"):
            eng.place_kw(masks[:1], 8, 8)
        tab = eng.place_kw(masks, 4, 4)["resample"]
        assert tuple(tab.shape) == (2, F, 8) and tab.dtype == torch.int32 and tab.is_cuda
        assert eng.place_kw(masks, 4, 4)["resample"] is tab  # cached per level
    finally:
        eng.transform, eng.placement, eng.shard = None, None, None
    assert eng.place_kw(masks, 8, 8) == {}


# ---- pipeline -----------------------------------------------------------------------------------------------------------
TRANSFORMS = [{"scale": "3/2", "flip": "h", "offset": tp.PATH}, {"scale": [1, 0.5], "flip": "v", "anchor": [40, 24], "offset": (-16, 8)}]
TRANSFORMS_LAT = ((3, 2, 3, 2, False, True, 8, 8, ((0, 1), (-1, 2), (-2, 3))), (1, 2, 1, 1, True, False, 6, 10, ((1, -2),) * 3))
SAMPLE = "sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection"


@contextlib.contextmanager
def _with_transforms(transforms):
    """test_placement_gpu.py's toy job passes ``obj_offsets``; here its sampling call is handed ``obj_transforms`` as well"""
    from mvoc_amd.pipeline import I2VGenXLPipeline
    orig = getattr(I2VGenXLPipeline, SAMPLE)

    def call(self, *a, **kw):
        return orig(self, *a, obj_transforms=transforms, **kw)

    setattr(I2VGenXLPipeline, SAMPLE, call)
    try:
        yield
    finally:
        setattr(I2VGenXLPipeline, SAMPLE, orig)


def _job(graphs, transforms=None, **kw):
    if transforms is None:
        return tp._placed_job(graphs, **kw)
    with _with_transforms(transforms):
        return tp._placed_job(graphs, **kw)


def _graph_keys(st):
    """the keys of a state's captured iterations without the mask key (entry 1: the device addresses of that job's masks)"""
    return {k[:1] + k[2:] for k in st["variants"]}


def test_transformed_composition_graph_replay_equals_eager_and_moves_the_result():
    from mvoc_amd import ops
    eager = _job(False, TRANSFORMS, count_calls=True)
    st = eager.state
    assert st["transform"] == TRANSFORMS_LAT and st["placement"] is None and st["place_dev"] is None
    rows = ops.transform_maps(TRANSFORMS_LAT, 8, 8, 8, 8)
    assert st["resample_dev"].tolist() == rows
    # the call's masks, everywhere, are the gathered ones: built once, in destination coordinates
    for j in range(2):
        for f, r in enumerate(rows[j]):
            want = _gather_last2(eager.masks[j][0][0, 0, f].cuda(), r[:8], r[8:])
            assert torch.equal(st["fusion_masks"][j, 0, 0, f], want) and torch.equal(st["masks"][j][0][0, 0, f].cuda().half(), want)
            assert torch.equal(st["masks"][j][1][0, 0, f].cuda(), _gather_last2(eager.masks[j][1][0, 0, f].cuda(), r[:8], r[8:]))
    # the per-level tables (8 x 8, 4 x 4, 2 x 2) stay alive with the state, whose graphs would read them
    assert len(st["place_tables"]) == 1 and {k[:2] for k in st["place_tables"][0]} == {(8, 8), (4, 4), (2, 2)}
    names = set().union(*eager.step_calls)
    assert {"mvoc_pnp_blend_scatter_tokens_resampled", "mvoc_pnp_blend_scatter_nchw_resampled", "mvoc_gather_planes_f16"} <= names
    assert not any(n.startswith("mvoc_pnp_blend") and not n.endswith("_resampled") for n in names), names
    assert "mvoc_shift_planes_f16" not in names
    # two fusion steps: the two fusion objects go through the gather kernel instead of a copy
    assert [c.get("mvoc_gather_planes_f16", 0) for c in eager.step_calls] == [2, 2, 0, 0, 0]
    graphed = _job(True, TRANSFORMS)
    assert torch.equal(graphed.out, eager.out) and torch.isfinite(eager.out).all()
    assert any("transform" in k for k in graphed.state["variants"])  # the transform is part of the graph-variant key
    plain = _job(False)
    assert plain.out.shape == eager.out.shape and not torch.equal(plain.out, eager.out)
    moved_only = _job(False, offsets=[tp.PATH, (-16, 8)])  # the same offsets without scale and mirror: another result
    assert not torch.equal(moved_only.out, eager.out)


def test_an_identity_transform_makes_the_calls_and_graphs_of_a_call_without_it():
    ident = [{"scale": 1.0, "flip": None, "offset": [(0, 0)] * 3, "anchor": [8, 16]}, {}]
    plain, same = _job(False, count_calls=True), _job(False, ident, count_calls=True)
    assert same.state["transform"] is None and same.state["placement"] is None and same.state["resample_dev"] is None
    assert len(plain.step_calls) == len(same.step_calls) == 5
    for i, (a, b) in enumerate(zip(plain.step_calls, same.step_calls)):
        assert a == b and sum(a.values()) > 0, (i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
        assert not any(n.endswith("_resampled") or n.endswith("_placed") or n == "mvoc_gather_planes_f16" for n in b)
    assert torch.equal(plain.out, same.out)
    gp, gs = _job(True), _job(True, ident)
    assert gp.graphs == gs.graphs >= 3 and torch.equal(gp.out, gs.out) and torch.equal(gp.out, plain.out)
    assert _graph_keys(gp.state) == _graph_keys(gs.state)  # the same graph keys


def test_a_translation_only_transform_makes_the_calls_and_graphs_of_the_obj_offsets_call():
    moves = [{"offset": tp.OFFSETS[0]}, {"offset": tp.OFFSETS[1], "scale": "2/2"}]
    placed, same = _job(False, offsets=tp.OFFSETS, count_calls=True), _job(False, moves, count_calls=True)
    assert same.state["transform"] is None and same.state["placement"] == placed.state["placement"] is not None
    for i, (a, b) in enumerate(zip(placed.step_calls, same.step_calls)):
        assert a == b and sum(a.values()) > 0, (i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
        assert not any(n.endswith("_resampled") or n == "mvoc_gather_planes_f16" for n in b)
    assert any(n.endswith("_placed") for c in same.step_calls for n in c)
    assert torch.equal(placed.out, same.out)
    gp, gs = _job(True, offsets=tp.OFFSETS), _job(True, moves)
    assert gp.graphs == gs.graphs and _graph_keys(gp.state) == _graph_keys(gs.state) and torch.equal(gp.out, gs.out)
    assert torch.equal(gp.out, placed.out)


def test_a_frame_sharded_pipeline_refuses_transforms():
    with pytest.raises(RuntimeError, match="frame shard"):
        _job(False, TRANSFORMS, shard=True)


def test_offsets_next_to_transforms_are_refused():
    with pytest.raises(ValueError, match="obj_transforms is given together with obj_offsets"):
        _job(False, TRANSFORMS, offsets=tp.OFFSETS)


def test_two_variants_share_one_transform():
    moved, plain = _job(True, TRANSFORMS, K=2), _job(True, K=2)
    assert moved.out.shape[0] == 2 and torch.isfinite(moved.out).all()
    assert moved.state["nvar"] == 2 and moved.state["transform"] == TRANSFORMS_LAT
    assert moved.graphs == plain.graphs  # the transform is one more part of the key, not one more step kind
    for k in range(2):
        assert not torch.equal(moved.out[k], plain.out[k]), k
    assert not torch.equal(moved.out[0], moved.out[1])
    eager = _job(False, TRANSFORMS, K=2)
    assert torch.equal(eager.out, moved.out)


def test_fusion_steps_use_the_gathered_latents_and_masks():
    from mvoc_amd import ops
    from mvoc_amd.schedulers import DDIMScheduler
    seen, orig = [], ops.latent_fusion

    def fusion(latents, bg, objs, masks, *a, **kw):
        seen.append((objs.clone(), masks.clone()))
        return orig(latents, bg, objs, masks, *a, **kw)

    ops.latent_fusion = fusion
    try:
        job = _job(False, TRANSFORMS)
    finally:
        ops.latent_fusion = orig
    assert len(seen) == 2  # fusion_steps = (0, 2)
    s = DDIMScheduler()
    s.set_timesteps(5)
    t0 = int(s.timesteps[0])  # both fusion steps read the objects' latents of the first timestep (the reference's counter stays 0)
    rows = ops.transform_maps(TRANSFORMS_LAT, 8, 8, 8, 8)
    for objs, masks in seen:
        for j, d in enumerate(("/virtual/o1", "/virtual/o2")):
            lat = job.pipe.latent_cache.get(d, t0).cuda().half()
            for f, r in enumerate(rows[j]):
                assert torch.equal(_i16(objs[j, 0, :, f]), _i16(_gather_last2(lat[0, :, f], r[:8], r[8:]))), (j, f)
                assert torch.equal(masks[j, 0, :, f], _gather_last2(job.masks[j][0][0, :, f].cuda(), r[:8], r[8:])), (j, f)
            assert not torch.equal(objs[j], lat)
