"""GPU: placement of objects at composition time -- per-frame integer translation.

* kernels: ``mvoc_shift_planes_f16`` against torch indexing with zero fill; the ``_placed`` blend entries against the EXISTING
  entries on inputs pre-shifted in torch (object chunks shifted with zero fill, masks nearest-resized to H x W and zeroed where
  the feature source is out of range) -- destination rows bit-identical (int16 views; no NaN / inf is planted, so the NaN-sign
  caveat of DESIGN.md 6i stays out of it), sources untouched; zero offsets equal the unplaced entries; bad arguments refused.
  Every case asserts that its placed result DIFFERS from the unplaced call: on a tree without the feature nothing here passes.
* engine: a placed forward of the toy UNet against the same forward with ``ops.pnp_blend_tokens`` / ``pnp_blend_nchw`` replaced
  by "pre-shift in torch, call the unplaced entry, restore the sources".
* pipeline: graph replay against eager, all-zero offsets against a call without the argument (latents, C-ABI calls, graph
  variants), a frame-sharded pipeline refused, K = 2 variants under one placement.

Helpers shared with test_variants_gpu.py are imported from it so that the files judge by the same bars.
"""
import ctypes as C
import itertools
import types

import pytest
import torch

import test_variants_gpu as tv

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_i16 = tv._i16


def _planted(x, g):
    """finite normals with a few +-0.0"""
    flat = x.view(-1)
    n = flat.numel()
    for v in (-0.0, 0.0):
        flat[torch.randint(0, n, (max(2, n // 53),), generator=g)] = v
    return x


def _shift_into(dst, src, dy, dx):
    """dst[y, x, ...] = src[y - dy, x - dx, ...] where that lies inside; dst keeps its (zero) fill elsewhere"""
    H, W = src.shape[:2]
    y0, y1, x0, x1 = max(0, dy), min(H, H + dy), max(0, dx), min(W, W + dx)
    if y0 < y1 and x0 < x1:
        dst[y0:y1, x0:x1] = src[y0 - dy:y1 - dy, x0 - dx:x1 - dx]


def _shifted(src, dy, dx):
    out = torch.zeros_like(src)
    _shift_into(out, src, dy, dx)
    return out


def _masks_eff(masks, offs, H, W):
    """the masks of the pre-shifted twin: nearest-resized to H x W, zero where the object's feature source is out of range"""
    m = torch.nn.functional.interpolate(masks, size=(H, W), mode="nearest") if tuple(masks.shape[2:]) != (H, W) else masks.clone()
    ones = torch.ones(H, W, dtype=m.dtype, device=m.device)
    for j, obj in enumerate(offs):
        for f, (dy, dx) in enumerate(obj):
            m[j, f] *= _shifted(ones, dy, dx)
    return m.contiguous()


def _table(offs):
    return torch.tensor(offs, dtype=torch.int32).cuda().contiguous()


def _offsets(nobj, H, W):
    """per object, per frame (F = 2) feature offsets: small ones, a zero, the last pixel that still overlaps, and -- from the
    third object on -- one object shifted entirely out of the frame"""
    table = [[(1, -2), (-1, 1)], [(0, 0), (2, -1)], [(H, 0), (-H - 3, W + 1)], [(-(H - 1), W - 1), (0, -1)]]
    return [list(o) for o in table[:nobj]]


def _maps(nobj):
    """the positional sources, and (two objects or more) a map with two objects on ONE chunk -- at different offsets"""
    return [None] if nobj == 1 else [None, (2, (1,) * nobj)]


def _chunk_frames_tokens(chunk, layout, F, H, W):
    """[F, H, W, cols] view of a chunk's rows (spatial: row = f * HW + p; temporal: row = p * F + f)"""
    return chunk.view(F, H, W, -1) if layout == "spatial" else chunk.view(H, W, F, -1).permute(2, 0, 1, 3)


def _shift_chunk_tokens(chunk, layout, F, H, W, obj_offs):
    out = torch.zeros_like(chunk)
    vi, vo = _chunk_frames_tokens(chunk, layout, F, H, W), _chunk_frames_tokens(out, layout, F, H, W)
    for f, (dy, dx) in enumerate(obj_offs):
        _shift_into(vo[f], vi[f], dy, dx)
    return out


def _shift_chunk_nchw(chunk, obj_offs):
    """chunk [F, C, H, W]"""
    out = torch.zeros_like(chunk)
    for f, (dy, dx) in enumerate(obj_offs):
        _shift_into(out[f].permute(1, 2, 0), chunk[f].permute(1, 2, 0), dy, dx)
    return out


def _tokens_placed_direct(buf, layout, F, H, W, c, masks, base0, ndst, smap, nvar, active, place):
    """the C entry itself; returns its status"""
    from mvoc_amd import ops
    ld, hw = buf.stride(0), H * W
    fs, ps = tv._strides(layout, ld, F, hw)
    d = ops._pnp_desc(buf[:, :c], buf[:, c:2 * c], masks, F * hw * ld, fs, ps, F, H, W, c, base0, ndst)
    nobj = masks.shape[0]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    return ops.lib.mvoc_pnp_blend_scatter_tokens_placed(C.byref(d), nsrc, arr, nvar, active, None if place is None else place.data_ptr(),
                                                        ops._stream())


def _nchw_placed_direct(x, masks, F, base0, ndst, smap, nvar, active, place):
    from mvoc_amd import ops
    d = ops._pnp_desc(x, None, masks, 0, 0, 0, F, x.shape[2], x.shape[3], x.shape[1], base0, ndst)
    nobj = masks.shape[0]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    return ops.lib.mvoc_pnp_blend_scatter_nchw_placed(C.byref(d), nsrc, arr, nvar, active, None if place is None else place.data_ptr(),
                                                      ops._stream())


def _run_tokens(buf, layout, F, H, W, c, masks, base0, ndst, smap=None, nvar=1, active=None, place=None):
    from mvoc_amd import ops
    ld, hw = buf.stride(0), H * W
    fs, ps = tv._strides(layout, ld, F, hw)
    kw = {} if place is None else {"place": place}
    ops.pnp_blend_tokens(buf[:, :c], masks, x2=buf[:, c:2 * c], frames=F, height=H, width=W, channels=c, chunk_stride=F * hw * ld,
                         f_stride=fs, p_stride=ps, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=nvar, active=active, **kw)


# (nvar, active): one variant; three with every bit set; three with a partial mask
VARIANTS = ((1, 0b1), (3, 0b111), (3, 0b101))


# ---- shift kernel ---------------------------------------------------------------------------------------------------------
def test_shift_planes_against_torch_indexing():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(1)
    npl, F, h, w = 3, 2, 5, 7
    src = _planted(torch.randn(npl, F, h, w, generator=g).half(), g).cuda()
    dys = [0, 1, -1, h - 1, -(h - 1), h, -h, h + 3, -(h + 3)]
    dxs = [0, 1, -1, w - 1, -(w - 1), w, -w, w + 3, -(w + 3)]
    n = 0
    for i, j in itertools.product(range(len(dys)), range(len(dxs))):
        offs = [(dys[i], dxs[j]), (dys[(i + 4) % 9], dxs[(j + 2) % 9])]  # the two frames move differently
        want = torch.zeros_like(src)
        for pl in range(npl):
            for f, (dy, dx) in enumerate(offs):
                _shift_into(want[pl, f], src[pl, f], dy, dx)
        out = torch.full_like(src, float("nan"))
        got = ops.shift_planes(src, _table(offs), out=out)
        assert got is out and torch.equal(_i16(got), _i16(want)), offs
        if any(v for pair in offs for v in pair):
            assert not torch.equal(_i16(got), _i16(src)), offs  # the planes did move
        n += 1
    assert n == 81
    # one [F, h, w] mask of a stack per call (nplane = 1), and zero offsets = a copy, signed zeros included
    one = ops.shift_planes(src[1], _table([(0, 0), (0, 0)]))
    assert torch.equal(_i16(one), _i16(src[1]))


def test_shift_planes_refuses_bad_arguments():
    from mvoc_amd import ops
    src = torch.ones(2, 2, 3, 4, dtype=torch.float16, device="cuda")
    dst = torch.zeros_like(src)
    tab = _table([(1, 1), (0, 0)])
    call = lambda s, d, t, dims=(2, 2, 3, 4): ops.lib.mvoc_shift_planes_f16(s, d, *dims, t, ops._stream())
    assert call(None, dst.data_ptr(), tab.data_ptr()) == -1 and "null" in ops.lib.mvoc_last_error().decode()
    assert call(src.data_ptr(), dst.data_ptr(), None) == -1 and "null" in ops.lib.mvoc_last_error().decode()
    assert call(src.data_ptr(), src.data_ptr(), tab.data_ptr()) == -1 and "in place" in ops.lib.mvoc_last_error().decode()
    assert call(src.data_ptr(), dst.data_ptr(), tab.data_ptr(), (2, 0, 3, 4)) == -1 and "dims" in ops.lib.mvoc_last_error().decode()
    with pytest.raises(RuntimeError, match="offsets must be"):
        ops.shift_planes(src, _table([(1, 1)] * 3))
    with pytest.raises(RuntimeError, match="offsets"):
        ops.shift_planes(src, tab.float())
    torch.cuda.synchronize()
    assert not dst.any() and bool((src == 1).all())


# ---- tokens -------------------------------------------------------------------------------------------------------------
def _expect_tokens(comp0, layout, F, H, W, c, masks, base0, ndst, smap, K, active, offs):
    """chunk index -> the rows the placed entry must leave there: per injecting variant the POSITIONAL entry on that variant's own
    batch [bg, shifted obj_1.., (u_k,) c_k]; an idle variant's chunks as they were"""
    nobj, rows = masks.shape[0], F * H * W
    nsrc = nobj + 1 if smap is None else smap[0]
    order = tv._src_order(smap, nobj)
    chunk = lambda t, i: t[i * rows:(i + 1) * rows]
    meff = _masks_eff(masks, offs, H, W)
    exp = {}
    for k in range(K):
        dst = [nsrc + d * K + k for d in range(ndst)]
        if not (active >> k) & 1:
            exp.update({i: chunk(comp0, i) for i in dst})
            continue
        parts = [chunk(comp0, order[0])] + [_shift_chunk_tokens(chunk(comp0, order[1 + j]).contiguous(), layout, F, H, W, offs[j])
                                            for j in range(nobj)] + [chunk(comp0, i) for i in dst]
        full = torch.cat(parts).contiguous()
        tv._run_tokens(full, layout, F, H, W, c, meff, base0, ndst)
        exp.update({i: chunk(full, nobj + 1 + d).clone() for d, i in enumerate(dst)})
    return exp


@pytest.mark.parametrize("layout", ["spatial", "temporal"])
@pytest.mark.parametrize("geo", [(4, 6, None), (4, 6, (8, 12)), (3, 5, (5, 9))], ids=["4x6-same", "4x6-mask8x12", "3x5-mask5x9"])
def test_tokens_placed_equal_the_existing_entries_on_preshifted_inputs(geo, layout):
    H, W, mres = geo
    mh, mw = mres or (H, W)
    F, c = 2, 16
    rows = F * H * W
    g = torch.Generator().manual_seed(7 * H + W + (layout == "temporal"))
    n = 0
    for nobj in (1, 2, 3, 4):
        offs = _offsets(nobj, H, W)
        place = _table(offs)
        for ndst, base0, (K, active), smap in itertools.product((1, 2), (False, True), VARIANTS, _maps(nobj)):
            masks = tv._masks(nobj, F, mh, mw, soft=bool(n % 2), g=g)
            nsrc = nobj + 1 if smap is None else smap[0]
            comp = _planted(torch.randn((nsrc + ndst * K) * rows, 3 * c, generator=g).half(), g).cuda()
            comp0 = comp.clone()
            what = (nobj, ndst, base0, K, bin(active), smap)
            exp = _expect_tokens(comp0, layout, F, H, W, c, masks, base0, ndst, smap, K, active, offs)
            _run_tokens(comp, layout, F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, place=place)
            chunk = lambda t, i: t[i * rows:(i + 1) * rows]
            for i, want in exp.items():
                assert torch.equal(_i16(chunk(comp, i)[:, :2 * c]), _i16(want[:, :2 * c])), (what, i)
            assert torch.equal(_i16(comp[:nsrc * rows]), _i16(comp0[:nsrc * rows])), what  # sources untouched
            assert torch.equal(_i16(comp[:, 2 * c:]), _i16(comp0[:, 2 * c:])), what  # v columns untouched
            # the unplaced call on the same inputs writes something else: the offsets matter
            plain = comp0.clone()
            _run_tokens(plain, layout, F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active)
            assert not torch.equal(_i16(plain[nsrc * rows:]), _i16(comp[nsrc * rows:])), what
            if smap is None and K > 1:
                # ... and the _variants / _variants_sel entry itself on the batch whose object chunks are shifted in place
                twin = comp0.clone()
                for j in range(nobj):
                    chunk(twin, 1 + j).copy_(_shift_chunk_tokens(chunk(comp0, 1 + j).contiguous(), layout, F, H, W, offs[j]))
                _run_tokens(twin, layout, F, H, W, c, _masks_eff(masks, offs, H, W), base0, ndst, None, nvar=K, active=active)
                assert torch.equal(_i16(twin[nsrc * rows:, :2 * c]), _i16(comp[nsrc * rows:, :2 * c])), what
            n += 1
    assert n == (1 + 3 * 2) * 2 * 2 * len(VARIANTS)


def test_a_negative_zero_base_becomes_positive_zero_where_the_object_is_absent():
    """value 0 and mask 0 enter blend16: -0.0 * 1 + 0 * 0 = +0.0, as under the positional kernel with a zero object and mask"""
    F, H, W, c = 2, 4, 6, 16
    rows = F * H * W
    masks = torch.ones(1, F, H, W, dtype=torch.float16, device="cuda")
    comp = torch.randn(4 * rows, 3 * c, generator=torch.Generator().manual_seed(2)).half().cuda()  # [bg, obj, u, c]
    comp[3 * rows:] = -0.0  # the base (the last chunk)
    twin = comp.clone()
    offs = [[(H, 0), (0, -W)]]  # entirely out of the frame in both frames
    _run_tokens(comp, "spatial", F, H, W, c, masks, False, 2, place=_table(offs))
    for i in (2, 3):
        got = comp[i * rows:(i + 1) * rows, :2 * c]
        assert bool((_i16(got) == 0).all())  # +0.0: no sign bit
    twin[rows:2 * rows] = 0.0  # the absent object
    _run_tokens(twin, "spatial", F, H, W, c, torch.zeros_like(masks), False, 2)
    assert torch.equal(_i16(twin[2 * rows:]), _i16(comp[2 * rows:]))


# ---- NCHW -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 8), (3, 5)])  # hw % 8 == 0: 8 pixels per work item / else 1
def test_nchw_placed_equal_the_existing_entries_on_preshifted_inputs(hw):
    from mvoc_amd import ops
    H, W = hw
    F, Cc = 2, 4
    g = torch.Generator().manual_seed(300 + W)
    n = 0
    for nobj in (1, 2, 3, 4):
        offs = _offsets(nobj, H, W)
        place = _table(offs)
        for ndst, base0, (K, active), smap, mres in itertools.product((1, 2), (False, True), VARIANTS, _maps(nobj), ("same", "other")):
            mh, mw = (H, W) if mres == "same" else (2 * H, W + 1)
            masks = tv._masks(nobj, F, mh, mw, soft=bool(n % 2), g=g)
            meff = _masks_eff(masks, offs, H, W)
            nsrc = nobj + 1 if smap is None else smap[0]
            order = tv._src_order(smap, nobj)
            comp = _planted(torch.randn((nsrc + ndst * K) * F, Cc, H, W, generator=g).half(), g).cuda()
            comp0 = comp.clone()
            chunk = lambda t, i: t[i * F:(i + 1) * F]
            what = (nobj, ndst, base0, K, bin(active), smap, mres)
            ops.pnp_blend_nchw(comp, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=place)
            for k in range(K):
                dst = [nsrc + d * K + k for d in range(ndst)]
                if not (active >> k) & 1:
                    for i in dst:
                        assert torch.equal(_i16(chunk(comp, i)), _i16(chunk(comp0, i))), (what, k)
                    continue
                parts = [chunk(comp0, order[0])] + [_shift_chunk_nchw(chunk(comp0, order[1 + j]), offs[j]) for j in range(nobj)]
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


# ---- zero offsets, bad arguments, profiler ----------------------------------------------------------------------------------
def test_zero_offsets_equal_the_unplaced_entries():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(11)
    F, H, W, c = 2, 3, 5, 16
    rows = F * H * W
    for nobj, ndst, base0, (K, active) in itertools.product((1, 3), (1, 2), (False, True), VARIANTS):
        zero = torch.zeros(nobj, F, 2, dtype=torch.int32, device="cuda")
        for smap in tv._maps(nobj)[:3]:
            masks = tv._masks(nobj, F, 5, 9, True, g)
            nsrc = nobj + 1 if smap is None else smap[0]
            comp = _planted(torch.randn((nsrc + ndst * K) * rows, 3 * c, generator=g).half(), g).cuda()
            twin = comp.clone()
            _run_tokens(comp, "temporal", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, place=zero)
            _run_tokens(twin, "temporal", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active)
            assert torch.equal(_i16(comp), _i16(twin)), (nobj, ndst, base0, K, active, smap)
            for hw in ((4, 8), (3, 5)):
                x = _planted(torch.randn((nsrc + ndst * K) * F, 4, *hw, generator=g).half(), g).cuda()
                y = x.clone()
                ops.pnp_blend_nchw(x, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=zero)
                ops.pnp_blend_nchw(y, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active)
                assert torch.equal(_i16(x), _i16(y)), (nobj, ndst, base0, K, active, smap, hw)


def test_placed_entries_refuse_bad_arguments_and_write_nothing():
    from mvoc_amd import ops
    F, H, W, c = 2, 4, 4, 8
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    buf = torch.zeros(9 * F * H * W, 3 * c, dtype=torch.float16, device="cuda")
    nchw = torch.zeros(9 * F, 4, H, W, dtype=torch.float16, device="cuda")
    place = _table([[(1, 1), (0, -1)], [(2, 0), (0, 0)]])
    err = lambda: ops.lib.mvoc_last_error().decode()
    cases = [  # (nvar, active, map, table, text)
        (0, 1, None, place, "nvar 0"), (9, 1, None, place, "nvar 9"),
        (3, 0, None, place, "active mask 0x0"), (3, 8, None, place, "active mask 0x8"), (1, 2, None, place, "active mask 0x2"),
        (2, 3, (0, (0, 0)), place, "nsrc 0"), (2, 3, (2, (0, 2)), place, "obj_chunk[1] = 2"), (2, 3, (2, (-1, 0)), place, "obj_chunk[0] = -1"),
        (2, 3, None, None, "null offset table"),
    ]
    for nvar, active, smap, tab, text in cases:
        assert _tokens_placed_direct(buf, "spatial", F, H, W, c, masks, False, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
        assert _nchw_placed_direct(nchw, masks, F, True, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
    # a valid call with the same buffers goes through (the refusals above were about the arguments)
    assert _tokens_placed_direct(buf, "spatial", F, H, W, c, masks, False, 2, None, 3, 0b111, place) == 0, err()
    assert _nchw_placed_direct(nchw, masks, F, True, 2, None, 1, 1, place) == 0, err()
    # the Python layer: the table's form, and an offset that does not fit its int32 fields
    with pytest.raises(RuntimeError, match=r"int32 \[nobj = 2, F = 2, 2\]"):
        _run_tokens(buf, "spatial", F, H, W, c, masks, False, 2, nvar=2, place=place[:1])
    with pytest.raises(RuntimeError, match="place"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, nvar=2, place=place.long())
    with pytest.raises(RuntimeError, match="does not fit int32"):
        ops.place_table((((2 ** 31, 0),) * F, ((0, 0),) * F), H, W, H, W, "cuda")
    with pytest.raises(RuntimeError, match="does not fit int32"):
        ops.place_table((((0, 0),) * F, ((0, -2 ** 31 - 1),) * F), H, W, H, W, "cuda")
    with pytest.raises(RuntimeError, match="storage ends"):
        ops.pnp_blend_nchw(nchw, masks, frames=F, ndst=2, nvar=4, place=place)  # 3 + 8 chunks in a buffer of 9
    torch.cuda.synchronize()
    assert not buf.any() and not nchw.any()  # zeros blended with zeros: nothing but zeros was ever written


def test_extreme_offsets_are_safe_and_mean_absent():
    """every int32 offset is valid to the kernels: the objects are out of the frame, the result is the base blended with zero
    objects under zero masks"""
    F, H, W, c = 2, 3, 5, 16
    rows = F * H * W
    g = torch.Generator().manual_seed(4)
    masks = tv._masks(2, F, H, W, False, g)
    comp = _planted(torch.randn(5 * rows, 3 * c, generator=g).half(), g).cuda()
    comp0 = comp.clone()
    twin = comp.clone()
    big = 2 ** 31 - 1
    _run_tokens(comp, "spatial", F, H, W, c, masks, True, 2, place=_table([[(big, -big - 1), (-big - 1, big)], [(big, big), (0, big)]]))
    twin[rows:3 * rows] = 0.0
    _run_tokens(twin, "spatial", F, H, W, c, torch.zeros_like(masks), True, 2)
    assert torch.equal(_i16(comp[3 * rows:]), _i16(twin[3 * rows:]))
    assert torch.equal(_i16(comp[:3 * rows]), _i16(comp0[:3 * rows]))


def test_profiler_counts_the_bytes_of_the_sel_entries():
    from mvoc_amd import ops
    F, H, W, c, K = 2, 4, 4, 8, 3
    rows = F * H * W
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    place = _table([[(1, 0), (0, 1)], [(0, 0), (-1, -1)]])
    ops.prof_enable(True)
    try:
        for base0, ndst, smap, active in ((True, 2, None, 0b101), (False, 2, None, 0b011), (False, 1, (2, (1, 1)), 0b100)):
            nsrc = 3 if smap is None else smap[0]
            work = []
            for pl in (None, place):
                buf = torch.zeros((nsrc + ndst * K) * rows, 3 * c, dtype=torch.float16, device="cuda")
                nchw = torch.zeros((nsrc + ndst * K) * F, c, H, W, dtype=torch.float16, device="cuda")
                kw = {} if pl is None else {"place": pl}
                ops.prof_reset()
                _run_tokens(buf, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, place=pl)
                torch.cuda.synchronize()
                t = ops.prof_collect()["pnp"]
                ops.prof_reset()
                ops.pnp_blend_nchw(nchw, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, **kw)
                torch.cuda.synchronize()
                n = ops.prof_collect()["pnp"]
                assert t["launches"] == 1 and n["launches"] == 1
                work.append((t["work"], n["work"]))
            assert work[0] == work[1] and work[0][0] > 0, (base0, ndst, smap, active, work)
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


# ---- engine -------------------------------------------------------------------------------------------------------------
class _PreShift:
    """``ops.pnp_blend_tokens`` / ``pnp_blend_nchw`` replaced by: shift the object chunks in torch (zero fill), call the unplaced
    entry with the masks resized and zeroed where the source is out of range, restore the source chunks"""

    def __init__(self):
        from mvoc_amd import ops
        self.ops, self.orig, self.calls = ops, (ops.pnp_blend_tokens, ops.pnp_blend_nchw), []

    def __enter__(self):
        self.ops.pnp_blend_tokens, self.ops.pnp_blend_nchw = self.tokens, self.nchw
        return self

    def __exit__(self, *exc):
        self.ops.pnp_blend_tokens, self.ops.pnp_blend_nchw = self.orig

    def tokens(self, x, masks, **kw):
        place = kw.pop("place")
        offs = place.cpu().tolist()
        F, H, W, c = kw["frames"], kw["height"], kw["width"], kw["channels"]
        nobj = masks.shape[0]
        assert kw.get("src_map") is None and tuple(place.shape) == (nobj, F, 2)
        nchunk = nobj + 1 + kw["ndst"] * kw.get("nvar", 1)
        self.calls.append(("tokens", H, W, offs))
        saved = []
        for t in (x, kw.get("x2")):
            if t is None:
                continue
            v = torch.as_strided(t, (nchunk, F, H, W, c), (kw["chunk_stride"], kw["f_stride"], kw["p_stride"] * W, kw["p_stride"], 1),
                                 t.storage_offset())
            keep = v[1:nobj + 1].clone()
            saved.append((v, keep))
            for j in range(nobj):
                for f, (dy, dx) in enumerate(offs[j]):
                    v[1 + j, f] = _shifted(keep[j, f], dy, dx)
        out = self.orig[0](x, _masks_eff(masks, offs, H, W), **kw)
        for v, keep in saved:
            v[1:nobj + 1] = keep
        return out

    def nchw(self, x, masks, **kw):
        place = kw.pop("place")
        offs = place.cpu().tolist()
        F, (H, W), nobj = kw["frames"], x.shape[2:], masks.shape[0]
        assert kw.get("src_map") is None and kw.get("x2") is None
        self.calls.append(("nchw", H, W, offs))
        keep = x[F:(nobj + 1) * F].clone()
        for j in range(nobj):
            x[(1 + j) * F:(2 + j) * F] = _shift_chunk_nchw(keep[j * F:(j + 1) * F], offs[j])
        out = self.orig[1](x, _masks_eff(masks, offs, H, W), **kw)
        x[F:(nobj + 1) * F] = keep
        return out


@pytest.mark.parametrize("kind", ["qk", "conv_out", "features"])
def test_unet_placed_forward_equals_the_preshifted_unplaced_forward(kind):
    """one Q/K step (spatial + temporal sites, the source tail pruned), one conv_out step (prune_dead_chunks: the NCHW blend on
    the source chunks' outputs) and, with prune_dead_chunks off, the same step through the resnet / temporal-conv feature sites"""
    from mvoc_amd import ops, pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    F, h, w, cd = 3, 8, 8, 64
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    placement = (((1, -2), (0, 1), (-2, 0)), ((3, 2),) * F)  # a per-frame path, and one constant offset (latent grid)
    moved, table = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False).place_masks(masks, placement)
    assert table.tolist() == [list(map(list, o)) for o in placement]
    for j in range(2):  # the masks in destination coordinates: both forms, every channel, types kept
        for a, b in zip(moved[j], masks[j]):
            assert a.dtype == b.dtype and a.shape == b.shape
            for f, (dy, dx) in enumerate(placement[j]):
                assert torch.equal(a[0, :, f], torch.stack([_shifted(b[0, ch, f], dy, dx) for ch in range(4)]))
    roles = tv._roles(F, h, w, cd, 4, 1)
    pipe, (t_feat, t_qk) = tv._arm(eng, 5)
    t = t_qk if kind == "qk" else t_feat
    names = ["S", "O", "P", "u0", "c0"]
    saved = eng.prune_dead_chunks

    def forward(pl):
        eng.placement, eng.prune_source_tail, eng.prune_dead_chunks = pl, True, kind != "features"
        try:
            return tv._fwd(eng, tv._batch(roles, names), t)
        finally:
            eng.placement, eng.prune_source_tail, eng.prune_dead_chunks = None, False, saved

    try:
        pnp_utils.register_time_all(pipe, t, moved)
        got = forward(placement)
        with _PreShift() as pre:
            ref = forward(placement)
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
    for c in pre.calls:  # every site was handed the offsets of its own level
        assert c[3] == [list(map(list, o)) for o in ops.level_offsets(placement, c[1], c[2], h, w)], c
    assert torch.equal(_i16(got[3:]), _i16(ref[3:])), kind
    assert torch.isfinite(got[3:]).all() and not torch.equal(got[3:], plain[3:]), kind  # the placement moved something
    assert eng.placement is None and len(eng._level_tables["placement"][1]) == len({c[1:3] for c in pre.calls})


def test_unet_with_a_frame_shard_refuses_a_placement():
    from mvoc_amd import pnp_utils
    F, h, w, cd = 3, 8, 8, 64
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    eng.placement = (((1, 0),) * F, ((0, 1),) * F)
    eng.shard = types.SimpleNamespace(rank=0, world=1)
    try:
        with pytest.raises(RuntimeError, match="frame shard"):
            eng.pnp_batch(5, masks)
        with pytest.raises(RuntimeError, match="frame shard"):
            eng.place_table(masks, 8, 8)
    finally:
        eng.placement, eng.shard = None, None
    assert eng.place_kw(masks, 8, 8) == {}


# ---- pipeline -----------------------------------------------------------------------------------------------------------
PATH = [(8, 0), (16, -8), (24, -16)]  # object 0 follows a path (dx, dy per frame, image pixels); object 1 moves by one pair
OFFSETS = [PATH, (-16, 8)]


def _placed_job(graphs, offsets="none", K=1, count_calls=False, shard=False, steps=5):
    """test_variants_gpu.py's toy composition (three distinct sources, two objects, five steps, fusion on the first two);
    ``offsets``: "none" = the call without the argument, else the ``obj_offsets`` it is given"""
    from launch_census import Recorder
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    _, eng = tv._toy_pair()
    g = torch.Generator().manual_seed(5)
    f, h, w, cd, n = 3, 8, 8, 64, steps
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
    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=graphs)
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
    states, step_calls = [], []
    make, step = pipe.make_composition_state, pipe.composition_step

    def make_state(*a, **k):
        states.append(make(*a, **k))
        return states[-1]

    rec = Recorder() if count_calls else None

    def one_step(*a, **k):
        if rec is not None:
            rec.calls.clear()
        step(*a, **k)
        if rec is not None:
            step_calls.append(dict(rec.calls))

    pipe.make_composition_state, pipe.composition_step = make_state, one_step
    clips = [[(r, i, False) for i in range(f)] for r in range(3)]
    if K == 1:
        var = dict(prompt="edit0", main_first_image=(4, 0, True), main_image_list=[(4, i, False) for i in range(f)], latents=x0.cuda(),
                   guidance_scale=9.0, negative_prompt="neg")
    else:
        var = dict(prompt=[f"edit{k}" for k in range(K)], main_first_image=[(4 + 2 * k, 0, True) for k in range(K)],
                   main_image_list=[[(4 + 2 * k, i, False) for i in range(f)] for k in range(K)], latents=x0.cuda(),
                   guidance_scale=[tv.GUIDANCE[k % 2] for k in range(K)], negative_prompt=["neg"] * K)
    if offsets != "none":
        var["obj_offsets"] = offsets
    if shard:
        eng.shard = types.SimpleNamespace(rank=0, world=1)
    if rec is not None:
        rec.install()
    try:
        out = pipe.sample_with_pnp_pipeline_with_edit_prompt_extraction_with_attn_injection(
            background_first_image=(0, 0, True), background_image_list=clips[0], objs_first_image=[(1, 0, True), (2, 0, True)],
            objs_image_list=[clips[1], clips[2]], height=h * 8, width=w * 8, num_frames=f, num_inference_steps=n,
            target_fps=8, output_type="latent", ddim_inv_prompt="", bg_inv_latents_path=dirs[0], obj_ddim_latents_path=dirs[1:],
            obj_ddim_latents_idx_offset=[0, 0], obj_masks_tensors=[(a.clone(), b.clone()) for a, b in cpu_masks],
            ddim_init_latents_t_idx=0, fusion_steps=(0, 2), random_noise_ratio=0.3, obj_random_noise_fusion=True, **var).frames
    finally:
        if rec is not None:
            rec.uninstall()
        eng.shard = None
    torch.cuda.synchronize()
    st = states[0]
    return types.SimpleNamespace(out=out, graphs=len(st["variants"]), step_calls=step_calls, state=st, masks=cpu_masks, pipe=pipe)


def test_placed_composition_graph_replay_equals_eager_and_moves_the_result():
    eager = _placed_job(False, OFFSETS, count_calls=True)
    st = eager.state
    assert st["placement"] == (((0, 1), (-1, 2), (-2, 3)), ((1, -2),) * 3)  # (dy, dx) on the latent grid
    # the call's masks, everywhere, are the shifted ones: built once, in destination coordinates
    for j, obj in enumerate(st["placement"]):
        for f, (dy, dx) in enumerate(obj):
            want = _shifted(eager.masks[j][0][0, 0, f].cuda(), dy, dx)
            assert torch.equal(st["fusion_masks"][j, 0, 0, f], want) and torch.equal(st["masks"][j][0][0, 0, f].cuda().half(), want)
            assert torch.equal(st["masks"][j][1][0, 0, f].cuda(), _shifted(eager.masks[j][1][0, 0, f].cuda(), dy, dx))
    # the per-level offset tables (8 x 8, 4 x 4, 2 x 2) stay alive with the state, whose graphs would read them
    assert len(st["place_tables"]) == 1 and {k[:2] for k in st["place_tables"][0]} == {(8, 8), (4, 4), (2, 2)}
    names = set().union(*eager.step_calls)
    assert {"mvoc_pnp_blend_scatter_tokens_placed", "mvoc_pnp_blend_scatter_nchw_placed", "mvoc_shift_planes_f16"} <= names
    assert not any(n.startswith("mvoc_pnp_blend") and not n.endswith("_placed") for n in names), names
    # two fusion steps: the two fusion objects go through the shift kernel instead of a copy
    assert [c.get("mvoc_shift_planes_f16", 0) for c in eager.step_calls] == [2, 2, 0, 0, 0]
    graphed = _placed_job(True, OFFSETS)
    assert torch.equal(graphed.out, eager.out) and torch.isfinite(eager.out).all()
    plain = _placed_job(False)
    assert plain.out.shape == eager.out.shape and not torch.equal(plain.out, eager.out)


def test_all_zero_offsets_make_the_calls_and_graphs_of_a_call_without_them():
    zeros = [[(0, 0)] * 3, (0, 0)]
    plain, zero = _placed_job(False, count_calls=True), _placed_job(False, zeros, count_calls=True)
    assert zero.state["placement"] is None and zero.state["place_dev"] is None
    assert len(plain.step_calls) == len(zero.step_calls) == 5
    for i, (a, b) in enumerate(zip(plain.step_calls, zero.step_calls)):
        assert a == b and sum(a.values()) > 0, (i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
        assert not any(n.endswith("_placed") or n == "mvoc_shift_planes_f16" for n in b)
    assert torch.equal(plain.out, zero.out)
    gp, gz = _placed_job(True), _placed_job(True, zeros)
    assert gp.graphs == gz.graphs >= 3 and torch.equal(gp.out, gz.out) and torch.equal(gp.out, plain.out)


def test_a_frame_sharded_pipeline_refuses_offsets():
    with pytest.raises(RuntimeError, match="frame shard"):
        _placed_job(False, OFFSETS, shard=True)


def test_two_variants_share_one_placement():
    placed, plain = _placed_job(True, OFFSETS, K=2), _placed_job(True, K=2)
    assert placed.out.shape[0] == 2 and torch.isfinite(placed.out).all()
    assert placed.state["nvar"] == 2 and placed.state["placement"] is not None
    assert placed.graphs == plain.graphs  # the placement is one more part of the key, not one more step kind
    for k in range(2):
        assert not torch.equal(placed.out[k], plain.out[k]), k
    assert not torch.equal(placed.out[0], placed.out[1])
