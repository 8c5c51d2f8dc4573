"""GPU: per-variant object placement in the K-variant composition loop.

* kernels: the ``_placed_variants`` blend entries against the ``_placed`` entries -- variant k's destination chunks equal the
  ``_placed`` entry run with nvar = 1 on that variant's own batch [sources.., (u_k,) c_k] with table k and masks k; sources and
  the chunks of idle variants untouched; nvar = 1, K equal placements and all-zero tables equal the existing entries; extreme
  offsets mean absent; bad arguments refused with nothing written; the profiler's byte count is the stated formula.
* engine: a K = 3 forward of the toy UNet under ``variant_placements`` (A, zeros, B) against the single-variant placed (or
  unplaced) forward of each variant, for each site kind.
* pipeline: a K = 3 call with ``variant_obj_offsets=[A, None, B]`` against three single-variant calls, graph replay against
  eager, once with per-variant injection thresholds and once with ``dedup_sources``; the two degenerate forms (all equal, all
  None / zero) against the calls they resolve to (latents, C-ABI calls, graph variants); a frame shard refused.

Every comparison is on the raw fp16 bits (int16 views): signed zeros count.  No NaN / inf is planted.  Helpers shared with
test_variants_gpu.py / test_placement_gpu.py are imported from them so that the files judge by the same bars.
"""
import ctypes as C
import gc
import itertools
import types

import pytest
import torch

import test_placement_gpu as tp
import test_variants_gpu as tv

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(autouse=True)
def _no_dead_graphs_across_tests():
    """``_job`` wraps the pipeline's methods in closures of its own, so a finished job is a reference cycle that holds captured
    graphs.  Collected here, between tests: the cyclic collector must not meet them inside a later job's graph capture (HIP
    refuses to destroy a graph while a stream captures)."""
    gc.collect()
    yield
    gc.collect()
_i16 = tv._i16
F3 = 3


# ---- kernels: helpers ---------------------------------------------------------------------------------------------------------
def _variant_offsets(K, nobj, F, H, W):
    """[K][nobj][F] feature offsets (dy, dx): both signs, different per variant, object and frame, up to the last pixel that
    still overlaps; the LAST variant's object 0 lies entirely outside the frame in every frame"""
    offs = [[[(((3 * k + 2 * j + f) % (2 * H - 1)) - (H - 1), ((5 * k + j + 2 * f + 1) % (2 * W - 1)) - (W - 1)) for f in range(F)]
             for j in range(nobj)] for k in range(K)]
    offs[K - 1][0] = [(H, 0), (0, -W), (-H - 2, W + 3)][:F] + [(H, 0)] * max(0, F - 3)
    return offs


def _vtable(offs):
    return torch.tensor(offs, dtype=torch.int32).cuda().contiguous()


def _vmasks(K, nobj, F, mh, mw, soft, g):
    return torch.stack([tv._masks(nobj, F, mh, mw, soft, g) for _ in range(K)]).contiguous()


def _active_for(K, n):
    """every variant on most cases; a partial mask on every third (0b101 of 3, as the issue names it)"""
    if K == 1 or n % 3:
        return (1 << K) - 1
    return {2: 0b10, 3: 0b101, 8: 0b10110101}[K]


def _run_tokens_v(buf, layout, F, H, W, c, masks, base0, ndst, smap, nvar, active, place):
    """ops.pnp_blend_tokens with whatever table / masks it is given (4-D + 5-D: the new entry)"""
    tp._run_tokens(buf, layout, F, H, W, c, masks, base0, ndst, smap, nvar=nvar, active=active, place=place)


def _direct(kind, x, x2, masks, geo, c, strides, base0, ndst, smap, nvar, active, place):
    """the C entry itself; returns its status"""
    from mvoc_amd import ops
    F, H, W = geo
    d = ops._pnp_desc(x, x2, masks, *strides, F, H, W, c, base0, ndst)
    nobj = masks.shape[-4]
    nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
    arr = (C.c_int32 * len(chunks))(*chunks)
    fn = getattr(ops.lib, f"mvoc_pnp_blend_scatter_{kind}_placed_variants")
    return fn(C.byref(d), nsrc, arr, nvar, active, None if place is None else place.data_ptr(), ops._stream())


def _tokens_direct(buf, layout, F, H, W, c, masks, base0, ndst, smap, nvar, active, place):
    ld, hw = buf.stride(0), H * W
    fs, ps = tv._strides(layout, ld, F, hw)
    return _direct("tokens", buf[:, :c], buf[:, c:2 * c], masks, (F, H, W), c, (F * hw * ld, fs, ps), base0, ndst, smap, nvar, active, place)


def _nchw_direct(x, masks, F, base0, ndst, smap, nvar, active, place):
    return _direct("nchw", x, None, masks, (F, x.shape[2], x.shape[3]), x.shape[1], (0, 0, 0), base0, ndst, smap, nvar, active, place)


def _dst(nsrc, ndst, K, k):
    return [nsrc + d * K + k for d in range(ndst)]


# ---- tokens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["spatial", "temporal"])
@pytest.mark.parametrize("geo", [(4, 6, None), (4, 6, (8, 12)), (3, 5, (5, 9))], ids=["4x6-same", "4x6-mask8x12", "3x5-mask5x9"])
def test_tokens_placed_variants_equal_the_placed_entry_per_variant(geo, layout):
    H, W, mres = geo
    mh, mw = mres or (H, W)
    F = F3
    hw = H * W
    rows = F * hw
    g = torch.Generator().manual_seed(11 * H + W + (layout == "temporal"))
    chunk = lambda t, i: t[i * rows:(i + 1) * rows]
    n = partial = 0
    for nobj, K in itertools.product((1, 2, 3, 4), (1, 2, 3, 8)):
        offs = _variant_offsets(K, nobj, F, H, W)
        place = _vtable(offs)
        for ndst, base0, smap in itertools.product((1, 2), (False, True), tp._maps(nobj)):
            c = (8, 16)[n % 2]
            active = _active_for(K, n)
            partial += active != (1 << K) - 1
            masks = _vmasks(K, nobj, F, mh, mw, bool((n // 2) % 2), g)
            nsrc = nobj + 1 if smap is None else smap[0]
            comp = tp._planted(torch.randn((nsrc + ndst * K) * rows, 3 * c, generator=g).half(), g).cuda()
            comp0 = comp.clone()
            what = (nobj, K, ndst, base0, smap, c, bin(active))
            _run_tokens_v(comp, layout, F, H, W, c, masks, base0, ndst, smap, K, active, place)
            for k in range(K):
                dst = _dst(nsrc, ndst, K, k)
                if not (active >> k) & 1:  # neither read nor written
                    for i in dst:
                        assert torch.equal(_i16(chunk(comp, i)), _i16(chunk(comp0, i))), (what, k)
                    continue
                own = torch.cat([comp0[:nsrc * rows]] + [chunk(comp0, i) for i in dst]).contiguous()  # [sources.., (u_k,) c_k]
                tp._run_tokens(own, layout, F, H, W, c, masks[k], base0, ndst, smap, nvar=1, active=1, place=place[k])
                for d, i in enumerate(dst):
                    assert torch.equal(_i16(chunk(comp, i)[:, :2 * c]), _i16(chunk(own, nsrc + d)[:, :2 * c])), (what, k, d)
            assert torch.equal(_i16(comp[:nsrc * rows]), _i16(comp0[:nsrc * rows])), what  # sources untouched
            assert torch.equal(_i16(comp[:, 2 * c:]), _i16(comp0[:, 2 * c:])), what  # v columns untouched
            if K > 1 and active == (1 << K) - 1:  # the variants did get different placements
                a, b = _dst(nsrc, ndst, K, 0)[-1], _dst(nsrc, ndst, K, K - 1)[-1]
                if base0:  # (one base: only the objects' placement can tell the variants apart)
                    assert not torch.equal(_i16(chunk(comp, a)[:, :2 * c]), _i16(chunk(comp, b)[:, :2 * c])), what
            n += 1
    assert n == 4 * 4 * (1 + 3 * 2) and partial >= 8, (n, partial)


# ---- NCHW -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 8), (3, 5)])  # hw % 8 == 0: base and destinations 8 pixels per work item / else 1
def test_nchw_placed_variants_equal_the_placed_entry_per_variant(hw):
    from mvoc_amd import ops
    H, W = hw
    F, Cc = F3, 4
    g = torch.Generator().manual_seed(500 + W)
    chunk = lambda t, i: t[i * F:(i + 1) * F]
    n = 0
    for nobj, K in itertools.product((1, 2, 3, 4), (1, 2, 3, 8)):
        offs = _variant_offsets(K, nobj, F, H, W)
        place = _vtable(offs)
        for ndst, base0, smap in itertools.product((1, 2), (False, True), tp._maps(nobj)):
            mh, mw = (H, W) if n % 2 else (2 * H, W + 1)
            active = _active_for(K, n)
            masks = _vmasks(K, nobj, F, mh, mw, bool((n // 2) % 2), g)
            nsrc = nobj + 1 if smap is None else smap[0]
            comp = tp._planted(torch.randn((nsrc + ndst * K) * F, Cc, H, W, generator=g).half(), g).cuda()
            comp0 = comp.clone()
            what = (nobj, K, ndst, base0, smap, (mh, mw), bin(active))
            ops.pnp_blend_nchw(comp, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=place)
            for k in range(K):
                dst = _dst(nsrc, ndst, K, k)
                if not (active >> k) & 1:
                    for i in dst:
                        assert torch.equal(_i16(chunk(comp, i)), _i16(chunk(comp0, i))), (what, k)
                    continue
                own = torch.cat([comp0[:nsrc * F]] + [chunk(comp0, i) for i in dst]).contiguous()
                ops.pnp_blend_nchw(own, masks[k], frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=1, active=1, place=place[k])
                for d, i in enumerate(dst):
                    assert torch.equal(_i16(chunk(comp, i)), _i16(chunk(own, nsrc + d))), (what, k, d)
            assert torch.equal(_i16(comp[:nsrc * F]), _i16(comp0[:nsrc * F])), what
            n += 1
    assert n == 4 * 4 * (1 + 3 * 2)


# ---- degenerate cases ---------------------------------------------------------------------------------------------------------
def _both_layouts(g, nobj, K, ndst, smap, F, H, W, c):
    rows = F * H * W
    nsrc = nobj + 1 if smap is None else smap[0]
    tok = tp._planted(torch.randn((nsrc + ndst * K) * rows, 3 * c, generator=g).half(), g).cuda()
    nchw = tp._planted(torch.randn((nsrc + ndst * K) * F, 4, H, W, generator=g).half(), g).cuda()
    return tok, nchw


def test_one_variant_is_the_placed_entry():
    """nvar = 1 through the C entries themselves: the bits of the _placed entry with the same table and masks"""
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(21)
    F, c = F3, 16
    for (H, W), nobj, ndst, base0 in itertools.product(((4, 8), (3, 5)), (1, 2, 4), (1, 2), (False, True)):
        for smap in tp._maps(nobj):
            offs = _variant_offsets(1, nobj, F, H, W)
            offs[0][0] = [(1, -2), (-1, 1), (0, 2)]  # (object 0 inside the frame here)
            masks = _vmasks(1, nobj, F, 5, 9, True, g)
            tok, nchw = _both_layouts(g, nobj, 1, ndst, smap, F, H, W, c)
            tok2, nchw2 = tok.clone(), nchw.clone()
            place = _vtable(offs)
            assert _tokens_direct(tok, "temporal", F, H, W, c, masks, base0, ndst, smap, 1, 1, place) == 0
            tp._run_tokens(tok2, "temporal", F, H, W, c, masks[0], base0, ndst, smap, nvar=1, active=1, place=place[0])
            assert torch.equal(_i16(tok), _i16(tok2)), (H, W, nobj, ndst, base0, smap)
            assert _nchw_direct(nchw, masks, F, base0, ndst, smap, 1, 1, place) == 0
            ops.pnp_blend_nchw(nchw2, masks[0], frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=1, active=1, place=place[0])
            assert torch.equal(_i16(nchw), _i16(nchw2)), (H, W, nobj, ndst, base0, smap)


def test_equal_placements_are_the_placed_entry_with_that_placement():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(22)
    F, c = F3, 8
    for (H, W), nobj, (K, active), ndst, base0 in itertools.product(((4, 8), (3, 5)), (1, 3), ((2, 0b11), (3, 0b101), (8, 0xff)), (1, 2),
                                                                    (False, True)):
        for smap in tp._maps(nobj):
            one = _variant_offsets(2, nobj, F, H, W)[0]
            masks = tv._masks(nobj, F, 5, 9, True, g)
            tok, nchw = _both_layouts(g, nobj, K, ndst, smap, F, H, W, c)
            tok2, nchw2 = tok.clone(), nchw.clone()
            place, vmasks = _vtable([one] * K), torch.stack([masks] * K).contiguous()
            _run_tokens_v(tok, "spatial", F, H, W, c, vmasks, base0, ndst, smap, K, active, place)
            tp._run_tokens(tok2, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, place=_vtable(one))
            assert torch.equal(_i16(tok), _i16(tok2)), (H, W, nobj, K, ndst, base0, smap)
            ops.pnp_blend_nchw(nchw, vmasks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=place)
            ops.pnp_blend_nchw(nchw2, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=_vtable(one))
            assert torch.equal(_i16(nchw), _i16(nchw2)), (H, W, nobj, K, ndst, base0, smap)


def test_zero_tables_equal_the_variants_and_the_sel_entries():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(23)
    F, c = F3, 16
    for (H, W), nobj, (K, active), ndst, base0 in itertools.product(((4, 8), (3, 5)), (1, 3), ((2, None), (3, 0b101), (8, None), (8, 0x5a)),
                                                                    (1, 2), (False, True)):
        for smap in tv._maps(nobj)[:3]:
            masks = tv._masks(nobj, F, 5, 9, True, g)
            tok, nchw = _both_layouts(g, nobj, K, ndst, smap, F, H, W, c)
            tok2, nchw2 = tok.clone(), nchw.clone()
            zero, vmasks = torch.zeros(K, nobj, F, 2, dtype=torch.int32, device="cuda"), torch.stack([masks] * K).contiguous()
            _run_tokens_v(tok, "temporal", F, H, W, c, vmasks, base0, ndst, smap, K, active, zero)
            tp._run_tokens(tok2, "temporal", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active)  # _variants / _variants_sel
            assert torch.equal(_i16(tok), _i16(tok2)), (H, W, nobj, K, active, ndst, base0, smap)
            ops.pnp_blend_nchw(nchw, vmasks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=zero)
            ops.pnp_blend_nchw(nchw2, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active)
            assert torch.equal(_i16(nchw), _i16(nchw2)), (H, W, nobj, K, active, ndst, base0, smap)


def test_extreme_offsets_are_safe_and_mean_absent():
    """offsets of +-(2^31 - 1) (and -2^31): the call returns 0 and the result is that of objects absent everywhere -- the base
    blended with zero objects under zero masks"""
    from mvoc_amd import ops
    F, H, W, c, K = F3, 3, 5, 16, 2
    rows = F * H * W
    g = torch.Generator().manual_seed(24)
    masks = _vmasks(K, 2, F, H, W, False, g)
    big = 2 ** 31 - 1
    offs = [[[(big, -big), (-big, big), (big, big)], [(-big, -big), (0, big), (-big - 1, 0)]],
            [[(-big, 0), (0, -big), (-big - 1, -big - 1)], [(big, 1), (1, -big), (big, -big - 1)]]]
    for base0 in (True, False):
        comp = tp._planted(torch.randn(7 * rows, 3 * c, generator=g).half(), g).cuda()  # [bg, o1, o2, u_0, u_1, c_0, c_1]
        comp0, twin = comp.clone(), comp.clone()
        assert _tokens_direct(comp, "spatial", F, H, W, c, masks, base0, 2, None, K, 0b11, _vtable(offs)) == 0
        twin[rows:3 * rows] = 0.0
        tv._run_tokens(twin, "spatial", F, H, W, c, torch.zeros_like(masks[0]), base0, 2, nvar=K)
        assert torch.equal(_i16(comp[3 * rows:]), _i16(twin[3 * rows:])), base0
        assert torch.equal(_i16(comp[:3 * rows]), _i16(comp0[:3 * rows])), base0
        for hw in ((4, 8), (3, 5)):
            x = tp._planted(torch.randn(7 * F, 4, *hw, generator=g).half(), g).cuda()
            x0, y = x.clone(), x.clone()
            assert _nchw_direct(x, masks, F, base0, 2, None, K, 0b11, _vtable(offs)) == 0
            y[F:3 * F] = 0.0
            ops.pnp_blend_nchw(y, torch.zeros_like(masks[0]), frames=F, base_chunk0=base0, ndst=2, nvar=K)
            assert torch.equal(_i16(x[3 * F:]), _i16(y[3 * F:])) and torch.equal(_i16(x[:3 * F]), _i16(x0[:3 * F])), (base0, hw)


def test_placed_variants_entries_refuse_bad_arguments_and_write_nothing():
    from mvoc_amd import ops
    F, H, W, c, K = 2, 4, 4, 8, 3
    g = torch.Generator().manual_seed(0)
    masks = _vmasks(8, 2, F, H, W, False, g)  # (room for every nvar tried below)
    buf = torch.randn(19 * F * H * W, 3 * c, generator=g).half().cuda()
    nchw = torch.randn(19 * F, 4, H, W, generator=g).half().cuda()
    buf0, nchw0 = buf.clone(), nchw.clone()
    place = _vtable(_variant_offsets(8, 2, F, H, W))
    err = lambda: ops.lib.mvoc_last_error().decode()
    cases = [  # (nvar, active, map, table, text)
        (0, 1, None, place, "nvar 0"), (9, 1, None, place, "nvar 9"), (-1, 1, None, place, "nvar -1"),
        (3, 0, None, place, "active mask 0x0"), (3, 8, None, place, "active mask 0x8"), (1, 2, None, place, "active mask 0x2"),
        (8, 256, None, place, "active mask 0x100"),
        (2, 3, (0, (0, 0)), place, "nsrc 0"), (2, 3, (4, (0, 1)), place, "nsrc 4"), (2, 3, (2, (0, 2)), place, "obj_chunk[1] = 2"),
        (2, 3, (2, (-1, 0)), place, "obj_chunk[0] = -1"),
        (2, 3, None, None, "null offset table"),
    ]
    for nvar, active, smap, tab, text in cases:
        assert _tokens_direct(buf, "spatial", F, H, W, c, masks, False, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
        assert _nchw_direct(nchw, masks, F, True, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
    torch.cuda.synchronize()
    assert torch.equal(_i16(buf), _i16(buf0)) and torch.equal(_i16(nchw), _i16(nchw0))  # nothing was written
    # the Python layer: the forms of the table and of the mask stack, in the style of the shared placement's check
    run = lambda m, p, nvar=K: _run_tokens_v(buf, "spatial", F, H, W, c, m, False, 2, None, nvar, None, p)
    with pytest.raises(RuntimeError, match=r"int32 \[K = 3, nobj = 2, F = 2, 2\]"):
        run(masks[:K], place[:2])
    with pytest.raises(RuntimeError, match=r"needs masks as a contiguous \[K = 3, nobj = 2, F = 2, mh, mw\] stack"):
        run(masks[0], place[:K])
    with pytest.raises(RuntimeError, match=r"needs masks as a contiguous \[K = 3"):
        run(masks[:2], place[:K])
    with pytest.raises(RuntimeError, match=r"mask stack needs place= as an int32 \[K, nobj, F, 2\] table"):
        run(masks[:K], place[0])
    with pytest.raises(RuntimeError, match=r"mask stack needs place="):
        ops.pnp_blend_nchw(nchw, masks[:K], frames=F, ndst=2, nvar=K)
    with pytest.raises(RuntimeError, match="place"):
        ops.pnp_blend_nchw(nchw, masks[:K], frames=F, ndst=2, nvar=K, place=place[:K].long())
    with pytest.raises(RuntimeError, match="storage ends"):  # 3 + 2 * 8 chunks in a buffer of 9
        ops.pnp_blend_nchw(torch.zeros(9 * F, 4, H, W, dtype=torch.float16, device="cuda"), masks, frames=F, ndst=2, nvar=8, place=place)
    torch.cuda.synchronize()
    assert torch.equal(_i16(buf), _i16(buf0)) and torch.equal(_i16(nchw), _i16(nchw0))
    # a valid call with the same buffers goes through (the refusals above were about the arguments)
    assert _tokens_direct(buf, "spatial", F, H, W, c, masks, False, 2, None, 8, 0xff, place) == 0, err()
    assert _nchw_direct(nchw, masks, F, True, 2, None, 1, 1, place) == 0, err()
    torch.cuda.synchronize()
    assert not torch.equal(_i16(buf), _i16(buf0)) and not torch.equal(_i16(nchw), _i16(nchw0))


def test_profiler_counts_the_stated_bytes():
    """per tensor: every injecting variant reads the distinct object chunks and one mask value per object and pixel and writes
    ndst chunks; the base once when it is chunk 0, else once per injecting variant; + the table, 8 * nvar * nobj * F bytes"""
    from mvoc_amd import ops
    F, H, W, c, K, nobj = 2, 4, 4, 8, 3, 2
    rows = F * H * W
    masks = _vmasks(K, nobj, F, H, W, False, torch.Generator().manual_seed(0))
    place = _vtable(_variant_offsets(K, nobj, F, H, W))
    chunk_bytes, table = 2.0 * rows * c, 8.0 * K * nobj * F
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
            _run_tokens_v(buf, "spatial", F, H, W, c, masks, base0, ndst, smap, K, active, place)
            torch.cuda.synchronize()
            t = ops.prof_collect()["pnp"]
            ops.prof_reset()
            ops.pnp_blend_nchw(nchw, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, place=place)
            torch.cuda.synchronize()
            n = ops.prof_collect()["pnp"]
            assert t["launches"] == 1 and t["work"] == 2 * want + table, (base0, ndst, smap, active, t, 2 * want + table)  # q and k
            assert n["launches"] == 1 and n["work"] == want + table, (base0, ndst, smap, active, n, want + table)
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


# ---- engine -------------------------------------------------------------------------------------------------------------
PL_A = (((1, -2), (0, 1), (-2, 0)), ((3, 2),) * F3)  # a per-frame path and one constant offset ((dy, dx) on the latent grid)
PL_B = (((-1, 1),) * F3, ((0, -3), (2, 2), (-8, 0)))  # ... object 1 leaves the frame in the last frame
PL_0 = (((0, 0),) * F3,) * 2


@pytest.mark.parametrize("kind", ["qk", "conv_out", "features"])
def test_unet_variant_placements_equal_the_single_variant_placed_forwards(kind):
    """K = 3 under variant_placements (A, zeros, B): variant k's destination chunks are those of the single-variant forward
    with placement k (the zero variant: the unplaced forward), for a Q/K step, a conv_out step (the NCHW blend on the source
    chunks' outputs) and, with prune_dead_chunks off, the same step through the resnet / temporal-conv feature sites"""
    from mvoc_amd import ops, pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    F, h, w, cd, K = F3, 8, 8, 64, 3
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    vp = (PL_A, PL_0, PL_B)
    glue = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False)
    vstate = glue.place_variant_masks(masks, vp)
    assert [t.tolist() for t in vstate["place_dev"]] == [[list(map(list, o)) for o in pl] for pl in vp]
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
        got = forward(names, variants=K, variant_placements=vp, variant_masks=vstate["masks"])
        tables = dict(eng._level_tables["variant_placements"][1])
        plain = forward(names, variants=K)
        refs = []
        for k, pl in enumerate(vp):
            moved = masks if pl is PL_0 else glue.place_masks(masks, pl)[0]
            pnp_utils.register_time_all(pipe, t, moved)
            refs.append(forward(src + [f"u{k}", f"c{k}"], placement=None if pl is PL_0 else pl))
    finally:
        eng.prune_dead_chunks = saved
        tv._disarm(eng, pipe)
    torch.cuda.synchronize()
    assert eng.variant_placements is None and eng.variant_masks is None and eng.variants == 1
    levels = {key[:2] for key in tables}  # every site was handed the [K, nobj, F, 2] table of its own level
    assert levels == {"qk": {(8, 8), (4, 4), (2, 2)}, "conv_out": {(8, 8)}}.get(kind, levels) and (8, 8) in levels, (kind, levels)
    for (H, W, mh, mw), tab in tables.items():
        assert (mh, mw) == (h, w) and tab.tolist() == [[list(map(list, o)) for o in ops.level_offsets(pl, H, W, h, w)] for pl in vp]
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
    for k in (0, 2):  # the placements moved something; the zero variant is the unplaced one
        assert not torch.equal(got[3 + K + k], plain[3 + K + k]), (kind, k)
    assert torch.equal(_i16(got[3 + K + 1]), _i16(plain[3 + K + 1])), kind


def test_unet_refuses_variant_placements_it_cannot_run():
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
        eng.variant_placements = (PL_A, PL_B)
        with pytest.raises(RuntimeError, match="variant_placements holds 2 placements, the call 3 variants"):
            tv._fwd(eng, tv._batch(roles, names), t_qk)
        eng.variant_placements = (PL_A, PL_0, PL_B[:1])
        with pytest.raises(RuntimeError, match=r"variant_placements\[2\] holds offsets for 1 objects, the hooks carry 2 masks"):
            tv._fwd(eng, tv._batch(roles, names), t_qk)
        eng.variant_placements, eng.placement = (PL_A, PL_0, PL_B), PL_A
        with pytest.raises(RuntimeError, match="variant_placements and placement are both set"):
            tv._fwd(eng, tv._batch(roles, names), t_qk)
        eng.placement, eng.shard = None, types.SimpleNamespace(rank=0, world=1)
        with pytest.raises(RuntimeError, match="frame shard"):
            eng.pnp_batch(9, masks)
        with pytest.raises(RuntimeError, match="frame shard"):
            eng.place_table(masks, 8, 8)
    finally:
        eng.variants, eng.variant_masks, eng.variant_placements, eng.placement, eng.shard = 1, None, None, None, None
        tv._disarm(eng, pipe)
    assert eng.place_kw(masks, 8, 8) == {}


# ---- pipeline -----------------------------------------------------------------------------------------------------------
OFF_A = [tp.PATH, (-16, 8)]  # object 0 follows a path, object 1 moves by one pair (dx, dy in image pixels)
OFF_B = [(-8, 16), [(0, -24), (16, 16), (0, -64)]]  # ... object 1 leaves the frame in the last frame
GUIDANCE = (9.0, 6.0, 7.5)
SPATIAL_STEPS = (3, 1, 5)  # per-variant thresholds: spatial Q/K injection stops after that many of the five steps


def _job(graphs, K=3, only=None, variant_offsets="none", offsets="none", thresholds=False, dedup=False, count_calls=False,
         shard=False):
    """test_placement_gpu.py's toy composition (two objects, five steps, fusion on the first two) with K variants.
    ``only`` = k: the single-variant call of variant k (its prompt, latents, guidance scale, main image -- and, with
    ``thresholds``, its spatial schedule as the shared one).  ``variant_offsets`` / ``offsets``: "none" = the call without the
    argument.  ``dedup``: one source behind every role and ``dedup_sources`` on (two objects on the background's chunk)."""
    from launch_census import Recorder
    from mvoc_amd import pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    _, eng = tv._toy_pair()
    g = torch.Generator().manual_seed(5)
    f, h, w, cd, n = F3, 8, 8, 64, 5
    nrow = 3 + 2 * K  # rows: bg, obj_1, obj_2, then (u_k, c_k) per variant
    cond = dict(encoder_hidden_states=torch.randn(nrow, 7, cd, generator=g).half(), image_embeddings=torch.randn(nrow, f, cd, generator=g).half(),
                image_latents_first=torch.randn(nrow, 4, f, h, w, generator=g).half(), image_latents=torch.randn(nrow, 4, f, h, w, generator=g).half())
    for key in cond:
        if dedup or key == "encoder_hidden_states":  # (the inversion prompt is one for all sources)
            cond[key][1] = cond[key][0]
            cond[key][2] = cond[key][0]
    for k in range(K):
        u, c = 3 + 2 * k, 4 + 2 * k
        cond["image_embeddings"][u] = 0
        cond["image_latents_first"][u] = cond["image_latents_first"][c]
        cond["image_latents"][c] = cond["image_latents_first"][c]
        cond["image_latents"][u] = cond["image_latents"][c]
    cpu_masks, _ = tv._hook_masks(f, h, w)
    s = DDIMScheduler()
    s.set_timesteps(n)
    dirs = ["/virtual/bg"] * 3 if dedup else ["/virtual/bg", "/virtual/o1", "/virtual/o2"]
    src = {d: {int(t): torch.randn(1, 4, f, h, w, generator=g).half() for t in s.timesteps} for d in dict.fromkeys(dirs)}
    x0 = torch.randn(K, 4, f, h, w, generator=g).half()
    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=graphs)
    pipe.dedup_sources = dedup
    ts = s.timesteps
    shared_spatial = SPATIAL_STEPS[only] if (thresholds and only is not None) else 3
    pnp_utils.register_temp_attention_pnp(pipe, ts[:4], False)
    pnp_utils.register_spatial_attention_pnp(pipe, ts[:shared_spatial], False)
    pnp_utils.register_temp_conv_injection(pipe, ts[:1])
    pnp_utils.register_out_conv_injection(pipe, ts[:1])
    pnp_utils.register_resnet_injection(pipe, ts[:1])
    if thresholds and only is None:
        pnp_utils.register_variant_schedules(pipe, spatial=[ts[:m] for m in SPATIAL_STEPS])
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
    if only is not None:
        k = only
        var = dict(prompt=f"edit{k}", main_first_image=(4 + 2 * k, 0, True), main_image_list=[(4 + 2 * k, i, False) for i in range(f)],
                   latents=x0[k:k + 1].cuda(), guidance_scale=GUIDANCE[k], negative_prompt="neg")
    else:
        var = dict(prompt=[f"edit{k}" for k in range(K)], main_first_image=[(4 + 2 * k, 0, True) for k in range(K)],
                   main_image_list=[[(4 + 2 * k, i, False) for i in range(f)] for k in range(K)], latents=x0.cuda(),
                   guidance_scale=[GUIDANCE[k] for k in range(K)], negative_prompt=["neg"] * K)
    if offsets != "none":
        var["obj_offsets"] = offsets
    if variant_offsets != "none":
        var["variant_obj_offsets"] = variant_offsets
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


def _compare_with_singles(job, singles, what):
    for k, one in enumerate(singles):
        a, b = job.out[k], one.out[0]
        diff = float((a.float() - b.float()).abs().max())
        print(f"{what}: variant {k} final latents vs its single-variant call: max-abs {diff:.3e}"
              f"{' (bit-identical)' if torch.equal(_i16(a), _i16(b)) else ''}")
    for k, one in enumerate(singles):
        assert torch.equal(_i16(job.out[k]), _i16(one.out[0])), (what, k)


def test_three_placements_in_one_loop_equal_three_single_calls_and_graph_replay():
    """variant_obj_offsets = [A, None, B]: the final latents of variant k are those of the single-variant call with obj_offsets
    A, none and B (two fusion steps included); graph replay equals eager"""
    eager = _job(False, variant_offsets=[OFF_A, None, OFF_B], count_calls=True)
    st = eager.state
    assert st["placement"] is None and st["place_dev"] is None
    assert st["variant_placements"] == ((((0, 1), (-1, 2), (-2, 3)), ((1, -2),) * 3), (((0, 0),) * 3,) * 2,
                                        (((2, -1),) * 3, ((-3, 0), (2, 2), (-8, 0))))
    # every variant's masks moved once, to ITS destination coordinates: the engine's stacks and the fusion masks
    soft, hard = st["vplace"]["masks"]
    for k, pl in enumerate(st["variant_placements"]):
        for j, obj in enumerate(pl):
            for f, (dy, dx) in enumerate(obj):
                want = tp._shifted(eager.masks[j][0][0, 0, f].cuda(), dy, dx)
                assert torch.equal(soft[k, j, f], want) and torch.equal(st["vplace"]["fusion_masks"][k][j, 0, 0, f], want)
                assert torch.equal(hard[k, j, f], tp._shifted(eager.masks[j][1][0, 0, f].cuda().half(), dy, dx))
    # the hooks keep the call's masks as they came; the per-level [K, nobj, F, 2] tables stay alive with the state
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(st["masks"], eager.masks))
    assert len(st["place_tables"]) == 1 and {k[:2] for k in st["place_tables"][0]} == {(8, 8), (4, 4), (2, 2)}
    assert all(tuple(t.shape) == (3, 2, 3, 2) for t in st["place_tables"][0].values())
    names = set().union(*eager.step_calls)
    assert {"mvoc_pnp_blend_scatter_tokens_placed_variants", "mvoc_pnp_blend_scatter_nchw_placed_variants", "mvoc_shift_planes_f16"} <= names
    assert not any(n.startswith("mvoc_pnp_blend") and not n.endswith("_placed_variants") for n in names), names
    # two fusion steps: per variant the two fusion objects through the shift kernel and one single-variant fusion launch
    assert [c.get("mvoc_shift_planes_f16", 0) for c in eager.step_calls] == [6, 6, 0, 0, 0]
    assert [c.get("mvoc_latent_fusion_f16", 0) for c in eager.step_calls] == [3, 3, 0, 0, 0]
    assert not any("mvoc_latent_fusion_variants_f16" in c for c in eager.step_calls)
    singles = [_job(False, only=0, offsets=OFF_A), _job(False, only=1), _job(False, only=2, offsets=OFF_B)]
    assert singles[0].state["placement"] == st["variant_placements"][0] and singles[1].state["placement"] is None
    _compare_with_singles(eager, singles, "eager")
    graphed = _job(True, variant_offsets=[OFF_A, None, OFF_B])
    assert graphed.graphs >= 3 and torch.equal(_i16(graphed.out), _i16(eager.out)) and torch.isfinite(eager.out).all()
    plain = _job(False)
    for k in (0, 2):
        assert not torch.equal(plain.out[k], eager.out[k]), k  # the placements moved the result


def test_variant_placements_with_per_variant_thresholds():
    job = _job(True, variant_offsets=[OFF_A, None, OFF_B], thresholds=True)
    singles = [_job(True, only=0, offsets=OFF_A, thresholds=True), _job(True, only=1, thresholds=True),
               _job(True, only=2, offsets=OFF_B, thresholds=True)]
    _compare_with_singles(job, singles, "per-variant thresholds")
    assert job.graphs == 4  # spatial Q/K injects for 3 / 1 / 5 steps: steps 0, 1..2, 3, 4 are four kinds


def test_variant_placements_with_deduplicated_sources():
    """one source behind every role: both objects read the background's chunk, each variant at its own offsets"""
    job = _job(False, variant_offsets=[OFF_B, OFF_A, None], dedup=True, count_calls=True)
    assert any(m is not None for m in job.state["maps"]), job.state["maps"].keys()  # a de-duplicated batch did run
    singles = [_job(False, only=0, offsets=OFF_B, dedup=True), _job(False, only=1, offsets=OFF_A, dedup=True), _job(False, only=2, dedup=True)]
    _compare_with_singles(job, singles, "dedup_sources")
    graphed = _job(True, variant_offsets=[OFF_B, OFF_A, None], dedup=True)
    assert torch.equal(_i16(graphed.out), _i16(job.out))


def _same_calls(a, b, forbidden):
    assert len(a.step_calls) == len(b.step_calls) == 5
    for i, (ca, cb) in enumerate(zip(a.step_calls, b.step_calls)):
        assert ca == cb and sum(ca.values()) > 0, (i, {k: (ca.get(k), cb.get(k)) for k in set(ca) | set(cb) if ca.get(k) != cb.get(k)})
        assert not any(forbidden(n) for n in cb), (i, cb)
    assert torch.equal(_i16(a.out), _i16(b.out))


def test_equal_variant_offsets_make_the_calls_and_graphs_of_the_shared_placement():
    shared, equal = _job(False, offsets=OFF_A, count_calls=True), _job(False, variant_offsets=[OFF_A] * 3, count_calls=True)
    assert equal.state["variant_placements"] is None and equal.state["vplace"] is None
    assert equal.state["placement"] == shared.state["placement"] is not None
    _same_calls(shared, equal, lambda n: n.endswith("_placed_variants"))
    assert any(n.endswith("_placed") for c in equal.step_calls for n in c)
    gs, ge = _job(True, offsets=OFF_A), _job(True, variant_offsets=[OFF_A] * 3)
    keys = lambda job: {(k[0],) + k[2:] for k in job.state["variants"]}  # (without the mask key: the ids of each job's own tensors)
    assert gs.graphs == ge.graphs >= 3 and keys(gs) == keys(ge)
    assert torch.equal(_i16(gs.out), _i16(ge.out)) and torch.equal(_i16(gs.out), _i16(shared.out))


def test_none_or_zero_variant_offsets_make_the_calls_and_graphs_of_a_call_without_them():
    zeros = [None, [[(0, 0)] * 3, (0, 0)], None]
    plain, zero = _job(False, count_calls=True), _job(False, variant_offsets=zeros, count_calls=True)
    assert zero.state["variant_placements"] is None and zero.state["placement"] is None and zero.state["place_dev"] is None
    _same_calls(plain, zero, lambda n: "_placed" in n or n == "mvoc_shift_planes_f16")
    gp, gz = _job(True), _job(True, variant_offsets=zeros)
    assert gp.graphs == gz.graphs >= 3 and torch.equal(_i16(gp.out), _i16(gz.out)) and torch.equal(_i16(gp.out), _i16(plain.out))


def test_a_frame_sharded_pipeline_refuses_variant_offsets():
    with pytest.raises(RuntimeError, match="frame shard"):
        _job(False, variant_offsets=[OFF_A, None, OFF_B], shard=True)


def test_the_call_refuses_both_arguments_and_a_wrong_length():
    with pytest.raises(ValueError, match="obj_offsets and variant_obj_offsets are both given"):
        _job(False, offsets=OFF_A, variant_offsets=[OFF_A, None, OFF_B])
    with pytest.raises(ValueError, match="2 entries for 3 variants"):
        _job(False, variant_offsets=[OFF_A, OFF_B])
