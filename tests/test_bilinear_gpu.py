"""GPU: bilinear sampling of warped objects on an exact fp16 chain.

* kernels: the ``_bilinear`` blend entries against the EXISTING unplaced entries on inputs interpolated beforehand in torch -- the
  chain restated with CPU fp16 operations only (one multiply or add per statement; torch rounds each once), object chunks
  interpolated through the tap table with +0.0 for a tap outside the plane, masks nearest-resized to H x W and zeroed where no tap
  is inside.  The WHOLE allocation is compared after the call, as int16, as tests/test_warp_gpu.py does: every element outside
  the described tensors holds NaN, and so does every chunk the contract says is not read.  Every case asserts that its result
  DIFFERS from the untransformed call and from the nearest (``_warped``) call.  A table with weights 0 returns the ``_warped``
  entry's values; every int32 pair is safe; ``warp_planes_bilinear`` against the torch chain; bad arguments refused.
* engine: a forward with ``warp`` + ``warp_filter = "bilinear"`` against the same forward with the blend functions replaced by
  "interpolate in torch, call the unplaced entry, restore the sources".
* pipeline: graph replay against eager, a translation-only call under the filter against the ``obj_offsets`` call, "nearest"
  against a call without the argument, the fusion steps, the refusals.

Helpers come from tests/test_warp_gpu.py so that the files judge by the same bars.  Inputs are finite everywhere inside the planes.
"""
import contextlib
import ctypes as C
import itertools
import types

import pytest
import torch

import pnp_contract as pc
import test_placement_gpu as tp
import test_resample_gpu as tr
import test_variants_gpu as tv
import test_warp_gpu as tw

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_i16, _Batch, _fill, _assert_bits = tw._i16, tw._Batch, tw._fill, tw._assert_bits
VARIANTS = tr.VARIANTS  # (nvar, active): one variant; two with every bit set; two with a partial mask
GUARD, NAN, D = pc.GUARD, float("nan"), 65536
F16 = torch.float16
C30, S30 = 56756, 32768


# ---- the chain in torch: CPU fp16 operations only ---------------------------------------------------------------------------------
def _decode(words):
    """int32 [n, 2] -> (row, column) of the upper-left tap and the two 9-bit weights, as the kernels read ANY pair"""
    w = words.detach().cpu().to(torch.int64) & 0xFFFFFFFF
    return (w[:, 0] >> 16) - 1, (w[:, 0] & 0xFFFF) - 1, (w[:, 1] >> 16) & 0x1FF, w[:, 1] & 0x1FF


def _interp(src, words):
    """src [H, W, ...] fp16 (any device) -> (the interpolated plane on src's device, the [H, W] bool 'present' plane).  One fp16
    operation per statement, on the CPU"""
    H, W = src.shape[:2]
    flat = src.detach().cpu().reshape(H * W, -1)
    r0, c0, qy, qx = _decode(words)
    assert r0.numel() == H * W

    def tap(r, c):
        ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        idx = torch.where(ok, r * W + c, torch.zeros_like(r))
        return torch.where(ok[:, None], flat[idx], torch.zeros_like(flat)), ok  # +0.0 where the tap is outside

    (v00, k00), (v01, k01), (v10, k10), (v11, k11) = tap(r0, c0), tap(r0, c0 + 1), tap(r0 + 1, c0), tap(r0 + 1, c0 + 1)
    u = torch.tensor(1.0 / 256, dtype=F16)
    wx1 = (qx.to(F16) * u)[:, None]
    wx0 = ((256 - qx).to(F16) * u)[:, None]
    wy1 = (qy.to(F16) * u)[:, None]
    wy0 = ((256 - qy).to(F16) * u)[:, None]

    def lerp(a, b, w0, w1):
        x = a * w0
        y = b * w1
        return x + y

    top = lerp(v00, v01, wx0, wx1)
    bot = lerp(v10, v11, wx0, wx1)
    v = lerp(top, bot, wy0, wy1)
    assert v.dtype == F16
    present = k00 | k01 | k10 | k11
    v = torch.where(present[:, None], v, torch.zeros_like(v))
    return v.view(src.shape).to(src.device), present.view(H, W)


def _masks_eff(masks, taps, H, W):
    """the masks of the interpolated twin: nearest-resized to H x W by the entries' own rule, zero where the object is absent"""
    ny = torch.tensor(pc.near(H, masks.shape[2]), device=masks.device)
    nx = torch.tensor(pc.near(W, masks.shape[3]), device=masks.device)
    m = masks[:, :, ny][:, :, :, nx].clone()
    for j in range(taps.shape[0]):
        for f in range(taps.shape[1]):
            r0, c0, _, _ = _decode(taps[j, f])
            present = ((r0 >= -1) & (r0 <= H - 1) & (c0 >= -1) & (c0 <= W - 1)).view(H, W)
            m[j, f] *= present.to(m.device, m.dtype)
    return m.contiguous()


def _expect(b, before, masks, taps, base0, ndst, smap, K, active):
    """the allocation the bilinear call must leave: ``before`` with, per injecting variant, the rows the POSITIONAL unplaced entry
    writes on that variant's own batch [bg, interpolated obj_1.., (u_k,) c_k]"""
    nobj, F, H, W, c = masks.shape[0], b.F, b.H, b.W, b.c
    nsrc = nobj + 1 if smap is None else smap[0]
    order = tv._src_order(smap, nobj)
    meff = _masks_eff(masks, taps, H, W)
    exp = _Batch(b.layout, b.nchunk, F, H, W, c, b.T, lead=(b.x[0].data_ptr() % 256) // 2)
    for t in range(b.T):
        _i16(exp.flat[t]).copy_(before[t])
    twin_layout = "nchw" if b.layout == "nchw" else "spatial"
    for t in range(b.T):
        src = b.logical(t)
        objs = [[_interp(src[order[1 + j], f], taps[j, f])[0] for f in range(F)] for j in range(nobj)]  # once, shared by the variants
        for k in range(K):
            if not (active >> k) & 1:
                continue
            dst = [nsrc + d * K + k for d in range(ndst)]
            twin = _Batch(twin_layout, nobj + 1 + ndst, F, H, W, c, 1)
            lg = twin.logical(0)
            lg[0] = src[order[0]]
            for j in range(nobj):
                for f in range(F):
                    lg[1 + j, f] = objs[j][f]
            for d, i in enumerate(dst):
                lg[nobj + 1 + d] = src[i]
            twin.run(meff, base0, ndst)
            for d, i in enumerate(dst):
                exp.logical(t)[i] = lg[nobj + 1 + d]
    return exp.bits()


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def _spec_warp(nobj, H, W, F=3):
    """per object the engine's warp value on a latent grid equal to the site: a 30-degree turn at scale 3/2 on a per-frame path;
    scale 1/2 about an anchor off the centre; -15 degrees, one frame moved entirely out of the plane; the first object again, on
    another path"""
    path = ((0, 0), (2, -2), (-2, 2))
    turn = (2 * C30, 2 * S30, -2 * S30, 2 * C30, 3 * D)  # the inverse of (3/2) * R(30 degrees)
    objs = [(H, W, tuple(turn + path[f % 3] for f in range(F))),
            (3, W + 1, tuple((2, 0, 0, 2, 1) + ((0, 0), (0, 1))[f % 2] for f in range(F))),
            (H, W, tuple((63303, -16962, 16962, 63303, D) + ((0, 0), (3 * H + 3, 0))[f % 2] for f in range(F))),
            (H - 1, W + 2, tuple(turn + path[(f + 1) % 3] for f in range(F)))]
    return tuple(objs[:nobj])


def _check_spec(taps, H, W):
    """what the two-object tables must exercise, over all (object, frame) planes: fractional weights on both axes at once, taps
    across each of the four borders of a present pixel, absent pixels; from three objects on, a fully absent (object, frame)"""
    flat = taps.reshape(-1, 2)
    r0, c0, qy, qx = _decode(flat)
    here = flat[:, 0] != -1
    frac = lambda q: (q > 0) & (q < 256)
    assert (frac(qy) & frac(qx) & here).any()
    assert (here & (r0 == -1)).any() and (here & (r0 == H - 1) & (qy > 0)).any()  # across the upper and the lower border
    assert (here & (c0 == -1)).any() and (here & (c0 == W - 1) & (qx > 0)).any()  # ... and across the left and the right one
    assert (~here).any()
    if taps.shape[0] >= 3:
        assert bool((taps[2, 1, :, 0] == -1).all()) and bool((taps[2, 0, :, 0] != -1).any())


def _spec_taps(nobj, H, W, F=3, grid=None):
    """-> (the device table of ``ops.warp_tap_table``, its CPU copy)"""
    from mvoc_amd import ops
    lh, lw = grid or (H, W)
    dev = ops.warp_tap_table(_spec_warp(nobj, lh, lw, F), H, W, lh, lw, "cuda")
    taps = dev.cpu()
    assert tuple(taps.shape) == (nobj, F, H * W, 2) and dev.dtype == torch.int32 and dev.is_contiguous()
    if grid is None and nobj >= 2:
        _check_spec(taps, H, W)
    return dev, taps


# ---- 1: the torch yardstick -------------------------------------------------------------------------------------------------------
SITES = [(5, 6, 0), (4, 6, 0), (4, 6, 1)]  # (H, W, lead): hw % 8 != 0 (VEC 1); VEC 8; VEC 8's shape 2 bytes off (VEC 1)


@pytest.mark.parametrize("layout", ["spatial", "temporal", "nchw"])
@pytest.mark.parametrize("site", SITES, ids=["5x6", "4x6", "4x6+2B"])
def test_bilinear_entries_equal_the_existing_entries_on_interpolated_inputs(site, layout):
    from mvoc_amd import ops
    H, W, lead = site
    F = 3
    g = torch.Generator().manual_seed(100 * H + 10 * lead + len(layout))
    n = 0
    seen = set()
    for nobj in (1, 2, 4):
        tables = {None: _spec_taps(nobj, H, W, F), (8, 12): _spec_taps(nobj, H, W, F, (8, 12))}
        nearest = ops.warp_table(_spec_warp(nobj, H, W, F), H, W, H, W, "cuda")
        for ndst, base0, (K, active), smap in itertools.product((1, 2), (False, True), VARIANTS, tp._maps(nobj)):
            x2, c, grid = bool(n % 2), (8, 16)[(n // 2) % 2], (None, (8, 12))[(n // 3) % 2]
            seen.add((x2, c, grid))
            mh, mw = grid or (H, W)
            dev, taps = tables[grid]
            masks = tv._masks(nobj, F, mh, mw, soft=bool((n // 5) % 2), g=g)
            nsrc = nobj + 1 if smap is None else smap[0]
            what = (nobj, ndst, base0, K, bin(active), smap, x2, c, grid)
            b = _Batch(layout, nsrc + ndst * K, F, H, W, c, 2 if x2 else 1, lead)
            _fill(b, nsrc, smap, nobj, base0, ndst, K, active, g)
            before = b.bits()
            n += 1
            if lead and layout != "nchw":  # the tokens entries read 16-byte vectors only: refused, nothing written
                assert b.direct("_bilinear", masks, base0, ndst, smap, K, active, dev) == -2, what
                _assert_bits(b.bits(), before, what)
                continue
            want = _expect(b, before, masks, taps, base0, ndst, smap, K, active)
            b.run(masks, base0, ndst, smap, nvar=K, active=active, warp_taps=dev)
            got = b.bits()
            _assert_bits(got, want, what)
            # the untransformed call and the nearest call on the same inputs write something else: the taps and weights matter
            for kw in [{}] + ([{"warp": nearest}] if grid is None else []):
                for t in range(b.T):
                    _i16(b.flat[t]).copy_(before[t])
                b.run(masks, base0, ndst, smap, nvar=K, active=active, **kw)
                assert any(not torch.equal(a, p) for a, p in zip(got, b.bits())), (what, list(kw))
    assert n == sum(len(tp._maps(k)) for k in (1, 2, 4)) * 2 * 2 * len(VARIANTS) == 60
    assert len(seen) == 8  # x2 given and not, C = 8 and 16, the latent grid equal to the site and 8 x 12: every combination


@pytest.mark.parametrize("group", ["tokens", "nchw8", "nchw1"])
def test_work_item_totals_around_the_block_size(group):
    """255, 256, 257 and 513 work items per tensor: the last block's idle lanes, exactly full blocks, one item in a new block"""
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(7)
    for (F, H, W, c), total in zip(pc.TOTALS[group], pc.TOTAL_TARGETS):
        layout = "spatial" if group == "tokens" else "nchw"
        assert total == (F * H * W * c // 8 if group != "nchw1" else F * H * W * c)
        assert group != "nchw8" or (H * W) % 8 == 0
        lead = 1 if group == "nchw1" and (H * W) % 8 == 0 else 0  # (64, 2, 2, 1) would take the 8-wide form: 2 bytes off, it cannot
        warp = ((H, W, tuple((C30, S30, -S30, C30, D, f % 2, -(f % 2)) for f in range(F))),
                (H + 1, W - 1, ((3, 0, 0, 3, 2, 0, 0),) * F))  # a turn on a path; scale 2/3 about a point off the centre
        dev = ops.warp_tap_table(warp, H, W, H, W, "cuda")
        masks = tv._masks(2, F, max(1, (H + 1) // 2), max(1, (W + 2) // 3), True, g)
        for base0, (K, active) in ((True, (2, 0b10)), (False, (1, 0b1))):
            b = _Batch(layout, 3 + 2 * K, F, H, W, c, 2, lead)
            _fill(b, 3, None, 2, base0, 2, K, active, g)
            before = b.bits()
            want = _expect(b, before, masks, dev.cpu(), base0, 2, None, K, active)
            b.run(masks, base0, 2, None, nvar=K, active=active, warp_taps=dev)
            _assert_bits(b.bits(), want, (group, total, base0, K))
            assert any(not torch.equal(a, p) for a, p in zip(b.bits(), before))


# ---- 2: identity weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["spatial", "temporal", "nchw"])
def test_a_table_of_zero_weights_returns_the_values_of_the_warped_entry(layout):
    """a quarter turn on a square site and an integer translation: q = 0 everywhere and (y0, x0) is the nearest map's pixel, so the
    chain is v * 1 + (neighbours) * 0 = v for sources without -0.0 (+0.0 stands in for them here).  The masks are in destination
    coordinates, as the entries document: zero where the nearest map says absent -- a pixel whose only tap inside the plane has
    weight 0 counts as present under the tap rule, with value 0"""
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(41)
    F, c = 3, 8
    quarter = lambda k: ((1, 0), (0, 1), (-1, 0), (0, -1))[k % 4]
    cases = [((6, 6), tuple((6, 6, tuple((quarter(k + f)[0], quarter(k + f)[1], -quarter(k + f)[1], quarter(k + f)[0], 1, 0, 0)
                                         for f in range(F))) for k in (1, 2))),
             ((4, 6), ((4, 6, ((1, 0, 0, 1, 1, 1, -1), (1, 0, 0, 1, 1, -2, 3), (1, 0, 0, 1, 1, 0, 0))),
                       (4, 6, ((1, 0, 0, 1, 1, 0, 2), (1, 0, 0, 1, 1, 7, 0), (1, 0, 0, 1, 1, -1, -1))))),
             ((5, 6), ((5, 6, ((1, 0, 0, 1, 1, 2, 1),) * F), (5, 6, ((1, 0, 0, 1, 1, -1, 0),) * F)))]
    for (H, W), warp in cases:
        taps, nearest = ops.warp_tap_table(warp, H, W, H, W, "cuda"), ops.warp_table(warp, H, W, H, W, "cuda")
        assert not bool((taps[..., 1] != 0).any())  # q = 0 on both axes, everywhere
        word = torch.where(nearest >= 0, ((nearest // W + 1) << 16) | (nearest % W + 1), torch.full_like(nearest, -1))
        inside = nearest >= 0
        assert torch.equal(taps[..., 0][inside], word[inside])  # (y0, x0) is the nearest pixel wherever that is inside
        masks = tv._masks(2, F, H, W, True, g) * inside.view(2, F, H, W).half()  # destination coordinates
        for (K, active), base0 in itertools.product(VARIANTS, (False, True)):
            b = _Batch(layout, 3 + 2 * K, F, H, W, c, 2)
            _fill(b, 3, None, 2, base0, 2, K, active, g)
            for f in b.flat:
                f[f == 0] = 0.0  # no -0.0 in any input
            before = b.bits()
            b.run(masks, base0, 2, None, nvar=K, active=active, warp_taps=taps)
            got = [x.clone() for x in b.x]
            got_bits = b.bits()
            for t in range(2):
                _i16(b.flat[t]).copy_(before[t])
            b.run(masks, base0, 2, None, nvar=K, active=active, warp=nearest)
            for t in range(2):
                written = ~torch.isnan(got[t])
                assert torch.equal(torch.isnan(b.x[t]), ~written) and bool((got[t][written] == b.x[t][written]).all()), (H, W, K, active, base0)
            assert any(not torch.equal(a, p) for a, p in zip(got_bits, before))


# ---- 3: table safety --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["spatial", "temporal", "nchw"])
def test_every_int32_pair_is_safe(layout):
    """random 64-bit garbage and the corner cases -- -1, INT32_MAX, rows / columns equal to H / W, weights above 256: no read lands
    outside the object chunks (every element around them is NaN and none reaches an output: the outputs are finite wherever the
    reference is, and equal to it), and nothing but the described destinations is written"""
    g = torch.Generator().manual_seed(53)
    F, c, nobj = 3, 8, 2
    for (H, W), base0 in itertools.product(((4, 6), (5, 6)), (True, False)):
        hw = H * W
        taps = torch.randint(-2 ** 63, 2 ** 63 - 1, (nobj, F, hw), generator=g, dtype=torch.int64).view(torch.int32).view(nobj, F, hw, 2).clone()
        word0 = lambda y0, x0: ((((y0 + 1) & 0xFFFF) << 16) | ((x0 + 1) & 0xFFFF))
        corner = [(-1, -1), (pc.I32MAX, pc.I32MAX), (pc.I32MIN, pc.I32MIN), (0, 0), (-1, (300 << 16) | 511), (word0(H, 0), 0),
                  (word0(0, W), 0), (word0(H - 1, W - 1), (256 << 16) | 256), (word0(H - 1, W - 1), (257 << 16) | 400),
                  (word0(-1, -1), (128 << 16) | 128), (word0(H, W), -1), (word0(65534, 65534), 0), (word0(2, 65534), (7 << 16) | 9)]
        for i, (a, bb) in enumerate(corner):
            wrap = lambda v: v - 2 ** 32 if v >= 2 ** 31 else v
            taps[i % nobj, i % F, i % hw] = torch.tensor([wrap(a & 0xFFFFFFFF), wrap(bb & 0xFFFFFFFF)], dtype=torch.int32)
        # a third of the pairs name taps around the plane with garbage weights: most of the random ones lie far outside
        r = torch.randint(-2, H + 1, (nobj, F, hw), generator=g)
        cc = torch.randint(-2, W + 1, (nobj, F, hw), generator=g)
        near_plane = (((r + 1) & 0xFFFF) << 16 | ((cc + 1) & 0xFFFF)).to(torch.int32)
        pick = torch.rand(nobj, F, hw, generator=g) < 0.34
        for i in range(len(corner)):
            pick[i % nobj, i % F, i % hw] = False  # the corner cases stay
        taps[..., 0] = torch.where(pick, near_plane, taps[..., 0])
        reads = [bool(_interp(torch.zeros(H, W, 1, dtype=F16), taps[j, f])[1].any()) for j in range(nobj) for f in range(F)]
        assert all(reads)  # in every (object, frame) some pairs do read the plane
        dev = taps.cuda().contiguous()
        masks = tv._masks(nobj, F, H, W, True, g)
        for K, active in VARIANTS:
            b = _Batch(layout, 3 + 2 * K, F, H, W, c, 2)
            _fill(b, 3, None, nobj, base0, 2, K, active, g)
            before = b.bits()
            want = _expect(b, before, masks, taps, base0, 2, None, K, active)
            b.run(masks, base0, 2, None, nvar=K, active=active, warp_taps=dev)
            torch.cuda.synchronize()
            got = b.bits()
            exp = _Batch(layout, b.nchunk, F, H, W, c, 2)
            for t in range(2):
                _i16(exp.flat[t]).copy_(want[t])
                finite = torch.isfinite(exp.x[t])
                assert bool(torch.isfinite(b.x[t][finite]).all()), (H, W, base0, K, active, t)  # no NaN guard reached an output
                for k in range(K):
                    if (active >> k) & 1:
                        assert bool(torch.isfinite(b.logical(t)[3 + K + k]).all()) and bool(finite.view(-1).any())
            _assert_bits(got, want, (H, W, base0, K, active))


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------
def test_bilinear_entries_refuse_bad_arguments_and_write_nothing():
    from mvoc_amd import ops
    F, H, W, c = 3, 4, 4, 8
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    tok, nchw = _Batch("spatial", 9, F, H, W, c, 2), _Batch("nchw", 9, F, H, W, c, 1)
    for b in (tok, nchw):
        for f in b.flat:
            f[GUARD:-GUARD] = 0
    before = tok.bits() + nchw.bits()
    table, _ = _spec_taps(2, H, W, F)
    err = lambda: ops.lib.mvoc_last_error().decode()
    cases = [  # (nvar, active, map, table, base_chunk0, text): the refusals of _warped
        (0, 1, None, table, None, "nvar 0"), (9, 1, None, table, None, "nvar 9"),
        (3, 0, None, table, None, "active mask 0x0"), (3, 8, None, table, None, "active mask 0x8"), (1, 2, None, table, None, "active mask 0x2"),
        (2, 3, (0, (0, 0)), table, None, "nsrc 0"), (2, 3, (2, (0, 2)), table, None, "obj_chunk[1] = 2"),
        (2, 3, (2, (-1, 0)), table, None, "obj_chunk[0] = -1"),
        (2, 3, None, None, None, "null tap table"),
        (1, 1, (2, (0, 1)), table, -1, "base_chunk0 = -1"),
    ]
    for nvar, active, smap, tab, b0, text in cases:
        assert tok.direct("_bilinear", masks, False if b0 is None else b0, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
        assert nchw.direct("_bilinear", masks, True if b0 is None else b0, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
    # the tokens alignment rules, and the 16-bit tap fields: a site of 65 535 rows or columns is refused by both layouts
    d = ops._pnp_desc(tok.x[0], tok.x[1], masks, F * H * W * c, H * W * c, c, F, H, W, c, False, 2)
    dn = ops._pnp_desc(nchw.x[0], None, masks, 0, 0, 0, F, H, W, c, True, 2)
    arr = (C.c_int32 * 2)(1, 2)
    call = lambda: ops.lib.mvoc_pnp_blend_scatter_tokens_bilinear(C.byref(d), 3, arr, 1, 1, table.data_ptr(), ops._stream())
    calln = lambda: ops.lib.mvoc_pnp_blend_scatter_nchw_bilinear(C.byref(dn), 3, arr, 1, 1, table.data_ptr(), ops._stream())
    for field, value, text in (("channels", 12, "multiples of 8"), ("p_stride", 12, "multiples of 8"), ("x", tok.x[0].data_ptr() + 2, "16-byte aligned"),
                               ("height", 65535, "16-bit tap fields"), ("width", 65535, "16-bit tap fields"), ("height", 2 ** 30, "does not fit")):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert call() == -2 and text in err(), (field, err())
        setattr(d, field, keep)
    for field, value, text in (("height", 65535, "16-bit tap fields"), ("width", 70000, "16-bit tap fields")):
        keep = getattr(dn, field)
        setattr(dn, field, value)
        assert calln() == -2 and text in err(), (field, err())
        setattr(dn, field, keep)
    # a valid call with the same buffers goes through (the refusals above were about the arguments)
    assert tok.direct("_bilinear", masks, False, 2, None, 3, 0b111, table) == 0, err()
    assert nchw.direct("_bilinear", masks, True, 2, None, 1, 1, table) == 0, err()
    # the Python layer: the table's form, and the arguments a tap table does not combine with
    form = r"warp_taps must be a contiguous int32 \[nobj = 2, F = 3, H \* W = 16, 2\] table"
    with pytest.raises(RuntimeError, match=form):
        tok.run(masks, False, 2, nvar=2, warp_taps=table[:1])
    with pytest.raises(RuntimeError, match=form):
        nchw.run(masks, True, 2, warp_taps=table[:, :, :15].contiguous())
    with pytest.raises(RuntimeError, match=form):
        nchw.run(masks, True, 2, warp_taps=table[..., 0].contiguous())  # the nearest table's form is another table
    with pytest.raises(RuntimeError, match=form):
        nchw.run(masks, True, 2, warp_taps=torch.stack([table, table]))  # no per-variant form
    with pytest.raises(RuntimeError, match="warp_taps"):
        nchw.run(masks, True, 2, nvar=2, warp_taps=table.long())
    nearest = tw._table(tw._spec_rows(2, H, W, F))
    axis = tr._table([[r[f % 2] for f in range(F)] for r in tr._spec_maps(2, H, W)])
    place = tp._table([[(1, 1), (0, -1), (0, 0)], [(2, 0), (0, 0), (1, 1)]])
    for b, b0 in ((tok, False), (nchw, True)):
        for other in ({"place": place}, {"resample": axis}, {"warp": nearest}):
            with pytest.raises(RuntimeError, match="warp_taps= is given together with place= / resample= / warp="):
                b.run(masks, b0, 2, warp_taps=table, **other)
        with pytest.raises(RuntimeError, match="does not take a .* mask stack"):
            b.run(torch.stack([masks, masks]).contiguous(), b0, 2, nvar=2, warp_taps=table)
    with pytest.raises(RuntimeError, match="no_background"):
        tok.run(masks, False, 2, warp_taps=table, no_background=True)
    with pytest.raises(RuntimeError, match="storage ends"):
        nchw.run(masks, True, 2, nvar=4, warp_taps=table)  # 3 + 8 chunks in a buffer of 9
    torch.cuda.synchronize()
    _assert_bits(tok.bits() + nchw.bits(), before, "zeros blended with zeros: nothing but zeros was ever written, NaN stays NaN")


# ---- 5: profiler bytes ------------------------------------------------------------------------------------------------------------
def test_profiler_counts_the_placed_bytes_and_the_tap_table():
    """the stated formula: the bytes of ``_placed`` (every distinct object chunk once, the base, the destinations, one mask set) +
    8 * nobj * F * H * W for the table"""
    from mvoc_amd import ops
    F, H, W, c, K = 3, 4, 4, 8, 3
    nrow = F * H * W
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    place = tp._table([[(1, 0), (0, 1), (0, 0)], [(0, 0), (-1, -1), (2, 0)]])
    table, _ = _spec_taps(2, H, W, F)
    ops.prof_enable(True)
    try:
        for base0, ndst, smap, active in ((True, 2, None, 0b101), (False, 1, (2, (1, 1)), 0b100)):
            nsrc = 3 if smap is None else smap[0]
            work = []
            for kw in ({"place": place}, {"warp_taps": table}):
                buf = torch.zeros((nsrc + ndst * K) * nrow, 3 * c, dtype=F16, device="cuda")
                nchw = torch.zeros((nsrc + ndst * K) * F, c, H, W, dtype=F16, device="cuda")
                ops.prof_reset()
                tr._run_tokens(buf, "spatial", F, H, W, c, masks, base0, ndst, smap, nvar=K, active=active, **kw)
                torch.cuda.synchronize()
                t = ops.prof_collect()["pnp"]
                ops.prof_reset()
                ops.pnp_blend_nchw(nchw, masks, frames=F, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=K, active=active, **kw)
                torch.cuda.synchronize()
                n = ops.prof_collect()["pnp"]
                assert t["launches"] == 1 and n["launches"] == 1
                work.append((t["work"], n["work"]))
            table_bytes = 8 * 2 * F * H * W
            assert work[1][0] == work[0][0] + table_bytes and work[1][1] == work[0][1] + table_bytes, (base0, ndst, smap, active, work)
            # ... and in absolute terms, per tensor: chunks of F * H * W * C fp16 + one set of nobj masks
            on, objc = bin(active).count("1"), (2 if smap is None else 1)
            chunks = (objc + 1 if base0 else objc + on) + ndst * on
            assert work[1][1] == nrow * c * 2 * chunks + 2 * 2 * nrow + table_bytes, (work, chunks)
            assert work[1][0] == 2 * (nrow * c * 2 * chunks + 2 * 2 * nrow) + table_bytes, (work, chunks)  # x and x2
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


# ---- 6: the plane mover -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nplane", [1, 4])
@pytest.mark.parametrize("hw", [(5, 7), (8, 8), (12, 23)])
def test_warp_planes_bilinear_against_the_torch_chain(hw, nplane):
    from mvoc_amd import ops
    h, w = hw
    F = 3
    g = torch.Generator().manual_seed(10 * h + nplane)
    n = nplane * F * h * w
    tb = lambda frames, ay2=h, ax2=w: ops.warp_taps(((ay2, ax2, tuple(frames)),), h, w, h, w)[0]
    turn = (2 * C30, 2 * S30, -2 * S30, 2 * C30, 3 * D)
    garbage = torch.randint(-2 ** 63, 2 ** 63 - 1, (F, h * w), generator=g, dtype=torch.int64).view(torch.int32).view(F, h * w, 2).clone()
    garbage[:, ::3, 0] = tb([(1, 0, 0, 1, 2, 0, 0)] * F)[:, ::3, 0]  # a third of the pairs read the plane, with garbage weights
    cases = [tb([turn + (0, 0), turn + (1, -2), (2, 0, 0, 2, 1, 0, 0)]),
             tb([(1, 0, 0, 1, 1, 0, 0), (1, 0, 0, 1, 1, 2 * h + 3, 0), (-1, 0, 0, -1, 1, 0, 0)]),
             tb([(63303, -16962, 16962, 63303, D, 0, 1)] * F, 3, w + 1),
             garbage]  # pairs no rule of ours writes: every one is safe
    assert bool((cases[1][1, :, 0] == -1).all()) and not bool((cases[1][0, :, 1] != 0).any())
    for taps in cases:
        src_buf = torch.full((n + 2 * GUARD,), NAN, dtype=F16)
        src_buf[GUARD:GUARD + n] = torch.randn(n, generator=g).half()
        src_buf = src_buf.cuda()
        src = src_buf[GUARD:GUARD + n].view(nplane, F, h, w)
        dst_buf = torch.full((n + 2 * GUARD,), 777.0, dtype=F16, device="cuda")
        out = dst_buf[GUARD:GUARD + n].view(nplane, F, h, w)
        want = torch.stack([torch.stack([_interp(src[pl, f], taps[f])[0] for f in range(F)]) for pl in range(nplane)])
        got = ops.warp_planes_bilinear(src if nplane > 1 else src[0], taps.cuda().contiguous(), out=out if nplane > 1 else out[0])
        torch.cuda.synchronize()
        assert torch.equal(_i16(got.reshape(want.shape)), _i16(want))
        assert torch.isfinite(out).all()
        assert bool((dst_buf[:GUARD] == 777).all()) and bool((dst_buf[GUARD + n:] == 777).all())  # nothing outside the extent
        assert torch.isnan(src_buf[:GUARD]).all() and torch.isnan(src_buf[GUARD + n:]).all()
    # weights 0 on the identity: a copy
    ident = tb([(1, 0, 0, 1, 1, 0, 0)] * F).cuda()
    src = torch.randn(nplane, F, h, w, generator=g).half().cuda()
    src[src == 0] = 0.0
    assert torch.equal(ops.warp_planes_bilinear(src, ident), src)


def test_warp_planes_bilinear_refuses_bad_arguments_and_writes_nothing():
    from mvoc_amd import ops
    src = torch.ones(2, 2, 3, 4, dtype=F16, device="cuda")
    dst = torch.zeros_like(src)
    tab = ops.warp_tap_table(((3, 4, ((1, 0, 0, 1, 1, 0, 0),) * 2),), 3, 4, 3, 4, "cuda")[0]
    call = lambda s, d, t, dims=(2, 2, 3, 4): ops.lib.mvoc_gather_planes_bilinear_f16(s, d, *dims, t, ops._stream())
    err = lambda: ops.lib.mvoc_last_error().decode()
    assert call(None, dst.data_ptr(), tab.data_ptr()) == -1 and "null" in err()
    assert call(src.data_ptr(), None, tab.data_ptr()) == -1 and "null" in err()
    assert call(src.data_ptr(), dst.data_ptr(), None) == -1 and "null" in err()
    assert call(src.data_ptr(), src.data_ptr(), tab.data_ptr()) == -1 and "in place" in err()
    for dims in ((0, 2, 3, 4), (2, 0, 3, 4), (2, 2, -1, 4), (2, 2, 3, 0)):
        assert call(src.data_ptr(), dst.data_ptr(), tab.data_ptr(), dims) == -1 and "dims" in err()
    for dims in ((1, 1, 65535, 1), (1, 1, 1, 65535)):
        assert call(src.data_ptr(), dst.data_ptr(), tab.data_ptr(), dims) == -2 and "16-bit tap fields" in err()
    with pytest.raises(RuntimeError, match="taps must be"):
        ops.warp_planes_bilinear(src, tab[:1])
    with pytest.raises(RuntimeError, match="taps must be"):
        ops.warp_planes_bilinear(src, tab[..., 0].contiguous())  # the nearest form (h * w entries) is another table
    with pytest.raises(RuntimeError, match="taps"):
        ops.warp_planes_bilinear(src, tab.float())
    with pytest.raises(RuntimeError, match="out must be"):
        ops.warp_planes_bilinear(src, tab, out=dst[:1])
    torch.cuda.synchronize()
    assert not dst.any() and bool((src == 1).all())
    assert call(src.data_ptr(), dst.data_ptr(), tab.data_ptr()) == 0 and torch.equal(dst, src)


# ---- 7: engine --------------------------------------------------------------------------------------------------------------------
class _PreInterp:
    """``ops.pnp_blend_tokens`` / ``pnp_blend_nchw`` replaced by: interpolate the object chunks in torch through the tap table, call
    the unplaced entry with the masks resized and zeroed where the object is absent, restore the source chunks"""

    def __init__(self):
        from mvoc_amd import ops
        self.ops, self.orig, self.calls = ops, (ops.pnp_blend_tokens, ops.pnp_blend_nchw), []

    def __enter__(self):
        self.ops.pnp_blend_tokens, self.ops.pnp_blend_nchw = self.tokens, self.nchw
        return self

    def __exit__(self, *exc):
        self.ops.pnp_blend_tokens, self.ops.pnp_blend_nchw = self.orig

    def tokens(self, x, masks, **kw):
        table = kw.pop("warp_taps")
        taps = table.cpu()
        F, H, W, c = kw["frames"], kw["height"], kw["width"], kw["channels"]
        nobj = masks.shape[0]
        assert kw.get("src_map") is None and not {"place", "resample", "warp"} & set(kw) and tuple(table.shape) == (nobj, F, H * W, 2)
        nchunk = nobj + 1 + kw["ndst"] * kw.get("nvar", 1)
        self.calls.append(("tokens", H, W, taps))
        saved = []
        for t in (x, kw.get("x2")):
            if t is None:
                continue
            v = torch.as_strided(t, (nchunk, F, H, W, c), (kw["chunk_stride"], kw["f_stride"], kw["p_stride"] * W, kw["p_stride"], 1),
                                 t.storage_offset())
            keep = v[1:nobj + 1].clone()
            saved.append((v, keep))
            for j in range(nobj):
                for f in range(F):
                    v[1 + j, f] = _interp(keep[j, f], taps[j, f])[0]
        out = self.orig[0](x, _masks_eff(masks, taps, H, W), **kw)
        for v, keep in saved:
            v[1:nobj + 1] = keep
        return out

    def nchw(self, x, masks, **kw):
        table = kw.pop("warp_taps")
        taps = table.cpu()
        F, (H, W), nobj = kw["frames"], x.shape[2:], masks.shape[0]
        assert kw.get("src_map") is None and kw.get("x2") is None and not {"place", "resample", "warp"} & set(kw)
        self.calls.append(("nchw", H, W, taps))
        keep = x[F:(nobj + 1) * F].clone()
        for j in range(nobj):
            for f in range(F):
                x[(1 + j) * F + f] = _interp(keep[j * F + f].permute(1, 2, 0).contiguous(), taps[j, f])[0].permute(2, 0, 1)
        out = self.orig[1](x, _masks_eff(masks, taps, H, W), **kw)
        x[F:(nobj + 1) * F] = keep
        return out


@pytest.mark.parametrize("kind", ["qk", "conv_out", "features"])
def test_unet_bilinear_forward_equals_the_preinterpolated_unplaced_forward(kind):
    """one Q/K step (spatial + temporal sites, the source tail pruned), one conv_out step (prune_dead_chunks: the NCHW blend on
    the source chunks' outputs) and, with prune_dead_chunks off, the same step through the resnet / temporal-conv feature sites"""
    from mvoc_amd import ops, pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    F, h, w, cd = 3, 8, 8, 64
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    warp = tw._engine_warp()
    moved, table, taps = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False).warp_masks_bilinear(masks, warp)
    lat_taps = ops.warp_taps(warp, h, w, h, w)
    assert torch.equal(taps.cpu(), lat_taps) and table.tolist() == ops.warp_maps(warp, h, w, h, w)
    for j in range(2):  # soft masks through the chain, hard masks through the nearest map (they stay 0 / 1), types kept
        (s_m, h_m), (s0, h0) = moved[j], masks[j]
        assert s_m.dtype == s0.dtype and h_m.dtype == h0.dtype == torch.bool and s_m.shape == s0.shape
        for f in range(F):
            for ch in range(s_m.shape[1]):
                assert torch.equal(_i16(s_m[0, ch, f]), _i16(_interp(s0[0, ch, f][..., None], lat_taps[j, f])[0][..., 0]))
                assert torch.equal(h_m[0, ch, f], tw._gather_pix(h0[0, ch, f], table[j, f].tolist()))
        assert not torch.equal(s_m, s0)
    nearest_soft = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False).warp_masks(masks, warp)[0]
    assert any(not torch.equal(moved[j][0], nearest_soft[j][0]) for j in range(2))
    roles = tv._roles(F, h, w, cd, 4, 1)
    pipe, (t_feat, t_qk) = tv._arm(eng, 5)
    t = t_qk if kind == "qk" else t_feat
    names = ["S", "O", "P", "u0", "c0"]
    saved = eng.prune_dead_chunks

    def forward(value, flt):
        eng.warp, eng.warp_filter, eng.prune_source_tail, eng.prune_dead_chunks = value, flt, True, kind != "features"
        try:
            return tv._fwd(eng, tv._batch(roles, names), t)
        finally:
            eng.warp, eng.warp_filter, eng.prune_source_tail, eng.prune_dead_chunks = None, None, False, saved

    try:
        pnp_utils.register_time_all(pipe, t, moved)
        n_nearest = len(eng._level_tables["warp"][1])
        got = forward(warp, "bilinear")
        with _PreInterp() as pre:
            ref = forward(warp, "bilinear")
        assert len(eng._level_tables["warp"][1]) == n_nearest  # the nearest cache holds nearest tables only: nothing was added
        levels = {c[1:3] for c in pre.calls}
        assert eng._tap_tables[0] == warp and {k[:2] for k in eng._tap_tables[1]} == levels
        nearest = forward(warp, None)
        assert len(eng._level_tables["warp"][1]) == len(levels) and {k[:2] for k in eng._tap_tables[1]} == levels
        plain = forward(None, None)
        with pytest.raises(RuntimeError, match="warp_filter is set but warp is not"):
            forward(None, "bilinear")
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
    for c in pre.calls:  # every site was handed the taps of its own level
        assert torch.equal(c[3], ops.warp_taps(warp, c[1], c[2], h, w)), c[:3]
    assert torch.equal(_i16(got[3:]), _i16(ref[3:])), kind
    assert torch.isfinite(got[3:]).all() and not torch.equal(got[3:], plain[3:]) and not torch.equal(got[3:], nearest[3:]), kind
    assert eng.warp is None and eng.warp_filter is None


def test_unet_refuses_the_filter_without_a_warp_and_keeps_the_warps_refusals():
    F, h, w = 3, 8, 8
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    eng.warp_filter = "bilinear"
    try:
        with pytest.raises(RuntimeError, match="warp_filter is set but warp is not"):
            eng.place_kw(masks, 8, 8)
        eng.transform = tr.ENGINE_TRANSFORM
        with pytest.raises(RuntimeError, match="warp_filter is set but warp is not"):
            eng.place_kw(masks, 8, 8)
        eng.warp = tw._engine_warp()
        with pytest.raises(RuntimeError, match="warp is set together with"):
            eng.place_kw(masks, 8, 8)
        eng.transform = None
        eng.shard = types.SimpleNamespace(rank=0, world=1)
        with pytest.raises(RuntimeError, match="a warp does not combine with the frame shard"):
            eng.place_kw(masks, 8, 8)
        eng.shard = None
        with pytest.raises(RuntimeError, match="warp holds 2 objects, the hooks carry 1 masks"):
            eng.place_kw(masks[:1], 8, 8)
        kw = eng.place_kw(masks, 4, 4)
        assert list(kw) == ["warp_taps"]
        tab = kw["warp_taps"]
        assert tuple(tab.shape) == (2, F, 16, 2) and tab.dtype == torch.int32 and tab.is_cuda
        assert eng.place_kw(masks, 4, 4)["warp_taps"] is tab  # cached per level
        assert eng._level_tables["warp"] == (None, {})  # ... in a cache of its own
        eng.warp_filter = None
        assert list(eng.place_kw(masks, 4, 4)) == ["warp"] and len(eng._level_tables["warp"][1]) == 1
    finally:
        eng.warp, eng.warp_filter, eng.transform, eng.shard = None, None, None, None
    assert eng.place_kw(masks, 8, 8) == {}


# ---- 8: pipeline ------------------------------------------------------------------------------------------------------------------
ROTATED = tw.ROTATED
_graph_keys = tr._graph_keys


@contextlib.contextmanager
def _with_arguments(**extra):
    """test_placement_gpu.py's toy job with more arguments of the sampling call (``obj_transforms``, ``obj_transform_filter``)"""
    from mvoc_amd.pipeline import I2VGenXLPipeline
    orig = getattr(I2VGenXLPipeline, tr.SAMPLE)

    def call(self, *a, **kw):
        return orig(self, *a, **extra, **kw)

    setattr(I2VGenXLPipeline, tr.SAMPLE, call)
    try:
        yield
    finally:
        setattr(I2VGenXLPipeline, tr.SAMPLE, orig)


def _job(graphs, transforms=None, flt="absent", **kw):
    extra = {} if transforms is None else {"obj_transforms": transforms}
    if flt != "absent":
        extra["obj_transform_filter"] = flt
    with _with_arguments(**extra):
        return tp._placed_job(graphs, **kw)


def test_bilinear_composition_graph_replay_equals_eager_and_differs_from_nearest():
    from mvoc_amd import ops
    eager = _job(False, ROTATED, "bilinear", count_calls=True)
    st = eager.state
    warp = tw._rotated_lat()
    assert st["warp"] == warp and st["warp_filter"] == "bilinear"
    assert all(st[k] is None for k in ("placement", "transform", "place_dev", "resample_dev"))
    taps = ops.warp_taps(warp, 8, 8, 8, 8)
    assert torch.equal(st["warp_taps_dev"].cpu(), taps) and st["warp_dev"].tolist() == ops.warp_maps(warp, 8, 8, 8, 8)
    # the per-level tap tables (8 x 8, 4 x 4, 2 x 2) stay alive with the state, whose graphs would read them
    assert len(st["place_tables"]) == 1 and {k[:2] for k in st["place_tables"][0]} == {(8, 8), (4, 4), (2, 2)}
    assert all(tuple(t.shape)[-1] == 2 and t.dim() == 4 for t in st["place_tables"][0].values())
    names = set().union(*eager.step_calls)
    assert {"mvoc_pnp_blend_scatter_tokens_bilinear", "mvoc_pnp_blend_scatter_nchw_bilinear", "mvoc_gather_planes_bilinear_f16"} <= names
    assert not any(n.startswith("mvoc_pnp_blend") and not n.endswith("_bilinear") for n in names), names
    assert not {"mvoc_shift_planes_f16", "mvoc_gather_planes_f16", "mvoc_gather_planes_warped_f16"} & names  # (inside the steps)
    # two fusion steps: the two fusion objects go through the bilinear mover instead of a copy
    assert [c.get("mvoc_gather_planes_bilinear_f16", 0) for c in eager.step_calls] == [2, 2, 0, 0, 0]
    graphed = _job(True, ROTATED, "bilinear")
    assert torch.equal(graphed.out, eager.out) and torch.isfinite(eager.out).all()
    assert all("bilinear" in k and "warp" in k and warp in k for k in graphed.state["variants"])  # the filter is part of the key
    nearest = _job(True, ROTATED)
    assert nearest.out.shape == eager.out.shape and not torch.equal(nearest.out, eager.out)
    assert not any("bilinear" in k for k in nearest.state["variants"]) and "warp_filter" not in nearest.state
    assert graphed.graphs == nearest.graphs  # one more part of the key, not one more step kind
    drop = lambda k: tuple(v for v in k[:1] + k[2:] if not (isinstance(v, str) and v == "bilinear"))  # (entry 1: the mask key)
    assert {drop(k) for k in graphed.state["variants"]} == {k[:1] + k[2:] for k in nearest.state["variants"]}
    assert all(k.index("bilinear") == k.index("warp") + 2 for k in graphed.state["variants"])  # right behind the warp's value
    # the state stays free of reference cycles: nothing it holds leads back to it (the job's own wrappers put away first)
    for job in (eager, graphed):
        for name in ("make_composition_state", "composition_step"):
            job.pipe.__dict__.pop(name)
        assert not _reaches(list(job.state.values()), job.state)


def _reaches(roots, target):
    """whether ``target`` is reachable from ``roots`` through strong references (functions: closure and defaults only; modules
    and classes are not entered)"""
    import gc
    seen, stack = set(), list(roots)
    while stack:
        o = stack.pop()
        if o is target:
            return True
        if id(o) in seen or isinstance(o, (types.ModuleType, type)):
            continue
        seen.add(id(o))
        if isinstance(o, types.FunctionType):
            stack.extend(c for c in (o.__closure__ or ()))
            stack.extend(o.__defaults__ or ())
        else:
            stack.extend(gc.get_referents(o))
    return False


def test_scale_and_mirror_under_the_filter_are_a_warp_for_all_objects():
    scaled = [{"scale": "3/2", "flip": "h", "offset": tp.PATH}, {}]
    near, bil = _job(False, scaled, count_calls=True), _job(False, scaled, "bilinear", count_calls=True)
    assert near.state["transform"] is not None and near.state["warp"] is None
    assert bil.state["transform"] is None and len(bil.state["warp"]) == 2 and bil.state["warp_filter"] == "bilinear"
    names = set().union(*bil.step_calls)
    assert not any(n.endswith("_resampled") or n.endswith("_warped") for n in names) and any(n.endswith("_bilinear") for n in names)
    assert torch.isfinite(bil.out).all() and not torch.equal(near.out, bil.out)


def test_a_translation_under_the_filter_makes_the_calls_and_graphs_of_the_obj_offsets_call():
    moved = [{"offset": tp.PATH}, {"offset": (-16, 8), "rotate": 360}]
    ref, same = _job(False, offsets=[tp.PATH, (-16, 8)], count_calls=True), _job(False, moved, "bilinear", count_calls=True)
    assert same.state["placement"] == ref.state["placement"] is not None and same.state["warp"] is None
    assert "warp_filter" not in same.state
    for i, (a, b) in enumerate(zip(ref.step_calls, same.step_calls)):
        assert a == b and sum(a.values()) > 0, (i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
        assert not any("_bilinear" in n or "_warped" in n for n in b)
    assert torch.equal(ref.out, same.out)
    gr, gs = _job(True, offsets=[tp.PATH, (-16, 8)]), _job(True, moved, "bilinear")
    assert gr.graphs == gs.graphs and _graph_keys(gr.state) == _graph_keys(gs.state) and torch.equal(gr.out, gs.out)
    # an identity call under the filter is the call without any argument
    plain, ident = _job(True), _job(True, [{}, {"rotate": 0}], "bilinear")
    assert _graph_keys(plain.state) == _graph_keys(ident.state) and torch.equal(plain.out, ident.out)


def test_the_nearest_filter_makes_the_calls_and_graphs_of_a_call_without_the_argument():
    for transforms in (ROTATED, None):
        ref, same = _job(False, transforms, count_calls=True), _job(False, transforms, "nearest", count_calls=True)
        assert "warp_filter" not in same.state and same.state["warp"] == ref.state["warp"]
        for i, (a, b) in enumerate(zip(ref.step_calls, same.step_calls)):
            assert a == b and sum(a.values()) > 0, (i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
            assert not any("_bilinear" in n for n in b)
        assert torch.equal(ref.out, same.out)
        gr, gs = _job(True, transforms), _job(True, transforms, "nearest")
        assert gr.graphs == gs.graphs and _graph_keys(gr.state) == _graph_keys(gs.state) and torch.equal(gr.out, gs.out)
        gn = _job(True, transforms, None)
        assert _graph_keys(gr.state) == _graph_keys(gn.state) and torch.equal(gr.out, gn.out)


def test_fusion_steps_use_the_interpolated_latents_and_soft_masks_and_the_nearest_hard_masks():
    from mvoc_amd import ops
    from mvoc_amd.schedulers import DDIMScheduler
    seen, orig = [], ops.latent_fusion

    def fusion(latents, bg, objs, masks, *a, **kw):
        seen.append((objs.clone(), masks.clone()))
        return orig(latents, bg, objs, masks, *a, **kw)

    ops.latent_fusion = fusion
    try:
        job = _job(False, ROTATED, "bilinear")
    finally:
        ops.latent_fusion = orig
    assert len(seen) == 2  # fusion_steps = (0, 2)
    s = DDIMScheduler()
    s.set_timesteps(5)
    t0 = int(s.timesteps[0])  # both fusion steps read the objects' latents of the first timestep (the reference's counter stays 0)
    warp = tw._rotated_lat()
    taps, rows = ops.warp_taps(warp, 8, 8, 8, 8), ops.warp_maps(warp, 8, 8, 8, 8)
    plane = lambda p, j, f: _interp(p[..., None], taps[j, f])[0][..., 0]
    for objs, masks in seen:
        for j, d in enumerate(("/virtual/o1", "/virtual/o2")):
            lat = job.pipe.latent_cache.get(d, t0).cuda().half()
            for f in range(3):
                for ch in range(4):
                    assert torch.equal(_i16(objs[j, 0, ch, f]), _i16(plane(lat[0, ch, f], j, f))), (j, f, ch)
                    assert torch.equal(_i16(masks[j, 0, ch, f]), _i16(plane(job.masks[j][0][0, ch, f].cuda().half(), j, f))), (j, f, ch)
            assert not torch.equal(objs[j], lat)
    st = job.state
    for j in range(2):  # the state's masks: soft interpolated, hard gathered through the nearest map (0 / 1)
        hard = st["masks"][j][1]
        assert hard.dtype == torch.bool
        for f in range(3):
            assert torch.equal(hard[0, 0, f].cuda(), tw._gather_pix(job.masks[j][1][0, 0, f].cuda(), rows[j][f]))
            assert torch.equal(_i16(st["fusion_masks"][j, 0, 0, f]), _i16(plane(job.masks[j][0][0, 0, f].cuda().half(), j, f)))
    soft = torch.stack([st["masks"][j][0].cuda().half() for j in range(2)])
    assert bool(((soft > 0) & (soft < 1)).any())


def test_argument_mixes_and_a_frame_shard_are_refused():
    with pytest.raises(ValueError, match="obj_transform_filter = 'bilinear' is given without obj_transforms"):
        _job(False, None, "bilinear")
    with pytest.raises(ValueError, match="obj_transform_filter = 'bilinear' is given together with obj_offsets"):
        _job(False, None, "bilinear", offsets=tp.OFFSETS)
    with pytest.raises(ValueError, match="obj_transform_filter = 'bilinear' is given together with obj_offsets / variant_obj_offsets / variant_obj_transforms"):
        with _with_arguments(variant_obj_transforms=[None, [{"scale": 2}, {}]]):
            _job(False, None, "bilinear", K=2)
    with pytest.raises(ValueError, match="obj_transforms is given together with obj_offsets"):
        _job(False, ROTATED, "bilinear", offsets=tp.OFFSETS)
    with pytest.raises(ValueError, match="obj_transform_filter 'cubic' is not one of None, 'nearest', 'bilinear'"):
        _job(False, ROTATED, "cubic")
    with pytest.raises(RuntimeError, match="obj_transforms do not combine with the frame shard"):
        _job(False, ROTATED, "bilinear", shard=True)
    # make_composition_state itself: the filter needs a warp
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    _, eng = tv._toy_pair()
    pipe = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False)
    with pytest.raises(ValueError, match="obj_transform_filter = 'bilinear' needs a warp"):
        pipe.make_composition_state(None, {}, [], 9.0, obj_transform_filter="bilinear")
    with pytest.raises(ValueError, match="is not one of None, 'nearest', 'bilinear'"):
        pipe.make_composition_state(None, {}, [], 9.0, obj_transform_filter="linear")
