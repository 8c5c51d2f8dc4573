"""GPU: rotation of objects at composition time -- nearest resampling through ONE 2-D index map.

* kernels: the ``_warped`` blend entries against the EXISTING unplaced entries on inputs gathered beforehand in torch (object chunks
  gathered through the map with zero fill, masks nearest-resized to H x W and zeroed where the map says absent).  The WHOLE
  allocation is compared after the call, as int16: the unplaced entry's rows at the described destinations, the bits from before
  the call everywhere else -- sources, idle variants, and the NaN that fills every element outside the described tensors (and the
  chunks the contract says are not read).  Every case asserts that its result DIFFERS from the untransformed call: on a tree
  without the feature nothing here passes.  A diagonal table equals ``_resampled``, a quarter turn the unplaced entry on
  ``torch.rot90``-ed chunks, every int32 entry is safe; ``warp_planes`` against torch indexing; bad arguments refused.
* engine: a warped forward of the toy UNet against the same forward with ``ops.pnp_blend_tokens`` / ``pnp_blend_nchw`` replaced by
  "gather in torch, call the unplaced entry, restore the sources".
* pipeline: graph replay against eager, ``rotate: 0`` against a call without the argument and ``rotate: 180`` against the
  ``flip: "hv"`` call (latents, C-ABI calls, graph keys), K = 2 variants under one warp, the fusion steps on gathered latents and
  masks, a frame-sharded pipeline refused.

Structure and helpers follow test_resample_gpu.py so that the files judge by the same bars.
"""
import ctypes as C
import itertools
import types

import pytest
import torch

import pnp_contract as pc
import test_placement_gpu as tp
import test_resample_gpu as tr
import test_variants_gpu as tv

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_i16 = tv._i16
_planted = tp._planted
VARIANTS = tr.VARIANTS  # (nvar, active): one variant; two with every bit set; two with a partial mask
GUARD = pc.GUARD
D = 65536
NAN = float("nan")


# ---- maps ---------------------------------------------------------------------------------------------------------------------
def _spec_rows(nobj, H, W, F=2):
    """per object, per frame the 2-D maps of an H x W site (the latent grid is the site itself), [nobj][F][H * W]: 30 degrees
    about the centre; 45 degrees at scale 3/2 with a moved second frame; 90 degrees with a flip, its second frame gathered entirely
    out of the frame; -15 degrees at scale 1/2 about an anchor off the centre"""
    from mvoc_amd import ops
    mp = lambda dy, dx, m, den, ay2=H, ax2=W: ops.level_warp_map(dy, dx, m, den, ay2, ax2, H, W, H, W)
    specs = [
        [mp(0, 0, (56756, 32768, -32768, 56756), D)] * 2,
        [mp(0, 0, (2 * 46341, 2 * 46341, -2 * 46341, 2 * 46341), 3 * D), mp(1, -1, (2 * 46341, 2 * 46341, -2 * 46341, 2 * 46341), 3 * D)],
        [mp(0, 0, (0, 1, 1, 0), 1), mp(2 * H + 3, 0, (0, 1, 1, 0), 1)],
        [mp(0, 0, (2 * 63303, -2 * 16962, 2 * 16962, 2 * 63303), D, 3, W + 1), mp(0, 1, (2 * 63303, -2 * 16962, 2 * 16962, 2 * 63303), D, 3, W + 1)],
    ]
    rows = [[obj[f % 2] for f in range(F)] for obj in specs[:nobj]]
    first = rows[0][0]
    # the first object's map is no (ymap, xmap) pair: one destination row reads several source rows
    assert any(len({v // W for v in first[iy * W:(iy + 1) * W] if v >= 0}) > 1 for iy in range(H)), first
    assert 2 * sum(v >= 0 for v in first) >= H * W, first  # at least half of its destination pixels show the object
    for j, obj in enumerate(rows):
        for f, r in enumerate(obj):  # one (object, frame) is nowhere; every other one shows some pixels
            assert all(v == -1 for v in r) == ((j, f % 2) == (2, 1)), (j, f, r)
    return rows


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32).cuda().contiguous()


def _clean(row, hw):
    return [v if 0 <= v < hw else -1 for v in row]


def _gather_pix(src, row):
    """src [H, W, ...] -> out[pixel] = src at the linear pixel row[pixel], or +0 where the entry is outside"""
    H, W = src.shape[:2]
    idx = torch.tensor(_clean(row, H * W), device=src.device)
    flat = src.reshape(H * W, -1)
    out = torch.where((idx >= 0)[:, None], flat[idx.clamp(min=0)], torch.zeros_like(flat))
    return out.view(src.shape)


def _masks_eff(masks, rows, H, W):
    """the masks of the gathered twin: nearest-resized to H x W by the entries' own rule (pnp_contract.near), zero where the
    object's map says absent"""
    ny = torch.tensor(pc.near(H, masks.shape[2]), device=masks.device)
    nx = torch.tensor(pc.near(W, masks.shape[3]), device=masks.device)
    m = masks[:, :, ny][:, :, :, nx].clone()
    for j, obj in enumerate(rows):
        for f, r in enumerate(obj):
            present = torch.tensor([0 <= v < H * W for v in r], device=m.device).view(H, W)
            m[j, f] *= present.to(m.dtype)
    return m.contiguous()


# ---- a batch inside a NaN-filled allocation -----------------------------------------------------------------------------------
class _Batch:
    """T tensors of nchunk chunks [F, H, W, C] in one of three layouts ("spatial" / "temporal" tokens, "nchw"), each in its own
    allocation with GUARD elements of NaN in front and behind; ``lead`` elements (2 bytes each) past the 256-byte boundary"""

    def __init__(self, layout, nchunk, F, H, W, c, T, lead=0):
        self.layout, self.nchunk, self.F, self.H, self.W, self.c, self.T = layout, nchunk, F, H, W, c, T
        self.n = nchunk * F * H * W * c
        self.flat = [torch.full((2 * GUARD + lead + self.n,), NAN, dtype=torch.float16, device="cuda") for _ in range(T)]
        self.x = [f[GUARD + lead:GUARD + lead + self.n] for f in self.flat]
        assert all(x.data_ptr() % 256 == 2 * lead for x in self.x)

    def logical(self, t):
        """[nchunk, F, H, W, C] view of tensor t"""
        n, F, H, W, c = self.nchunk, self.F, self.H, self.W, self.c
        if self.layout == "spatial":
            return self.x[t].view(n, F, H, W, c)
        if self.layout == "temporal":
            return self.x[t].view(n, H, W, F, c).permute(0, 3, 1, 2, 4)
        return self.x[t].view(n, F, c, H, W).permute(0, 1, 3, 4, 2)

    def bits(self):
        return [_i16(f).clone() for f in self.flat]

    def run(self, masks, base0, ndst, smap=None, nvar=1, active=None, **kw):
        from mvoc_amd import ops
        F, H, W, c = self.F, self.H, self.W, self.c
        x2 = self.x[1] if self.T == 2 else None
        if self.layout == "nchw":
            v = lambda x: None if x is None else x.view(self.nchunk * F, c, H, W)
            return ops.pnp_blend_nchw(v(self.x[0]), masks, frames=F, x2=v(x2), base_chunk0=base0, ndst=ndst, src_map=smap, nvar=nvar,
                                      active=active, **kw)
        fs, ps = tv._strides(self.layout, c, F, H * W)
        v = lambda x: None if x is None else x.view(-1, c)
        return ops.pnp_blend_tokens(v(self.x[0]), masks, x2=v(x2), frames=F, height=H, width=W, channels=c, chunk_stride=F * H * W * c,
                                    f_stride=fs, p_stride=ps, base_chunk0=base0, ndst=ndst, src_map=smap, nvar=nvar, active=active, **kw)

    def direct(self, entry, masks, base0, ndst, smap, nvar, active, table):
        """the C entry itself (``entry``: the suffix); returns its status"""
        from mvoc_amd import ops
        F, H, W, c = self.F, self.H, self.W, self.c
        x2 = self.x[1] if self.T == 2 else None
        if self.layout == "nchw":
            d = ops._pnp_desc(self.x[0], x2, masks, 0, 0, 0, F, H, W, c, base0, ndst)
        else:
            fs, ps = tv._strides(self.layout, c, F, H * W)
            d = ops._pnp_desc(self.x[0], x2, masks, F * H * W * c, fs, ps, F, H, W, c, base0, ndst)
        nobj = masks.shape[0]
        nsrc, chunks = smap if smap is not None else (nobj + 1, tuple(range(1, nobj + 1)))
        arr = (C.c_int32 * len(chunks))(*chunks)
        fn = getattr(ops.lib, f"mvoc_pnp_blend_scatter_{'nchw' if self.layout == 'nchw' else 'tokens'}{entry}")
        return fn(C.byref(d), nsrc, arr, nvar, active, None if table is None else table.data_ptr(), ops._stream())


def _fill(b, nsrc, smap, nobj, base0, ndst, K, active, g):
    """finite values (a few signed zeros) in every chunk the contract reads, NaN in the others: source chunks no object names
    (chunk 0 unless it is the base), every u_k, and c_k when the base is chunk 0 or variant k does not inject"""
    read = set(tv._src_order(smap, nobj)[1:]) | ({0} if base0 else set())
    for t in range(b.T):
        lg = b.logical(t)
        lg.copy_(_planted(torch.randn(tuple(lg.shape), generator=g).half(), g).cuda())
        for ch in range(nsrc):
            if ch not in read:
                lg[ch] = NAN
        for k in range(K):
            if ndst == 2:
                lg[nsrc + k] = NAN
            if base0 or not (active >> k) & 1:
                lg[nsrc + (ndst - 1) * K + k] = NAN


def _expect(b, before, masks, rows, base0, ndst, smap, K, active):
    """the allocation the warped call must leave: ``before`` with, per injecting variant, the rows the POSITIONAL unplaced entry
    writes on that variant's own batch [bg, gathered obj_1.., (u_k,) c_k]"""
    nobj, F, H, W, c = masks.shape[0], b.F, b.H, b.W, b.c
    nsrc = nobj + 1 if smap is None else smap[0]
    order = tv._src_order(smap, nobj)
    meff = _masks_eff(masks, rows, H, W)
    exp = _Batch(b.layout, b.nchunk, F, H, W, c, b.T, lead=(b.x[0].data_ptr() % 256) // 2)
    for t in range(b.T):
        _i16(exp.flat[t]).copy_(before[t])
    twin_layout = "nchw" if b.layout == "nchw" else "spatial"
    for k in range(K):
        if not (active >> k) & 1:
            continue
        dst = [nsrc + d * K + k for d in range(ndst)]
        for t in range(b.T):
            src = b.logical(t)
            twin = _Batch(twin_layout, nobj + 1 + ndst, F, H, W, c, 1)
            lg = twin.logical(0)
            lg[0] = src[order[0]]
            for j in range(nobj):
                for f in range(F):
                    lg[1 + j, f] = _gather_pix(src[order[1 + j], f], rows[j][f])
            for d, i in enumerate(dst):
                lg[nobj + 1 + d] = src[i]
            twin.run(meff, base0, ndst)
            for d, i in enumerate(dst):
                exp.logical(t)[i] = lg[nobj + 1 + d]
    return exp.bits()


def _assert_bits(got, want, what):
    for t, (a, e) in enumerate(zip(got, want)):
        assert torch.equal(a, e), (what, t, int((a != e).sum()))


# ---- the blend entries --------------------------------------------------------------------------------------------------------
SITES = [(5, 6, 0), (4, 6, 0), (4, 6, 1)]  # (H, W, lead): hw % 8 != 0 (VEC 1); VEC 8; VEC 8's shape 2 bytes off (VEC 1)


@pytest.mark.parametrize("layout", ["spatial", "temporal", "nchw"])
@pytest.mark.parametrize("site", SITES, ids=["5x6", "4x6", "4x6+2B"])
def test_warped_entries_equal_the_existing_entries_on_gathered_inputs(site, layout):
    H, W, lead = site
    F = 2
    g = torch.Generator().manual_seed(100 * H + 10 * lead + len(layout))
    n = 0
    seen = set()
    for nobj in (1, 2, 3, 4):
        rows = _spec_rows(nobj, H, W)
        table = _table(rows)
        for ndst, base0, (K, active), smap in itertools.product((1, 2), (False, True), VARIANTS, tp._maps(nobj)):
            x2, c, (mh, mw) = bool(n % 2), (8, 24)[(n // 2) % 2], ((H, W), (8, 12))[(n // 3) % 2]
            seen.add((x2, c, mh))
            masks = tv._masks(nobj, F, mh, mw, soft=bool((n // 5) % 2), g=g)
            nsrc = nobj + 1 if smap is None else smap[0]
            what = (nobj, ndst, base0, K, bin(active), smap, x2, c, (mh, mw))
            b = _Batch(layout, nsrc + ndst * K, F, H, W, c, 2 if x2 else 1, lead)
            _fill(b, nsrc, smap, nobj, base0, ndst, K, active, g)
            before = b.bits()
            n += 1
            if lead and layout != "nchw":  # the tokens entries read 16-byte vectors only: refused, nothing written
                assert b.direct("_warped", masks, base0, ndst, smap, K, active, table) == -2, what
                _assert_bits(b.bits(), before, what)
                continue
            want = _expect(b, before, masks, rows, base0, ndst, smap, K, active)
            b.run(masks, base0, ndst, smap, nvar=K, active=active, warp=table)
            got = b.bits()
            _assert_bits(got, want, what)
            # the untransformed call on the same inputs writes something else: the map matters
            for t in range(b.T):
                _i16(b.flat[t]).copy_(before[t])
            b.run(masks, base0, ndst, smap, nvar=K, active=active)
            assert any(not torch.equal(a, p) for a, p in zip(got, b.bits())), what
    assert n == (1 + 3 * 2) * 2 * 2 * len(VARIANTS)
    assert len(seen) == 8  # x2 given and not, C = 8 and 24, masks at the site's size and at 8 x 12: every combination


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
        rows = [[ops.level_warp_map(f % 2, -(f % 2), (56756, 32768, -32768, 56756), D, H, W, H, W, H, W) for f in range(F)],
                [ops.level_warp_map(0, 0, (0, 1, -1, 0), 1, H, W, H, W, H, W)] * F]
        masks = tv._masks(2, F, max(1, (H + 1) // 2), max(1, (W + 2) // 3), True, g)
        for base0, (K, active) in ((True, (2, 0b10)), (False, (1, 0b1))):
            b = _Batch(layout, 3 + 2 * K, F, H, W, c, 2, lead)
            _fill(b, 3, None, 2, base0, 2, K, active, g)
            before = b.bits()
            want = _expect(b, before, masks, rows, base0, 2, None, K, active)
            b.run(masks, base0, 2, None, nvar=K, active=active, warp=_table(rows))
            _assert_bits(b.bits(), want, (group, total, base0, K))
            assert any(not torch.equal(a, p) for a, p in zip(b.bits(), before))


# ---- identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["temporal", "nchw"])
def test_a_table_built_from_a_diagonal_matrix_returns_the_bits_of_the_resampled_entries(layout):
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(31)
    F, c = 2, 8
    for (H, W), nobj, (K, active), base0 in itertools.product(((4, 6), (5, 6)), (1, 3), VARIANTS, (False, True)):
        # (py, qy, px, qx, flip_y, flip_x, ay2, ax2, offsets): scale, mirror, an anchor off the centre, a moved frame
        tr3 = [(3, 2, 3, 2, False, True, H, W, ((0, 0), (1, -1))), (1, 2, 1, 1, True, False, 3, W + 1, ((0, 1), (0, 0))),
               (1, 1, 5, 4, False, False, H, W, ((-1, 0), (2 * H + 3, 0)))][:nobj]
        warp = tuple((t[6], t[7], tuple(((-1 if t[4] else 1) * t[1] * t[2], 0, 0, (-1 if t[5] else 1) * t[3] * t[0], t[0] * t[2], dy, dx)
                                        for dy, dx in t[8])) for t in tr3)
        axis = ops.resample_table(tuple(tr3), H, W, H, W, "cuda")
        full = ops.warp_table(warp, H, W, H, W, "cuda")
        assert tuple(full.shape) == (nobj, F, H * W) and tuple(axis.shape) == (nobj, F, H + W)
        masks = tv._masks(nobj, F, 8, 12, True, g)
        for smap in tp._maps(nobj):
            nsrc = nobj + 1 if smap is None else smap[0]
            a = _Batch(layout, nsrc + 2 * K, F, H, W, c, 2)
            _fill(a, nsrc, smap, nobj, base0, 2, K, active, g)
            before = a.bits()
            a.run(masks, base0, 2, smap, nvar=K, active=active, warp=full)
            got = a.bits()
            for t in range(2):
                _i16(a.flat[t]).copy_(before[t])
            a.run(masks, base0, 2, smap, nvar=K, active=active, resample=axis)
            _assert_bits(got, a.bits(), (H, W, nobj, K, active, base0, smap))
            assert any(not torch.equal(x, y) for x, y in zip(got, before))


@pytest.mark.parametrize("layout", ["spatial", "nchw"])
def test_a_quarter_turn_on_a_square_site_is_the_unplaced_entry_on_rot90_chunks(layout):
    from mvoc_amd import ops
    from mvoc_amd.pipeline import resolve_obj_transforms
    g = torch.Generator().manual_seed(32)
    F, S, c = 2, 6, 8
    for k in (1, 2, 3):
        warp = resolve_obj_transforms([{"rotate": 90 * k}, {"rotate": [90 * k, -90 * (4 - k)]}] if k != 2 else
                                      [{"rotate": [180, 90]}, {"rotate": 180.0}], 2, F, S, S)[2]
        turns = [[k, k], [k, k]] if k != 2 else [[2, 1], [2, 2]]
        table = ops.warp_table(warp, S, S, S, S, "cuda")
        masks = tv._masks(2, F, S, S, True, g)
        b = _Batch(layout, 5, F, S, S, c, 1)
        _fill(b, 3, None, 2, True, 2, 1, 1, g)
        before = b.bits()
        twin = _Batch(layout, 5, F, S, S, c, 1)
        _i16(twin.flat[0]).copy_(before[0])
        for j in range(2):
            for f in range(F):
                twin.logical(0)[1 + j, f] = torch.rot90(b.logical(0)[1 + j, f], turns[j][f], (0, 1))
        twin.run(masks, True, 2)
        b.run(masks, True, 2, warp=table)
        assert torch.equal(_i16(b.logical(0)[3:]), _i16(twin.logical(0)[3:])), k
        assert torch.equal(_i16(b.flat[0])[:GUARD + 3 * F * S * S * c], before[0][:GUARD + 3 * F * S * S * c])  # sources, guard


@pytest.mark.parametrize("layout", ["spatial", "nchw"])
def test_every_int32_table_entry_is_safe_and_means_absent(layout):
    """INT32_MIN, -1, H * W and INT32_MAX: the objects are absent everywhere, the result is the base blended with zero objects under
    zero masks, and nothing outside the batch is read (the source chunks hold NaN: one stray load would show)"""
    g = torch.Generator().manual_seed(33)
    F, c = 2, 8
    for (H, W), base0 in itertools.product(((4, 6), (5, 6)), (True, False)):
        junk = [pc.I32MIN, -1, H * W, pc.I32MAX]
        rows = [[[junk[(p + f + j) % 4] for p in range(H * W)] for f in range(F)] for j in range(2)]
        masks = tv._masks(2, F, H, W, True, g)
        b = _Batch(layout, 5, F, H, W, c, 2)
        _fill(b, 3, None, 2, base0, 2, 1, 1, g)
        for t in range(2):
            b.logical(t)[1:3] = NAN  # the object chunks: never read
        before = b.bits()
        b.run(masks, base0, 2, warp=_table(rows))
        got = b.bits()
        twin = _Batch(layout, 5, F, H, W, c, 2)
        for t in range(2):
            _i16(twin.flat[t]).copy_(before[t])
            twin.logical(t)[1:3] = 0.0
        twin.run(torch.zeros_like(masks), base0, 2)
        for t in range(2):
            assert torch.equal(_i16(b.logical(t)[3:]), _i16(twin.logical(t)[3:])), (H, W, base0, t)
            assert not torch.isnan(b.logical(t)[3:]).any()
            lo = GUARD + 3 * F * H * W * c
            assert torch.equal(got[t][:lo], before[t][:lo]) and torch.equal(got[t][-GUARD:], before[t][-GUARD:])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_warped_entries_refuse_bad_arguments_and_write_nothing():
    from mvoc_amd import ops
    F, H, W, c = 2, 4, 4, 8
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    tok, nchw = _Batch("spatial", 9, F, H, W, c, 2), _Batch("nchw", 9, F, H, W, c, 1)
    for b in (tok, nchw):
        for f in b.flat:
            f[GUARD:-GUARD] = 0
    before = tok.bits() + nchw.bits()
    table = _table(_spec_rows(2, H, W))
    err = lambda: ops.lib.mvoc_last_error().decode()
    cases = [  # (nvar, active, map, table, base_chunk0, text)
        (0, 1, None, table, None, "nvar 0"), (9, 1, None, table, None, "nvar 9"),
        (3, 0, None, table, None, "active mask 0x0"), (3, 8, None, table, None, "active mask 0x8"), (1, 2, None, table, None, "active mask 0x2"),
        (2, 3, (0, (0, 0)), table, None, "nsrc 0"), (2, 3, (2, (0, 2)), table, None, "obj_chunk[1] = 2"),
        (2, 3, (2, (-1, 0)), table, None, "obj_chunk[0] = -1"),
        (2, 3, None, None, None, "null map table"),
        (1, 1, (2, (0, 1)), table, -1, "base_chunk0 = -1"),
    ]
    for nvar, active, smap, tab, b0, text in cases:
        assert tok.direct("_warped", masks, False if b0 is None else b0, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
        assert nchw.direct("_warped", masks, True if b0 is None else b0, 2, smap, nvar, active, tab) == -1, text
        assert text in err(), (text, err())
    # the tokens alignment rules: channels and strides in multiples of 8, 16-byte aligned pointers
    d = ops._pnp_desc(tok.x[0], tok.x[1], masks, F * H * W * c, H * W * c, c, F, H, W, c, False, 2)
    arr = (C.c_int32 * 2)(1, 2)
    call = lambda: ops.lib.mvoc_pnp_blend_scatter_tokens_warped(C.byref(d), 3, arr, 1, 1, table.data_ptr(), ops._stream())
    for field, value, text in (("channels", 12, "multiples of 8"), ("p_stride", 12, "multiples of 8"), ("x", tok.x[0].data_ptr() + 2, "16-byte aligned")):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert call() == -2 and text in err(), (field, err())
        setattr(d, field, keep)
    # a valid call with the same buffers goes through (the refusals above were about the arguments)
    assert tok.direct("_warped", masks, False, 2, None, 3, 0b111, table) == 0, err()
    assert nchw.direct("_warped", masks, True, 2, None, 1, 1, table) == 0, err()
    # the Python layer: the table's form, and the arguments a warp table does not combine with
    form = r"warp must be a contiguous int32 \[nobj = 2, F = 2, H \* W = 16\] table"
    with pytest.raises(RuntimeError, match=form):
        tok.run(masks, False, 2, nvar=2, warp=table[:1])
    with pytest.raises(RuntimeError, match=form):
        nchw.run(masks, True, 2, warp=table[:, :, :15].contiguous())
    with pytest.raises(RuntimeError, match=form):
        nchw.run(masks, True, 2, warp=torch.stack([table, table]))  # no per-variant form
    with pytest.raises(RuntimeError, match="warp"):
        nchw.run(masks, True, 2, nvar=2, warp=table.long())
    axis = tr._table(tr._spec_maps(2, H, W))
    place = tp._table([[(1, 1), (0, -1)], [(2, 0), (0, 0)]])
    for b, b0 in ((tok, False), (nchw, True)):
        with pytest.raises(RuntimeError, match="warp= is given together with place= / resample="):
            b.run(masks, b0, 2, warp=table, place=place)
        with pytest.raises(RuntimeError, match="warp= is given together with place= / resample="):
            b.run(masks, b0, 2, warp=table, resample=axis)
        with pytest.raises(RuntimeError, match="does not take a .* mask stack"):
            b.run(torch.stack([masks, masks]).contiguous(), b0, 2, nvar=2, warp=table)
    with pytest.raises(RuntimeError, match="no_background"):
        tok.run(masks, False, 2, warp=table, no_background=True)
    with pytest.raises(RuntimeError, match="storage ends"):
        nchw.run(masks, True, 2, nvar=4, warp=table)  # 3 + 8 chunks in a buffer of 9
    torch.cuda.synchronize()
    _assert_bits(tok.bits() + nchw.bits(), before, "zeros blended with zeros: nothing but zeros was ever written, NaN stays NaN")


def test_profiler_counts_the_placed_bytes_and_the_table():
    from mvoc_amd import ops
    F, H, W, c, K = 2, 4, 4, 8, 3
    nrow = F * H * W
    masks = tv._masks(2, F, H, W, False, torch.Generator().manual_seed(0))
    place = tp._table([[(1, 0), (0, 1)], [(0, 0), (-1, -1)]])
    table = _table(_spec_rows(2, H, W))
    ops.prof_enable(True)
    try:
        for base0, ndst, smap, active in ((True, 2, None, 0b101), (False, 1, (2, (1, 1)), 0b100)):
            nsrc = 3 if smap is None else smap[0]
            work = []
            for kw in ({"place": place}, {"warp": table}):
                buf = torch.zeros((nsrc + ndst * K) * nrow, 3 * c, dtype=torch.float16, device="cuda")
                nchw = torch.zeros((nsrc + ndst * K) * F, c, H, W, dtype=torch.float16, device="cuda")
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
            table_bytes = 4 * 2 * F * H * W
            assert work[1][0] == work[0][0] + table_bytes and work[1][1] == work[0][1] + table_bytes, (base0, ndst, smap, active, work)
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


# ---- the plane mover ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nplane", [1, 4])
@pytest.mark.parametrize("hw", [(5, 7), (8, 8), (12, 23)])
def test_warp_planes_against_torch_indexing(hw, nplane):
    from mvoc_amd import ops
    h, w = hw
    F = 3
    g = torch.Generator().manual_seed(10 * h + nplane)
    n = nplane * F * h * w
    mp = lambda dy, dx, m, den: ops.level_warp_map(dy, dx, m, den, h, w, h, w, h, w)
    junk = [pc.I32MIN, pc.I32MAX, h * w, -1, -7, h * w + 1]
    cases = [
        [mp(0, 0, (56756, 32768, -32768, 56756), D), mp(1, -2, (2 * 46341, 2 * 46341, -2 * 46341, 2 * 46341), 3 * D), mp(0, 0, (0, 1, 1, 0), 1)],
        [list(range(h * w)), mp(2 * h + 3, 0, (1, 0, 0, 1), 1), mp(0, 0, (-1, 0, 0, -1), 1)],
        # entries no rule of ours writes: every int32 value means "absent" unless it is a valid pixel
        [[junk[i % len(junk)] if i % 3 == 0 else (i * 5) % (h * w) for i in range(h * w)]] * 3,
    ]
    assert all(v == -1 for v in cases[1][1]) and sorted(cases[1][2]) == list(range(h * w))
    for rows in cases:
        src_buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float16)
        src_buf[GUARD:GUARD + n] = _planted(torch.randn(n, generator=g).half(), g)
        src_buf = src_buf.cuda()
        src = src_buf[GUARD:GUARD + n].view(nplane, F, h, w)
        dst_buf = torch.full((n + 2 * GUARD,), 777.0, dtype=torch.float16, device="cuda")
        out = dst_buf[GUARD:GUARD + n].view(nplane, F, h, w)
        want = torch.stack([torch.stack([_gather_pix(src[pl, f], rows[f]) for f in range(F)]) for pl in range(nplane)])
        got = ops.warp_planes(src if nplane > 1 else src[0], _table(rows), out=out if nplane > 1 else out[0])
        torch.cuda.synchronize()
        assert torch.equal(_i16(got.reshape(want.shape)), _i16(want)), rows
        assert not torch.isnan(out).any()
        assert bool((dst_buf[:GUARD] == 777).all()) and bool((dst_buf[GUARD + n:] == 777).all())  # nothing outside the extent
        assert torch.isnan(src_buf[:GUARD]).all() and torch.isnan(src_buf[GUARD + n:]).all()


def test_warp_planes_refuses_bad_arguments_and_writes_nothing():
    from mvoc_amd import ops
    src = torch.ones(2, 2, 3, 4, dtype=torch.float16, device="cuda")
    dst = torch.zeros_like(src)
    tab = _table([list(range(12))] * 2)
    call = lambda s, d, t, dims=(2, 2, 3, 4): ops.lib.mvoc_gather_planes_warped_f16(s, d, *dims, t, ops._stream())
    err = lambda: ops.lib.mvoc_last_error().decode()
    assert call(None, dst.data_ptr(), tab.data_ptr()) == -1 and "null" in err()
    assert call(src.data_ptr(), None, tab.data_ptr()) == -1 and "null" in err()
    assert call(src.data_ptr(), dst.data_ptr(), None) == -1 and "null" in err()
    assert call(src.data_ptr(), src.data_ptr(), tab.data_ptr()) == -1 and "in place" in err()
    for dims in ((0, 2, 3, 4), (2, 0, 3, 4), (2, 2, -1, 4), (2, 2, 3, 0)):
        assert call(src.data_ptr(), dst.data_ptr(), tab.data_ptr(), dims) == -1 and "dims" in err()
    with pytest.raises(RuntimeError, match="map must be"):
        ops.warp_planes(src, tab[:1])
    with pytest.raises(RuntimeError, match="map must be"):
        ops.warp_planes(src, _table([list(range(7))] * 2))  # the per-axis form (h + w entries) is another table
    with pytest.raises(RuntimeError, match="map"):
        ops.warp_planes(src, tab.float())
    with pytest.raises(RuntimeError, match="out must be"):
        ops.warp_planes(src, tab, out=dst[:1])
    torch.cuda.synchronize()
    assert not dst.any() and bool((src == 1).all())
    assert call(src.data_ptr(), dst.data_ptr(), tab.data_ptr()) == 0 and torch.equal(dst, src)


# ---- engine -------------------------------------------------------------------------------------------------------------------
class _PreGather:
    """``ops.pnp_blend_tokens`` / ``pnp_blend_nchw`` replaced by: gather the object chunks in torch through the 2-D map (zero fill),
    call the unplaced entry with the masks resized and zeroed where the map says absent, restore the source chunks"""

    def __init__(self):
        from mvoc_amd import ops
        self.ops, self.orig, self.calls = ops, (ops.pnp_blend_tokens, ops.pnp_blend_nchw), []

    def __enter__(self):
        self.ops.pnp_blend_tokens, self.ops.pnp_blend_nchw = self.tokens, self.nchw
        return self

    def __exit__(self, *exc):
        self.ops.pnp_blend_tokens, self.ops.pnp_blend_nchw = self.orig

    def tokens(self, x, masks, **kw):
        table = kw.pop("warp")
        rows = table.cpu().tolist()
        F, H, W, c = kw["frames"], kw["height"], kw["width"], kw["channels"]
        nobj = masks.shape[0]
        assert kw.get("src_map") is None and "place" not in kw and "resample" not in kw and tuple(table.shape) == (nobj, F, H * W)
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
                    v[1 + j, f] = _gather_pix(keep[j, f], r)
        out = self.orig[0](x, _masks_eff(masks, rows, H, W), **kw)
        for v, keep in saved:
            v[1:nobj + 1] = keep
        return out

    def nchw(self, x, masks, **kw):
        table = kw.pop("warp")
        rows = table.cpu().tolist()
        F, (H, W), nobj = kw["frames"], x.shape[2:], masks.shape[0]
        assert kw.get("src_map") is None and kw.get("x2") is None and "place" not in kw and "resample" not in kw
        self.calls.append(("nchw", H, W, rows))
        keep = x[F:(nobj + 1) * F].clone()
        for j in range(nobj):
            for f, r in enumerate(rows[j]):
                x[(1 + j) * F + f] = _gather_pix(keep[j * F + f].permute(1, 2, 0), r).permute(2, 0, 1)
        out = self.orig[1](x, _masks_eff(masks, rows, H, W), **kw)
        x[F:(nobj + 1) * F] = keep
        return out


# 30 degrees at scale 3/2, mirrored left-right, on a per-frame path; a turn that grows along the clip about an off-centre anchor
ENGINE_ROTATED = [{"rotate": 30, "scale": "3/2", "flip": "h", "offset": [(-16, 8), (8, 0), (0, -16)]},
                  {"rotate": [-15, 0, "45/2"], "anchor": [40, 24], "offset": (0, 8)}]


def _engine_warp():
    from mvoc_amd.pipeline import resolve_obj_transforms
    pl, trf, warp = resolve_obj_transforms(ENGINE_ROTATED, 2, 3, 8, 8)
    assert pl is None and trf is None and len(warp) == 2
    return warp


@pytest.mark.parametrize("kind", ["qk", "conv_out", "features"])
def test_unet_warped_forward_equals_the_pregathered_unplaced_forward(kind):
    """one Q/K step (spatial + temporal sites, the source tail pruned), one conv_out step (prune_dead_chunks: the NCHW blend on
    the source chunks' outputs) and, with prune_dead_chunks off, the same step through the resnet / temporal-conv feature sites"""
    from mvoc_amd import ops, pnp_utils
    from mvoc_amd.pipeline import I2VGenXLPipeline
    from mvoc_amd.schedulers import DDIMScheduler
    F, h, w, cd = 3, 8, 8, 64
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    warp = _engine_warp()
    moved, table = I2VGenXLPipeline(eng, DDIMScheduler(), use_graphs=False).warp_masks(masks, warp)
    lat_rows = ops.warp_maps(warp, h, w, h, w)
    assert table.tolist() == lat_rows and table.dtype == torch.int32 and tuple(table.shape) == (2, F, h * w)
    for j in range(2):  # the masks in destination coordinates: both forms, every channel, types kept
        for a, b in zip(moved[j], masks[j]):
            assert a.dtype == b.dtype and a.shape == b.shape
            for f, r in enumerate(lat_rows[j]):
                for ch in range(a.shape[1]):
                    assert torch.equal(a[0, ch, f], _gather_pix(b[0, ch, f], r))
        assert not torch.equal(moved[j][0], masks[j][0])
    roles = tv._roles(F, h, w, cd, 4, 1)
    pipe, (t_feat, t_qk) = tv._arm(eng, 5)
    t = t_qk if kind == "qk" else t_feat
    names = ["S", "O", "P", "u0", "c0"]
    saved = eng.prune_dead_chunks

    def forward(value):
        eng.warp, eng.prune_source_tail, eng.prune_dead_chunks = value, True, kind != "features"
        try:
            return tv._fwd(eng, tv._batch(roles, names), t)
        finally:
            eng.warp, eng.prune_source_tail, eng.prune_dead_chunks = None, False, saved

    try:
        pnp_utils.register_time_all(pipe, t, moved)
        got = forward(warp)
        with _PreGather() as pre:
            ref = forward(warp)
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
        assert c[3] == ops.warp_maps(warp, c[1], c[2], h, w), c[:3]
    assert torch.equal(_i16(got[3:]), _i16(ref[3:])), kind
    assert torch.isfinite(got[3:]).all() and not torch.equal(got[3:], plain[3:]), kind  # the warp moved something
    assert eng.warp is None and len(eng._level_tables["warp"][1]) == len({c[1:3] for c in pre.calls})


def test_unet_refuses_a_warp_with_a_shard_another_mode_or_a_wrong_object_count():
    F, h, w = 3, 8, 8
    _, eng = tv._toy_pair()
    _, masks = tv._hook_masks(F, h, w)
    eng.warp = _engine_warp()
    try:
        eng.shard = types.SimpleNamespace(rank=0, world=1)
        with pytest.raises(RuntimeError, match="a warp does not combine with the frame shard"):
            eng.pnp_batch(5, masks)
        with pytest.raises(RuntimeError, match="a warp does not combine with the frame shard"):
            eng.place_kw(masks, 8, 8)
        eng.shard = None
        eng.transform = tr.ENGINE_TRANSFORM
        with pytest.raises(RuntimeError, match="warp is set together with"):
            eng.place_kw(masks, 8, 8)
        eng.transform = None
        with pytest.raises(RuntimeError, match="warp holds 2 objects, the hooks carry 1 masks"):
            eng.place_kw(masks[:1], 8, 8)
        tab = eng.place_kw(masks, 4, 4)["warp"]
        assert tuple(tab.shape) == (2, F, 16) and tab.dtype == torch.int32 and tab.is_cuda
        assert eng.place_kw(masks, 4, 4)["warp"] is tab  # cached per level
        assert eng.place_table(masks, 4, 4) is None  # (the place= argument alone: a warp is not one)
    finally:
        eng.warp, eng.transform, eng.shard = None, None, None
    assert eng.place_kw(masks, 8, 8) == {}


# ---- pipeline -----------------------------------------------------------------------------------------------------------------
ROTATED = [{"rotate": 30, "scale": "3/2", "flip": "h", "offset": tp.PATH}, {"rotate": [-15, 0, "45/2"], "anchor": [40, 24], "offset": (-16, 8)}]
_job, _graph_keys = tr._job, tr._graph_keys


def _rotated_lat():
    from mvoc_amd.pipeline import resolve_obj_transforms
    return resolve_obj_transforms(ROTATED, 2, 3, 8, 8)[2]


def test_warped_composition_graph_replay_equals_eager_and_moves_the_result():
    from mvoc_amd import ops
    eager = _job(False, ROTATED, count_calls=True)
    st = eager.state
    warp = _rotated_lat()
    assert st["warp"] == warp and all(st[k] is None for k in ("placement", "transform", "place_dev", "resample_dev"))
    rows = ops.warp_maps(warp, 8, 8, 8, 8)
    assert st["warp_dev"].tolist() == rows
    # the call's masks, everywhere, are the gathered ones: built once, in destination coordinates (the S = L maps)
    for j in range(2):
        for f, r in enumerate(rows[j]):
            want = _gather_pix(eager.masks[j][0][0, 0, f].cuda(), r)
            assert torch.equal(st["fusion_masks"][j, 0, 0, f], want) and torch.equal(st["masks"][j][0][0, 0, f].cuda().half(), want)
            assert torch.equal(st["masks"][j][1][0, 0, f].cuda(), _gather_pix(eager.masks[j][1][0, 0, f].cuda(), r))
    # the per-level tables (8 x 8, 4 x 4, 2 x 2) stay alive with the state, whose graphs would read them
    assert len(st["place_tables"]) == 1 and {k[:2] for k in st["place_tables"][0]} == {(8, 8), (4, 4), (2, 2)}
    names = set().union(*eager.step_calls)
    assert {"mvoc_pnp_blend_scatter_tokens_warped", "mvoc_pnp_blend_scatter_nchw_warped", "mvoc_gather_planes_warped_f16"} <= names
    assert not any(n.startswith("mvoc_pnp_blend") and not n.endswith("_warped") for n in names), names
    assert "mvoc_shift_planes_f16" not in names and "mvoc_gather_planes_f16" not in names
    # two fusion steps: the two fusion objects go through the warp mover instead of a copy
    assert [c.get("mvoc_gather_planes_warped_f16", 0) for c in eager.step_calls] == [2, 2, 0, 0, 0]
    graphed = _job(True, ROTATED)
    assert torch.equal(graphed.out, eager.out) and torch.isfinite(eager.out).all()
    assert any("warp" in k and warp in k for k in graphed.state["variants"])  # the warp is part of the graph-variant key
    plain = _job(False)
    assert plain.out.shape == eager.out.shape and not torch.equal(plain.out, eager.out)
    unturned = _job(False, [{k: v for k, v in d.items() if k != "rotate"} for d in ROTATED])  # the same job without the turn
    assert unturned.state["warp"] is None and unturned.state["transform"] is not None
    assert not torch.equal(unturned.out, eager.out)


def test_rotate_zero_makes_the_calls_and_graphs_of_a_call_without_it():
    zero = [{"rotate": 0}, {"rotate": [0, 360, -720.0]}]
    plain, same = _job(False, count_calls=True), _job(False, zero, count_calls=True)
    assert all(same.state[k] is None for k in ("warp", "warp_dev", "transform", "placement"))
    assert len(plain.step_calls) == len(same.step_calls) == 5
    for i, (a, b) in enumerate(zip(plain.step_calls, same.step_calls)):
        assert a == b and sum(a.values()) > 0, (i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
        assert not any("_warped" in n or n.endswith("_resampled") or n.endswith("_placed") for n in b)
    assert torch.equal(plain.out, same.out)
    gp, gs = _job(True), _job(True, zero)
    assert gp.graphs == gs.graphs >= 3 and torch.equal(gp.out, gs.out) and torch.equal(gp.out, plain.out)
    assert _graph_keys(gp.state) == _graph_keys(gs.state)


def test_rotate_180_makes_the_calls_and_graphs_of_the_flip_hv_call():
    half = [{"rotate": 180, "scale": "3/2", "offset": tp.PATH}, {"rotate": -180.0, "flip": "h"}]
    flip = [{"flip": "hv", "scale": "3/2", "offset": tp.PATH}, {"flip": "v"}]
    flipped, same = _job(False, flip, count_calls=True), _job(False, half, count_calls=True)
    assert same.state["warp"] is None and same.state["transform"] == flipped.state["transform"] is not None
    for i, (a, b) in enumerate(zip(flipped.step_calls, same.step_calls)):
        assert a == b and sum(a.values()) > 0, (i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
        assert not any("_warped" in n for n in b)
    assert any(n.endswith("_resampled") for c in same.step_calls for n in c)
    assert torch.equal(flipped.out, same.out)
    gf, gs = _job(True, flip), _job(True, half)
    assert gf.graphs == gs.graphs and _graph_keys(gf.state) == _graph_keys(gs.state) and torch.equal(gf.out, gs.out)
    assert torch.equal(gf.out, flipped.out)


def test_a_frame_sharded_pipeline_refuses_a_rotation():
    with pytest.raises(RuntimeError, match="obj_transforms do not combine with the frame shard"):
        _job(False, ROTATED, shard=True)


def test_offsets_next_to_a_rotation_are_refused():
    with pytest.raises(ValueError, match="obj_transforms is given together with obj_offsets"):
        _job(False, ROTATED, offsets=tp.OFFSETS)


def test_two_variants_share_one_warp():
    moved, plain = _job(True, ROTATED, K=2), _job(True, K=2)
    assert moved.out.shape[0] == 2 and torch.isfinite(moved.out).all()
    assert moved.state["nvar"] == 2 and moved.state["warp"] == _rotated_lat()
    assert moved.graphs == plain.graphs  # the warp is one more part of the key, not one more step kind
    for k in range(2):
        assert not torch.equal(moved.out[k], plain.out[k]), k
    assert not torch.equal(moved.out[0], moved.out[1])
    eager = _job(False, ROTATED, K=2)
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
        job = _job(False, ROTATED)
    finally:
        ops.latent_fusion = orig
    assert len(seen) == 2  # fusion_steps = (0, 2)
    s = DDIMScheduler()
    s.set_timesteps(5)
    t0 = int(s.timesteps[0])  # both fusion steps read the objects' latents of the first timestep (the reference's counter stays 0)
    rows = ops.warp_maps(_rotated_lat(), 8, 8, 8, 8)
    for objs, masks in seen:
        for j, d in enumerate(("/virtual/o1", "/virtual/o2")):
            lat = job.pipe.latent_cache.get(d, t0).cuda().half()
            for f, r in enumerate(rows[j]):
                for ch in range(4):
                    assert torch.equal(_i16(objs[j, 0, ch, f]), _i16(_gather_pix(lat[0, ch, f], r))), (j, f, ch)
                    assert torch.equal(masks[j, 0, ch, f], _gather_pix(job.masks[j][0][0, ch, f].cuda(), r)), (j, f, ch)
            assert not torch.equal(objs[j], lat)
