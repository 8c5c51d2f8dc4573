"""What include/mvoc_hip.h promises about the blend-scatter family, the two plane movers and the loop glue (mvoc_amd/csrc/pnp.hip,
pnp_variants2.hip, pnp_blend.h), through the C ABI (mvoc_amd._ffi: mvoc_amd.ops cannot say every pitch and pointer offset).  The header
declares sixteen mvoc_pnp_blend_scatter_* entries (eight per layout), mvoc_shift_planes_f16 / mvoc_gather_planes_f16 and four glue
entries; every one is documented BIT-EXACT against the reference's eager fp16 op chain, and every one is compared here with ONE plain
numpy-float16 restatement of the header (tests/pnp_contract.py: blend_reference, the plane and glue references), never with another
kernel.  tests/test_pnp_contract_cpu.py shows the references equal to oracle/ and to the reference's captures and the walk able to fail.

  W  the walk, per entry and layout (test_blend_walk): a pairwise covering array over geometry (1x1x1; non-integer mask ratios; a vector
     that straddles two rows; a mask coarser than the features; the (in -> out) pairs 26->22, 14->46, 39->33 on which F.interpolate's
     float rule is not the exact quotient, on both axes and in both NCHW forms), channels (tokens 8 / 24 / 64, NCHW 1 / 3 / 20), nobj
     1..4, ndst 0 / 1 / 2, base_chunk0 0 / 1 (-1 on the positional tokens entry), source maps (identity, reversed, all objects on one
     chunk with nsrc = 2, an object on chunk 0), (nvar, active) in (1, 1) (2, 3) (3, 0b101) (8, 0xff) (8, 0x80), offset tables and index
     maps (zeros / identity, small shifts, an object absent in one frame, scale 3/2, scale 1/2, mirror, entries of INT32_MIN, INT32_MAX,
     height, width and -1), a table and masks per variant, hard and soft masks, x2 given and NULL, and for tokens the spatial and the
     temporal strides, pitch C and 3C (x2 = columns [C, 2C) of the same rows), chunk_stride dense and + 8 rows, x 16 and 128 bytes past
     a 256-byte boundary; then shapes of 255, 256, 257 and 513 work items per tensor for the tokens, the 8-wide and the 1-wide NCHW
     item (the tail block, a full block, a block and an item, three blocks); an index mask (base 0, object 1.0, mask cell = a distinct
     small integer) on the float-rule pairs, so the result IS the sampled cell; and the special-value atlas -- 16 fp16 values (+-0,
     +-1, +-65504, +-inf, NaN, subnormals, the neighbours of 2^-14) as base x the same as object x 6 mask values, 1 536 combinations,
     unmoved in frame 0 and with pixels that lose their object in frame 1
  in EVERY blend and plane case: the entry returns 0; the WHOLE allocation equals, as int16, the reference at the described destination
     elements and the bytes from before the call everywhere else (guards in front and behind, pitch columns, chunk gaps, every source
     chunk, the chunks of variants whose bit is clear, masks, tables); everything the contract says is not read held fp16 NaN (chunk 0
     when it is neither base nor an object's chunk, every u_k, every c_k under base_chunk0 = 1, the masks of idle variants; their table
     rows INT32_MIN); where the reference is NaN the result must be NaN (sign and payload free, tests/test_variants_gpu.py says why):
     no element of a random case, 15 to 18.4 % of an atlas
  P  shift_planes / gather_planes: sizes 1 .. 513 elements, every table kind, random and special values, the copy bit for bit
  G  loop glue (test_ddim_walk, test_fusion_walk): n and n_per in 1, 100, 255, 256, 257, 513, nvar 1, 2, 3, 8 with a coefficient row
     per variant, uncond NULL and given, nobj 0, 1, 2, 4, obj_random_noise_fusion 0 and 1, hard and soft masks, three rows each of the
     DDIM and the inverse table of mvoc_amd.schedulers and hand-made rows, the 16 special values in every operand, NaN guards around
     every operand, the output allocation compared whole
  I  every scalar product alone (test_*_product_over_every_operand): the seven product sites of the DDIM step and the four of the
     fusion, each over ALL 65 536 fp16 patterns of its free operand with the other products multiplied by 0 or 1, through the single
     and the variants kernel; scalars 0.3 / 0.99 (126 / 310 operands on which one rounding and two differ; 9.0, 0.8 and 0.5 have
     none); and mix = 0.65, where f32(1.0 - mix) and 1.0f - f32(mix) differ
  A  the alignment the vector forms need: a tokens entry refuses x or x2 off a 16-byte boundary (-2, nothing launched); the NCHW
     entries run H * W = 24 with x two bytes past a boundary through the 1-wide form, bit-exact.  Before this file existed the host
     checked channels and strides but not the pointers.  Nothing here launches a tokens entry on a misaligned pointer.
  E  refusals, every documented one of the 22 entries: the code, a text that names the family and the cause, not one byte of any
     operand changed, and the same buffers with the described arguments then run bit-exact

What it cannot hold: launches beyond 2^31 bytes, the profiler's byte counts, dispatch policy, speed; two mask sets or tables that
overlap; the tokens kernels at a channel count that is no multiple of 8 (refused).

Kernel perturbations tried on an MI355X against this file (never committed; each changes arithmetic or reads inside the test's own
allocations, so wrong data at most):
  * the empty asm of smul16 removed (hipcc contracts the product and its rounding): 18 of 55 tests tripped -- every test of I with
    exactly the CPU's counts (126 of 65 536 elements per DDIM site, 126 / 310 / 280 / 310 for the fusion), the glue refusals'
    corrected calls, and G by ONE element (n100_nvar3_u0: 1 of 300; n1_nvar3_nobj1_rnf1_soft: 1 of 3).  Sizes of a few hundred
    elements hold a product by luck; section I is what holds it.
  * the nearest rule in integers (dst * in / out): all 16 test_blend_walk tripped, first on the 1x39 -> 1x33 geometry of the
    pairwise rows (192 elements), none of the other sections.
  * var_dst's two blocks swapped: the 12 test_blend_walk and the 12 test_blend_refusals of the entries with variants tripped (the
    base read from a NaN u_k; c_k written where u_k belongs); the positional and mapped kernels do not use var_dst.
  * blend16_h replaced by the float form behind the select, in two spellings (blend16 on converted operands; float masks through
    the DIRECT branch for every source rule): NOT seen, all 55 passed both times.  With this compiler neither spelling produced the
    +0.0 that pnp_blend.h describes.  The atlas holds the combination that would show it (base -0.0, object -1.0, mask 0, frame 0:
    the product -0.0 decides the sign of the sum), and the CPU mutation product_plus_zero trips every entry's atlas.

No defect of the kernels was found.  The one change to the library is A.

Measured on an MI355X: the whole file, 55 tests and about 1 800 launches (971 of them the blend walk), takes 3.7 to 4.0 s; the slowest
test is test_blend_walk[tokens-pos] at 0.27 s (46 launches and the process's first); no other test takes more than 0.22 s."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_contract as PC  # noqa: E402
from mvoc_amd._ffi import PnpDesc, i32, lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5A5A  # what an output allocation of the glue holds before the call


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return lib.mvoc_last_error().decode()


def _dev(a):
    t = torch.from_numpy(a).to(DEV)
    assert t.data_ptr() % 256 == 0
    return t


# ---- the blend entries ------------------------------------------------------------------------------------------------------------
class Launch:
    """the device buffers of one packed case and the arguments of its entry"""

    def __init__(self, c):
        self.c, self.P = c, PC.pack(c)
        P = self.P
        self.feat, self.masks = _dev(P.feat), _dev(P.masks)
        self.table = _dev(P.table) if P.table is not None else None
        self.set_args()

    def set_args(self):
        """the arguments the case describes, on this object's buffers"""
        c, P = self.c, self.P
        x = [self.feat.data_ptr() + 2 * o for o in P.x_off]
        self.d = PnpDesc(x=x[0], x2=x[1] if c.T == 2 else None, masks=self.masks.data_ptr() + 2 * P.m_off,
                         chunk_stride=P.chunk_stride, f_stride=P.f_stride, p_stride=P.p_stride, nobj=c.nobj, frames=c.F, height=c.H,
                         width=c.W, channels=c.C, mask_h=c.mh, mask_w=c.mw, base_chunk0=c.base, ndst=c.ndst)
        self.dptr = C.byref(self.d)
        self.nsrc, self.nvar, self.active = c.nsrc, c.nvar, c.active
        self.oc = (i32 * c.nobj)(*c.obj_chunk)
        self.tptr = self.table.data_ptr() + 4 * P.t_off if self.table is not None else None

    def call(self):
        e = self.c.entry
        args = [self.dptr]
        if e != "pos":
            args += [self.nsrc, self.oc]
        if e not in ("pos", "mapped"):
            args += [self.nvar]
        if e not in ("pos", "mapped", "variants"):
            args += [self.active]
        if PC.SRC_RULE[e] != "direct":
            args += [self.tptr]
        return getattr(lib, PC.symbol(self.c.layout, e))(*args, _stream())

    def after(self):
        torch.cuda.synchronize()
        return self.feat.cpu().numpy()

    def inputs_unchanged(self):
        ok = np.array_equal(self.masks.cpu().numpy(), self.P.masks)
        return ok and (self.table is None or np.array_equal(self.table.cpu().numpy(), self.P.table))

    def check(self):
        """the WHOLE allocation: the reference at the described destination elements, the bytes from before everywhere else"""
        after = self.after()
        bad, nan = PC.compare(after, self.P.expect, self.P.dest)
        if bad:
            where = np.flatnonzero(~np.where(np.isnan(self.P.expect.view(PC.F16)) & self.P.dest, np.isnan(after.view(PC.F16)),
                                             after == self.P.expect))
            pytest.fail(f"{self.c}: {bad} elements differ ({int(self.P.dest[where].sum())} of them destination elements), first at "
                        f"{where[:4].tolist()}: got {after[where[:4]].tolist()}, want {self.P.expect[where[:4]].tolist()}")
        assert self.inputs_unchanged(), f"{self.c}: the masks or the table changed"
        return nan


def _run(c):
    L = Launch(c)
    rc = L.call()
    assert rc == 0, (str(c), rc, _err())
    nan = L.check()
    if c.kind != "atlas":
        assert nan == 0, c  # on random data no NaN reaches a result
    else:
        assert 0 < nan < L.P.dest.sum() / 4, c


@pytest.mark.parametrize("entry", PC.ENTRIES)
@pytest.mark.parametrize("layout", PC.LAYOUTS)
def test_blend_walk(layout, entry):
    """the pairwise walk, the work-item totals 255 / 256 / 257 / 513, the nearest-rule index masks and the special-value atlas"""
    w = PC.walk_cases(layout, entry)
    for kind in ("pairs", "totals", "index"):
        for c in w[kind]:
            _run(c)
    for c in w["atlas"]:
        _run(c)


def test_nchw_two_bytes_past_an_aligned_address():
    """H * W = 24 would take the 8-wide form; x two bytes past a 16-byte boundary must go through the 1-wide form, bit-exact"""
    c = PC.nchw_misaligned_case()
    L = Launch(c)
    assert L.d.x % 16 == 2 and c.H * c.W == 24
    assert L.call() == 0, _err()
    L.check()


# ---- planes ------------------------------------------------------------------------------------------------------------------------
def _plane_buffers(src, table, ref):
    n, G = src.size, PC.GUARD
    s = np.full(n + 2 * G, PC.NAN_BITS, np.int16)
    s[G:G + n] = PC.bits(src).ravel()
    t = np.full(table.size + 32, PC.I32MIN, np.int32)
    t[16:16 + table.size] = table.ravel()
    before = np.full(n + 2 * G, SENTINEL, np.int16)
    expect = before.copy()
    expect[G:G + n] = PC.bits(ref).ravel()
    return s, t, before, expect


def _plane_fn(kind):
    return lib.mvoc_shift_planes_f16 if kind == "shift" else lib.mvoc_gather_planes_f16


@pytest.mark.parametrize("special", [False, True], ids=["random", "special_values"])
def test_planes(special):
    for kind, npl, Fr, h, w, tk, seed in PC.plane_cases():
        src, table, ref = PC.plane_case(kind, npl, Fr, h, w, tk, seed, special)
        s, t, before, expect = _plane_buffers(src, table, ref)
        ds, dt, dd = _dev(s), _dev(t), _dev(before)
        G = PC.GUARD
        rc = _plane_fn(kind)(ds.data_ptr() + 2 * G, dd.data_ptr() + 2 * G, npl, Fr, h, w, dt.data_ptr() + 64, _stream())
        assert rc == 0, _err()
        torch.cuda.synchronize()
        # a moved element keeps its bits (NaN payloads included): a copy, not arithmetic
        assert np.array_equal(dd.cpu().numpy(), expect), (kind, npl, Fr, h, w, tk)
        assert np.array_equal(ds.cpu().numpy(), s) and np.array_equal(dt.cpu().numpy(), t)


# ---- loop glue ---------------------------------------------------------------------------------------------------------------------
def _guarded(a, fill=PC.NAN_BITS):
    """fp16 operand with NaN guards -> (device tensor, pointer to the data, host copy)"""
    G = PC.GUARD
    flat = PC.bits(np.ascontiguousarray(a)).ravel()
    host = np.full(flat.size + 2 * G, fill, np.int16)
    host[G:G + flat.size] = flat
    dev = _dev(host)
    return dev, dev.data_ptr() + 2 * G, host


def _out_buffer(n):
    """an output allocation, SENTINEL throughout -> (device tensor, pointer to the described elements)"""
    dev = _dev(np.full(n + 2 * PC.GUARD, SENTINEL, np.int16))
    return dev, dev.data_ptr() + 2 * PC.GUARD


def _check_out(dev, ref, what):
    G = PC.GUARD
    torch.cuda.synchronize()
    after = dev.cpu().numpy()
    n = ref.size
    expect = np.full(n + 2 * G, SENTINEL, np.int16)
    expect[G:G + n] = PC.bits(ref).ravel()
    dest = np.zeros(n + 2 * G, bool)
    dest[G:G + n] = True
    bad, nan = PC.compare(after, expect, dest)
    assert bad == 0, f"{what}: {bad} of {n} elements differ"
    return nan


def _ddim(nvar, x, vu, vc, coef, what):
    """nvar = 0: mvoc_ddim_step_f16 on row 0; else the variants entry on [nvar][n_per]"""
    K, n = x.shape
    ops = [_guarded(x), _guarded(vu) if vu is not None else (None, None, None), _guarded(vc)]
    cf = np.full(5 * K + 16, np.nan, np.float32)
    cf[8:8 + 5 * K] = np.asarray(coef, np.float32).ravel()
    dcf = _dev(cf)
    out = _out_buffer(K * n)
    if nvar == 0:
        rc = lib.mvoc_ddim_step_f16(ops[0][1], ops[1][1], ops[2][1], dcf.data_ptr() + 32, out[1], n, _stream())
        ref = PC.ddim_reference(x[0], None if vu is None else vu[0], vc[0], coef[0])
    else:
        rc = lib.mvoc_ddim_step_variants_f16(ops[0][1], ops[1][1], ops[2][1], dcf.data_ptr() + 32, out[1], n, nvar, _stream())
        ref = PC.ddim_variants_reference(x, vu, vc, coef)
    assert rc == 0, (what, _err())
    nan = _check_out(out[0], ref, what)
    for dev, _, host in ops:
        assert dev is None or np.array_equal(dev.cpu().numpy(), host), what
    return nan


def _fusion(nvar, lat, bg, objs, masks, mix, rnf, what):
    K, n = lat.shape
    nobj = len(objs)
    pad = np.zeros((1, n), PC.F16)  # nobj = 0: the entry still wants non-NULL pointers
    ops = [_guarded(lat), _guarded(bg), _guarded(objs if nobj else pad), _guarded(masks if nobj else pad)]
    out = _out_buffer(K * n)
    if nvar == 0:
        rc = lib.mvoc_latent_fusion_f16(ops[0][1], ops[1][1], ops[2][1], ops[3][1], out[1], nobj, n, float(mix), int(rnf), _stream())
        ref = PC.fusion_reference(lat[0], bg, objs, masks, mix, rnf)
    else:
        rc = lib.mvoc_latent_fusion_variants_f16(ops[0][1], ops[1][1], ops[2][1], ops[3][1], out[1], nobj, n, nvar, float(mix), int(rnf),
                                                 _stream())
        ref = PC.fusion_variants_reference(lat, bg, objs, masks, mix, rnf)
    assert rc == 0, (what, _err())
    nan = _check_out(out[0], ref, what)
    for dev, _, host in ops:
        assert np.array_equal(dev.cpu().numpy(), host), what
    return nan


def test_ddim_walk():
    """n and n_per in 1, 100, 255, 256, 257, 513 (n_per = 100, nvar = 8: three variants in one block), uncond NULL and given, nvar 1,
    2, 3, 8 with a coefficient row per variant, scheduler and hand-made rows, the 16 special values in x, v and uncond"""
    for name, nvar, x, vu, vc, coef in PC.ddim_cases(PC.scheduler_rows()):
        nan = _ddim(nvar, x, vu, vc, coef, name)
        assert nan == 0 or name.startswith("special"), name


def test_fusion_walk():
    for name, nvar, lat, bg, objs, masks, mix, rnf in PC.fusion_cases():
        nan = _fusion(nvar, lat, bg, objs, masks, mix, rnf, name)
        assert nan == 0 or name.startswith("special"), name


@pytest.mark.parametrize("site", PC.DDIM_SITES)
def test_ddim_product_over_every_operand(site):
    """one scalar product alone, over all 65 536 fp16 patterns of its operand, on both kernels: a product rounded once differs from
    the reference in at least 32 of these elements (tests/test_pnp_contract_cpu.py)"""
    x, vu, vc, coef = PC.ddim_isolating_case(site)
    one = lambda a: None if a is None else a[None]
    two = lambda a: None if a is None else a.reshape(2, -1)
    _ddim(0, one(x), one(vu), one(vc), [coef], site)
    _ddim(2, two(x), two(vu), two(vc), [coef, coef], site + " (variants)")


@pytest.mark.parametrize("site", PC.FUSION_SITES + ("omix_form",))
def test_fusion_product_over_every_operand(site):
    lat, bg, objs, masks, mix, rnf = PC.fusion_isolating_case(site)
    _fusion(0, lat[None], bg, objs, masks, mix, rnf, site)
    # the variants entry reads bg / objs / masks of n_per elements for every variant: the free operand must be per element, so the
    # 65 536 patterns go through it as ONE variant when they sit in a shared operand, as two when they sit in the latents
    if site in ("mix_lat", "mix_fg"):
        h = 32768
        for half in (slice(0, h), slice(h, None)):
            _fusion(2, np.stack([lat[half], lat[half]]), bg[half], objs[:, half], masks[:, half], mix, rnf, site + " (variants)")
    else:
        _fusion(1, lat[None], bg, objs, masks, mix, rnf, site + " (variants)")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _set_d(**kw):
    def change(L):
        for k, v in kw.items():
            setattr(L.d, k, v)
    return change


def _add_d(name, n):
    def change(L):
        setattr(L.d, name, getattr(L.d, name) + n)
    return change


def _set(**kw):
    def change(L):
        for k, v in kw.items():
            setattr(L, k, v)
    return change


def _oc(j, v):
    def change(L):
        L.oc[j] = v(L) if callable(v) else v
    return change


def _refusals(layout, entry):
    """(what, change, code, a piece of the text)"""
    r = [("null descriptor", _set(dptr=None), -1, "null operand"), ("null x", _set_d(x=None), -1, "null operand"),
         ("null masks", _set_d(masks=None), -1, "null operand"), ("nobj 0", _set_d(nobj=0), -2, "nobj"), ("nobj 5", _set_d(nobj=5), -2, "nobj"),
         ("ndst 3", _set_d(ndst=3), -1, "ndst")]
    r += [(f"{dim} 0", _set_d(**{dim: 0}), -1, "bad dims") for dim in ("frames", "height", "width", "channels", "mask_h", "mask_w")]
    if layout == "tokens":
        r += [("channels 12", _set_d(channels=12), -2, "multiples of 8")]
        r += [(f"{s} + 4", _add_d(s, 4), -2, "multiples of 8") for s in ("chunk_stride", "f_stride", "p_stride")]
        # the alignment refusal: returned before anything is launched (the check of the whole allocation below would not survive a
        # launch, and the call after it runs on the aligned pointers)
        r += [("x 2 bytes off", _add_d("x", 2), -2, "16-byte aligned"), ("x 8 bytes off", _add_d("x", 8), -2, "16-byte aligned"),
              ("x2 8 bytes off", _add_d("x2", 8), -2, "16-byte aligned")]
    if entry != "pos":
        r += [("null obj_chunk", _set(oc=None), -1, "null obj_chunk"), ("nsrc 0", _set(nsrc=0), -1, "nsrc"),
              ("nsrc nobj + 2", _set(nsrc=4), -1, "nsrc"), ("obj_chunk -1", _oc(0, -1), -1, "obj_chunk[0]"),
              ("obj_chunk nsrc", _oc(1, lambda L: L.nsrc), -1, "obj_chunk[1]")]
    if entry not in ("pos", "mapped"):
        r += [("nvar 0", _set(nvar=0), -1, "nvar"), ("nvar 9", _set(nvar=9), -1, "nvar")]
    if entry not in ("pos", "mapped", "variants"):
        r += [("active 0", _set(active=0), -1, "active"), ("active 1 << nvar", _set(active=4), -1, "active")]
    if PC.SRC_RULE[entry] != "direct":
        r += [("null table", _set(tptr=None), -1, "table")]
    if (layout, entry) != ("tokens", "pos"):
        r += [("base_chunk0 -1", _set_d(base_chunk0=-1), -1, PC.symbol(layout, entry) + ":")]
    return r


def _refusal_case(layout, entry):
    var = (2, 3) if entry not in ("pos", "mapped") else (1, 1)
    table = {"direct": "none", "shift": "small", "map": "small"}[PC.SRC_RULE[entry]]
    return PC.Case(layout, entry, (2, 4, 6, 8, 12), PC.CHANNELS[layout][0] if layout == "tokens" else 3, 2, 2, 0, "ident", var, table, "soft",
                   True, lead=128 if layout == "tokens" else 256, seed=31337)


@pytest.mark.parametrize("entry", PC.ENTRIES)
@pytest.mark.parametrize("layout", PC.LAYOUTS)
def test_blend_refusals(layout, entry):
    """the documented code, a text that names the family (and says what is wrong), not one byte of any operand changed, and the
    corrected call -- the same buffers, the unchanged arguments -- then succeeds bit-exact"""
    c = _refusal_case(layout, entry)
    for what, change, code, text in _refusals(layout, entry):
        L = Launch(c)
        change(L)
        rc = L.call()
        assert rc == code, (what, rc, _err())
        assert "pnp" in _err() and text in _err(), (what, _err())
        assert np.array_equal(L.after(), L.P.feat) and L.inputs_unchanged(), what
        L.set_args()  # the very buffers of the refused call, the arguments as the case describes them
        assert L.call() == 0, (what, _err())
        L.check()


@pytest.mark.parametrize("kind", ["shift", "gather"])
def test_plane_refusals(kind):
    src, table, ref = PC.plane_case(kind, 2, 2, 4, 6, "small", 5)
    s, t, before, expect = _plane_buffers(src, table, ref)
    G = PC.GUARD
    for what, edit in (("null src", dict(src=None)), ("null dst", dict(dst=None)), ("null table", dict(tab=None)), ("src == dst", dict(dst="src")),
                       ("nplane 0", dict(npl=0)), ("frames 0", dict(Fr=0)), ("h 0", dict(h=0)), ("w 0", dict(w=0))):
        ds, dt, dd = _dev(s), _dev(t), _dev(before)
        a = dict(src=ds.data_ptr() + 2 * G, dst=dd.data_ptr() + 2 * G, npl=2, Fr=2, h=4, w=6, tab=dt.data_ptr() + 64)
        good = dict(a)
        a.update(edit)
        if a["dst"] == "src":
            a["dst"] = a["src"]
        order = ("src", "dst", "npl", "Fr", "h", "w", "tab")
        assert _plane_fn(kind)(*[a[k] for k in order], _stream()) == -1, (what, _err())
        assert f"{kind}_planes" in _err(), _err()
        torch.cuda.synchronize()
        assert np.array_equal(dd.cpu().numpy(), before) and np.array_equal(ds.cpu().numpy(), s) and np.array_equal(dt.cpu().numpy(), t), what
        assert _plane_fn(kind)(*[good[k] for k in order], _stream()) == 0, _err()
        torch.cuda.synchronize()
        assert np.array_equal(dd.cpu().numpy(), expect), what


@pytest.mark.parametrize("entry", ["ddim_step", "ddim_step_variants", "latent_fusion", "latent_fusion_variants"])
def test_glue_refusals(entry):
    rng = np.random.default_rng(11)
    variants, ddim = entry.endswith("variants"), entry.startswith("ddim")
    K, n = (2, 100) if variants else (1, 100)
    fn = getattr(lib, f"mvoc_{entry}_f16")
    if ddim:
        data = dict(x=rng.standard_normal((K, n)).astype(PC.F16), vu=rng.standard_normal((K, n)).astype(PC.F16),
                    vc=rng.standard_normal((K, n)).astype(PC.F16))
        coef = np.array([PC.HAND_ROWS[0], PC.HAND_ROWS[1]][:K], np.float32)
        ref = PC.ddim_variants_reference(data["x"], data["vu"], data["vc"], coef)
        nulls, order = ("x", "vc", "coef", "out"), ("x", "vu", "vc", "coef", "out", "n") + (("nvar",) if variants else ())
    else:
        data = dict(lat=rng.standard_normal((K, n)).astype(PC.F16), bg=rng.standard_normal(n).astype(PC.F16),
                    objs=rng.standard_normal((2, n)).astype(PC.F16), masks=(rng.integers(0, 256, (2, n)) / 255).astype(PC.F16))
        ref = PC.fusion_variants_reference(data["lat"], data["bg"], data["objs"], data["masks"], 0.3, 1)
        nulls = ("lat", "bg", "objs", "masks", "out")
        order = ("lat", "bg", "objs", "masks", "out", "nobj", "n") + (("nvar",) if variants else ()) + ("mix", "rnf")
    edits = [(f"null {k}", {k: None}) for k in nulls] + [("n 0", dict(n=0))]
    if variants:
        edits += [("nvar 0", dict(nvar=0)), ("nvar 9", dict(nvar=9))]
    if not ddim:
        edits += [("nobj -1", dict(nobj=-1))]
    for what, edit in edits:
        bufs = {k: _guarded(v) for k, v in data.items()}
        out = _out_buffer(K * n)
        before = out[0].cpu().numpy()
        a = {k: b[1] for k, b in bufs.items()}
        a.update(out=out[1], n=n, nvar=K, nobj=2, mix=0.3, rnf=1)
        if ddim:
            dcf = _dev(coef.ravel().copy())
            a.update(coef=dcf.data_ptr())
        good = dict(a)
        a.update(edit)
        assert fn(*[a[k] for k in order], _stream()) == -1, (what, _err())
        assert entry in _err(), _err()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), before), what
        assert all(np.array_equal(b[0].cpu().numpy(), b[2]) for b in bufs.values()), what
        assert fn(*[good[k] for k in order], _stream()) == 0, _err()
        _check_out(out[0], ref, what)
