"""What include/mvoc_hip.h promises about the one-thread-per-output entries of mvoc_amd/csrc/stem.hip and about mvoc_softmax_rows_f16
(norm.hip): the case walk, the poisoned layouts and one reference per entry (helper module, not collected by pytest; torch and numpy
only, nothing here calls the library).  tests/test_stem_contract_cpu.py shows the constructions sound without a GPU,
tests/test_stem_contract_gpu.py launches every case through the C ABI.

A case is (entry, kind, parameters).  ``problem(case)`` turns it into
  * ``ins``   the input operands, each the exact content of its view: the elements the header says are not read (pitch columns past c,
              a table nobody indexes) hold fp16 NaN / INT32_MIN / the census byte, and so does the allocation around the view,
  * ``outs``  per output its element count, which elements the header describes (``dest``), their reference and the rule of comparison,
  * ``args``  the C arguments in order (a string names an operand, None is a NULL pointer),
  * ``emulate(views, mutation)`` an independent torch formulation of the entry that writes into sentinel-filled views, and, with a
              mutation name, a subtly wrong one.
``Placed`` puts the operands into allocations of their own (launch_census.alloc: 64 KB of slack behind, the lead in front) at leads of
0, 16 and 128 bytes mod 256; ``Placed.verify`` holds the described elements to the reference, every other byte of every output
allocation to the sentinel, and every input allocation to its bytes from before.

Rules: ``bits`` (bit for bit; a NaN for a NaN, sign and payload free), ``bound`` (|got - ref| <= bound where ref is finite, the same
class elsewhere), ``alts`` (the census's accepted-neighbour rule: ref or one of two named neighbours), ``l2`` (rel-L2 and max-abs).

Work-item totals.  Each entry is walked at geometries whose work-item total (what one thread handles) is 1, 255, 256, 257 and 513, in
several factorisations with pairwise different extents.  Two things cannot be had: a prime total (257) or 1 has no factorisation
without repeated ones, and mvoc_timestep_embedding_f16 has an even work-item count (nb * dim, dim even), so it is walked at 2, 254,
256, 258, 512 and 514; mvoc_clip_patches_f16 writes at least kpad >= 3 elements (REACHABLE).
"""
import ctypes as C
import itertools
import math
import zlib

import numpy as np
import torch

import launch_census as LC
from launch_census import F32, F64, H16, I32, U8

I16 = torch.int16
I32MIN = -(2 ** 31)
NAN = float("nan")
LEADS = (0, 16, 128)
TOTALS = (1, 255, 256, 257, 513)
REACHABLE = {"timestep_embedding": (2, 254, 256, 258, 512, 514), "clip_patches": (3, 255, 256, 257, 513)}
ACT_SILU, ACT_GELU = 2, 3

ENTRIES = ("timestep_embedding", "act", "add", "conv3x3_small", "adaptive_avgpool", "ncfhw_to_tokens", "tokens_to_ncfhw",
           "temporal_encoder4", "conv1x1_small", "softmax_rows", "gaussian_sample", "scale", "image_to_tokens", "tokens_to_image",
           "mask_resize_u8", "mask_finish", "clip_patches", "clip_embed", "permute_rows")
SYMBOL = {e: "mvoc_" + e + ("" if e in ("mask_resize_u8", "mask_finish") else "_f16") for e in ENTRIES}

# factorisations of the totals: pairwise different extents wherever the total has them
FACT2 = {1: [(1, 1)], 255: [(15, 17), (17, 15), (3, 85)], 256: [(8, 32), (32, 8), (4, 64)], 257: [(1, 257), (257, 1)],
         513: [(27, 19), (19, 27), (171, 3)]}
FACT3 = {1: [(1, 1, 1)], 255: [(1, 15, 17), (15, 17, 1), (5, 1, 51)], 256: [(2, 8, 16), (16, 2, 8), (8, 16, 2)],
         257: [(1, 257, 1), (257, 1, 1), (1, 1, 257)], 513: [(1, 27, 19), (19, 1, 27), (27, 19, 1)]}
FACT4 = {1: [(1, 1, 1, 1)], 255: [(1, 3, 5, 17), (5, 17, 1, 3), (17, 1, 3, 5)], 256: [(1, 2, 8, 16), (16, 8, 2, 1), (2, 1, 16, 8)],
         257: [(1, 1, 257, 1), (257, 1, 1, 1), (1, 1, 1, 257)], 513: [(1, 3, 9, 19), (19, 9, 3, 1), (3, 19, 1, 9)]}

# the special-value atlas of tests/pnp_contract.py (SPECIALS), as bit patterns: +-0, +-1, +-65504, +-inf, NaN, subnormals, the
# neighbours of 2^-14, and three ordinary values
SPECIAL_BITS = (0x0000, 0x8000, 0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x0001, 0x8001, 0x0401, 0x83FF, 0x3555, 0xC248,
                0x2E66)


def f16_bits(b):
    return torch.tensor(np.asarray(b, dtype=np.uint16).view(np.int16)).view(H16)


SPECIALS = f16_bits(SPECIAL_BITS)
_all_bits = np.arange(65536, dtype=np.uint16)
for _b in (0x7C5A, 0x7E5A, 0xFC5A, 0xFE5A):  # a NaN that a kernel may turn into the sentinel's own pattern (quieted, sign flipped) and
    _all_bits[_b] = 0x7E00                   # that would then read as "unwritten"
ALL_F16 = f16_bits(_all_bits)        # every fp16 bit pattern


class Case:
    def __init__(self, entry, kind, **p):
        self.entry, self.kind, self.p = entry, kind, p

    def __repr__(self):
        return f"{self.entry}[{self.kind}] " + " ".join(f"{k}={v}" for k, v in self.p.items())

    @property
    def seed(self):
        return zlib.crc32(repr(self).encode())


class Out:
    """one output operand: ``n`` elements of ``dtype``; ``dest`` (bool [n], None = all) the elements the header describes; ``ref`` and
    ``rule`` over the described elements in order; ``init`` the content before the call of an operand updated in place"""

    def __init__(self, n, dtype, ref, rule=("bits",), dest=None, init=None):
        self.n, self.dtype, self.ref, self.rule, self.dest, self.init = int(n), dtype, ref, rule, dest, init


class Problem:
    def __init__(self, ins, outs, args, emulate, work):
        self.ins, self.outs, self.args, self.emulate, self.work = ins, outs, args, emulate, work


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def compare(got, ref, rule):
    """-> (bool tensor of wrong elements, worst deviation in units of the bound: 0 for the exact rules)"""
    kind = rule[0]
    if kind == "bits":
        if got.dtype == H16:
            r = ref.to(H16)
            ok = torch.where(r.isnan(), got.isnan(), got.view(I16) == r.view(I16))
        else:
            ok = got == ref.to(got.dtype)
        return ~ok, 0.0
    g = got.to(F64)
    if kind == "bound":
        bound = rule[1]
        fin = ref.isfinite()
        dev = (g - ref).abs()
        ok = torch.where(fin, dev <= bound, torch.where(ref.isnan(), g.isnan(), g == ref))
        sel = fin & (bound > 0) & dev.isfinite()
        return ~ok, float((dev[sel] / bound[sel]).max()) if bool(sel.any()) else 0.0
    if kind == "alts":
        lo, hi = rule[1], rule[2]
        ok = (g == ref) | (g == lo) | (g == hi) | (ref.isnan() & g.isnan())
        return ~ok, 0.0
    if kind == "l2":
        rel_bound, abs_bound = rule[1], rule[2]
        rel = float((g - ref).norm() / ref.norm())
        mx = float((g - ref).abs().max())
        bad = torch.zeros_like(g, dtype=torch.bool)
        if not (rel <= rel_bound and mx <= abs_bound):  # (NaN fails)
            bad[:] = True
        return bad, max(rel / rel_bound, mx / abs_bound)
    raise ValueError(kind)


POISON = {H16: NAN, F32: NAN, I32: I32MIN, U8: LC.U8_SENTINEL}


def _bytes(t):
    return t.contiguous().view(U8)


class Placed:
    """the operands of a problem in allocations of their own on `device`; operand i sits LEADS[(lead_index + i) % 3] bytes past a
    256-byte boundary"""

    def __init__(self, prob, lead_index=0, device="cpu"):
        self.prob, self.T, self.before = prob, {}, {}
        i = lead_index
        for name, data in prob.ins.items():
            v = LC.alloc(data.numel(), data.dtype, LEADS[i % 3], device, fill=POISON[data.dtype])
            v.copy_(data)
            self.T[name] = v
            self.before[name] = _bytes(v.base_alloc).clone()
            i += 1
        for name, o in prob.outs.items():
            v = LC.alloc(o.n, o.dtype, LEADS[i % 3], device)
            LC.fill_sentinel(v)
            if o.init is not None:
                v.copy_(o.init)
            self.T[name] = v
            i += 1

    def ptr(self, name):
        return None if name is None else self.T[name].data_ptr()

    def c_args(self):
        return [self.ptr(a) if (a is None or isinstance(a, str)) else a for a in self.prob.args]

    def out_bytes(self):
        return {name: _bytes(self.T[name].base_alloc).clone() for name in self.prob.outs}

    def emulate(self, mutation=None):
        self.prob.emulate({name: self.T[name] for name in self.prob.outs}, mutation)

    def verify(self, what=""):
        """-> worst deviation in units of the bound; raises AssertionError with the first differences"""
        worst = 0.0
        for name, v in self.T.items():
            if name in self.prob.outs:
                continue
            assert torch.equal(_bytes(v.base_alloc), self.before[name]), f"{what}: the input `{name}` (or the bytes around it) changed"
        for name, o in self.prob.outs.items():
            v = self.T[name]
            assert LC.stray_writes(v) == 0, f"{what}: `{name}`: {LC.stray_writes(v)} elements written outside the operand"
            got = v.cpu()
            dest = torch.ones(o.n, dtype=torch.bool) if o.dest is None else o.dest
            if o.init is None:
                sent = got.view(I16) == LC.OUT_SENTINEL if o.dtype == H16 else got == LC.U8_SENTINEL
                sib = int((~sent & ~dest).sum())
                assert sib == 0, f"{what}: `{name}`: {sib} elements the header does not describe were written (sibling channels)"
                if o.dtype == H16:
                    assert int((sent & dest).sum()) == 0, f"{what}: `{name}`: {int((sent & dest).sum())} described elements unwritten"
            bad, ratio = compare(got[dest], o.ref, o.rule)
            if bool(bad.any()):
                w = bad.nonzero().reshape(-1)[:4]
                raise AssertionError(f"{what}: `{name}`: {int(bad.sum())} of {int(dest.sum())} described elements wrong (rule {o.rule[0]}, "
                                     f"ratio {ratio:.3g}), first at {w.tolist()}: got {got[dest][w].tolist()}, want {o.ref[w].tolist()}")
            worst = max(worst, ratio)
        return worst


def fails(placed, what=""):
    try:
        placed.verify(what)
    except AssertionError:
        return True
    return False


# ---- data --------------------------------------------------------------------------------------------------------------------------
def _gen(case):
    return torch.Generator().manual_seed(case.seed)


def _ints(shape, g, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(H16)


def _randn(shape, g, scale=1.0):
    return (torch.randn(tuple(shape), generator=g) * scale).to(H16)


def _distinct(n, g=None):
    """n fp16 values, finite and all different (bit patterns from 0x0400 up, both signs), shuffled"""
    n = int(n)
    assert n <= 2 * 0x7700
    b = np.arange(n, dtype=np.int64)
    bits = (0x0400 + b // 2) | ((b % 2) << 15)
    t = f16_bits(bits.astype(np.uint16))
    return t[torch.randperm(n, generator=g)] if g is not None else t


def _pitched(data2d, ld, fill=NAN):
    """rows of data2d at pitch ld, the columns past its width poisoned -> 1-D"""
    rows, c = data2d.shape
    out = torch.full((rows, ld), fill, dtype=data2d.dtype)
    out[:, :c] = data2d
    return out.reshape(-1)


def _dest_cols(rows, ld, c0, c):
    d = torch.zeros((rows, ld), dtype=torch.bool)
    d[:, c0:c0 + c] = True
    return d.reshape(-1)


def _write(view, dest, values):
    view[dest.to(view.device)] = values.reshape(-1).to(view.device, view.dtype)


def _all(n):
    return torch.ones(int(n), dtype=torch.bool)


# ---- timestep_embedding ------------------------------------------------------------------------------------------------------------
T_VALUES = (0.0, 1.0, 8.0, 16.0, 500.0, 981.0, 999.0, 123.456)


def timestep_embedding64(t, dim):
    """-> (cos | sin of t * 10000^(-k / half) in fp64 [nb, dim], the bound of a float32 evaluation rounded to fp16).

    bound = ulp16(ref) / 2 + |ang| (3 x + 3) 2^-24 + 2^-23 |ref|,  x = ln(10000) k / half, ang = t * exp(-x):
      * ulp16(ref) / 2: the one rounding to fp16 of the exact value;
      * 3 x 2^-24 |ang|: the exponent -ln(10000) * k / half is formed with three fp32 roundings (the constant, the product, the
        quotient), each of relative size 2^-24 at magnitude x; d exp(-x) = exp(-x) dx, so each moves ang by |ang| x 2^-24;
      * 3 2^-24 |ang|: expf is documented at 1 ulp (HIP math API: expf, maximum error 1 ULP), at most 2^-23 = 2 units relative, and
        the product with t rounds once, 1 unit; |d sin|, |d cos| <= |d ang|;
      * 2^-23 |ref|: the device sinf / cosf.  hipcc at -O3 -ffp-contract=on (no fast-math flag, so no v_sin_f32 / v_cos_f32 shortcut)
        calls OCML's sinf / cosf, documented at 1 ULP over the whole range (HIP math API: sinf 1, cosf 1): one fp32 ulp of the result,
        at most 2^-23 |result|.  The issue's `+ 3` leaves nothing for them once expf takes its documented ulp, so this term is added.
    """
    half = dim // 2
    k = torch.arange(half, dtype=F64)
    x = math.log(10000.0) * k / half
    ang = t.to(F64)[:, None] * torch.exp(-x)[None, :]
    ref = torch.cat([torch.cos(ang), torch.sin(ang)], 1)
    fp32 = (ang.abs() * (3 * x[None, :] + 3) * 2.0 ** -24).repeat(1, 2)
    return ref, LC.ulp16(ref) / 2 + fp32 + 2.0 ** -23 * ref.abs(), LC.ulp16(ref) / 2 + fp32


def timestep_embedding_f32(t, dim, mutation=None):
    """the reference's float32 chain (oracle.unet_ref.timestep_embedding restated so that it can be mutated)"""
    half = dim // 2
    div = half - 1 if mutation == "half_minus_1" else half
    exponent = -math.log(10000.0) * torch.arange(half, dtype=F32) / div
    ang = t.to(F32)[:, None] * torch.exp(exponent)[None, :]
    parts = [torch.cos(ang), torch.sin(ang)]
    if mutation == "cos_sin_swapped":
        parts.reverse()
    return torch.cat(parts, -1)


def _p_timestep_embedding(case):
    p = case.p
    nb, dim = p["nb"], p["dim"]
    t = torch.tensor([T_VALUES[(p["t0"] + i) % len(T_VALUES)] + (0.0 if i < len(T_VALUES) else 0.37 * i) for i in range(nb)], dtype=F32)
    ref, bound, _ = timestep_embedding64(t, dim)

    def emulate(views, mutation):
        _write(views["out"], _all(nb * dim), timestep_embedding_f32(t, dim, mutation).to(H16))

    return Problem({"t": t}, {"out": Out(nb * dim, H16, ref.reshape(-1), ("bound", bound.reshape(-1)))}, ["t", nb, dim, "out"], emulate,
                   nb * dim)


def _c_timestep_embedding():
    cs = [Case("timestep_embedding", "entry", nb=1, dim=dim, t0=t0) for dim in (2, 6, 320) for t0 in range(len(T_VALUES))]
    cs += [Case("timestep_embedding", "entry", nb=5, dim=dim, t0=t0) for dim in (2, 6, 320) for t0 in (0, 3)]
    for nb, dim in ((1, 2), (127, 2), (1, 254), (1, 256), (2, 128), (128, 2), (3, 86), (43, 6), (1, 512), (4, 128), (257, 2), (1, 514)):
        cs.append(Case("timestep_embedding", "totals", nb=nb, dim=dim, t0=nb % 5))
    return cs


# ---- elementwise: act, add, scale, gaussian_sample, mask_finish ----------------------------------------------------------------------
# GELU of mvoc_act_f16 is 0.5 x (1 + erff(x / sqrt 2)) in fp32 (common.h: gelu_erf_f).  Against fp64: erff is documented at 4 ulp (HIP
# math API), of a value below 1: 4 * 2^-24 = 2^-22; the argument's rounding moves erf by z erf'(z) 2^-24 < 2^-24; 1 + erf rounds once,
# 2^-24; so |0.5 x (1 + erf)| is off by at most 0.5 |x| (2^-22 + 2^-23), and the last product adds 2^-24 |result| <= 2^-24 |x|:
# together under 2^-22 |x|.  An absolute term, as for the GEMM epilogues' GELU_ABS: where gelu(x) is tiny (x <= -4) it is many ulps of
# the result.  SiLU (v_exp + v_rcp, a few fp32 ulps relative, no cancellation) needs none: its rounding flip is one fp16 ulp.
GELU_ERF_ABS = 2.0 ** -22


def gelu_erf64(x):
    x = x.to(F64)
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def act64(x, act):
    """-> (fp64 value rounded once, bound): ulp16 of the fp64 value (the rounding flip) plus the fp32 evaluation error"""
    x = x.to(F64)
    a = LC.silu64(x) if act == ACT_SILU else gelu_erf64(x)
    extra = GELU_ERF_ABS * x.abs() if act == ACT_GELU else torch.zeros_like(x)
    extra = torch.where(extra.isfinite(), extra, torch.zeros_like(extra))
    return LC.r16(a), LC.ulp16(torch.where(a.isfinite(), a, torch.ones_like(a))) + extra


def _elementwise_data(case, g, scale=3.0):
    n, kind = case.p["n"], case.kind
    if kind == "atlas":
        return ALL_F16.clone()
    return _randn((n,), g, scale)


def _p_act(case):
    g = _gen(case)
    x = _elementwise_data(case, g)
    n, act = x.numel(), case.p["act"]
    ref, bound = act64(x, act)

    def emulate(views, mutation):
        xf = x.to(F32)  # (written out: F.gelu(inf) is NaN on the CPU)
        y = xf / (1.0 + torch.exp(-xf)) if act == ACT_SILU else 0.5 * xf * (1.0 + torch.special.erf(xf * math.sqrt(0.5)))
        _write(views["out"], _all(n), y.to(H16))

    return Problem({"x": x}, {"out": Out(n, H16, ref, ("bound", bound))}, ["x", "out", n, act], emulate, n)


def tie_pairs():
    """pairs of fp16 values whose exact sum lies half way between two fp16 values (round to even decides), and pairs that overflow"""
    a = torch.tensor([2048.0, 2050.0, 1.0, 1.0, 4096.0, -2048.0, -2050.0, 65504.0, 65504.0, 32768.0, 2.0 ** -14, 0.5], dtype=F64)
    b = torch.tensor([1.0, 1.0, 2.0 ** -11, 3 * 2.0 ** -11, 2.0, -1.0, -1.0, 16.0, 15.0, 32768.0, 2.0 ** -24, 2.0 ** -12], dtype=F64)
    return a.to(H16), b.to(H16)


def _p_add(case):
    g = _gen(case)
    if case.kind == "atlas":
        a = SPECIALS.repeat_interleave(16)
        b = SPECIALS.repeat(16)
        ta, tb = tie_pairs()
        a, b = torch.cat([a, ta, tb]), torch.cat([b, tb, ta])
    else:
        a, b = _randn((case.p["n"],), g, 3.0), _randn((case.p["n"],), g, 3.0)
    n = a.numel()
    ref = (a.to(F64) + b.to(F64)).to(H16)  # the exact sum, rounded once

    def emulate(views, mutation):
        _write(views["out"], _all(n), (a.to(F32) + b.to(F32)).to(H16))

    return Problem({"a": a, "b": b}, {"out": Out(n, H16, ref)}, ["a", "b", "out", n], emulate, n)


SCALES = (0.18215, 1 / 0.18215, -1.5)  # latents * scaling_factor, 1 / scaling_factor * latents (pipeline_i2vgen_xl.py), one negative


def _p_scale(case):
    g = _gen(case)
    x = _elementwise_data(case, g, 4.0)
    n, s = x.numel(), case.p["scale"]
    ref = LC.scale64(x, s)

    def emulate(views, mutation):
        _write(views["out"], _all(n), (x.to(F32) * torch.tensor(s, dtype=F32)).to(H16))

    return Problem({"x": x}, {"out": Out(n, H16, ref)}, ["x", "out", n, float(s)], emulate, n)


LOGVAR_EDGES = (-40.0, -30.02, -30.0, -29.98, 0.0, 19.98, 20.0, 20.02, 30.0)  # at and past both clamps


def _p_gaussian_sample(case):
    g = _gen(case)
    if case.kind == "atlas":
        lv = torch.cat([SPECIALS, torch.tensor(LOGVAR_EDGES).to(H16)])
        m, l, z = torch.meshgrid(SPECIALS, lv, SPECIALS, indexing="ij")
        mean, logvar, noise = m.reshape(-1).clone(), l.reshape(-1).clone(), z.reshape(-1).clone()
    else:
        n = case.p["n"]
        mean, logvar, noise = _randn((n,), g), _randn((n,), g, 4.0), _randn((n,), g)
        e = torch.tensor(LOGVAR_EDGES).to(H16)[:n]
        logvar[:e.numel()] = e
    n = mean.numel()
    ref, (lo, hi) = LC.gaussian_sample64(mean, logvar, noise)

    def emulate(views, mutation):
        r = lambda v: v.to(H16).to(F32)
        sd = r(torch.exp(r(0.5 * logvar.to(F32).clamp(-30.0, 20.0))))
        _write(views["out"], _all(n), (mean.to(F32) + r(sd * noise.to(F32))).to(H16))

    return Problem({"mean": mean, "logvar": logvar, "noise": noise}, {"out": Out(n, H16, ref, ("alts", lo, hi))},
                   ["mean", "logvar", "noise", "out", n], emulate, n)


def _p_mask_finish(case):
    g = _gen(case)
    n = case.p["n"]
    v = torch.randint(0, 256, (n,), generator=g).to(U8)
    if case.kind == "atlas":
        v = torch.arange(256).to(U8)[torch.randperm(256, generator=g)]  # every byte value
    fl = (v.to(F64) / 255.0).to(F32).to(H16)
    bl = (v > 10).to(U8)

    def emulate(views, mutation):
        _write(views["float_mask"], _all(n), (v.to(F32) / 255.0).to(H16))
        _write(views["bool_mask"], _all(n), (v >= 10 if mutation == "threshold_ge_10" else v > 10).to(U8))

    return Problem({"v": v}, {"float_mask": Out(n, H16, fl), "bool_mask": Out(n, U8, bl)}, ["v", "float_mask", "bool_mask", n], emulate, n)


def _c_elementwise(entry, variants):
    cs = []
    for kw in variants:
        cs += [Case(entry, "totals", n=n, **kw) for n in TOTALS]
        cs.append(Case(entry, "atlas", n={"mask_finish": 256}.get(entry, 0), **kw))
    return cs


# ---- conv3x3_small ------------------------------------------------------------------------------------------------------------------
def _p_conv3x3_small(case):
    p, g = case.p, _gen(case)
    nimg, h, w, cin, cout, stride, silu = (p[k] for k in ("nimg", "h", "w", "cin", "cout", "stride", "silu"))
    x = _ints((nimg, h, w, cin), g, -2, 2)
    W = _ints((cout, cin, 3, 3), g, -2, 2)
    bias = _ints((cout,), g, -4, 4) if p["bias"] else None
    v, bound = LC.conv3x3_small64(x, W, bias, stride, silu)
    n = v.numel()
    ins = {"x": x.reshape(-1), "w": W.permute(0, 2, 3, 1).reshape(-1)}  # [cout][3][3][cin]
    if bias is not None:
        ins["bias"] = bias

    def emulate(views, mutation):
        Wm = W.transpose(2, 3) if mutation == "ky_kx_swapped" else W
        xi = x.permute(0, 3, 1, 2).to(F32)
        b = None if bias is None else bias.to(F32)
        if mutation == "stride2_origin_shifted" and stride == 2:
            y = torch.nn.functional.conv2d(torch.nn.functional.pad(xi, (0, 2, 0, 2)), Wm.to(F32), b, stride=2)[:, :, :v.shape[1], :v.shape[2]]
        else:
            y = torch.nn.functional.conv2d(xi, Wm.to(F32), b, stride=stride, padding=1)
        y = (y + 0.0).to(H16).to(F32)  # (+ 0.0: the kernel's sum starts at +0, so it never holds -0)
        if silu:
            y = torch.nn.functional.silu(y)
        _write(views["out"], _all(n), y.permute(0, 2, 3, 1).to(H16))

    rule = ("bound", bound.reshape(-1)) if silu else ("bits",)
    return Problem(ins, {"out": Out(n, H16, v.reshape(-1), rule)},
                   ["x", "w", "bias" if bias is not None else None, "out", nimg, h, w, cin, cout, stride, int(silu)], emulate, n)


def _c_conv3x3_small():
    cs = []
    for (h, w), stride, cin, cout, bias, silu in itertools.product(((1, 1), (1, 5), (2, 3), (5, 4), (7, 9)), (1, 2), (3, 4, 8), (1, 5, 32),
                                                                  (True, False), (False, True)):
        cs.append(Case("conv3x3_small", "entry", nimg=2, h=h, w=w, cin=cin, cout=cout, stride=stride, bias=bias, silu=silu))
    for total in TOTALS:
        for i, (nimg, h, w, cout) in enumerate(FACT4[total]):
            cs.append(Case("conv3x3_small", "totals", nimg=nimg, h=h, w=w, cin=(3, 4, 8)[i], cout=cout, stride=1, bias=i != 1, silu=i == 2))
        # stride 2: the output extents (h + 1) / 2, (w + 1) / 2 carry the total, the input edge is odd
        nimg, ho, wo, cout = FACT4[total][0]
        cs.append(Case("conv3x3_small", "totals", nimg=nimg, h=2 * ho - 1, w=2 * wo - 1, cin=4, cout=cout, stride=2, bias=True, silu=False))
    return cs


# ---- adaptive_avgpool ---------------------------------------------------------------------------------------------------------------
def avgpool_windows(n_in, n_out, floored_end=False):
    s = [(o * n_in) // n_out for o in range(n_out)]
    e = [((o + 1) * n_in) // n_out if floored_end else -(-((o + 1) * n_in) // n_out) for o in range(n_out)]
    return s, e


def adaptive_avgpool_ref(x, oh, ow, floored_end=False):
    """x [n, h, w, c] of integers -> [n, oh, ow, c]: the exact window sum, divided in float32 by the float32 count, rounded once"""
    n, h, w, c = x.shape
    ys, ye = avgpool_windows(h, oh, floored_end)
    xs, xe = avgpool_windows(w, ow, floored_end)
    out = torch.empty((n, oh, ow, c), dtype=H16)
    xi = x.to(torch.int64)
    for oy in range(oh):
        for ox in range(ow):
            s = xi[:, ys[oy]:ye[oy], xs[ox]:xe[ox]].sum((1, 2))
            cnt = max((ye[oy] - ys[oy]) * (xe[ox] - xs[ox]), 0)
            out[:, oy, ox] = (s.to(F32) / torch.tensor(float(cnt), dtype=F32)).to(H16) if cnt else torch.zeros((n, c), dtype=H16)
    return out


def _p_adaptive_avgpool(case):
    p, g = case.p, _gen(case)
    nimg, h, w, c, oh, ow = (p[k] for k in ("nimg", "h", "w", "c", "oh", "ow"))
    x = _ints((nimg, h, w, c), g, -9, 9)
    ref = adaptive_avgpool_ref(x, oh, ow)
    n = ref.numel()

    def emulate(views, mutation):
        if mutation == "window_end_floored":
            y = adaptive_avgpool_ref(x, oh, ow, floored_end=True)
        else:
            y = torch.nn.functional.adaptive_avg_pool2d(x.permute(0, 3, 1, 2).to(F32), (oh, ow)).permute(0, 2, 3, 1).to(H16)
        _write(views["out"], _all(n), y)

    return Problem({"x": x.reshape(-1)}, {"out": Out(n, H16, ref.reshape(-1))}, ["x", "out", nimg, h, w, c, oh, ow], emulate, n)


POOL_GEOMETRIES = (((4, 4), (4, 4)), ((5, 7), (5, 7)), ((8, 6), (4, 2)), ((6, 9), (2, 3)), ((7, 9), (4, 5)), ((3, 2), (5, 4)), ((1, 1), (1, 1)),
                   ((5, 3), (1, 1)), ((1, 1), (3, 2)))


def _c_adaptive_avgpool():
    cs = [Case("adaptive_avgpool", "entry", nimg=nimg, h=h, w=w, c=c, oh=oh, ow=ow)
          for ((h, w), (oh, ow)), (nimg, c) in itertools.product(POOL_GEOMETRIES, ((1, 3), (2, 1), (3, 8)))]
    for total in TOTALS:
        for i, (nimg, oh, ow, c) in enumerate(FACT4[total]):
            h, w = ((oh + 3, ow + 2), (2 * oh, 3 * ow), (max(oh - 1, 1), ow + 1))[i]  # ragged, divisible, upsampling rows
            cs.append(Case("adaptive_avgpool", "totals", nimg=nimg, h=h, w=w, c=c, oh=oh, ow=ow))
    return cs


# ---- layout entries -----------------------------------------------------------------------------------------------------------------
def ncfhw_to_tokens_ref(x, b, c, f, hw):
    """x [b, c, f, hw] -> rows (b, f, hw) of c channels, by index arithmetic"""
    r = torch.arange(b * f * hw)
    bi, fi, p = r // (f * hw), (r // hw) % f, r % hw
    ch = torch.arange(c)
    return x.reshape(-1)[((bi[:, None] * c + ch[None, :]) * f + fi[:, None]) * hw + p[:, None]]


def _p_ncfhw_to_tokens(case):
    p, g = case.p, _gen(case)
    b, c, f, hw, ldo, coff = (p[k] for k in ("b", "c", "f", "hw", "ldo", "coff"))
    x = _distinct(b * c * f * hw, g)
    rows = b * f * hw
    ref = ncfhw_to_tokens_ref(x, b, c, f, hw)
    dest = _dest_cols(rows, ldo, coff, c)

    def emulate(views, mutation):
        xv = x.reshape(b, c, f, hw)
        y = xv.permute(0, 2, 3, 1)
        if mutation == "c_f_swapped":
            y = x.reshape(b, f, c, hw).permute(0, 1, 3, 2)
        d = _dest_cols(rows, ldo, 0, c) if mutation == "coff_ignored" else dest
        _write(views["out"], d, y.reshape(rows, c))
        if mutation == "sibling_written":
            col = coff + c if coff + c < ldo else coff - 1
            if 0 <= col < ldo:
                _write(views["out"], _dest_cols(rows, ldo, col, 1), torch.zeros(rows, dtype=H16))

    return Problem({"x": x}, {"out": Out(rows * ldo, H16, ref.reshape(-1), dest=dest)}, ["x", "out", b, c, f, hw, ldo, coff], emulate, rows)


def _c_ncfhw_to_tokens():
    cs = []
    for c in (4, 3):
        for ldo, coff in ((c, 0), (8, 0), (8, 4), (11, 5)):
            cs += [Case("ncfhw_to_tokens", "pitch", b=2, c=c, f=5, hw=7, ldo=ldo, coff=coff)]
            for total in TOTALS:
                i = (ldo + coff + c + total) % 3
                b, f, hw = FACT3[total][i % len(FACT3[total])]
                cs.append(Case("ncfhw_to_tokens", "totals", b=b, c=c, f=f, hw=hw, ldo=ldo, coff=coff))
    cs += [Case("ncfhw_to_tokens", "totals", b=b, c=4, f=f, hw=hw, ldo=8, coff=0) for total in TOTALS for b, f, hw in FACT3[total]]
    return cs


def _p_tokens_to_ncfhw(case):
    p, g = case.p, _gen(case)
    b, c, f, hw, ld = (p[k] for k in ("b", "c", "f", "hw", "ld"))
    rows = b * f * hw
    data = _distinct(rows * c, g).reshape(rows, c)
    i = torch.arange(b * c * f * hw)
    pp, fi, ch, bi = i % hw, (i // hw) % f, (i // (hw * f)) % c, i // (hw * f * c)
    ref = data[(bi * f + fi) * hw + pp, ch]
    n = ref.numel()

    def emulate(views, mutation):
        y = data.reshape(b, f, hw, c).permute(0, 3, 1, 2)
        if mutation == "c_f_swapped":
            y = data.reshape(b, f, hw, c).permute(0, 1, 3, 2)
        _write(views["out"], _all(n), y)

    return Problem({"x": _pitched(data, ld)}, {"out": Out(n, H16, ref)}, ["x", "out", b, c, f, hw, ld], emulate, n)


def _c_tokens_to_ncfhw():
    cs = []
    for total in TOTALS:
        for i, (b, c, f, hw) in enumerate(FACT4[total]):
            for ld in (c, c + 3):
                cs.append(Case("tokens_to_ncfhw", "totals", b=b, c=c, f=f, hw=hw, ld=ld))
    cs += [Case("tokens_to_ncfhw", "pitch", b=2, c=4, f=5, hw=7, ld=ld) for ld in (4, 7, 8)]
    return cs


def _p_image_to_tokens(case):
    p, g = case.p, _gen(case)
    n, c, hw = p["n"], p["c"], p["hw"]
    x = _distinct(n * c * hw, g)
    i = torch.arange(n * hw * c)
    ref = x[((i // (c * hw)) * c + i % c) * hw + (i // c) % hw]

    def emulate(views, mutation):
        _write(views["out"], _all(n * c * hw), x.reshape(n, c, hw).permute(0, 2, 1))

    return Problem({"x": x}, {"out": Out(n * c * hw, H16, ref)}, ["x", "out", n, c, hw], emulate, n * c * hw)


def _p_tokens_to_image(case):
    p, g = case.p, _gen(case)
    n, c, hw, ld = p["n"], p["c"], p["hw"], p["ld"]
    data = _distinct(n * hw * c, g).reshape(n * hw, c)
    i = torch.arange(n * c * hw)
    ref = data[(i // (c * hw)) * hw + i % hw, (i // hw) % c]

    def emulate(views, mutation):
        _write(views["out"], _all(n * c * hw), data.reshape(n, hw, c).permute(0, 2, 1))

    return Problem({"x": _pitched(data, ld)}, {"out": Out(n * c * hw, H16, ref)}, ["x", "out", n, c, hw, ld], emulate, n * c * hw)


def _c_image_tokens(entry):
    cs = []
    for total in TOTALS:
        for n, c, hw in FACT3[total]:
            for ld in ((c, c + 3) if entry == "tokens_to_image" else (None,)):
                cs.append(Case(entry, "totals", n=n, c=c, hw=hw, **({"ld": ld} if ld else {})))
    return cs


def _p_permute_rows(case):
    p, g = case.p, _gen(case)
    shape4, perm, c = p["shape4"], p["perm"], p["c"]
    rows = int(np.prod(shape4))
    x = _distinct(rows * c, g).reshape(rows, c)
    st = [shape4[1] * shape4[2] * shape4[3], shape4[2] * shape4[3], shape4[3], 1]
    dims, strides = [shape4[q] for q in perm], [st[q] for q in perm]
    idx = torch.arange(rows)
    src = torch.zeros(rows, dtype=torch.int64)
    div = rows
    for k in range(4):  # out row (i0, i1, i2, i3) over dims <- source row sum_k i_k * strides[k]
        div //= dims[k]
        src += ((idx // div) % dims[k]) * strides[k]
    ref = x[src]

    def emulate(views, mutation):
        _write(views["out"], _all(rows * c), x.reshape(*shape4, c).permute(*perm, 4))

    return Problem({"x": x.reshape(-1)}, {"out": Out(rows * c, H16, ref.reshape(-1))},
                   ["x", "out", (C.c_int64 * 4)(*dims), (C.c_int64 * 4)(*strides), c], emulate, rows * c // 8)


def _c_permute_rows():
    perms = list(itertools.permutations(range(4)))
    cs = [Case("permute_rows", "orders", shape4=(2, 3, 4, 5), perm=pm, c=8) for pm in perms]
    cs += [Case("permute_rows", "orders", shape4=(2, 3, 4, 5), perm=pm, c=24) for pm in ((3, 1, 0, 2), (1, 0, 3, 2))]
    cs += [Case("permute_rows", "orders", shape4=(3, 1, 4, 2), perm=pm, c=8) for pm in ((1, 3, 0, 2), (2, 0, 3, 1), (3, 2, 1, 0))]
    for total in TOTALS:
        for i, shape4 in enumerate(FACT4[total]):
            cs.append(Case("permute_rows", "totals", shape4=shape4, perm=perms[(7 * i + total) % 24], c=8))
        a, b_, c8 = FACT3[total][0]
        cs.append(Case("permute_rows", "totals", shape4=(a, 1, b_, 1) if c8 > 1 else (1, a, 1, b_), perm=(2, 3, 0, 1), c=8 * c8))
    return cs


# ---- conv1x1_small ------------------------------------------------------------------------------------------------------------------
def _p_conv1x1_small(case):
    p, g = case.p, _gen(case)
    rows, cin, cout = p["rows"], p["cin"], p["cout"]
    x, w = _ints((rows, cin), g, -3, 3), _ints((cout, cin), g, -3, 3)
    bias = _ints((cout,), g, -8, 8) if p["bias"] else None
    ref = LC.r16(x.to(F64) @ w.to(F64).t() + (bias.to(F64) if bias is not None else 0)).reshape(-1)
    ins = {"x": x.reshape(-1), "w": w.reshape(-1)}
    if bias is not None:
        ins["bias"] = bias

    def emulate(views, mutation):
        _write(views["out"], _all(rows * cout), (torch.nn.functional.linear(x.to(F32), w.to(F32), None if bias is None else bias.to(F32)) + 0.0).to(H16))  # (+ 0.0: the kernel's sum starts at +0, so it never holds -0)

    return Problem(ins, {"out": Out(rows * cout, H16, ref)}, ["x", "w", "bias" if bias is not None else None, "out", rows, cin, cout], emulate,
                   rows * cout)


def _c_conv1x1_small():
    cs = []
    for total in TOTALS:
        for i, (rows, cout) in enumerate(FACT2[total]):
            if cout > 64:  # (refused above 64)
                rows, cout = cout, rows
            cs.append(Case("conv1x1_small", "totals", rows=rows, cin=(3, 8, 64)[i], cout=cout, bias=i != 1))
    cs += [Case("conv1x1_small", "entry", rows=9, cin=cin, cout=cout, bias=b) for cin, cout, b in ((8, 8, True), (4, 4, True), (1, 64, False), (64, 1, True))]
    return cs


# ---- softmax_rows -------------------------------------------------------------------------------------------------------------------
def _p_softmax_rows(case):
    p, g = case.p, _gen(case)
    rows, cols = p["rows"], p["cols"]
    x = _randn((rows, cols), g, 3.0)
    for r in range(rows):
        kind = (r + p["shift"]) % 4
        if kind == 0:
            x[r] = x[r, 0]                                   # a constant row
        elif kind == 1:
            x[r, (5 * r + 3) % cols] = float(x[r].max()) + 41.0  # one score 40 above the rest (and more)
        elif kind == 2:
            x[r, (3 * r + 1) % cols] = -65504.0              # the most negative finite score beside ordinary ones
    v, (lo, hi) = LC.softmax64(x)

    def emulate(views, mutation):
        _write(views["x"], _all(rows * cols), torch.softmax(x.to(F32), -1).to(H16))

    return Problem({}, {"x": Out(rows * cols, H16, v.reshape(-1), ("alts", lo.reshape(-1), hi.reshape(-1)), init=x.reshape(-1))},
                   ["x", rows, cols], emulate, rows)


def _c_softmax_rows():
    cs = [Case("softmax_rows", "entry", rows=rows, cols=cols, shift=i) for i, (rows, cols) in
          enumerate(itertools.product((1, 3, 4, 5, 9), (8, 504, 512, 520, 1032)))]
    cs += [Case("softmax_rows", "totals", rows=rows, cols=cols, shift=rows % 3) for rows in TOTALS for cols in (8, 24)]
    return cs


# ---- CLIP ---------------------------------------------------------------------------------------------------------------------------
def _p_clip_patches(case):
    p, g = case.p, _gen(case)
    nimg, size, patch, kpad = p["nimg"], p["size"], p["patch"], p["kpad"]
    gr = size // patch
    x = _distinct(nimg * 3 * size * size, g).reshape(nimg, 3, size, size)
    ref = LC.clip_patches_ref(x, patch, kpad).reshape(-1)
    n = ref.numel()

    def emulate(views, mutation):
        # Conv2d(3, N, patch, stride=patch) as a matrix product: unfold's columns are Conv2d's weight.view(N, -1) order
        src = x.transpose(2, 3) if mutation == "py_px_swapped" else x
        cols = torch.nn.functional.unfold(src.to(F32), patch, stride=patch).transpose(1, 2).reshape(nimg * gr * gr, 3 * patch * patch)
        if mutation == "py_px_swapped":  # (the grid stays, the order inside a patch flips)
            cols = x.reshape(nimg, 3, gr, patch, gr, patch).permute(0, 2, 4, 1, 5, 3).reshape(nimg * gr * gr, -1).to(F32)
        _write(views["out"], _all(n), torch.nn.functional.pad(cols, (0, kpad - cols.shape[1])).to(H16))

    return Problem({"pixels": x.reshape(-1)}, {"out": Out(n, H16, ref)}, ["pixels", "out", nimg, size, patch, kpad], emulate, n)


def _c_clip_patches():
    cs = []
    for size, patch in ((4, 2), (6, 3), (28, 14)):
        k = 3 * patch * patch
        cs += [Case("clip_patches", "entry", nimg=nimg, size=size, patch=patch, kpad=kpad) for nimg, kpad in ((1, k), (2, k + 5), (3, (k + 63) // 64 * 64))]
    for nimg, size, patch, kpad in ((1, 1, 1, 3), (1, 1, 1, 255), (17, 2, 2, 15), (5, 1, 1, 51), (2, 2, 1, 32), (4, 4, 1, 4), (1, 4, 2, 64),
                                    (1, 1, 1, 257), (1, 2, 2, 257), (19, 3, 1, 3), (1, 3, 1, 57), (27, 1, 1, 19)):
        cs.append(Case("clip_patches", "totals", nimg=nimg, size=size, patch=patch, kpad=kpad))
    return cs


VOCAB = 13


def _p_clip_embed(case):
    p, g = case.p, _gen(case)
    form, nb, t, c = p["form"], p["nb"], p["t"], p["c"]
    rows = nb * t
    pos = _randn((t, c), g)
    ins = {}
    if form == "text":
        table = _randn((VOCAB, c), g)
        ids = torch.randint(0, VOCAB, (rows,), generator=g).to(I32)
        ids[0] = 0
        ids[-1] = VOCAB - 1            # the last row of the table
        if rows > 3:
            ids[1] = ids[2] = 7        # a repeat
        cls = None
        ins.update(table=table.reshape(-1), ids=ids)
    else:
        ids, cls = None, _randn((c,), g)
        table = _randn((nb * (t - 1), c), g) if t > 1 else torch.full((8, c), NAN, dtype=H16)  # t == 1: never read
        ins.update(table=table.reshape(-1), cls=cls)
    ins["pos"] = pos.reshape(-1)
    ref = LC.clip_embed_ref(table if (form == "text" or t > 1) else table[:0], ids, cls, pos, rows, t).reshape(-1)

    def emulate(views, mutation):
        # transformers: inputs_embeds + position_embedding(position_ids), position_ids = arange(t) for every sequence; the vision
        # tower concatenates the class embedding in front of the patch embeddings first
        if form == "text":
            emb = torch.nn.functional.embedding(ids.long(), table.to(F32)).reshape(nb, t, c)
        else:
            parts = [cls.to(F32).expand(nb, 1, c), (table if t > 1 else table[:0]).to(F32).reshape(nb, t - 1, c)]
            if mutation == "class_row_last":
                parts.reverse()
            emb = torch.cat(parts, 1)
        pe = pos.to(F32)[None].expand(nb, t, c)
        if mutation == "pos_row_div_t":
            pe = pos.to(F32)[(torch.arange(rows) // t) % t].reshape(nb, t, c)
        _write(views["out"], _all(rows * c), (emb + pe).to(H16))

    args = ["table", "ids" if ids is not None else None, "cls" if cls is not None else None, "pos", "out", rows, t, c]
    return Problem(ins, {"out": Out(rows * c, H16, ref)}, args, emulate, rows * c // 8)


def _c_clip_embed():
    cs = [Case("clip_embed", "entry", form=form, nb=nb, t=t, c=c) for form in ("text", "vision") for t in (1, 2, 5) for c in (8, 24)
          for nb in (1, 3)]
    for form in ("text", "vision"):
        for nb, t, c8 in ((1, 1, 1), (3, 5, 17), (17, 5, 3), (1, 17, 15), (4, 8, 8), (8, 1, 32), (2, 4, 32), (257, 1, 1), (1, 257, 1), (9, 3, 19),
                          (1, 19, 27), (19, 1, 27)):
            cs.append(Case("clip_embed", "totals", form=form, nb=nb, t=t, c=8 * c8))
    return cs


# ---- mask_resize_u8 -----------------------------------------------------------------------------------------------------------------
def resize8_pass(a, bounds, kk):
    """one pass of PIL's 8-bit resize along the last axis from its tables: [..., n_in] uint8 -> [..., n_out]"""
    a = a.to(torch.int64)
    out = torch.empty(a.shape[:-1] + (bounds.shape[0],), dtype=torch.int64)
    for xx in range(bounds.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (a[..., x0:x0 + n] * torch.from_numpy(kk[xx, :n].astype(np.int64))).sum(-1) + (1 << 21)
        out[..., xx] = (acc >> 22).clamp(0, 255)
    return out.to(U8)


def mask_frames(n, H, W, g):
    """random frames, then all 0, all 255 and a checkerboard of 0 and 255 (the bicubic lobes overshoot: the clip to 0 and 255)"""
    fr = torch.randint(0, 256, (n, H, W), generator=g).to(U8)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    special = [torch.zeros(H, W), torch.full((H, W), 255.0), ((yy // 2 + xx // 2) % 2) * 255.0, ((yy + xx) % 2) * 255.0]
    for i, s in enumerate(special):
        if 1 + i < n:
            fr[1 + i] = s.to(U8)
    return fr


def _p_mask_resize_u8(case):
    from mvoc_amd.utils import pil_bicubic_tables
    p, g = case.p, _gen(case)
    n, H, W, h, w = (p[k] for k in ("n", "H", "W", "h", "w"))
    fr = mask_frames(n, H, W, g)
    if n == 1 and case.kind == "totals":
        fr = mask_frames(4, H, W, g)[p.get("frame", 3):][:1]
    bh, kh = pil_bicubic_tables(W, w)
    bv, kv = pil_bicubic_tables(H, h)
    tmp = LC.pil_resize_u8(fr, w, H).reshape(-1)
    out = LC.pil_resize_u8(fr, w, h).reshape(-1)
    ins = {"in": fr.reshape(-1), "bounds_h": torch.from_numpy(bh).reshape(-1), "kk_h": torch.from_numpy(kh).reshape(-1),
           "bounds_v": torch.from_numpy(bv).reshape(-1), "kk_v": torch.from_numpy(kv).reshape(-1)}

    def emulate(views, mutation):
        t = resize8_pass(fr, bh, kh)                                         # [n, H, w]
        o = resize8_pass(t.transpose(1, 2), bv, kv).transpose(1, 2)          # [n, h, w]
        _write(views["tmp"], _all(n * H * w), t)
        _write(views["out"], _all(n * h * w), o)

    return Problem(ins, {"tmp": Out(n * H * w, U8, tmp), "out": Out(n * h * w, U8, out)},
                   ["in", "tmp", "out", n, H, W, h, w, "bounds_h", "kk_h", kh.shape[1], "bounds_v", "kk_v", kv.shape[1]], emulate, n * h * w)


def _c_mask_resize_u8():
    cs = [Case("mask_resize_u8", "entry", n=5, H=H, W=W, h=h, w=w) for (H, W), (h, w) in (((8, 8), (1, 1)), ((16, 24), (2, 3)), ((17, 23), (2, 2)),
                                                                                         ((40, 72), (5, 9)))]
    for n, (H, W), (h, w) in ((1, (8, 8), (1, 1)), (255, (8, 8), (1, 1)), (17, (12, 20), (3, 5)), (5, (51, 9), (17, 3)), (256, (9, 7), (1, 1)),
                              (32, (8, 16), (2, 4)), (8, (16, 24), (4, 8)), (257, (8, 8), (1, 1)), (1, (7, 514), (1, 257)), (513, (8, 9), (1, 1)),
                              (19, (12, 27), (3, 9)), (3, (27, 57), (9, 19))):
        cs.append(Case("mask_resize_u8", "totals", n=n, H=H, W=W, h=h, w=w))
    return cs


# ---- temporal_encoder4 --------------------------------------------------------------------------------------------------------------
ENC_KEYS = ("norm1.weight", "norm1.bias", "attn1.to_q.weight", "attn1.to_k.weight", "attn1.to_v.weight", "attn1.to_out.0.weight",
            "attn1.to_out.0.bias", "ff.net.0.proj.weight", "ff.net.0.proj.bias", "ff.net.2.weight", "ff.net.2.bias")  # the blob's order
ENC_SHAPES = ((4,), (4,), (8, 4), (8, 4), (8, 4), (4, 8), (4,), (16, 4), (16,), (4, 16), (4,))


def enc_weights(g, dominant=False):
    """fp16-valued weights of I2VGenXLTransformerTemporalEncoder(4, 2, 4, 16) by state_dict key.  ``dominant``: beta = 1/2, every row
    of to_q is 2 * ones (q = 2 * sum(y) = 4 in every dimension, whatever the frame), every row of to_k reads channel 0 alone (k = 2 y0):
    score(i, j) = 0.5 * 4 * 4 * 2 y0_j = 16 y0_j in both heads, so the one frame whose channel 0 is the row's outlier
    (y0 = 1.73 + 0.5 against -0.58 + 0.5) leads by more than 30"""
    W = {}
    for k, shp in zip(ENC_KEYS, ENC_SHAPES):
        if k == "norm1.weight":
            t = 1 + 0.2 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            t = 0.2 * torch.randn(shp, generator=g)
        else:
            t = torch.randn(shp, generator=g) * (0.7 / math.sqrt(shp[1])) * (1.6 if "to_q" in k or "to_k" in k else 1.0)
        W[k] = t.to(H16)
    if dominant:
        W["norm1.weight"] = torch.ones(4, dtype=H16)
        W["norm1.bias"] = torch.full((4,), 0.5, dtype=H16)
        W["attn1.to_q.weight"] = torch.full((8, 4), 2.0, dtype=H16)
        wk = torch.zeros(8, 4)
        wk[:, 0] = 2.0
        W["attn1.to_k.weight"] = wk.to(H16)
    return W


def enc_blob(W):
    return torch.cat([W[k].reshape(-1) for k in ENC_KEYS])


def enc_module(W, dtype):
    from oracle import unet_ref as U
    enc = U.I2VGenXLTransformerTemporalEncoder(4, 2, 4, 16)
    enc.load_state_dict({k: v.to(F32) for k, v in W.items()})
    return enc.to(dtype).eval()


def enc_scores64(x, W):
    """the attention scores of sequences x [s, f, 4] in fp64: [s, 2 heads, f queries, f keys]"""
    y = LC.layernorm64(x, W["norm1.weight"], W["norm1.bias"], 1e-5)
    q = (y @ W["attn1.to_q.weight"].to(F64).t()).reshape(*y.shape[:2], 2, 4)
    k = (y @ W["attn1.to_k.weight"].to(F64).t()).reshape(*y.shape[:2], 2, 4)
    return torch.einsum("sihd,sjhd->shij", q, k) * 0.5


def enc_reference(x, W):
    """x [b, f, hw, 4] fp16 -> (the oracle module in fp64 [b, f, hw, 4], rel-L2 and max-abs of the same module run in the reference's own
    precision on the CPU -- half weights, half activations, op by op -- against it: the yardstick)"""
    b, f, hw, _ = x.shape
    seq = x.permute(0, 2, 1, 3).reshape(b * hw, f, 4)
    with torch.no_grad():
        ref = enc_module(W, F64)(seq.to(F64))
        eager = enc_module(W, H16)(seq).to(F64)
    back = lambda t: t.reshape(b, hw, f, 4).permute(0, 2, 1, 3).contiguous()
    rel = float((eager - ref).norm() / ref.norm())
    mx = float((eager - ref).abs().max())
    return back(ref), rel, mx


def enc_emulate(x, W, mutation=None):
    """the encoder in float32, written out (x [b, f, hw, 4] -> the same shape), with the mutations of the CPU file"""
    x = x.to(F32)
    w = {k: v.to(F32) for k, v in W.items()}
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + 1e-5) * w["norm1.weight"] + w["norm1.bias"]
    split = lambda t: t.reshape(*t.shape[:-1], 2, 4)
    q, k, v = (split(y @ w[f"attn1.to_{n}.weight"].t()) for n in "qkv")
    scale = 1.0 if mutation == "score_scale_dropped" else 0.5
    if mutation == "softmax_over_pixels":
        s = torch.einsum("bfphd,bfrhd->bfhpr", q, k) * scale
        att = torch.einsum("bfhpr,bfrhd->bfphd", torch.softmax(s, -1), v)
    else:
        s = torch.einsum("bfphd,bgphd->bphfg", q, k) * scale
        att = torch.einsum("bphfg,bgphd->bfphd", torch.softmax(s, -1), v)
    if mutation == "heads_swapped":
        att = att.flip(-2)
    a = att.reshape(*x.shape[:-1], 8) @ w["attn1.to_out.0.weight"].t() + w["attn1.to_out.0.bias"]
    h1 = a if mutation == "residual_dropped" else a + x
    ff = torch.nn.functional.gelu(h1 @ w["ff.net.0.proj.weight"].t() + w["ff.net.0.proj.bias"]) @ w["ff.net.2.weight"].t() + w["ff.net.2.bias"]
    return ff + h1


def enc_data(case):
    """(x [b, f, hw, 4] fp16, weights): every pixel different data"""
    p, g = case.p, _gen(case)
    b, f, hw = p["b"], p["f"], p["hw"]
    W = enc_weights(torch.Generator().manual_seed(p.get("wseed", 5)), dominant=case.kind == "dominant")
    x = _randn((b, f, hw, 4), g, 1.5)
    if case.kind == "dominant":
        # every row an outlier pattern: the outlier sits in channel 0 in frame (pixel % f) only, in channels 1..3 elsewhere
        base = 0.25 * torch.randn((b, f, hw, 4), generator=g)
        lead = (torch.arange(hw)[None, None, :] % f) == torch.arange(f)[None, :, None]
        ch = torch.where(lead, torch.zeros((b, f, hw), dtype=torch.int64), torch.randint(1, 4, (b, f, hw), generator=g))
        x = (base * 0.1 + 3.0 * torch.nn.functional.one_hot(ch, 4)).to(H16)
    if case.kind == "constant_row":
        x[:, ::2, ::3] = x[:, ::2, ::3, :1]  # rows of four equal values: the LayerNorm variance is 0
    return x, W


def _enc_problem(case, x, W, ref, rule):
    p = case.p
    b, f, hw, ldo, coff = (p[k] for k in ("b", "f", "hw", "ldo", "coff"))
    rows = b * f * hw
    dest = _dest_cols(rows, ldo, coff, 4)

    def emulate(views, mutation):
        y = enc_emulate(x, W, None if mutation in ("coff_ignored", "sibling_written") else mutation).to(H16)
        _write(views["out"], _dest_cols(rows, ldo, 0, 4) if mutation == "coff_ignored" else dest, y.reshape(rows, 4))
        if mutation == "sibling_written":
            col = coff + 4 if coff + 4 < ldo else coff - 1
            if 0 <= col < ldo:
                _write(views["out"], _dest_cols(rows, ldo, col, 1), torch.zeros(rows, dtype=H16))

    return Problem({"x": x.reshape(-1), "params": enc_blob(W)}, {"out": Out(rows * ldo, H16, ref, rule, dest=dest)},
                   ["x", "params", "out", b, f, hw, ldo, coff], emulate, rows)


_ENC_CACHE = {}


def _p_temporal_encoder4(case):
    """the accuracy cases: the oracle module in fp64, rel-L2 and max-abs at twice the yardstick"""
    key = repr(case)
    if key not in _ENC_CACHE:
        x, W = enc_data(case)
        _ENC_CACHE[key] = (x, W) + enc_reference(x, W)
    x, W, ref, rel, mx = _ENC_CACHE[key]
    return _enc_problem(case, x, W, ref.reshape(-1), ("l2", 2 * rel, 2 * mx))


def enc_yardstick(case):
    _p_temporal_encoder4(case)
    return _ENC_CACHE[repr(case)][3:]


ENC_PITCH = ((4, 0), (8, 4), (9, 3))


def _c_temporal_encoder4():
    cs = [Case("temporal_encoder4", "accuracy", b=2, f=f, hw=33, ldo=ENC_PITCH[i % 3][0], coff=ENC_PITCH[i % 3][1])
          for i, f in enumerate((1, 2, 5, 16, 32))]
    cs.append(Case("temporal_encoder4", "dominant", b=2, f=5, hw=33, ldo=8, coff=4))
    cs.append(Case("temporal_encoder4", "constant_row", b=2, f=5, hw=33, ldo=9, coff=3))
    return cs


def enc_relayout_cases():
    """(b, f, hw, (ldo, coff)) of the relayout-invariance launches: the totals 255, 256, 257 and 513 (and 1) in every factorisation"""
    out = []
    for total in TOTALS:
        for i, (b, f, hw) in enumerate(FACT3[total]):
            out.append((b, f, hw, ENC_PITCH[(i + total) % 3]))
    out += [(3, 5, 17, (8, 4)), (17, 3, 5, (4, 0))]  # 255 with three different extents
    return out


def enc_relayout_pair(b, f, hw, pitch, seed=0):
    """two problems on the same data: the launch (b, f, hw) and the launch (b * hw, f, 1) on the data re-laid; a pixel depends on its
    own f rows only, so the outputs are equal bit for bit, pixel by pixel.  -> (problem A, problem B, index of B's rows in A's order)"""
    g = torch.Generator().manual_seed(1000 * b + 10 * f + hw + seed)
    W = enc_weights(torch.Generator().manual_seed(5))
    x = _randn((b, f, hw, 4), g, 1.5)
    x2 = x.permute(0, 2, 1, 3).reshape(b * hw, f, 1, 4).contiguous()
    ldo, coff = pitch
    ca = Case("temporal_encoder4", "relayout", b=b, f=f, hw=hw, ldo=ldo, coff=coff)
    cb = Case("temporal_encoder4", "relayout", b=b * hw, f=f, hw=1, ldo=ldo, coff=coff)
    rows = b * f * hw
    pa = _enc_problem(ca, x, W, None, None)
    pb = _enc_problem(cb, x2, W, None, None)
    # row (bi, fi, p) of A is row (bi * hw + p, fi, 0) of B
    r = torch.arange(rows)
    bi, fi, p = r // (f * hw), (r // hw) % f, r % hw
    return pa, pb, (bi * hw + p) * f + fi, _dest_cols(rows, ldo, coff, 4)


def relayout_equal(placed_a, placed_b, index, dest, what=""):
    """the structure checks of both launches (sentinels, inputs) and the bit-for-bit equality of the re-laid outputs"""
    rows = index.numel()
    outs = []
    for pl in (placed_a, placed_b):
        v = pl.T["out"]
        assert LC.stray_writes(v) == 0, f"{what}: elements written outside the operand"
        got = v.cpu()
        sent = got.view(I16) == LC.OUT_SENTINEL
        assert int((~sent & ~dest).sum()) == 0, f"{what}: sibling channels written"
        assert int((sent & dest).sum()) == 0, f"{what}: described elements unwritten"
        for name in ("x", "params"):
            assert torch.equal(_bytes(pl.T[name].base_alloc), pl.before[name]), f"{what}: input `{name}` changed"
        outs.append(got[dest].reshape(rows, 4))
    a, b = outs[0].view(I16), outs[1][index].view(I16)
    assert not outs[0].isnan().any()
    bad = int((a != b).any(1).sum())
    assert bad == 0, f"{what}: {bad} of {rows} rows differ between the (b, f, hw) launch and the (b * hw, f, 1) launch"


# ---- registry -----------------------------------------------------------------------------------------------------------------------
_PROBLEMS = {
    "timestep_embedding": _p_timestep_embedding, "act": _p_act, "add": _p_add, "conv3x3_small": _p_conv3x3_small,
    "adaptive_avgpool": _p_adaptive_avgpool, "ncfhw_to_tokens": _p_ncfhw_to_tokens, "tokens_to_ncfhw": _p_tokens_to_ncfhw,
    "temporal_encoder4": _p_temporal_encoder4, "conv1x1_small": _p_conv1x1_small, "softmax_rows": _p_softmax_rows,
    "gaussian_sample": _p_gaussian_sample, "scale": _p_scale, "image_to_tokens": _p_image_to_tokens, "tokens_to_image": _p_tokens_to_image,
    "mask_resize_u8": _p_mask_resize_u8, "mask_finish": _p_mask_finish, "clip_patches": _p_clip_patches, "clip_embed": _p_clip_embed,
    "permute_rows": _p_permute_rows,
}
_CASES = {
    "timestep_embedding": _c_timestep_embedding,
    "act": lambda: _c_elementwise("act", [dict(act=ACT_SILU), dict(act=ACT_GELU)]),
    "add": lambda: _c_elementwise("add", [{}]),
    "conv3x3_small": _c_conv3x3_small, "adaptive_avgpool": _c_adaptive_avgpool, "ncfhw_to_tokens": _c_ncfhw_to_tokens,
    "tokens_to_ncfhw": _c_tokens_to_ncfhw, "temporal_encoder4": _c_temporal_encoder4, "conv1x1_small": _c_conv1x1_small,
    "softmax_rows": _c_softmax_rows,
    "gaussian_sample": lambda: _c_elementwise("gaussian_sample", [{}]),
    "scale": lambda: _c_elementwise("scale", [dict(scale=s) for s in SCALES]),
    "image_to_tokens": lambda: _c_image_tokens("image_to_tokens"), "tokens_to_image": lambda: _c_image_tokens("tokens_to_image"),
    "mask_resize_u8": _c_mask_resize_u8,
    "mask_finish": lambda: _c_elementwise("mask_finish", [{}]),
    "clip_patches": _c_clip_patches, "clip_embed": _c_clip_embed, "permute_rows": _c_permute_rows,
}


def cases(entry):
    return _CASES[entry]()


def problem(case):
    return _PROBLEMS[case.entry](case)


# mutation -> the entries whose emulation knows it (tests/test_stem_contract_cpu.py: each must fail at least one case of each)
MUTATIONS = {
    "cos_sin_swapped": ("timestep_embedding",), "half_minus_1": ("timestep_embedding",),
    "window_end_floored": ("adaptive_avgpool",),
    "ky_kx_swapped": ("conv3x3_small",), "stride2_origin_shifted": ("conv3x3_small",),
    "coff_ignored": ("ncfhw_to_tokens", "temporal_encoder4"), "sibling_written": ("ncfhw_to_tokens", "temporal_encoder4"),
    "c_f_swapped": ("ncfhw_to_tokens", "tokens_to_ncfhw"),
    "py_px_swapped": ("clip_patches",),
    "pos_row_div_t": ("clip_embed",), "class_row_last": ("clip_embed",),
    "score_scale_dropped": ("temporal_encoder4",), "heads_swapped": ("temporal_encoder4",), "residual_dropped": ("temporal_encoder4",),
    "softmax_over_pixels": ("temporal_encoder4",),
    "threshold_ge_10": ("mask_finish",),
}
