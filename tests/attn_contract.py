"""Constructors and checkers of the attention contract tests (helper module, not collected by pytest).

What include/mvoc_hip.h promises about mvoc_flash_attn_f16, mvoc_temporal_attn_f16 and mvoc_temporal_qkv_attn_f16, as inputs whose
answer is known without running a softmax:
  * ``Layout`` / ``TLayout``: a descriptor with its operands inside allocations the test owns.  Every input element the descriptor
    does not describe holds fp16 NaN (padding rows behind a batch entry, columns of a row that belong to no operand, the gaps between
    operands, the tail of the allocation); every output allocation holds launch_census.OUT_SENTINEL.  A kernel that lets one such
    element into a result returns NaN, and one that writes outside the described extents destroys a sentinel.
  * ``onehot_case``: every query matches ONE key overwhelmingly; integer values: the output row EQUALS the selected value row.
  * ``uniform_case``: every score is exactly 0; integer values: the output is the exact column mean, to one fp16 rounding.
  * ``staircase_case`` / ``causal_boundary_case``: exact cases for the deferred running maximum and for the causal mask's boundary.
  * ``emulate``: the documented rounding chain in torch, for the CPU test that shows the constructions sound.
Everything is pure torch and works on CPU and GPU; the generators draw on the CPU (one torch.Generator, reproducible).
"""
import math
import zlib

import torch

import launch_census as LC
from launch_census import OUT_SENTINEL, alloc, attn_view, tattn_view, ulp16  # noqa: F401  (re-exported for the tests)
from mvoc_amd._ffi import AttnDesc, TAttnDesc

H16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN16 = 0x7E00      # the poison: fp16 quiet NaN
LEAD, GAP = 64, 64  # poisoned elements in front of the first operand and between two operands (multiples of 8: 16-byte alignment)

# ---- the shapes of the GPU file (tests/test_attention_contract_gpu.py); the CPU file walks the same lists -----------------------------
FLASH_TQ = (1, 33, 130)
FLASH_TK = (1, 2, 64, 77, 145, 193, 257)
FORMS = ((1, 1, 1), (3, 2, 1), (6, 1, 3), (2, 5, 2))     # (nbatch, heads, kv_bdiv)
HD96_TK = (17, 257)
CAUSAL_ONEHOT_T = (1, 77, 200)
CAUSAL_UNIFORM_T = (1, 65, 200)
LONG_TK = (192, 256, 320, 513, 2049, 4159)
LONG_TQ = 130
HUGE_TK, HUGE_TQ = 14399, 33
STAIR_STEPS = (1, 8)  # key ramp per tile: x 16 (the query's ramp entry) / 8 (scale) = 2 / 16 in natural units = 2.9 / 23.1 in log2 units
T_FRAMES = tuple(range(1, 33))
T_HW = (1, 3, 4, 5)
T_HEADS = (1, 5)
RAND_TQ = (1, 31, 32, 33, 127, 128, 129, 257)
RAND_TK = (1, 63, 64, 65, 127, 128, 129, 145, 191, 192, 193)
RAND_FORMS = ((3, 2, 1), (6, 1, 3))
# further random cases at (tq, tk) = (33, 145) / (129, 77) so that every grid size 1..9 is launched: (nbatch, heads, kv_bdiv, tq, tk)
GRID_EXTRA = ((1, 1, 1, 33, 145), (1, 1, 1, 129, 77), (3, 1, 1, 33, 145), (2, 2, 2, 33, 145), (5, 1, 1, 33, 145), (1, 7, 1, 33, 145),
              (4, 2, 2, 33, 145), (3, 3, 1, 33, 145), (2, 1, 1, 129, 77))
RAND_T_HW = (1, 4, 5, 21)
TATTN_BOUND = (2e-3, 1e-2)    # test_ops_gpu.py: test_temporal_attn
TFUSED_BOUND = (3e-3, 2e-2)   # test_ops_gpu.py: test_temporal_qkv_attn_fused
TF_C, TF_FRAMES, TF_HW, TF_NS = (64, 128, 320), (8, 16, 32), (1, 2, 7, 8, 9, 17), (1, 3)


def gen_of(*key):
    """a CPU generator seeded from the case's own parameters (the same draw in every process and on every machine)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def flash_grid(nbatch, heads, tq):
    """blocks of a mvoc_flash_attn_f16 launch: 128 queries per block (include/mvoc_hip.h says nothing of it; used only to COUNT the
    grid sizes the cases reach)"""
    return -(-tq // 128) * heads * nbatch


# ---- allocations ---------------------------------------------------------------------------------------------------------------------
def poisoned(numel, device):
    """`numel` fp16 elements, all NaN16, inside a larger all-NaN16 allocation (launch_census.alloc: 64 KB of slack behind, and with
    the address 128 mod 256 at least 64 elements in front)"""
    v = alloc(numel, H16, 128, device)
    v.base_alloc.view(torch.int16).fill_(NAN16)
    return v


def sentinel(numel, device):
    v = alloc(numel, H16, 128, device)
    v.base_alloc.view(torch.int16).fill_(OUT_SENTINEL)
    return v


def _mask_like(buf):
    return torch.zeros(buf.base_alloc.numel(), dtype=torch.bool, device=buf.device)


class _LayoutBase:
    """shared bookkeeping: self.inp (one poisoned allocation with every input operand), self.T (name -> 1-D operand buffer that
    starts at the operand's first element and spans its extent), self.views (name -> callable(buf) -> logical strided view)"""

    inputs = ()
    outputs = ()

    def put(self, name, x):
        self.views[name](self.T[name]).copy_(x.to(self.device, H16))

    def described_inputs(self):
        """bool mask over the input allocation: the elements some operand describes"""
        m = _mask_like(self.inp)
        for name in self.inputs:
            self.views[name](m[self.T[name].storage_offset():]).fill_(True)
        return m

    def extent_of(self, name):
        """last described element - first + 1, counted from the operand's own mask (not from the stride formula)"""
        buf = self.T[name]
        m = _mask_like(buf)
        self.views[name](m[buf.storage_offset():]).fill_(True)
        idx = torch.nonzero(m).reshape(-1)
        assert int(idx[0]) == buf.storage_offset()
        return int(idx[-1]) - int(idx[0]) + 1

    def check_poison(self):
        """no described input element is poisoned, every other element of the input allocation is"""
        m = self.described_inputs()
        raw = self.inp.base_alloc.view(torch.int16)
        assert bool((raw[~m] == NAN16).all()), "an undescribed input element lost its poison"
        assert not bool(torch.isnan(self.inp.base_alloc[m]).any()), "a described input element is NaN"
        assert int((~m).sum()) > 0

    def reset_outputs(self):
        for name in self.outputs:
            self.T[name].base_alloc.view(torch.int16).fill_(OUT_SENTINEL)

    def check_out(self, name="out"):
        """section D on one output: every described element written and not NaN; no element of the allocation outside the described
        ones touched (padding rows, padding columns inside a row, the slack).  Returns the described elements, logical shape."""
        buf = self.T[name]
        vals = self.views[name](buf).contiguous()
        nanc, unw = int(torch.isnan(vals).sum()), LC.unwritten(vals)
        assert unw == 0, f"{name}: {unw} described elements were never written"
        assert nanc == 0, f"{name}: {nanc} described elements are NaN (a poisoned, undescribed input element reached a result, or the arithmetic overflowed)"
        stray = LC.stray_writes(buf)
        assert stray == 0, f"{name}: {stray} elements outside the operand's extent were written"
        m = _mask_like(buf)
        self.views[name](m[buf.storage_offset():]).fill_(True)
        inner = int((buf.base_alloc.view(torch.int16)[~m] != OUT_SENTINEL).sum())
        assert inner == 0, f"{name}: {inner} undescribed elements (padding rows / columns) were written"
        return vals


class Layout(_LayoutBase):
    """mvoc_attn_desc + operands.  fused: q is the middle column block of a [rows, 3c + pad_cols] buffer, k / v / v2 the three column
    blocks of another (the views the UNet takes of its fused projections); else every operand contiguous (row stride c) in a
    region of its own.  pad_rows: extra rows behind every batch entry (*_bs = (t + pad_rows) * *_ts).  out / out2: row stride
    c + pad_cols, batch stride with pad_rows, an allocation each."""

    def __init__(self, device, nbatch, heads, tq, tk, *, kv_bdiv=1, hd=64, causal=0, scale=0.0, pair=False, fused=True, pad_rows=2,
                 pad_cols=8):
        assert nbatch % kv_bdiv == 0 and pad_cols % 8 == 0
        self.device = torch.device(device)
        self.nbatch, self.heads, self.tq, self.tk, self.kv_bdiv, self.hd = nbatch, heads, tq, tk, kv_bdiv, hd
        self.causal, self.scale, self.pair = causal, scale, pair
        c = heads * hd
        nkv = self.nkv = nbatch // kv_bdiv
        self.inputs = ("q", "k", "v") + (("v2",) if pair else ())
        self.outputs = ("out",) + (("out2",) if pair else ())
        geo = {}  # name -> (offset in self.inp, batches, batch stride, rows, row stride)
        cur = [LEAD]

        def region(rows, ts):
            off = cur[0]
            cur[0] += rows * ts + GAP
            return off

        if fused:
            ts = 3 * c + pad_cols
            qo, kvo = region(nbatch * (tq + pad_rows), ts), region(nkv * (tk + pad_rows), ts)
            geo["q"] = (qo + c, nbatch, (tq + pad_rows) * ts, tq, ts)
            for i, name in enumerate(("k", "v", "v2")):
                geo[name] = (kvo + i * c, nkv, (tk + pad_rows) * ts, tk, ts)
        else:
            geo["q"] = (region(nbatch * (tq + pad_rows), c), nbatch, (tq + pad_rows) * c, tq, c)
            for name in ("k", "v", "v2"):
                if name in self.inputs:
                    geo[name] = (region(nkv * (tk + pad_rows), c), nkv, (tk + pad_rows) * c, tk, c)
        self.inp = poisoned(cur[0], self.device)
        self.T, self.views, self.geo = {}, {}, geo
        for name in self.inputs:
            off, nb, bs, t, ts = geo[name]
            self.T[name] = self.inp[off:off + (nb - 1) * bs + (t - 1) * ts + c]
            self.T[name].base_alloc = self.inp.base_alloc
            self.views[name] = (lambda nb, bs, t, ts: lambda buf: attn_view(buf, nb, bs, t, ts, heads, hd))(nb, bs, t, ts)
        o_ts = c + pad_cols
        o_bs = (tq + pad_rows) * o_ts
        for name in self.outputs:
            geo[name] = (0, nbatch, o_bs, tq, o_ts)
            self.T[name] = sentinel((nbatch - 1) * o_bs + (tq - 1) * o_ts + c, self.device)
            self.views[name] = lambda buf: attn_view(buf, nbatch, o_bs, tq, o_ts, heads, hd)

    def desc(self, pipelined=0):
        d = AttnDesc()
        g = self.geo
        d.q, d.k, d.v, d.out = (self.T[n].data_ptr() for n in ("q", "k", "v", "out"))
        d.q_bs, d.q_ts, d.k_bs, d.k_ts, d.v_bs, d.v_ts = g["q"][2], g["q"][4], g["k"][2], g["k"][4], g["v"][2], g["v"][4]
        d.o_bs, d.o_ts = g["out"][2], g["out"][4]
        d.nbatch, d.heads, d.tq, d.tk, d.kv_bdiv = self.nbatch, self.heads, self.tq, self.tk, self.kv_bdiv
        d.head_dim, d.causal, d.scale, d.pipelined = (0 if self.hd == 64 else self.hd), self.causal, self.scale, pipelined
        if self.pair:
            d.v2, d.out2 = self.T["v2"].data_ptr(), self.T["out2"].data_ptr()
        return d

    def fill(self, case):
        """operands from a case of `groups = nkv * heads` draws with `nqb = kv_bdiv` query batches each (see the generators)"""
        nkv, heads, nqb = self.nkv, self.heads, self.kv_bdiv
        q = case["q"].reshape(nkv, heads, nqb, self.tq, self.hd).permute(0, 2, 3, 1, 4).reshape(self.nbatch, self.tq, heads, self.hd)
        self.put("q", q)
        for name in self.inputs[1:]:
            self.put(name, case[name].reshape(nkv, heads, self.tk, self.hd).permute(0, 2, 1, 3))

    def expected(self, case, key="exp"):
        """a case's expectation [groups, nqb, tq, hd] in the output's logical shape [nbatch, tq, heads, hd]"""
        x = case[key].reshape(self.nkv, self.heads, self.kv_bdiv, self.tq, self.hd)
        return x.permute(0, 2, 3, 1, 4).reshape(self.nbatch, self.tq, self.heads, self.hd)


class TLayout(_LayoutBase):
    """mvoc_tattn_desc + operands in the canonical [sample][frame][pixel][channel] order with padding at every level: pad_cols behind
    a pixel's channels (fused: q / k / v are the column blocks of one [rows, 3c + pad_cols] buffer), pad_pix pixels behind a frame,
    pad_frames frames behind a sample."""

    def __init__(self, device, nsample, hw, frames, heads, *, fused=True, pad_cols=8, pad_pix=1, pad_frames=1):
        self.device = torch.device(device)
        self.nsample, self.hw, self.frames, self.heads = nsample, hw, frames, heads
        c = heads * 64
        self.inputs, self.outputs = ("q", "k", "v"), ("out",)
        self.d = d = TAttnDesc()
        d.nsample, d.hw, d.heads, d.frames = nsample, hw, heads, frames

        def strides(p, ps):
            ts = (hw + pad_pix) * ps
            bs = (frames + pad_frames) * ts
            setattr(d, p + "_ps", ps), setattr(d, p + "_ts", ts), setattr(d, p + "_bs", bs)
            return bs * nsample, (nsample - 1) * bs + (hw - 1) * ps + (frames - 1) * ts + c

        offs, cur = {}, LEAD
        if fused:
            for i, p in enumerate("qkv"):
                size, ext = strides(p, 3 * c + pad_cols)
                offs[p] = (LEAD + i * c, ext)
            cur = LEAD + size + GAP
        else:
            for p in "qkv":
                size, ext = strides(p, c)
                offs[p] = (cur, ext)
                cur += size + GAP
        self.inp = poisoned(cur, self.device)
        self.T = {p: self.inp[o:o + e] for p, (o, e) in offs.items()}
        for t_ in self.T.values():
            t_.base_alloc = self.inp.base_alloc
        _, ext = strides("o", c + pad_cols)
        self.T["out"] = sentinel(ext, self.device)
        self.views = {p: (lambda p: lambda buf: tattn_view(d, buf, p))(p) for p in "qkv"}
        self.views["out"] = lambda buf: tattn_view(d, buf, "o")
        d.q, d.k, d.v, d.out = (self.T[n].data_ptr() for n in ("q", "k", "v", "out"))

    def desc(self):
        return self.d

    def _logical(self, x):
        """[groups = nsample * hw * heads, frames, 64] -> [nsample, hw, frames, heads, 64]"""
        return x.reshape(self.nsample, self.hw, self.heads, self.frames, 64).permute(0, 1, 3, 2, 4)

    def fill(self, case):
        self.put("q", self._logical(case["q"][:, 0]))
        self.put("k", self._logical(case["k"]))
        self.put("v", self._logical(case["v"]))

    def expected(self, case, key="exp"):
        return self._logical(case[key][:, 0])


# ---- cases: every generator returns q [G, nqb, nq, hd], k / v / v2 [G, tk, hd] (fp16) and exp / exp2 [G, nqb, nq, hd] (fp64), G
# ---- independent draws (one per (kv batch entry, head) or per (sample, pixel, head)) -------------------------------------------------
def _ints(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F32)


def _codes(idx, dims, hd):
    """idx [G, n] (int64), dims [G, L]: rows of +-24, bit b of the index at column dims[:, b], zero elsewhere -> [G, n, hd] fp32"""
    G, n = idx.shape
    L = dims.shape[1]
    bits = ((idx[:, :, None] >> torch.arange(L)) & 1).to(F32) * 48 - 24
    out = torch.zeros(G, n, hd)
    out.scatter_(2, dims[:, None, :].expand(G, n, L), bits)
    return out


def _rows(x, sel):
    """x [G, t, hd], sel [G, nqb, nq] -> x[g, sel[g, b, i]] : [G, nqb, nq, hd]"""
    G, nqb, nq = sel.shape
    return torch.gather(x[:, None].expand(G, nqb, *x.shape[1:]), 2, sel[..., None].expand(G, nqb, nq, x.shape[2]))


def _value_rows(gen, G, tk, hd, hd_real, amp):
    v = torch.zeros(G, tk, hd)
    v[:, :, :hd_real] = _ints(gen, -amp, amp, (G, tk, hd_real))
    return v


def _pack(q, k, v, v2, exp, exp2, **more):
    out = {"q": q.to(H16), "k": k.to(H16), "v": v.to(H16), "v2": v2.to(H16), "exp": exp.to(F64), "exp2": exp2.to(F64)}
    for name in ("q", "k", "v", "v2"):  # every operand value is exact in fp16 or the case says nothing
        src = {"q": q, "k": k, "v": v, "v2": v2}[name]
        if more.get("exact", True):
            assert torch.equal(out[name].to(src.dtype), src), name
    out.update({k_: v_ for k_, v_ in more.items() if k_ != "exact"})
    return out


def onehot_case(tk, nq, hd_real, gen, *, hd=64, causal=False, ndims=None, groups=1, nqb=1):
    """keys: the +-24 code of the key index over L = ceil(log2 tk) (>= 1) dims, drawn per group among the hd_real real ones, zero
    elsewhere; queries: the code of a random key (causal: a random key <= the query index).  The selected key's score exceeds every
    other by >= 2 * 576 * scale (144 at scale 1/8, 128.8 at 1/sqrt(80)) in natural units: every other probability underflows to 0 in
    fp32, so out == v[selected] bit for bit, whatever the tiling and the order of the sums."""
    L = ndims or max(1, (tk - 1).bit_length())
    dims = torch.argsort(torch.rand(groups, hd_real, generator=gen), 1)[:, :L]
    k = _codes(torch.arange(tk).expand(groups, tk), dims, hd)
    if causal:
        assert nq == tk
        sel = (torch.rand(groups, nqb, nq, generator=gen) * (torch.arange(nq) + 1)).long().clamp(max=torch.arange(nq))
    else:
        sel = torch.randint(0, tk, (groups, nqb, nq), generator=gen)
    v, v2 = _value_rows(gen, groups, tk, hd, hd_real, 64), _value_rows(gen, groups, tk, hd, hd_real, 64)
    return _pack(_rows(k, sel), k, v, v2, _rows(v, sel), _rows(v2, sel), sel=sel)


def staircase_case(tk, nq, step, gen, *, groups=1, nqb=1):
    """one-hot selection on top of a STAIRCASE of scores (head_dim 64, scale 1/8): every key of tile t (64 keys) scores
    16 * step * t / 8 through one ramp dim, so a row's running maximum grows by 2 * step in natural units (2.885 * step in log2
    units) from tile to tile -- below the deferral threshold of the flash kernels (2^8) for step 1, so that probabilities > 1 against
    a stale maximum and a later rescale both happen, and between fp16's range (2^16) and 2^40 for step 8, so that a kernel which
    does not rescale there overflows fp16.  The keys of the LAST tile carry a 6-dim +-24 code and every query carries the code of
    one of them: the selected key exceeds the rest of its tile by >= 144 and every earlier tile by >= 432 natural units, so
    out == v[selected] bit for bit."""
    hd, nt = 64, -(-tk // 64)
    last0 = 64 * (nt - 1)
    nlast = tk - last0
    perm = torch.argsort(torch.rand(groups, hd, generator=gen), 1)
    dims, rd = perm[:, :6], perm[:, 6]
    k = torch.zeros(groups, tk, hd)
    k[:, last0:] = _codes(torch.arange(nlast).expand(groups, nlast), dims, hd)
    ramp = (torch.arange(tk) // 64).to(F32) * step
    k.scatter_(2, rd[:, None, None].expand(groups, tk, 1), ramp[None, :, None].expand(groups, tk, 1))
    sel = last0 + torch.randint(0, nlast, (groups, nqb, nq), generator=gen)
    q = _rows(k, sel)
    q.scatter_(3, rd[:, None, None, None].expand(groups, nqb, nq, 1), torch.full((groups, nqb, nq, 1), 16.0))
    v, v2 = _value_rows(gen, groups, tk, hd, hd, 64), _value_rows(gen, groups, tk, hd, hd, 64)
    return _pack(q, k, v, v2, _rows(v, sel), _rows(v2, sel), sel=sel)


def causal_boundary_case(t, gen, *, hd=64, hd_real=64, groups=1):
    """the causal mask's boundary, row by row: keys 2m and 2m + 1 carry the SAME code (of m), query i the code of i / 2.  An even
    query sees key i but not its twin i + 1: out == v[i]; an odd query sees both twins with equal scores: out == (v[i-1] + v[i]) / 2
    (integers: exact).  A mask that lets key i + 1 through, or hides key i, changes an even or an odd row by whole halves."""
    L = max(1, ((t + 1) // 2 - 1).bit_length())
    dims = torch.argsort(torch.rand(groups, hd_real, generator=gen), 1)[:, :L]
    k = _codes((torch.arange(t) // 2).expand(groups, t), dims, hd)
    v, v2 = _value_rows(gen, groups, t, hd, hd_real, 64), _value_rows(gen, groups, t, hd, hd_real, 64)

    def exp(x):
        prev = torch.cat([x[:, :1], x[:, :-1]], 1)
        odd = (torch.arange(t) % 2 == 1)[None, :, None]
        return torch.where(odd, (x.double() + prev.double()) / 2, x.double())[:, None]

    return _pack(k[:, None].clone(), k, v, v2, exp(v), exp(v2))


def uniform_case(tk, nq, gen, *, hd=64, hd_real=None, causal=False, groups=1, nqb=1):
    """queries non-zero only in dims 0..31, keys only in dims 32..hd-1 (3 * randn there): every score is exactly 0, every
    probability exactly 1, the fp32 sums of the integer values (|v| <= 8) exact: out = S / n up to the kernel's fp32 reciprocal and
    multiply (a few fp32 ulps) and ONE fp16 rounding, i.e. |out - S / n| < ulp16(S / n).  n = tk, or the prefix i + 1 (causal)."""
    hd_real = hd_real or hd
    q = torch.zeros(groups, nqb, nq, hd)
    q[..., :32] = (3 * torch.randn(groups, nqb, nq, 32, generator=gen)).to(H16).to(F32)
    k = torch.zeros(groups, tk, hd)
    k[..., 32:] = (3 * torch.randn(groups, tk, hd - 32, generator=gen)).to(H16).to(F32)
    v, v2 = _value_rows(gen, groups, tk, hd, hd_real, 8), _value_rows(gen, groups, tk, hd, hd_real, 8)

    def exp(x):
        if causal:
            assert nq == tk
            m = x.double().cumsum(1) / (torch.arange(tk) + 1).double()[None, :, None]
            return m[:, None].expand(groups, nqb, nq, hd)
        return (x.double().sum(1) / tk)[:, None, None, :].expand(groups, nqb, nq, hd)

    return _pack(q, k, v, v2, exp(v), exp(v2))


def random_case(tk, nq, gen, *, hd=64, groups=1, nqb=1, amp=1.0):
    """randn operands (section C); no expectation: the caller takes launch_census.attn_ref / tattn_ref on the filled layout"""
    q = (amp * torch.randn(groups, nqb, nq, hd, generator=gen)).to(H16)
    k, v, v2 = ((amp * torch.randn(groups, tk, hd, generator=gen)).to(H16) for _ in range(3))
    z = torch.zeros(groups, nqb, nq, hd)
    return _pack(q, k, v, v2, z, z, exact=False)


# ---- checkers ------------------------------------------------------------------------------------------------------------------------
def assert_equal_rows(out, exp, what):
    out, exp = out.double().cpu(), exp.double().cpu()
    bad = out != exp
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the selected rows, first at " \
                                f"{tuple(torch.nonzero(bad)[0].tolist())}: {float(out[bad][0])} != {float(exp[bad][0])}"


def assert_within_ulp(out, exp, what):
    out, exp = out.double().cpu(), exp.double().cpu()
    err, bound = (out - exp).abs(), ulp16(exp)
    bad = ~(err < bound)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements are an fp16 ulp or more from the exact mean, " \
                                f"worst {float((err / bound).max()):.3g} ulp"


def slice_errors(out, ref, slice_dims):
    """(worst rel-L2 over the slices, max abs): `slice_dims` are the dims that index a slice (e.g. (0, 2) = batch entry, head)"""
    out, ref = out.double(), ref.double()
    red = tuple(i for i in range(out.dim()) if i not in slice_dims)
    num, den = ((out - ref) ** 2).sum(red).sqrt(), (ref ** 2).sum(red).sqrt()
    rel = torch.where(den > 0, num / den.clamp_min(1e-300), num)
    return float(rel.max()), float((out - ref).abs().max())


def assert_close_slices(out, ref, slice_dims, bound, what):
    rel, mab = slice_errors(out, ref, slice_dims)
    assert rel < bound[0] and mab < bound[1], f"{what}: worst slice rel-L2 {rel:.3g} (bound {bound[0]}), max abs {mab:.3g} (bound {bound[1]})"


def emulate(q, k, v, scale, causal=False):
    """the rounding chain include/mvoc_hip.h and attention.hip document, in torch: scores in fp32, probabilities against the row
    maximum rounded to fp16, fp32 sums of those (numerator and denominator), one fp16 rounding of the quotient.  q [..., nq, hd],
    k / v [..., tk, hd] (leading dims broadcast) -> fp16 [..., nq, hd]"""
    s = torch.matmul(q.to(F32), k.to(F32).transpose(-1, -2)) * scale
    if causal:
        nq, tk = s.shape[-2:]
        s = s.masked_fill(torch.arange(tk, device=s.device)[None, :] > torch.arange(nq, device=s.device)[:, None], float("-inf"))
    p = torch.exp(s - s.max(-1, keepdim=True).values).to(H16).to(F32)
    return (torch.matmul(p, v.to(F32)) / p.sum(-1, keepdim=True)).to(H16)


def emulate_case(case, scale, causal=False):
    """emulate on a generator's case: ([G, nqb, nq, hd] for v, the same for v2)"""
    return tuple(emulate(case["q"], case["k"][:, None], case[n][:, None], scale, causal) for n in ("v", "v2"))


def default_scale(hd, hd_real=None):
    return 0.125 if hd == 64 else 1.0 / math.sqrt(hd_real or hd)
