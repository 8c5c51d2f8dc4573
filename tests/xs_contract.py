"""Constructors, checkers and runners of the xs_linear contract tests (helper module, not collected by pytest).

What include/mvoc_hip.h promises about mvoc_xs_linear_f16, held on inputs whose answer is known, at the shapes where the kernel's
hand-counted waits and clamped rows can go wrong (one to five 32-channel stages, one row to two blocks and a row), inside poisoned
allocations:
  * ``XsLayout``: a mvoc_xs_desc with every operand inside an allocation the test owns.  Every input element the descriptor does not
    describe holds fp16 NaN: the lead and tail of x and of wp, bytes 128..1023 of every constants piece, the residual's columns
    >= n_store, the gaps between its rows, its lead and slack.  The output allocation holds launch_census.OUT_SENTINEL.
  * ``walk(k)``: the deterministic list of cases of one K.  tests/test_xs_contract_cpu.py asserts what it covers.
  * ``draw``: the constructions A (integers, exact), B (balanced rows: the folded LayerNorm gives exactly +-1, exact), C (sparse
    draws, activations held to launch_census.xs_ref's derived bound), D (random against fp64, per 32-row group), S (weight sets).
  * ``emulate``: the documented rounding chain in torch fp32 / fp16, for the CPU test that shows the constructions sound.
  * ``run_case`` / ``run_sections``: one code path for the GPU tests, the forced-form worker (tests/xs_forced_worker.py) and the
    CPU test: the `kernel` argument is the library's entry or ``emulate_into``.
Everything is pure torch and works on CPU and GPU; every draw is made on the CPU from a generator seeded by the case's parameters.
"""
import ctypes as C
import itertools

import torch
import torch.nn.functional as F

import launch_census as LC
from attn_contract import NAN16, _LayoutBase, gen_of
from launch_census import OUT_SENTINEL, alloc  # noqa: F401  (re-exported for the tests)
from mvoc_amd._ffi import ACT_GEGLU, ACT_GELU, ACT_NONE, ACT_SILU, XsDesc

H16, F32, F64, I16 = torch.float16, torch.float32, torch.float64, torch.int16
LEAD = 128  # poisoned (outputs: sentinel) elements in front of every operand: 256 bytes, so the address mod 256 is the allocation's

# ---- the shapes of the GPU file (tests/test_xs_contract_gpu.py); the CPU file walks the same lists ----------------------------------
M = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)  # below / at / above a wave's 32 rows, a 128-row block (RG 1), a 256-row block (RG 2)
T = (1, 2, 3, 4, 5)                                # 32-channel stages: n = 32 T
GEGLU_N = (64, 128, 192)
K = (64, 128, 320)
ACTS = (ACT_NONE, ACT_SILU, ACT_GELU, ACT_GEGLU)
TRIMS = (0, 8, 24)        # n_store = n - trim
GEGLU_TRIMS = (0, 8)      # n_store = n / 2 - trim
LDO_PAD, LDR_PAD, ADDR = (0, 8), (0, 16), (0, 16, 128)
PLACEMENTS = tuple(itertools.product(LDO_PAD, LDR_PAD, ADDR))  # (ldo - cols, ldr - cols, address mod 256 of out and resid)
SET_ROWS, SET_M = 256, (512, 768)
OFFSET_M, OFFSET_T = 257, 3  # the large-offset rows of section D
EPS = 1e-5
D_BOUND, D_BOUND_LN = 1.5e-3, 2.5e-3  # test_ops_gpu.py: test_xs_linear_matches_tiled_gemm, test_xs_linear_layernorm_fold
EXACT_LIMIT = 2048                    # |integer| < 2^11: exact in fp16
SECTIONS = ("A", "B", "C", "D", "S")
ACT_NAME = {ACT_NONE: "none", ACT_SILU: "silu", ACT_GELU: "gelu", ACT_GEGLU: "geglu"}


def full_cols(n, act):
    return n // 2 if act == ACT_GEGLU else n


def _case(i, k, m, n, act, resid, normalize, trim_i, **more):
    trims = GEGLU_TRIMS if act == ACT_GEGLU else TRIMS
    ldo_pad, ldr_pad, addr = PLACEMENTS[i % len(PLACEMENTS)]
    p = dict(i=i, k=k, m=m, n=n, act=act, resid=bool(resid), normalize=int(normalize), trim=trims[trim_i % len(trims)], ldo_pad=ldo_pad,
             ldr_pad=ldr_pad, addr=addr, set_rows=0, offset=False, big_mean=False)
    p.update(more)
    p["n_store"] = full_cols(n, act) - p["trim"]
    return p


def _combos():
    """(act, residual, normalize): the residual is never present with GEGLU"""
    return [(a, r, nm) for a in ACTS for r in (0, 1) for nm in (0, 1) if not (a == ACT_GEGLU and r)]


def walk(k):
    """the cases of one K, three loops, the other options cycling with the case index (as flash_layout(i, ...) does):
      1. every (act, residual, normalize) with every T (GEGLU: every n of GEGLU_N);
      2. every M with and without residual and normalize, act none (so the exact sections A and B see every M);
      3. every n_store trim with and without residual, for every act
    and every (ldo, ldr, address) placement several times over."""
    out = []

    def add(*a, **kw):
        out.append(_case(len(out), k, *a, **kw))

    for act, resid, nm in _combos():
        for n in (GEGLU_N if act == ACT_GEGLU else tuple(32 * t for t in T)):
            add(M[(3 * len(out) + 1) % len(M)], n, act, resid, nm, len(out))
    for m in M:
        for resid in (0, 1):
            for nm in (0, 1):
                add(m, 32 * T[len(out) % len(T)], ACT_NONE, resid, nm, len(out))
    for act in ACTS:
        for resid in ((0,) if act == ACT_GEGLU else (0, 1)):
            for ti in range(len(GEGLU_TRIMS if act == ACT_GEGLU else TRIMS)):
                n = GEGLU_N[len(out) % 3] if act == ACT_GEGLU else 32 * T[len(out) % len(T)]
                add(M[(7 * len(out)) % len(M)], n, act, resid, len(out) % 2, ti)
    return out


def set_cases(k):
    """section S: a weight set per 256 rows (mvoc_groupnorm_fold_xs_f16's consumer form), two and three sets, construction A"""
    return [_case(i, k, m, 32 * T[(i + 1) % len(T)], ACT_NONE, resid, 0, i, set_rows=SET_ROWS)
            for i, (m, resid) in enumerate(itertools.product(SET_M, (0, 1)))]


def offset_case(k):
    """section D's rows of large mean against their spread (test_layernorm_fold_rows_with_large_offset), two blocks and a row"""
    return _case(0, k, OFFSET_M, 32 * OFFSET_T, ACT_NONE, 0, 1, 0, offset=True)


def big_mean_case(k):
    """section B's balanced rows about a mean of +-1000 (every x an integer below 2048: exact in fp16): the two-pass moments of the
    kernel stay exact, sum x^2 = 3.2e8 does not fit fp32's 24 bits -- a one-pass E[x^2] - mu^2 variance is wrong by tens of per cent
    and the output, which EQUALS the integer answer, shows it.  (The random large-offset rows of section D do not: there an fp32
    one-pass form is off by 1.2e-3 to 1.6e-3 per 32-row group, inside the project's bound of 2.5e-3.)"""
    return _case(1, k, OFFSET_M, 32 * OFFSET_T, ACT_NONE, 1, 1, 1, big_mean=True)


def section_cases(section, k):
    w = walk(k)
    if section == "A":
        return [p for p in w if p["act"] == ACT_NONE and not p["normalize"]]
    if section == "B":
        return [p for p in w if p["act"] == ACT_NONE and p["normalize"]] + [big_mean_case(k)]
    if section == "C":
        return [p for p in w if p["act"] != ACT_NONE]
    if section == "D":
        return w + [offset_case(k)]
    assert section == "S"
    return set_cases(k)


def case_key(section, p):
    return f"{section}_k{p['k']}_{'offset' if p['offset'] else 'bigmean' if p['big_mean'] else p['i']}"


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
def _region(numel, addr_mod, device, fill):
    v = alloc(LEAD + numel, H16, addr_mod, device)
    v.base_alloc.view(I16).fill_(fill)
    t = v[LEAD:]
    t.base_alloc = v.base_alloc
    assert t.data_ptr() % 256 == addr_mod
    return t


class XsLayout(_LayoutBase):
    """mvoc_xs_desc + operands, an allocation each: x [m][k] and the packed stream(s) wp with a poisoned lead and tail, resid
    [m][cols] at pitch ldr = cols + ldr_pad, out [m][cols] at pitch ldo = cols + ldo_pad, out and resid at `addr` mod 256.
    cols = n_store (GEGLU: of n / 2).  The descriptor says n_store = 0 (all columns) where nothing is trimmed and the pitch is tight."""

    def __init__(self, device, p):
        self.device = torch.device(device)
        self.p = p
        m, n, k = p["m"], p["n"], p["k"]
        self.m, self.n, self.k, self.nk = m, n, k, k // 16
        self.cols = cols = p["n_store"]
        self.ldo, self.ldr = cols + p["ldo_pad"], cols + p["ldr_pad"]
        self.nsets = m // p["set_rows"] if p["set_rows"] else 1
        self.inputs = ("x", "wp") + (("resid",) if p["resid"] else ())
        self.outputs = ("out",)
        wp_numel = self.nsets * (n // 32) * (self.nk + 1) * 512
        self.T = {"x": _region(m * k, 128, self.device, NAN16), "wp": _region(wp_numel, 128, self.device, NAN16),
                  "out": _region((m - 1) * self.ldo + cols, p["addr"], self.device, OUT_SENTINEL)}
        if p["resid"]:
            self.T["resid"] = _region((m - 1) * self.ldr + cols, p["addr"], self.device, NAN16)
        self.views = {"x": lambda b: b.as_strided((m, k), (k, 1), b.storage_offset()),
                      "wp": lambda b: b.as_strided((wp_numel,), (1,), b.storage_offset()),
                      "resid": lambda b: b.as_strided((m, cols), (self.ldr, 1), b.storage_offset()),
                      "out": lambda b: b.as_strided((m, cols), (self.ldo, 1), b.storage_offset())}

    def desc(self):
        p, d = self.p, XsDesc()
        d.x, d.wp, d.out = (self.T[n].data_ptr() for n in ("x", "wp", "out"))
        d.resid = self.T["resid"].data_ptr() if p["resid"] else None
        d.m, d.n, d.k, d.act, d.normalize, d.ln_eps = self.m, self.n, self.k, p["act"], p["normalize"], EPS
        d.n_store = 0 if (p["trim"] == 0 and p["ldo_pad"] == 0) else self.cols
        d.ldo, d.ldr, d.wp_set_rows = self.ldo, (self.ldr if p["resid"] else 0), p["set_rows"]
        return d

    def _wp_tails(self, buf):
        """[tiles][448]: the halves behind the 32 fp32 constants of every tile's constants piece"""
        return self.views["wp"](buf).view(-1, self.nk + 1, 512)[:, self.nk, 64:]

    def described(self, name):
        """bool mask over the operand's allocation: the elements the descriptor describes"""
        buf = self.T[name]
        mask = torch.zeros(buf.base_alloc.numel(), dtype=torch.bool, device=self.device)
        self.views[name](mask[buf.storage_offset():]).fill_(True)
        if name == "wp":
            self._wp_tails(mask[buf.storage_offset():]).fill_(False)
        return mask

    def fill(self, case):
        from mvoc_amd.unet import pack_geglu, pack_xs_weights
        self.put("x", case["x"])
        packs = []
        for w, c in zip(case["W"], case["c"]):
            if self.p["act"] == ACT_GEGLU:
                w, c = pack_geglu(w, c)
            packs.append(pack_xs_weights(w, c).reshape(-1))
        self.put("wp", torch.cat(packs))
        self._wp_tails(self.T["wp"]).view(I16).fill_(NAN16)  # the packer zero-fills what the header leaves undescribed
        if self.p["resid"]:
            self.put("resid", case["resid"])
        self.logical = {"W": [w.to(self.device) for w in case["W"]], "c": [c.to(self.device) for c in case["c"]]}

    def check_poison(self):
        """no described input element is NaN (a constant: not finite as fp32), every other element of the input allocations is poison"""
        for name in self.inputs:
            mask = self.described(name)
            base = self.T[name].base_alloc
            assert bool((base.view(I16)[~mask] == NAN16).all()), f"{name}: an undescribed element lost its poison"
            assert int((~mask).sum()) >= LEAD + (LC.SLACK_BYTES // 2)
            if name == "wp":
                pieces = self.views["wp"](self.T["wp"]).view(-1, self.nk + 1, 512)
                assert not bool(torch.isnan(pieces[:, :self.nk]).any()), "wp: a described weight is NaN"
                assert bool(torch.isfinite(pieces[:, self.nk, :64].contiguous().view(F32)).all()), "wp: a described constant is not finite"
            else:
                assert not bool(torch.isnan(base[mask]).any()), f"{name}: a described element is NaN"

    def check_out(self, name="out"):
        """attn_contract's check (every described element written and not NaN, nothing else of the allocation touched: rows >= m,
        columns >= n_store within ldo, the lead, the slack), and every described element FINITE: two poison halves read as one fp32
        constant are 4.3e37, which reaches the output as inf, not NaN"""
        vals = super().check_out(name)
        bad = int((~torch.isfinite(vals)).sum())
        assert bad == 0, f"{name}: {bad} described elements are not finite (a poisoned, undescribed input element reached a result)"
        return vals

    def ref_buffers(self):
        """what launch_census.xs_ref reads: x [m * k] and the residual as m rows of pitch ldr (the last row's padding lies in the slack)"""
        bufs = {"x": self.T["x"]}
        if self.p["resid"]:
            r = self.T["resid"]
            bufs["resid"] = r.base_alloc[r.storage_offset():r.storage_offset() + self.m * self.ldr]
        return bufs

    def reference(self):
        """launch_census.xs_ref on the layout's own buffers and the case's logical weights: (fp64 stored values, bound) [m, cols]"""
        d, bufs = self.desc(), self.ref_buffers()
        rows = self.p["set_rows"] or self.m
        parts = [LC.xs_ref(d, bufs, self.logical, r0, r0 + rows) for r0 in range(0, self.m, rows)]
        ref, bound = torch.cat([a for a, _ in parts]), torch.cat([b for _, b in parts])
        return ref[:, :self.cols], bound[:, :self.cols]


# ---- constructions -------------------------------------------------------------------------------------------------------------------
def _ints(gen, lo, hi, shape, dtype=H16):
    return LC._ints(shape, gen, "cpu", lo, hi, dtype)


def balanced_rows(gen, m, k, big_mean=False):
    """launch_census.build_xs's rows for normalize: mu + v * (+-1), half of each sign, the sign pattern drawn per row, mu in [-2, 2],
    v in [1, 3]: mean and variance exact in fp32, the normalised values round to exactly +-1 in fp16.  Returns (x, the +-1 pattern)"""
    mu, v = _ints(gen, -2, 2, (m, 1), F32), _ints(gen, 1, 3, (m, 1), F32)
    if big_mean:
        mu = mu + 2000.0 * _ints(gen, 0, 1, (m, 1), F32) - 1000.0
    sign = torch.ones(m, k)
    sign[:, k // 2:] = -1
    sign = torch.gather(sign, 1, torch.argsort(torch.rand(m, k, generator=gen), 1))
    return (mu + v * sign).to(H16), sign


def preact(case):
    """x (normalised where the case says so) @ W^T + c in fp64, per weight set, rows concatenated"""
    x = case["xn"].to(F64)
    rows = x.shape[0] // len(case["W"])
    return torch.cat([x[s * rows:(s + 1) * rows] @ w.to(F64).t() + c.to(F64) for s, (w, c) in enumerate(zip(case["W"], case["c"]))])


def draw(section, p):
    """the operands of a case, drawn on the CPU from a generator seeded by the case's own parameters: x [m, k] fp16, W / c: per weight
    set [n, k] fp16 (logical row order: GEGLU's value rows first, then the gate rows) and [n] fp32, resid [m, cols] fp16 or None, xn:
    what the MFMAs see (x, or the rows after the folded LayerNorm where that is exact)"""
    m, n, k, cols = p["m"], p["n"], p["k"], p["n_store"]
    nsets = m // p["set_rows"] if p["set_rows"] else 1
    for attempt in range(16):
        gen = gen_of(section, attempt, sorted(p.items()))
        xn = None
        if section in ("A", "S"):
            assert not p["normalize"]
            x = _ints(gen, -3, 3, (m, k))
            W = [_ints(gen, -2, 2, (n, k)) for _ in range(nsets)]
            c = [_ints(gen, -8, 8, (n,), F32) for _ in range(nsets)]
            r = _ints(gen, -16, 16, (m, cols))
        elif section == "B":
            x, xn = balanced_rows(gen, m, k, p["big_mean"])
            W, c, r = [_ints(gen, -2, 2, (n, k))], [_ints(gen, -8, 8, (n,), F32)], _ints(gen, -16, 16, (m, cols))
        elif section == "C":
            x, xn = balanced_rows(gen, m, k) if p["normalize"] else (_ints(gen, -1, 1, (m, k)), None)
            W, c, r = [LC._ints_sparse((n, k), gen, "cpu")], [_ints(gen, -4, 4, (n,), F32)], _ints(gen, -4, 4, (m, cols))
        else:
            assert section == "D"
            if p["offset"]:
                x = (40.0 + 0.5 * torch.randn(m, k, generator=gen)).to(H16)
                x[::7] = (-25.0 + 0.25 * torch.randn(x[::7].shape, generator=gen)).to(H16)
            else:
                x = (1.5 * torch.randn(m, k, generator=gen) + 0.3).to(H16)
            W = [(torch.randn(n, k, generator=gen) / k ** 0.5).to(H16)]
            c = [(0.2 * torch.randn(n, generator=gen)).to(H16).to(F32)]  # an fp16 bias, as the product's packers receive it
            r = torch.randn(m, cols, generator=gen).to(H16)
        case = {"x": x, "xn": x if xn is None else xn, "W": W, "c": c, "resid": r if p["resid"] else None}
        if section != "C":
            break
        # C: at least half of the pre-activations where the activations are not trivially y or 0 (a draw that misses is drawn again)
        case["share"] = float((preact(case).abs() <= 8).double().mean())
        if case["share"] >= 0.5:
            break
    if m > 1:  # the rows are pairwise different: a dropped or duplicated row changes the answer
        assert torch.unique(case["x"], dim=0).shape[0] == m
    return case


# ---- the documented rounding chain ---------------------------------------------------------------------------------------------------
def _r16(x):
    return x.to(H16).to(F32)


def layernorm_fold(x16, eps, one_pass=False):
    """the folded LayerNorm as xslin.hip does it, fp32: the mean, then the moments of x - c with c the mean rounded to fp16 (the
    subtraction in fp16), the normalised row rounded to fp16.  one_pass: the E[x^2] - mu^2 form the kernel must NOT use, accumulated
    in sequence in fp32 as a lane would (planted defect 8)."""
    x = x16.to(F32)
    k = x.shape[1]
    if one_pass:
        s1, s2 = torch.zeros(x.shape[0]), torch.zeros(x.shape[0])
        for j in range(k):
            s1, s2 = s1 + x[:, j], s2 + x[:, j] * x[:, j]
        mu = (s1 / k)[:, None]
        var = (s2 / k)[:, None] - mu * mu
    else:
        mu = x.sum(1, keepdim=True) / k
        d = (x16 - mu.to(H16)).to(F32)
        dm = d.sum(1, keepdim=True) / k
        var = (d * d).sum(1, keepdim=True) / k - dm * dm
    return _r16((x - mu) * torch.rsqrt(var.clamp_min(0) + eps))


def epilogue(y, act, resid, n_store):
    """+ c done by the caller; r16, the activation, r16, + residual, the final rounding; GEGLU rounds value and gate separately"""
    if act == ACT_GEGLU:
        inner = y.shape[1] // 2
        out = (_r16(y[:, :inner]) * _r16(F.gelu(_r16(y[:, inner:])))).to(H16)
    else:
        v = _r16(y)
        if act == ACT_SILU:
            v = _r16(F.silu(v))
        elif act == ACT_GELU:
            v = _r16(F.gelu(v))
        out = v.to(H16)
    out = out[:, :n_store]
    if resid is not None:
        out = (out.to(F32) + resid.to(F32)).to(H16)
    return out


def emulate(x16, W, c, act, resid, normalize, n_store, eps=EPS, one_pass=False):
    """the chain of include/mvoc_hip.h and xslin.hip in torch fp32 / fp16 on the CPU: W / c per weight set (logical row order),
    rows split evenly over the sets -> fp16 [m, n_store]"""
    x = layernorm_fold(x16, eps, one_pass) if normalize else x16.to(F32)
    rows = x.shape[0] // len(W)
    y = torch.cat([x[s * rows:(s + 1) * rows] @ w.to(F32).t() + cs.to(F32) for s, (w, cs) in enumerate(zip(W, c))])
    return epilogue(y, act, resid, n_store)


def unpack_layout(L):
    """what a kernel reads of a filled layout, taken from the layout's BUFFERS: x, the per-set logical (W, c) unpacked from the
    stream, the residual view -- and `tails`, the first 32 fp32 of the bytes behind every tile's constants (planted defect 7)"""
    p = L.p
    x = L.views["x"](L.T["x"]).cpu()
    stream = L.views["wp"](L.T["wp"]).cpu().reshape(L.nsets, -1)
    W, c, tails = [], [], []
    for s in range(L.nsets):
        w, cs = LC.unpack_xs_weights(stream[s], L.n, L.k)
        tl = stream[s].reshape(L.n // 32, L.nk + 1, 512)[:, L.nk, 64:128].contiguous().view(F32).reshape(L.n)
        if p["act"] == ACT_GEGLU:  # packed order: blocks of 32 value rows then their 32 gate rows -> logical order
            idx = torch.arange(L.n).reshape(L.n // 64, 2, 32).permute(1, 0, 2).reshape(-1)
            w, cs, tl = w[idx], cs[idx], tl[idx]
        W.append(w), c.append(cs), tails.append(tl)
    resid = L.views["resid"](L.T["resid"]).cpu() if p["resid"] else None
    return x, W, c, resid, tails


def emulate_into(L, defect=None):
    """the CPU stand-in for the kernel: reads the layout's buffers, writes the described output elements.  `defect`: a planted fault
    (tests/test_xs_contract_cpu.py: each must trip the check named there)"""
    p = L.p
    x, W, c, resid, tails = unpack_layout(L)
    m, cols = L.m, L.cols
    if defect == "next_tile_constants":
        c = [torch.roll(cs.reshape(-1, 32), -1, 0).reshape(-1) for cs in c]
    elif defect == "previous_tile_residual":
        resid = torch.cat([resid[:, :32], resid[:, :cols - 32]], 1)
    elif defect == "constants_tail":
        c = [torch.where(torch.arange(L.n) == 5, tl, cs) for cs, tl in zip(c, tails)]
    out = emulate(x, W, c, p["act"], resid, p["normalize"], cols, one_pass=defect == "one_pass_variance")
    if defect == "row_copies_neighbour":
        out[m // 2] = out[m // 2 - 1]
    elif defect == "tiles_swapped":
        out = torch.cat([out[:, 32:64], out[:, :32], out[:, 64:]], 1)
    view = L.views["out"](L.T["out"])
    if defect == "trim_every_tile":  # the last tile's trim applied to every tile: the columns behind it in each tile are not stored
        keep = (torch.arange(cols) % 32) < 32 - p["trim"]
        view[:, keep] = out[:, keep].to(L.device)
    else:
        view.copy_(out.to(L.device))
    flat = L.T["out"].base_alloc
    if defect == "row_m_written":
        flat[L.T["out"].storage_offset() + m * L.ldo] = 1.0
    elif defect == "columns_past_n_store":
        o = L.T["out"].storage_offset() + (m // 2) * L.ldo + cols
        flat[o:o + 8] = 1.0


# ---- checkers ------------------------------------------------------------------------------------------------------------------------
def assert_equal_bits(out, ref, what):
    """out (fp16) EQUALS the fp64 answer, compared as bits of the fp16 value"""
    ref = (ref.cpu() + 0.0)
    assert bool((ref.abs() < EXACT_LIMIT).all()) and torch.equal(ref.to(H16).to(F64), ref), f"{what}: the answer is not exact in fp16"
    bad = out.cpu().view(I16) != ref.to(H16).view(I16)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact answer, first at " \
                                f"{tuple(torch.nonzero(bad)[0].tolist())}: {float(out.cpu()[bad][0])} != {float(ref[bad][0])}"


def assert_within_bound(out, ref, bound, what):
    err = (out.to(F64) - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the derived bound, worst " \
                                f"{float((err - bound).max()):.3g} over it"


def group_errors(out, ref):
    """rel-L2 per 32-row group (a wave's rows): [ceil(m / 32)]"""
    out, ref = out.to(F64), ref.to(F64)
    m = out.shape[0]
    pad = -m % 32
    num = F.pad(((out - ref) ** 2).sum(1), (0, pad)).reshape(-1, 32).sum(1).sqrt()
    den = F.pad((ref ** 2).sum(1), (0, pad)).reshape(-1, 32).sum(1).sqrt()
    return torch.where(den > 0, num / den.clamp_min(1e-300), num)


def assert_close_groups(out, ref, bound, what):
    rel = group_errors(out, ref)
    assert bool((rel < bound).all()), f"{what}: 32-row group {int(rel.argmax())} has rel-L2 {float(rel.max()):.3g} (bound {bound})"


# ---- runners: one code path for the GPU tests, the forced-form worker and the CPU test -----------------------------------------------
def library_kernel(lib, stream_fn):
    def kernel(L):
        rc = lib.mvoc_xs_linear_f16(C.byref(L.desc()), stream_fn())
        assert rc == 0, lib.mvoc_last_error().decode()
    return kernel


def run_case(section, p, device, kernel, figures=None):
    """draw, lay out, check_poison, launch, check_out, the section's comparison: the bits of the described output [m, cols] (int16, CPU)"""
    what = f"{case_key(section, p)} m {p['m']} n {p['n']} act {ACT_NAME[p['act']]} resid {p['resid']} ln {p['normalize']} trim {p['trim']} " \
           f"ldo +{p['ldo_pad']} ldr +{p['ldr_pad']} addr {p['addr']}"
    case = draw(section, p)
    L = XsLayout(device, p)
    L.fill(case)
    L.check_poison()
    ref, bound = L.reference()
    if section in ("A", "B", "S"):
        assert bool((preact(case).abs() < EXACT_LIMIT).all()) and bool((ref.abs() < EXACT_LIMIT).all()), what  # before launching
    if section == "C":
        assert case["share"] >= 0.5, (what, case["share"])
    kernel(L)
    out = L.check_out("out")
    if section in ("A", "B", "S"):
        assert_equal_bits(out, ref, what)
    elif section == "C":
        assert_within_bound(out, ref, bound, what)
    else:
        lim = D_BOUND_LN if p["normalize"] else D_BOUND
        if figures is not None:
            figures.append((what, float(group_errors(out, ref).max()), lim))
        assert_close_groups(out, ref, lim, what)
    return out.cpu().view(I16).clone()


def run_sections(k, device, kernel, sections=SECTIONS, figures=None):
    """every case of the sections at one K: case key -> output bits"""
    return {case_key(s, p): run_case(s, p, device, kernel, figures) for s in sections for p in section_cases(s, k)}
