"""Constructors, layouts and a CPU model of the fused temporal QKV-attention contract tests (helper module, not collected by pytest).

What include/mvoc_hip.h promises about mvoc_temporal_qkv_attn_f16 (mvoc_amd/csrc/tfused.hip: LayerNorm -> to_q / to_k / to_v -> softmax
over the frame axis in one kernel), as inputs whose answer is known without running a LayerNorm or a softmax.  Every case goes through
``Linear.fold_layernorm`` and ``pack_tfused_weights``: the packing is under test with the kernel.

  A  exact selection.  Frame f of pixel p of sample n is the two-valued row  x = B + u (1 + e s) / 2:  s the +-1 Walsh
     (Sylvester-Hadamard) row of order 64 with index 32 + (class * F + f), class = (p + n) mod (32 / F), tiled C / 64 times; e = +-1
     drawn per (sample, pixel).  Indices 32..63 are balanced and mutually orthogonal, the 32 / F pixels that share a wave have a pattern
     class each.  The row's mean is B + u / 2 and its variance u^2 / 4, both exact, and with ln_eps = 1e-5 and u >= 0.5 the kernel's
     LayerNorm returns EXACTLY e s in fp16 (the eps term moves it by < 2^-12).
       W'q[place(j)] = (a / C) sum_class s_{class, sigma^-1(j)},  W'k[place(j)] = (a / C) sum_class s_{class, j},  every other row zero
     (W' = W gamma; a / C a power of two; place: the identity on the head's first F dims, or F dims drawn among all 64 so that both
     32-channel tiles of q and k carry codes): q = e a onehot(place(sigma(f))), k = e a onehot(place(f)), so a query scores a^2 / 8
     against frame sigma(f) of its own pixel and 0 against every other key of it.  a = 16 / 16 / 20 at C = 64 / 128 / 320 puts every
     other exp2 argument at -46 or below: P is one-hot in fp16 and the fp32 row sum exactly 1.  a = 2 C is the large-score twin (scores
     up to 51 200: infinite without the max subtraction).  W'v: integers in [-2, 2]; beta = 3 gamma w1 (w1 the Walsh row 1: W'q beta =
     W'k beta = 0 exactly, W'v beta an integer) and an integer bias on the value rows: v is an integer with |v| <= 2 C + 6 C + 3 < 2048.
     A key of ANOTHER pixel of the wave (block mask leaked) scores +-a^2 / 8: where the two pixels' signs e agree it ties with the
     selected key and the output is the mean of two different integer rows.
     expected:  out[n, f, p, head] = v[n, sigma_head(f), p, head], from the definitions in fp64, required to be integers.
  B  uniform attention: W'q = W'k = 0 with section A's integer V: within one fp16 ulp of the exact frame mean; and all-zero input rows
     under RANDOM weights: x^ = 0, every row of a pixel is the same, every score equal: out EQUALS fp16(ln_bias) of the value channels.
  L  section A (a = 16 / 16 / 20) at every (B, u) of ``PAIRS``: LayerNorm is the only thing that varies.  (1023, 2) makes a one-pass
     fp32 E[x^2] - mean^2 variance miss at every C.  ``edge_case``: constant rows (variance 0, rstd = 1 / sqrt(eps)) and rows with
     sigma ~ 0.01 about a mean of order 1, held to section R's bound.
  R  random data against launch_census.tfused_ref (fp64) per (sample, head) slice at ``HEAD_BOUND`` and per sample at
     attn_contract.TFUSED_BOUND, three distributions: randn * 1.4 + 0.3, 0.01 * randn, randn + 20.
  D  ``TFLayout``: every operand inside a larger allocation, at address 0 / 16 / 128 mod 256 (the fp32 vectors also at 4); all NaN
     outside x[nsample frames hw][c], wp[3c c], ln_rowsum[3c], ln_bias[3c]; out holds launch_census.OUT_SENTINEL.

``emulate(case, defect)`` is the rounding chain tfused.hip's comments document, in fp32 torch, with named defects; the CPU test shows
every construction sound on it and every defect caught.  Pure torch: works on CPU and GPU; the generators draw on the CPU.
"""
import zlib

import torch

import launch_census as LC
from launch_census import OUT_SENTINEL, alloc, ulp16  # noqa: F401  (re-exported for the tests)
from mvoc_amd._ffi import TFusedDesc
from mvoc_amd.unet import Linear, pack_tfused_weights

H16, F32, F64 = torch.float16, torch.float32, torch.float64
LN_EPS = 1e-5
C_ALL, FRAMES, NSAMPLE = (64, 128, 320), (8, 16, 32), (1, 3)
ADDR = (0, 16, 128)        # gemm_contract.ADDR; 16 is the least alignment of x, wp and out
LN_ADDR = (0, 4, 16, 128)  # the fp32 vectors: 4 is their least alignment
PAIRS = ((0, 2), (0, 0.5), (-1, 2), (512, 2), (1024, 4), (-2048, 8), (8192, 32), (1023, 2))   # (B, u)
# one more for section L: the mean 1024.5 is no fp16 value, so the kernel subtracts 1024 and dm^2 = 0.25 is the whole of the variance
# (a kernel without the correction returns 1 / sqrt(2)).  Exact with the exact mean only: the rounding of mean * rstd (half an fp32 ulp at
# 2049, 2^-13) plus eps' 2e-5 stays inside fp16's half ulp below 1 (2^-12), a mean one fp32 ulp off does not.
DM2_PAIR = (1024, 1)
L_PAIRS = PAIRS + (DM2_PAIR,)
A_SMALL = {64: 16, 128: 16, 320: 20}
DISTRIBUTIONS = ("wide", "small", "offset")   # randn * 1.4 + 0.3 | 0.01 * randn | randn + 20
SCALE_LOG2 = float(torch.tensor(0.125, dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32))  # tfused.hip: 0.125f * log2(e)f

# Section R's bound per (sample, head) slice: (rel-L2, max abs).  Measured on the CPU model (``emulate``) against
# launch_census.tfused_ref (fp64) over every case of section R (every geometry x the three distributions, 666 cases):
#     distribution   worst slice rel-L2                      worst element
#     wide           9.08e-4  (c 320, 8 frames, hw 1)        5.20e-3  (c 128, 8 frames, hw 8)
#     small          8.47e-4  (c 320, 8 frames, hw 1)        3.54e-3
#     offset         8.40e-4  (c 128, 8 frames, hw 1)        5.12e-3
# (section L's inexact edges on the same model: constant rows 1.67e-4 / 4.9e-4, narrow rows 7.77e-4 / 4.73e-3.)  The bound is twice the
# worst figure: the MFMA's summation order and the hardware's rsqrt / exp2 / rcp differ from the model's in the last fp32 bits, which a
# rounding to fp16 turns into a whole fp16 ulp now and then.  It is never taken from the library's output;
# tests/test_tfused_contract_cpu.py: test_model_random_figures recomputes the figure.
MODEL_HEAD_FIGURE = (9.08e-4, 5.20e-3)
HEAD_BOUND = (2 * MODEL_HEAD_FIGURE[0], 2 * MODEL_HEAD_FIGURE[1])


def gen_of(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def pixels_per_block(frames, waves=4):
    return waves * 32 // frames


def hw_list(frames):
    """below, at and above the block edges of both forms (16 / 8 / 4 pixels at 8 / 16 / 32 frames with 4 waves, twice that with 8), and
    three blocks of either form"""
    edges = {pixels_per_block(frames, w) + e for w in (4, 8) for e in (-1, 0, 1)}  # adds 3, 4, 5 at 32 frames
    return tuple(sorted({1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 2 * pixels_per_block(frames) + 1, 2 * pixels_per_block(frames, 8) + 1} | edges))


def geometries():
    """(index, c, frames, hw, nsample): the full product"""
    out = []
    for c in C_ALL:
        for frames in FRAMES:
            for hw in hw_list(frames):
                for ns in NSAMPLE:
                    out.append((len(out), c, frames, hw, ns))
    return out


def _walsh64():
    """Sylvester-Hadamard matrix of order 64: H[i][j] = (-1)^popcount(i & j)"""
    i = torch.arange(64)
    x = i[:, None] & i[None, :]
    par = torch.zeros_like(x)
    for b in range(6):
        par ^= (x >> b) & 1
    return (1 - 2 * par).to(F64)


WALSH = _walsh64()


def patterns(c, frames):
    """[32 / F classes, F, c] of +-1 (fp64): Walsh rows 32 + class F + f, tiled c / 64 times"""
    ppw = 32 // frames
    return WALSH[32:].reshape(ppw, frames, 64).repeat(1, 1, c // 64)


# ---- weights -------------------------------------------------------------------------------------------------------------------------
def _sigma(kind, frames, gen):
    if kind == 0:
        return torch.arange(frames)
    if kind == 1:
        return torch.arange(frames - 1, -1, -1)
    while True:  # a random permutation that is no involution (q and k exchanged select sigma^-1, which must differ)
        s = torch.randperm(frames, generator=gen)
        if not torch.equal(s[s], torch.arange(frames)):
            return s


def _finish(c, frames, w_eff, gamma, beta, bias, **more):
    """the logical Linear and its folded / packed form through the product's own packers"""
    w = (w_eff / gamma[None, :]).to(H16)
    assert torch.equal(w.to(F64) * gamma[None, :], w_eff), "W * gamma is not exact"
    lin = Linear(w, bias.to(H16) if bias is not None else None).fold_layernorm(gamma.to(H16), beta.to(H16), LN_EPS)
    out = {"c": c, "frames": frames, "heads": c // 64, "w": w, "gamma": gamma.to(H16), "beta": beta.to(H16),
           "bias": None if bias is None else bias.to(H16), "lin": lin, "wp": pack_tfused_weights(lin.w_ln, c // 64).reshape(-1).contiguous(),
           "ln_rowsum": lin.ln[0], "ln_bias": lin.ln[1]}
    out.update(more)
    return out


_WEIGHTS = {}


def exact_weights(c, frames, variant, a, zero_qk=False):
    """section A's weights (cached: shared by every geometry and (B, u) of a (c, frames, variant, a)).  variant: which permutation each
    head gets (head + variant mod 3: identity, reversal, random; heads 3 and 4 random) and where the codes sit in the head's 64 dims
    (even: the first F; odd: F drawn among the 64, both tiles used)"""
    key = (c, frames, variant, a, zero_qk)
    if key in _WEIGHTS:
        return _WEIGHTS[key]
    gen = gen_of("W", c, frames, variant)
    heads, pat = c // 64, patterns(c, frames)
    gamma = torch.exp2(torch.randint(-1, 2, (c,), generator=gen).to(F64))
    w1 = WALSH[1].repeat(c // 64)
    beta = 3.0 * gamma * w1
    weff = torch.zeros(3 * c, c, dtype=F64)
    sigmas, places = [], []
    for hd in range(heads):
        sg = _sigma((hd + variant) % 3 if hd < 3 else 2, frames, gen)
        if variant % 2 == 0:
            place = torch.arange(frames)
        else:
            while True:
                place = torch.randperm(64, generator=gen)[:frames]
                if bool((place < 32).any()) and bool((place >= 32).any()):
                    break
        inv = torch.argsort(sg)
        for j in range(frames):
            weff[hd * 64 + int(place[j])] = (a / c) * pat[:, int(inv[j])].sum(0)
            weff[c + hd * 64 + int(place[j])] = (a / c) * pat[:, j].sum(0)
        sigmas.append(sg)
        places.append(place)
    if zero_qk:
        weff[:2 * c] = 0
    weff[2 * c:] = torch.randint(-2, 3, (c, c), generator=gen).to(F64)
    bias = torch.zeros(3 * c, dtype=F64)
    bias[2 * c:] = torch.randint(-3, 4, (c,), generator=gen).to(F64)
    vconst = weff[2 * c:] @ (3.0 * w1) + bias[2 * c:]
    W = _finish(c, frames, weff, gamma, beta, bias, sigmas=sigmas, places=places, veff=weff[2 * c:].clone(), vconst=vconst, a=a)
    # what the folding must have produced, exactly
    assert torch.equal(W["lin"].w_ln[:3 * c].to(F64), weff) and torch.equal(W["ln_bias"][:2 * c].to(F64), torch.zeros(2 * c, dtype=F64))
    assert torch.equal(W["ln_bias"][2 * c:3 * c].to(F64), vconst)
    _WEIGHTS[key] = W
    return W


def random_weights(c, frames, seed_key):
    key = ("R", c, frames, seed_key)
    if key in _WEIGHTS:
        return _WEIGHTS[key]
    gen = gen_of("WR", c, frames, seed_key)
    w = (torch.randn(3 * c, c, generator=gen) / c ** 0.5).to(H16)
    gm = (1 + 0.3 * torch.randn(c, generator=gen)).to(H16)
    bt = (0.3 * torch.randn(c, generator=gen)).to(H16)
    lin = Linear(w).fold_layernorm(gm, bt, LN_EPS)
    W = {"c": c, "frames": frames, "heads": c // 64, "w": w, "gamma": gm, "beta": bt, "bias": None, "lin": lin,
         "wp": pack_tfused_weights(lin.w_ln, c // 64).reshape(-1).contiguous(), "ln_rowsum": lin.ln[0], "ln_bias": lin.ln[1]}
    _WEIGHTS[key] = W
    return W


# ---- cases: {"W": weights, "x": [nsample, frames, hw, c] fp16, "exp": fp64 [nsample, frames, hw, c] or None, "key", "check"} -----------
def _signs(c, frames, hw, ns):
    return (1 - 2 * torch.randint(0, 2, (ns, 1, hw, 1), generator=gen_of("e", c, frames, hw, ns))).to(F64)


def _xhat(c, frames, hw, ns):
    """[ns, F, hw, c] of +-1: e(n, p) * pattern[(p + n) mod ppw, f]"""
    ppw = 32 // frames
    pat = patterns(c, frames)
    cls = (torch.arange(hw)[None, :] + torch.arange(ns)[:, None]) % ppw          # [ns, hw]
    return pat[cls].permute(0, 2, 1, 3) * _signs(c, frames, hw, ns)             # pat[cls]: [ns, hw, F, c]


_BASE = {}


def _exact_base(geo):
    """(x^ = e s, the integer values v, the selected rows) of a geometry: shared by its (B, u) pairs and both a (the value weights and
    the permutations depend on (c, frames, variant) alone); the last geometry is kept"""
    if geo not in _BASE:
        i, c, frames, hw, ns = geo
        W = exact_weights(c, frames, i % 6, A_SMALL[c])
        s = _xhat(c, frames, hw, ns)
        v = s @ W["veff"].t() + W["vconst"]                                      # [ns, F, hw, c] integers
        exp = torch.empty_like(v)
        for hd in range(c // 64):
            exp[..., hd * 64:(hd + 1) * 64] = v[:, W["sigmas"][hd], :, hd * 64:(hd + 1) * 64]
        assert torch.equal(exp, exp.round()) and float(exp.abs().max()) < 2048
        _BASE.clear()
        _BASE[geo] = (s, v, exp)
    return _BASE[geo]


def exact_case(geo, pair, large=False, section="A"):
    i, c, frames, hw, ns = geo
    B, u = pair
    W = exact_weights(c, frames, i % 6, 2 * c if large else A_SMALL[c])
    s, v, exp = _exact_base(geo)
    x = B + u * (1 + s) / 2
    assert torch.equal(x.to(H16).to(F64), x), "a row value is not exact in fp16"
    return {"W": W, "x": x.to(H16), "xhat": s, "exp": exp, "check": "equal", "geo": geo, "pair": pair,
            "key": f"tf{section}_c{c}_f{frames}_hw{hw}_ns{ns}_B{B}_u{u}_{'large' if large else 'small'}"}


def uniform_case(geo):
    """W'q = W'k = 0, section A's integer V: the exact frame mean"""
    i, c, frames, hw, ns = geo
    W = exact_weights(c, frames, i % 6, A_SMALL[c], zero_qk=True)
    s, v, _ = _exact_base(geo)
    exp = v.mean(1, keepdim=True).expand_as(v).contiguous()
    assert torch.equal(exp * frames, (exp * frames).round())
    return {"W": W, "x": (1 + s).to(H16), "xhat": s, "exp": exp, "check": "ulp", "geo": geo, "key": f"tfB_c{c}_f{frames}_hw{hw}_ns{ns}_mean"}


def zero_rows_case(geo):
    """all-zero rows under random weights: out == fp16(ln_bias) of the value channels, every row"""
    i, c, frames, hw, ns = geo
    W = random_weights(c, frames, "zero")
    exp = W["ln_bias"][2 * c:3 * c].to(H16).to(F64).expand(ns, frames, hw, c).contiguous()
    return {"W": W, "x": torch.zeros(ns, frames, hw, c, dtype=H16), "exp": exp, "check": "equal", "geo": geo,
            "key": f"tfB_c{c}_f{frames}_hw{hw}_ns{ns}_zero"}


def random_case(geo, dist):
    i, c, frames, hw, ns = geo
    gen = gen_of("R", c, frames, hw, ns, dist)
    z = torch.randn(ns, frames, hw, c, generator=gen)
    x = {"wide": z * 1.4 + 0.3, "small": 0.01 * z, "offset": z + 20}[dist]
    return {"W": random_weights(c, frames, i % 3), "x": x.to(H16), "exp": None, "check": "random", "geo": geo,
            "key": f"tfR_c{c}_f{frames}_hw{hw}_ns{ns}_{dist}"}


def edge_case(geo, kind):
    """section L's inexact edges, held to section R's bound: 'const' rows (one value per row: variance 0, rstd = 1 / sqrt(eps); the
    kernel's x rstd - mean rstd leaves a residue of order 2^-24 |x| rstd) and 'narrow' rows (sigma 0.01 about a row mean of order 1)"""
    i, c, frames, hw, ns = geo
    gen = gen_of("E", c, frames, hw, ns, kind)
    m = torch.randn(ns, frames, hw, 1, generator=gen) * 1.5
    x = m.expand(ns, frames, hw, c) if kind == "const" else m + 0.01 * torch.randn(ns, frames, hw, c, generator=gen)
    return {"W": random_weights(c, frames, i % 3), "x": x.to(H16).contiguous(), "exp": None, "check": "random", "geo": geo,
            "key": f"tfL_c{c}_f{frames}_hw{hw}_ns{ns}_{kind}"}


def section_geometries(section, c=None):
    """A, B, R: the full product.  L, with eleven cases per geometry: every (c, frames, hw), nsample 1 and 3 in turn"""
    geos = [g for g in geometries() if c is None or g[1] == c]
    if section == "L":
        geos = [g for g in geos if g[0] % 2 == (g[0] // 2) % 2]
    return geos


def section_cases(section, c=None):
    """every case of a section (of one c), in a fixed order; built lazily"""
    for geo in section_geometries(section, c):
        if section == "A":
            yield exact_case(geo, PAIRS[0])
            yield exact_case(geo, PAIRS[0], large=True)
        elif section == "B":
            yield uniform_case(geo)
            yield zero_rows_case(geo)
        elif section == "L":
            for pair in L_PAIRS:
                yield exact_case(geo, pair, section="L")
            yield edge_case(geo, "const")
            yield edge_case(geo, "narrow")
        elif section == "R":
            for dist in DISTRIBUTIONS:
                yield random_case(geo, dist)
        else:
            raise ValueError(section)


EXACT_SECTIONS = ("A", "B", "L")


def fp64_reference(case):
    """launch_census.tfused_ref on a case: [ns, F, hw, c] fp64"""
    i, c, frames, hw, ns = case["geo"]
    W = case["W"]
    d = TFusedDesc()
    d.nsample, d.frames, d.hw, d.c, d.heads, d.ln_eps = ns, frames, hw, c, c // 64, LN_EPS
    dev = case["x"].device
    w = W["w"].to(dev)
    ref = LC.tfused_ref(d, {"x": case["x"].reshape(-1)}, {"w": w, "gamma": W["gamma"].to(dev), "beta": W["beta"].to(dev)})
    assert W["bias"] is None
    return ref.reshape(ns, frames, hw, c)


# ---- checkers ------------------------------------------------------------------------------------------------------------------------
def head_errors(out, ref):
    """(worst rel-L2 over the (sample, head) slices, max abs); out / ref [ns, F, hw, c]"""
    ns, frames, hw, c = ref.shape
    o, r = out.to(F64).cpu().reshape(ns, frames * hw, c // 64, 64), ref.to(F64).cpu().reshape(ns, frames * hw, c // 64, 64)
    num, den = ((o - r) ** 2).sum((1, 3)).sqrt(), (r ** 2).sum((1, 3)).sqrt()
    rel = torch.where(den > 0, num / den.clamp_min(1e-300), num)
    return float(rel.max()), float((o - r).abs().max())


def sample_errors(out, ref):
    ns = ref.shape[0]
    o, r = out.to(F64).cpu().reshape(ns, -1), ref.to(F64).cpu().reshape(ns, -1)
    return float(((o - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-300)).max()), float((o - r).abs().max())


def failure(case, out, ref=None, sample_bound=None):
    """None, or why `out` ([ns, F, hw, c] fp16) misses the case's check"""
    what = case["check"]
    if bool(torch.isnan(out).any()):
        return f"{case['key']}: {int(torch.isnan(out).sum())} NaN"
    if what == "equal":
        exp = case["exp"].to(out.device)
        bad = out.to(F64) != exp
        if bool(bad.any()):
            at = tuple(torch.nonzero(bad)[0].tolist())
            return f"{case['key']}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: {float(out[at])} != {float(exp[at])}"
        return None
    if what == "ulp":
        exp = case["exp"].to(out.device)
        err, bound = (out.to(F64) - exp).abs(), ulp16(exp)
        if not bool((err < bound).all()):
            return f"{case['key']}: worst {float((err / bound).max()):.3g} fp16 ulp from the exact mean"
        return None
    rel, mab = head_errors(out, ref)
    if not (rel < HEAD_BOUND[0] and mab < HEAD_BOUND[1]):
        return f"{case['key']}: worst (sample, head) rel-L2 {rel:.3g} (bound {HEAD_BOUND[0]}), max abs {mab:.3g} (bound {HEAD_BOUND[1]})"
    if sample_bound is not None:
        rel, mab = sample_errors(out, ref)
        if not (rel < sample_bound[0] and mab < sample_bound[1]):
            return f"{case['key']}: worst sample rel-L2 {rel:.3g} (bound {sample_bound[0]}), max abs {mab:.3g} (bound {sample_bound[1]})"
    return None


# ---- section D: the layout -------------------------------------------------------------------------------------------------------------
class TFLayout:
    """mvoc_tfused_desc + operands, each inside an allocation of its own: inputs all NaN outside the described elements, out all
    OUT_SENTINEL.  Addresses mod 256 walk ADDR / LN_ADDR with the case's index."""

    def __init__(self, device, case, shift=0):
        i, c, frames, hw, ns = case["geo"]
        i += shift
        W = case["W"]
        rows = ns * frames * hw
        nan = float("nan")
        self.case, self.rows, self.c = case, rows, c
        self.T = {"x": alloc(rows * c, H16, ADDR[i % 3], device, nan), "wp": alloc(3 * c * c, H16, ADDR[(i + 1) % 3], device, nan),
                  "ln_rowsum": alloc(3 * c, F32, LN_ADDR[i % 4], device, nan), "ln_bias": alloc(3 * c, F32, LN_ADDR[(i + 1) % 4], device, nan),
                  "out": alloc(rows * c, H16, ADDR[(i + 2) % 3], device)}
        self.T["x"].copy_(case["x"].reshape(-1))
        self.T["wp"].copy_(W["wp"])
        self.T["ln_rowsum"].copy_(W["ln_rowsum"][:3 * c])
        self.T["ln_bias"].copy_(W["ln_bias"][:3 * c])
        self.reset_out()
        d = self.d = TFusedDesc()
        d.x, d.wp, d.ln_rowsum, d.ln_bias, d.out = (self.T[n].data_ptr() for n in ("x", "wp", "ln_rowsum", "ln_bias", "out"))
        d.nsample, d.frames, d.hw, d.c, d.heads, d.ln_eps = ns, frames, hw, c, c // 64, LN_EPS
        self.shape = (ns, frames, hw, c)

    def desc(self):
        return LC.copy_desc(self.d)

    def reset_out(self):
        self.T["out"].base_alloc.view(torch.int16).fill_(OUT_SENTINEL)

    def check_poison(self):
        """every element of the input allocations outside the described ones is NaN, none inside is"""
        for name in ("x", "wp", "ln_rowsum", "ln_bias"):
            t = self.T[name]
            b = t.base_alloc
            off = (t.data_ptr() - b.data_ptr()) // b.element_size()
            assert not bool(torch.isnan(t).any()), name
            assert bool(torch.isnan(b[:off]).all()) and bool(torch.isnan(b[off + t.numel():]).all()), name
            assert b.numel() > t.numel()

    def untouched(self):
        return bool((self.T["out"].base_alloc.view(torch.int16) == OUT_SENTINEL).all())

    def check_out(self):
        """every described element written, nothing else: the described elements [ns, F, hw, c]"""
        out = self.T["out"]
        unw, stray = LC.unwritten(out), LC.stray_writes(out)
        assert unw == 0, f"{self.case['key']}: {unw} described elements were never written"
        assert stray == 0, f"{self.case['key']}: {stray} elements outside out[rows][c] were written"
        return out.reshape(self.shape).clone()


# ---- the CPU model ---------------------------------------------------------------------------------------------------------------------
DEFECTS = ("one_pass_variance", "dm2_dropped", "no_max_subtraction", "mask_dropped", "qk_swapped", "row0_q1", "row0_k1", "row0_v1",
           "head_values_swapped", "sigma_ignored")
TILE_OFF = lambda c: (0, c, 32, c + 32, 2 * c, 2 * c + 32)  # noqa: E731  (include/mvoc_hip.h: row0 = 64 head + this[tile])


def unpack(wp, c, defect=None):
    """the [3c, c] matrix the kernel multiplies by, from the stream include/mvoc_hip.h describes: [head][tile q0 k0 q1 k1 v0 v1][k16 step
    s][lane][8], element = W'[row0 + (lane & 31)][16 s + 8 (lane >> 5) + j]"""
    heads = c // 64
    t = wp.reshape(heads, 6, c // 16, 2, 32, 8).clone()        # lane = 32 h + r
    if defect == "qk_swapped":
        t = t[:, [1, 0, 3, 2, 4, 5]]
    if defect in ("row0_q1", "row0_k1", "row0_v1"):
        dst = {"row0_q1": 2, "row0_k1": 3, "row0_v1": 5}[defect]
        t[0, dst] = t[0, dst - 2 if dst < 4 else 4]
    if defect == "head_values_swapped" and heads > 1:
        t[[0, 1], 4:] = t[[1, 0], 4:]
    w = torch.zeros(3 * c, c, dtype=wp.dtype, device=wp.device)
    rows = t.permute(0, 1, 4, 2, 3, 5).reshape(heads, 6, 32, c)  # [head, tile, r, (s, h, j)] = channel 16 s + 8 h + j
    for hd in range(heads):
        for tile, off in enumerate(TILE_OFF(c)):
            w[hd * 64 + off:hd * 64 + off + 32] = rows[hd, tile]
    return w


def _seq_sum_sq(x32):
    """sum of squares over the last dim, one fp32 addition per element in channel order (torch's own reductions accumulate wider)"""
    s = torch.zeros(x32.shape[:-1], dtype=F32, device=x32.device)
    for j in range(x32.shape[-1]):
        s = s + x32[..., j] * x32[..., j]
    return s


def layernorm_model(x, eps=LN_EPS, defect=None, mean_ulps=0):
    """tfused.hip's LayerNorm on fp16 rows [..., c] -> x^ fp16: the fp32 mean; the moments of x - fp16(mean) in packed fp16 with fp32
    accumulation, corrected by dm^2; one fused multiply-add per element rounded once to fp16"""
    c = x.shape[-1]
    x32 = x.to(F32)
    mu = x32.sum(-1) / c
    for _ in range(abs(mean_ulps)):
        mu = torch.nextafter(mu, torch.full_like(mu, float("inf") if mean_ulps > 0 else float("-inf")))
    c16 = mu.to(H16)
    d = (x32 - c16.to(F32)[..., None]).to(H16).to(F32)          # v_pk_add_f16: one rounding of the exact difference
    q2 = (d * d).sum(-1)
    dm = mu - c16.to(F32)
    if defect == "one_pass_variance":
        s2 = (_seq_sum_sq(x32) / c - mu * mu).clamp_min(0)
    elif defect == "dm2_dropped":
        s2 = q2 / c
    else:
        s2 = (q2 / c - dm * dm).clamp_min(0)
    rs = torch.rsqrt(s2 + torch.tensor(eps, dtype=F32))
    nb = -mu * rs
    return (x.to(F64) * rs.to(F64)[..., None] + nb.to(F64)[..., None]).to(H16)


def emulate(case, defect=None, mean_ulps=0):
    """the rounding chain tfused.hip documents -> [ns, F, hw, c] fp16.  Rows are grouped as the kernel's waves group them (32 / F
    consecutive pixels; the rows of a pixel past hw are pixel 0's, as the kernel loads them), which only 'mask_dropped' can see."""
    assert defect is None or defect in DEFECTS, defect
    i, c, frames, hw, ns = case["geo"]
    W, heads, ppw = case["W"], c // 64, 32 // frames
    xh = layernorm_model(case["x"], LN_EPS, defect, mean_ulps)
    w = unpack(W["wp"], c, defect).to(F32)
    qkv = (xh.to(F32) @ w.t() + W["ln_bias"][:3 * c]).to(H16).to(F32)              # q / k / v = fp16(acc + c)
    nw = -(-hw // ppw)
    pix = torch.cat([torch.arange(hw), torch.zeros(nw * ppw - hw, dtype=torch.long)])
    t = qkv[:, :, pix].reshape(ns, frames, nw, ppw, 3, heads, 64).permute(4, 0, 2, 5, 3, 1, 6).reshape(3, ns, nw, heads, 32, 64)
    q, k, v = t[0], t[1], t[2]                                                     # wave row r = pixel-in-wave * F + frame
    if defect == "sigma_ignored":
        q = k
    s = (q @ k.transpose(-1, -2)) * torch.tensor(SCALE_LOG2, dtype=F32)
    if defect != "mask_dropped":
        r = torch.arange(32) // frames
        s = s.masked_fill(r[:, None] != r[None, :], float("-inf"))
    mx = torch.zeros_like(s[..., :1]) if defect == "no_max_subtraction" else s.max(-1, keepdim=True).values
    p = torch.exp2(s - mx)
    inv = 1.0 / p.sum(-1, keepdim=True)                                           # the row sum stays fp32
    o = ((p.to(H16).to(F32) @ v) * inv).to(H16)                                    # P rounded to fp16; O * (1 / sum) rounded to fp16
    o = o.reshape(ns, nw, heads, ppw, frames, 64).permute(0, 4, 1, 3, 2, 5).reshape(ns, frames, nw * ppw, c)
    return o[:, :, :hw].contiguous()


def one_pass_misses(c, pair):
    """does the one-pass fp32 variance of a section A row at (B, u) differ from the exact u^2 / 4?"""
    B, u = pair
    x = (B + u * (1 + patterns(c, 8)[0, 0]) / 2).to(F32)
    var = _seq_sum_sq(x) / c - (x.sum() / c) ** 2
    return float(var) != u * u / 4


def model_figures(cases):
    """worst (sample, head) rel-L2 and max abs of the undamaged model against the fp64 reference over `cases`"""
    rel = mab = 0.0
    for case in cases:
        r, m = head_errors(emulate(case), fp64_reference(case))
        rel, mab = max(rel, r), max(mab, m)
    return rel, mab


# ---- the unfused twin: mvoc_row_stats_f16 -> mvoc_gemm_f16 (LayerNorm folded) -> mvoc_temporal_attn_f16 ---------------------------------
# What that chain can and cannot return on sections A and L, from its documented arithmetic.  mvoc_row_stats_f16 takes the mean and the
# squared deviations in two fp32 passes: the rows' sums (|B + u| C <= 2.7e6 on the grid u / 2) and deviations (+-u / 2) are exact, so
# mean = B + u / 2 and rstd = rsqrt(u^2 / 4 + eps) = (2 / u) (1 - delta), delta = 1 - 1 / sqrt(1 + 4 eps / u^2): 5e-6 at u = 2, 8e-5 at
# u = 0.5.  mvoc_gemm_f16 returns fp16(rstd * (acc - mean * rowsum) + c) with ONE rounding to fp16 at the end.  The raw-row accumulator is
# a sum of multiples of 2^-5 (W'q / W'k entries are multiples of a / C >= 2^-4, W'v entries integers, row values multiples of 0.5) that
# stays below 2^24 units of its grid (8224 * 0.25 * 320 = 6.6e5 on q / k rows, 8224 * 2 * 320 = 5.3e6 on v rows; the a = 2 C twin runs
# at B = 0), and so does mean * rowsum (rowsum is 0 on q / k rows, an integer <= 640 on v rows): acc - mean * rowsum is the exact
# (u / 2) t, with t the integer W' x^.  Hence
#     q, k  = fp16(a (1 - delta)) = a exactly (no constant, delta < 2^-12): the selection is exact, P one-hot as in the fused kernel;
#     v     = fp16(t (1 - delta) + c),  c the integer constant of the channel (beta @ W^T + bias).
# The fused kernel rounds x^ to fp16 first, which absorbs delta; this chain carries delta in fp32 up to the addition of c, so wherever t
# and c cancel (the integer result r = t + c is small against t) the residue delta t is NOT rounded away: r = 0 comes out as -delta t
# (1.5e-4 for t = 30 at u = 2).  Every pair has elements with r = 0 and only (8192, 32) is free of it in fp32 (delta = 2e-8 vanishes in
# 256 + eps).  So the chain is held, per element, to
#     out == r                                          where delta |t| + 2^-22 |t| < 0.24 ulp16(r)   (the residue cannot flip the rounding:
#                                                       below a power of two the fp16 spacing is half of ulp16(r))
#     |out - (r - delta t)| <= ulp16(r - delta t) + 2^-22 |t|   everywhere
# 2^-22 |t| covers the fp32 evaluation: rsqrt to an ulp (2^-23), the product's and the sum's rounding (2^-24 each of values <= |t| + |c|,
# and |c| enters only where the sum does not cancel, where ulp16 dominates).
def twin_failure(case, out):
    """None, or why the unfused chain's `out` misses what its documented arithmetic allows on an exact case"""
    assert case["check"] == "equal" and "pair" in case
    W, (B, u) = case["W"], case["pair"]
    r = case["exp"].to(out.device)
    t = r - W["vconst"].to(out.device)
    delta = 1.0 - 1.0 / (1.0 + 4.0 * LN_EPS / (u * u)) ** 0.5
    fp32 = 2.0 ** -22 * t.abs()
    o = out.to(F64)
    if bool(torch.isnan(o).any()):
        return f"{case['key']}: NaN"
    must_equal = delta * t.abs() + fp32 < 0.24 * ulp16(r)
    bad = must_equal & (o != r)
    if bool(bad.any()):
        at = tuple(torch.nonzero(bad)[0].tolist())
        return f"{case['key']}: {int(bad.sum())} elements differ from the selected integers, first at {at}: {float(o[at])} != {float(r[at])}"
    e = r - delta * t
    bad = ~((o - e).abs() <= ulp16(e) + fp32)
    if bool(bad.any()):
        at = tuple(torch.nonzero(bad)[0].tolist())
        return f"{case['key']}: {int(bad.sum())} elements beyond one fp16 ulp of t (1 - delta) + c, first at {at}: {float(o[at])} against {float(e[at])}"
    return None


def twin_exact_share(case):
    """share of a case's elements on which twin_failure demands the integer itself"""
    W, (B, u) = case["W"], case["pair"]
    r = case["exp"]
    t = r - W["vconst"]
    delta = 1.0 - 1.0 / (1.0 + 4.0 * LN_EPS / (u * u)) ** 0.5
    return float((delta * t.abs() + 2.0 ** -22 * t.abs() < 0.24 * ulp16(r)).double().mean())


def emulate_unfused(case):
    """the unfused chain's documented arithmetic in fp32 torch (two-pass row statistics; fp16(rstd * (acc - mean * rowsum) + c); scores in
    fp32, probabilities against the row maximum rounded to fp16, fp32 sums, one fp16 rounding of the quotient) -> [ns, F, hw, c] fp16"""
    i, c, frames, hw, ns = case["geo"]
    W = case["W"]
    x = case["x"].to(F32)
    mu = x.sum(-1, keepdim=True) / c
    rs = torch.rsqrt(((x - mu) ** 2).sum(-1, keepdim=True) / c + torch.tensor(LN_EPS, dtype=F32))
    acc = x @ W["lin"].w_ln[:3 * c].to(F32).t()
    qkv = (rs * (acc - mu * W["ln_rowsum"][:3 * c]) + W["ln_bias"][:3 * c]).to(H16).to(F32)
    q, k, v = (qkv[..., j * c:(j + 1) * c].reshape(ns, frames, hw, c // 64, 64).permute(0, 2, 3, 1, 4) for j in range(3))
    s = (q @ k.transpose(-1, -2)) * 0.125
    p = torch.exp(s - s.max(-1, keepdim=True).values).to(H16).to(F32)
    o = ((p @ v) / p.sum(-1, keepdim=True)).to(H16)                                # [ns, hw, heads, F, 64]
    return o.permute(0, 3, 1, 2, 4).reshape(ns, frames, hw, c)
