"""Constructors, emulations and checkers of the norm contract tests (helper module, not collected by pytest).

What include/mvoc_hip.h promises about the seven entries of mvoc_amd/csrc/norm.hip (mvoc_groupnorm_f16, _moments_f16, _apply_moments_f16,
_fold_xs_f16, mvoc_layernorm_f16, mvoc_row_stats_f16, mvoc_row_stats_from_moments_f32), as inputs whose statistics are known without
running a reduction:
  * ``balanced_gn`` / ``balanced_rows``: every row of a group holds b + a on half of its channels and b - a on the other half.  Every
    partial sum is an integer below 2^24, so the statistics are EXACT in fp32 under every chunking, lane assignment and merge order.
  * ``random_gn`` / ``random_rows``: randn * 2 + 0.5, held to the project's own bounds PER SAMPLE.
  * ``GnLayout`` / ``fp16 and fp32 poison``: every input inside an allocation whose undescribed elements are NaN, every output inside
    one that holds a sentinel, the workspace 4 KB larger than asked for and NaN all over before every call.
  * ``emulate_*``: the documented fp32 chains in torch, for the CPU test that shows the constructions and their bounds sound and that
    the checkers see planted defects.
Everything is pure torch and works on CPU and GPU.

The bounds (all derived, none measured).  Balanced data, group (a, b), n = R * cpg elements:
  moments  every per-thread, per-chunk and per-slab sum is n' * b and every sum of squares n' * (b^2 + a^2): integers below 2^24 (asserted
           by the constructors), exact in any order.  mean = s / n' = b exactly (a correctly rounded quotient of an exact multiple),
           q - s * mean = n' * a^2 exactly (fused or not: both products are integers below 2^24), every Chan merge has delta == 0 (the
           first one: delta = b against an empty accumulator, weight nb / nt == 1).  Hence (count, mean, M2) == (n, b, n a^2) as fp32
           VALUES whatever the geometry (compared with ==, which only forgives the sign of a zero mean).
  rstd     var = M2 / n = a^2 exactly; a^2 + eps is rounded once (relative 2^-24, halved by the square root: 2^-25), v_rsq_f32 is
           good to 1 ulp (2^-23): 2^-25 + 2^-23 < 2^-22, with a margin of two: 2^-21.
  output   e = (x - b) gamma / sqrt(a^2 + eps) + beta in fp64.  The kernel computes sc = rstd * gamma, sh = beta - mean * sc and
           fma(x, sc, sh) in fp32: rstd (2^-22) and three roundings (2^-24 each) on terms of size |(x - b) gamma rstd|, |b gamma rstd| and
           |beta| -- below 8 * 2^-24 of their sum -- then ONE rounding to fp16, which moves a value by at most half an ulp of the
           binade it lands in, i.e. by at most ulp16(e) when e sits just below a power of two:
               |out - e| < ulp16(e) + 8 * 2^-24 (|(x - b) gamma rstd| + |beta| + |b gamma rstd|).
           The second term matters only where e cancels to nearly zero.
  SiLU     the kernel rounds the pre-activation to fp16 FIRST, and silu has slope up to 1.1: against silu64(e) the error reaches
           1.5 ulp16.  The rounded pre-activation is one of the two fp16 neighbours of e, so `out` is accepted when it is within
           ulp16(s) (+ the fp32 term) of s = silu64(y) for y either neighbour.
  varying  ``balanced_gn(..., slab_rows=k)`` draws the amplitude per slab of k rows.  Sums stay integers (M2 = k cpg sum a_slab^2, still
           bit for bit); var = M2 / n now takes one rounding more (2^-25 in rstd: inside the factor 8 above).  This variant exists
           because on the plain construction ANY set of whole rows of a group has the same mean and variance: a dropped row or a skipped
           slab shows in the count and M2 of mvoc_groupnorm_moments_f16, never in an output.  With amplitudes that differ from slab to
           slab a skipped slab of the producer sums (which have no moments output) moves rstd by (a_slab^2 - var) / (2 nslab var).
"""
import types

import torch

import launch_census as LC
from attn_contract import H16, F32, F64, NAN16, gen_of, poisoned, sentinel, slice_errors  # noqa: F401  (re-exported for the tests)
from launch_census import OUT_SENTINEL, alloc, r16, silu64, ulp16  # noqa: F401

I16, I32 = torch.int16, torch.int32
NAN32 = 0x7FC5A5A5   # fp32 poison and sentinel: a quiet NaN with a payload no kernel produces
WS_EXCESS = 4096     # bytes of workspace behind what mvoc_groupnorm_workspace_bytes asks for
RSTD_REL = 2.0 ** -21
FP32_TERM = 8 * 2.0 ** -24
FOLD_BOUND = 1.5e-3  # test_ops_gpu.py: test_groupnorm_folded_into_xs_linear (rel-L2)
GN_EPS, LN_EPS = 1e-5, 1e-5


# ---- the shapes of the GPU file (tests/test_norm_contract_gpu.py); the CPU file walks the same lists ---------------------------------
GN_CG = ((8, 1, None), (16, 8, None), (64, 8, None), (192, 24, None), (320, 32, None), (512, 256, None), (960, 32, None),
         (1280, 32, None), (1920, 32, 1280), (2048, 32, None), (2064, 8, None), (2560, 32, None))   # (c, G, c1); group 21 straddles 1280
GN_CG_RANDOM = ((24, 8, None), (40, 8, None), (72, 8, None))   # odd cpg: the random class only
GN_NSAMPLE = (1, 3)
GN_FINAL_EXTRA = ((1, 300, 1280, 32), (15, 300, 1280, 32), (16, 300, 1280, 32))  # (nsample, R, c, G): gn_final on 4 / 4 / 1 blocks
GN_WANT_EXTRA = ((2049, 2, 8, 1),)                                                # want = 2048 / nsample -> 0 -> 1
PARTS = (1, 2, 3, 8)
SUMS_CG = ((64, 8, None), (192, 24, None), (320, 32, None), (384, 32, None), (1280, 32, None), (1920, 32, 960))
SUMS_CG_RANDOM = ((40, 8, None),)
SUMS_NSLAB = (1, 2, 3, 4, 5, 15, 16, 17)
SUMS_NSLAB_LONG = (64, 65, 66)
SUMS_LONG_C = (64, 320)
SUMS_LONG_NSAMPLE = (1, 16)
FOLD_CN = ((64, 64), (128, 128), (320, 320))
FOLD_R = (256, 512)
FOLD_NSAMPLE, FOLD_G = 3, 32
LN_C = (8, 16, 64, 320, 504, 512, 520, 1024, 1280, 2040, 2048)
LN_ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 1001)
TILE_N = (8, 255, 256, 257, 320, 321, 640, 1280, 2560)
TILE_W = (256, 320)
TILE_ROWS = (1, 255, 256, 257)


def gn_rows_list(c):
    """the rows_per_sample values of a channel count: below, at and above one pass of the thread-rows, the 4-row unroll and its tail.  RY
    restates gn_geometry only to BUILD the list; nothing is asserted about it."""
    cw = min(c // 8, 256)
    ry = 256 // cw
    rs = (1, ry - 1, ry, ry + 1, 4 * ry - 1, 4 * ry, 4 * ry + 1, 8 * ry + 3, 37, 300)
    return tuple(sorted({r for r in rs if r > 0}))


# ---- constructions -------------------------------------------------------------------------------------------------------------------
def _device_gen(gen, device):
    device = torch.device(device)
    if device.type == "cpu":
        return gen
    return torch.Generator(device=device).manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen)))


def _signs(rows, groups, cpg, gen, device):
    """[rows, groups * cpg] of +-1: per (row, group) a random permutation of cpg / 2 ones and cpg / 2 minus ones"""
    out = torch.empty(rows, groups * cpg, dtype=F32, device=device)
    step = max(1, (1 << 22) // (groups * cpg))
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        rank = torch.rand(n, groups, cpg, generator=gen, device=device).argsort(-1)
        out[r0:r0 + n] = ((rank < cpg // 2).to(F32) * 2 - 1).reshape(n, -1)
    return out


def _distinct_codes(shape, gen):
    """codes of (a, b) in [1, 4] x [-8, 8] (68 of them) on a 2-D grid; neighbours along either axis never share one"""
    k = torch.randint(0, 68, shape, generator=gen)
    for _ in range(1000):
        bad = torch.zeros(shape, dtype=torch.bool)
        bad[:, 1:] |= k[:, 1:] == k[:, :-1]
        bad[1:] |= k[1:] == k[:-1]
        if not bool(bad.any()):
            return k // 17 + 1, k % 17 - 8
        k[bad] = torch.randint(0, 68, (int(bad.sum()),), generator=gen)
    raise RuntimeError("no neighbour-free draw")


def _affine(c, gen, device):
    """gamma / beta as launch_census.build_gn draws them"""
    gamma = (1 + 0.2 * torch.randn(c, generator=gen)).to(H16).to(device)
    beta = (0.2 * torch.randn(c, generator=gen)).to(H16).to(device)
    return gamma, beta


def _gn_case(nsample, R, c, G, c1, x, gamma, beta, eps):
    return types.SimpleNamespace(nsample=nsample, R=R, c=c, G=G, cpg=c // G, c1=c if c1 is None else c1, x=x, gamma=gamma, beta=beta, eps=eps,
                                 balanced=False)


def balanced_gn(nsample, R, c, G, gen, c1=None, *, device="cpu", slab_rows=None, eps=GN_EPS, unit_rows=None):
    """the exact GroupNorm case (module docstring).  x [nsample * R, c] fp16 is the CONCAT (a group that straddles c1 takes its halves from
    the two sources when the layout splits it); a, b integer per (sample, group) -- a per (sample, slab, group) with ``slab_rows``;
    ``moments`` [nsample, G, 3] fp32 and ``var`` [nsample, G] fp64 are the expected statistics.  ``unit_rows``: the most rows any ONE fp32
    sum of the entry covers before a subtraction (the sample for the rows route, 256 for producer sums)."""
    device = torch.device(device)
    cpg = c // G
    assert c % G == 0 and cpg % 2 == 0, "balanced rows need an even number of channels per group"
    nsl = 1 if slab_rows is None else R // slab_rows
    assert slab_rows is None or R % slab_rows == 0
    a, b = _distinct_codes((nsample, G), gen)
    a = a[:, None, :].repeat(1, nsl, 1)
    if nsl > 1:
        a = torch.randint(1, 5, (nsample, nsl, G), generator=gen)
    unit = R if unit_rows is None else min(R, unit_rows)
    # every sum any summation order can meet is an integer below 2^24: one unit's sum of squares, the sample's count and M2
    assert unit * cpg * int((b * b + a.amax(1) ** 2).max()) < 2 ** 24 and R * cpg * 16 < 2 ** 24
    dgen = _device_gen(gen, device)
    x = torch.empty(nsample * R, c, dtype=H16, device=device)
    for s in range(nsample):
        sg = _signs(R, G, cpg, dgen, device)
        a_rows = a[s].to(F32).to(device).repeat_interleave(R // nsl, 0).repeat_interleave(cpg, 1)   # [R, c]
        v = b[s].to(F32).to(device).repeat_interleave(cpg)[None, :] + a_rows * sg
        x[s * R:(s + 1) * R] = v.to(H16)
        assert torch.equal(x[s * R:(s + 1) * R].to(F32), v)
    gamma, beta = _affine(c, gen, device)
    case = _gn_case(nsample, R, c, G, c1, x, gamma, beta, eps)
    a2 = (a.to(F64) ** 2).sum(1)                                                                    # [nsample, G]
    case.balanced, case.a, case.b = True, a, b
    case.var = (a2 / nsl).to(device)
    case.mean = b.to(F64).to(device)
    case.moments = torch.stack([torch.full((nsample, G), float(R * cpg), dtype=F64), b.to(F64), a2 * (R // nsl) * cpg], -1).to(F32).to(device)
    return case


def random_gn(nsample, R, c, G, gen, c1=None, *, device="cpu", eps=GN_EPS):
    dgen = _device_gen(gen, device)
    x = (torch.randn(nsample * R, c, generator=dgen, device=device) * 2 + 0.5).to(H16)
    gamma, beta = _affine(c, gen, device)
    return _gn_case(nsample, R, c, G, c1, x, gamma, beta, eps)


def balanced_rows(rows, c, gen, *, device="cpu", eps=LN_EPS):
    """the exact per-row case: (a, b) per row, b + a on half of the row's channels, b - a on the other half, in a random permutation"""
    device = torch.device(device)
    a = torch.randint(1, 5, (rows,), generator=gen)
    b = torch.randint(-8, 9, (rows,), generator=gen)
    assert c % 2 == 0 and c * 80 < 2 ** 24
    v = b.to(F32).to(device)[:, None] + a.to(F32).to(device)[:, None] * _signs(rows, 1, c, _device_gen(gen, device), device)
    x = v.to(H16)
    assert torch.equal(x.to(F32), v)
    gamma, beta = _affine(c, gen, device)
    return types.SimpleNamespace(rows=rows, c=c, x=x, gamma=gamma, beta=beta, eps=eps, balanced=True, a=a, b=b,
                                 mean=b.to(F64).to(device), var=(a.to(F64) ** 2).to(device))


def random_rows(rows, c, gen, *, device="cpu", eps=LN_EPS):
    x = (torch.randn(rows, c, generator=_device_gen(gen, device), device=device) * 2 + 0.5).to(H16)
    gamma, beta = _affine(c, gen, device)
    return types.SimpleNamespace(rows=rows, c=c, x=x, gamma=gamma, beta=beta, eps=eps, balanced=False)


def tile_counts(n, tile_w):
    return [min(tile_w, n - t * tile_w) for t in range(-(-n // tile_w))]


def balanced_tiles(rows, n, tile_w, ld, gen, *, device="cpu", eps=LN_EPS):
    """{sum, sum of squares} per row and tile of rows with one common mean b and variance a^2 in every tile: [rows, ld, 2] fp32, the unused
    entries NaN.  (count_t b, count_t (b^2 + a^2)) are integers below 2^24; mean == b exactly, M2 / n == a^2 exactly."""
    a = torch.randint(1, 5, (rows,), generator=gen)
    b = torch.randint(-8, 9, (rows,), generator=gen)
    cnt = torch.tensor(tile_counts(n, tile_w), dtype=F64)
    mom = torch.full((rows, ld, 2), float("nan"), dtype=F64)
    mom[:, :len(cnt), 0] = cnt[None] * b[:, None]
    mom[:, :len(cnt), 1] = cnt[None] * (b * b + a * a)[:, None]
    return types.SimpleNamespace(rows=rows, n=n, tile_w=tile_w, ld=ld, eps=eps, mom=mom.to(F32).to(device), balanced=True,
                                 mean=b.to(F64).to(device), var=(a.to(F64) ** 2).to(device))


def random_tiles(rows, n, tile_w, ld, gen, *, device="cpu", eps=LN_EPS):
    """one mean per tile: the moments of random rows, rounded to fp32 as a GEMM epilogue leaves them"""
    x = (torch.randn(rows, n, generator=gen) * 2 + 0.5).to(H16).to(device)
    mom = LC.row_moments64(x, tile_w, ld)
    mom[:, len(tile_counts(n, tile_w)):] = float("nan")
    return types.SimpleNamespace(rows=rows, n=n, tile_w=tile_w, ld=ld, eps=eps, mom=mom.to(F32), balanced=False, x=x)


def split_parts(case, nparts, gen):
    """[nparts, nsample, G, 3] fp32: the sample's rows split over the parts (all means b, all variances a^2: the merge is exact); with more
    than one part, one of them has count 0"""
    assert case.balanced and case.a.shape[1] == 1
    live = max(1, nparts - 1)
    zero = int(torch.randint(0, nparts, (1,), generator=gen)) if nparts > 1 else -1
    cuts = torch.sort(torch.randperm(case.R + live - 1, generator=gen)[:live - 1]).values   # stars and bars: parts of >= 0 rows
    edges = torch.cat([torch.tensor([-1]), cuts, torch.tensor([case.R + live - 1])])
    rows = (edges[1:] - edges[:-1] - 1).tolist()
    assert sum(rows) == case.R
    parts = torch.zeros(nparts, case.nsample, case.G, 3, dtype=F64)
    it = iter(rows)
    for p in range(nparts):
        if p == zero:
            continue
        n = next(it) * case.cpg
        parts[p, ..., 0] = n
        if n:
            parts[p, ..., 1] = case.b.to(F64)
            parts[p, ..., 2] = n * case.a[:, 0].to(F64) ** 2
    return parts.to(F32)


# ---- expectations and checkers -------------------------------------------------------------------------------------------------------
def _sample_blocks(case, budget=1 << 22):
    step = max(1, budget // (case.R * case.c))
    return [(s0, min(case.nsample, s0 + step)) for s0 in range(0, case.nsample, step)]


def _per_channel(t, cpg):
    return t.repeat_interleave(cpg, -1)


def affine_ratio(out, x, mean, var, gamma, beta, eps, silu):
    """worst |out - expected| / bound of the output rule of the module docstring.  x [..., rows, c] fp16, mean / var broadcastable fp64."""
    rstd = 1.0 / torch.sqrt(var + eps)
    g, bt = gamma.to(F64), beta.to(F64)
    dev = (x.to(F64) - mean) * g * rstd
    e = dev + bt
    t32 = FP32_TERM * (dev.abs() + bt.abs() + (mean * g * rstd).abs())
    out = out.to(F64)
    if not silu:
        return float(((out - e).abs() / (ulp16(e) + t32)).max())
    u = ulp16(e)
    ratios = []
    for y in (torch.floor(e / u) * u, torch.ceil(e / u) * u):   # the fp16 neighbours of e (equal when e is an fp16 value)
        s = silu64(y)
        ratios.append((out - s).abs() / (ulp16(s) + t32))
    return float(torch.minimum(*ratios).max())


def gn_out_ratio(case, out, silu, mean=None, var=None):
    """balanced GroupNorm output against the derived bound: worst error / bound over all samples (< 1 passes)"""
    mean = case.mean if mean is None else mean
    var = case.var if var is None else var
    worst = 0.0
    out = out.reshape(case.nsample, case.R, case.c)
    x = case.x.reshape(case.nsample, case.R, case.c)
    for s0, s1 in _sample_blocks(case):
        m = _per_channel(mean[s0:s1], case.cpg)[:, None, :]
        v = _per_channel(var[s0:s1], case.cpg)[:, None, :]
        worst = max(worst, affine_ratio(out[s0:s1], x[s0:s1], m, v, case.gamma, case.beta, case.eps, silu))
    return worst


def gn_random_ratio(case, out, silu):
    """random class: rel-L2 and max-abs PER SAMPLE against fp64, in units of launch_census.GN_BOUND"""
    worst = 0.0
    out = out.reshape(case.nsample, case.R, case.c)
    for s0, s1 in _sample_blocks(case):
        ref = LC.groupnorm64(case.x[s0 * case.R:s1 * case.R], s1 - s0, case.G, case.eps, case.gamma, case.beta, silu)
        rel, mab = slice_errors(out[s0:s1], ref.reshape(s1 - s0, case.R, case.c), (0,))
        worst = max(worst, rel / LC.GN_BOUND[0], mab / LC.GN_BOUND[1])
    return worst


def gn_ratio(case, out, silu):
    return gn_out_ratio(case, out, silu) if case.balanced else gn_random_ratio(case, out, silu)


def assert_moments(mom, case, what):
    mom = mom.reshape(case.nsample, case.G, 3)
    assert not bool(torch.isnan(mom).any()), f"{what}: NaN moments"
    bad = mom != case.moments.to(mom.device)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} moments differ from (R cpg, b, R cpg a^2), first at " \
                                f"{tuple(torch.nonzero(bad)[0].tolist())}: {float(mom[bad][0])} != {float(case.moments.to(mom.device)[bad][0])}"


def rows_ratio(case, out):
    """LayerNorm output: balanced -> the derived bound, random -> launch_census.LN_BOUND with the ROW as the slice (the unit of a row
    statistic; one fp16 rounding is at most 2^-11 = 4.9e-4 relative per element, so a row of any width can meet 1e-3)"""
    out = out.reshape(case.rows, case.c)
    if case.balanced:
        return affine_ratio(out, case.x, case.mean[:, None], case.var[:, None], case.gamma, case.beta, case.eps, False)
    rel, mab = slice_errors(out, LC.layernorm64(case.x, case.gamma, case.beta, case.eps), (0,))
    return max(rel / LC.LN_BOUND[0], mab / LC.LN_BOUND[1])


def stats_ratio(case, st, x=None):
    """[rows, 2] fp32 {mean, rstd}: balanced -> mean == b and rstd within 2^-21 (a wrong mean returns inf); random -> row_stats_ratio"""
    st = st.reshape(-1, 2)
    if not case.balanced:
        return LC.row_stats_ratio(st, case.x if x is None else x, case.eps)
    if bool(torch.isnan(st).any()) or not bool((st[:, 0].to(F64) == case.mean).all()):
        return float("inf")
    rstd = 1.0 / torch.sqrt(case.var + case.eps)
    return float(((st[:, 1].to(F64) - rstd).abs() / (RSTD_REL * rstd)).max())


def fold_ratios(case, w, bias, wk, ck):
    """the unpacked sets of mvoc_groupnorm_fold_xs_f16 on balanced data: wk [nsample, n, k] fp16, ck [nsample, n] fp32.
    weights: r16(W gamma rstd) up to one fp16 neighbour (same rule as an output: one rounding + the fp32 chain); constants: bias +
    sum_k (W beta - W' mean) with W' the weight AS ROUNDED by the kernel (norm.hip says so: the consumer multiplies that one), an fp32 sum of
    2 k + 1 terms in a fixed order: 2^-20 of sum |terms| covers k <= 320 (k 2^-24 would be the worst case of a sequential sum; the kernel
    sums 8 interleaved partials)."""
    rstd = _per_channel(1.0 / torch.sqrt(case.var + case.eps), case.cpg)[:, None, :]     # [nsample, 1, k]
    mean = _per_channel(case.mean, case.cpg)[:, None, :]
    w64, g, bt = w.to(F64)[None], case.gamma.to(F64), case.beta.to(F64)
    ws = w64 * g * rstd
    wr = float(((wk.to(F64) - ws).abs() / (ulp16(ws) + FP32_TERM * ws.abs())).max())
    t1, t2 = w64 * bt, wk.to(F64) * mean
    const = (t1 - t2).sum(-1) + (bias.to(F64) if bias is not None else 0.0)
    mag = (t1.abs() + t2.abs()).sum(-1) + (bias.to(F64).abs() if bias is not None else 0.0)
    cr = float(((ck.to(F64) - const).abs() / (2.0 ** -20 * mag)).max())
    return wr, cr


# ---- the documented fp32 chains, in torch (CPU test) ---------------------------------------------------------------------------------
def _shuffled_sums(v, gen):
    """v [..., m] fp32 -> (sum, sum of squares) over the last dim in a random order"""
    v = v[..., torch.randperm(v.shape[-1], generator=gen)]
    return v.sum(-1), (v * v).sum(-1)


def chan_merge32(acc, nb, mb, m2b):
    """gn_merge of norm.hip on fp32 tensors (a part with count <= 0 is skipped)"""
    n, mean, m2 = acc
    nt = n + nb
    safe = nt.clamp_min(1.0)
    delta = mb - mean
    on = nb > 0
    return (torch.where(on, nt, n), torch.where(on, mean + delta * (nb / safe), mean), torch.where(on, m2 + (m2b + delta * delta * (n * nb / safe)), m2))


def _merge_all(parts, gen):
    acc = tuple(torch.zeros_like(parts[0][0]) for _ in range(3))
    for i in torch.randperm(len(parts), generator=gen).tolist():
        acc = chan_merge32(acc, *parts[i])
    return torch.stack(acc, -1)


def emulate_moments_rows(x, nsample, R, G, gen, *, drop_last=False, take_next=False, chan_shift=0, max_chunks=6):
    """one-pass (count, mean, M2) per chunk of rows, random chunk cuts, random element order inside a chunk, Chan merge in a random chunk
    order: [nsample, G, 3] fp32.  Defects: the sample's last row dropped / the next sample's first row included / every group boundary
    shifted by `chan_shift` channels."""
    c = x.shape[1]
    cpg = c // G
    xs = torch.roll(x, -chan_shift, 1) if chan_shift else x
    out = []
    for s in range(nsample):
        idx = list(range(s * R, (s + 1) * R))
        if drop_last:
            idx = idx[:-1]
        if take_next and s + 1 < nsample:
            idx.append((s + 1) * R)
        idx = torch.tensor(idx)[torch.randperm(len(idx), generator=gen)]
        k = int(torch.randint(1, min(max_chunks, len(idx)) + 1, (1,), generator=gen))
        cuts = [0] + sorted((torch.randperm(len(idx) - 1, generator=gen)[:k - 1] + 1).tolist()) + [len(idx)]
        parts = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            v = xs[idx[r0:r1]].to(F32).reshape(r1 - r0, G, cpg).permute(1, 0, 2).reshape(G, -1)
            sm, sq = _shuffled_sums(v, gen)
            n = torch.full((G,), float(v.shape[1]))
            mean = sm / n
            parts.append((n, mean, (sq - sm * mean).clamp_min(0)))
        out.append(_merge_all(parts, gen))
    return torch.stack(out)


def emulate_moments_sums(sums, G, gen, *, skip=None):
    """gn_fold_slab + merge: sums [nsample, nslab, c, 2] fp32 -> [nsample, G, 3]; `skip`: one slab left out (defect)"""
    ns, nslab, c, _ = sums.shape
    cpg = c // G
    perm = torch.randperm(cpg, generator=gen)
    v = sums.reshape(ns, nslab, G, cpg, 2)[:, :, :, perm]
    sx, sq = v[..., 0].sum(-1), v[..., 1].sum(-1)
    n = torch.full((ns, G), 256.0 * cpg)
    parts = []
    for sl in range(nslab):
        if sl == skip:
            continue
        mean = sx[:, sl] / n
        parts.append((n, mean, (sq[:, sl] - sx[:, sl] * mean).clamp_min(0)))
    return _merge_all(parts, gen)


def finalize32(mom, eps):
    """(mean, rstd) fp32 from (count, mean, M2)"""
    return mom[..., 1], torch.rsqrt(mom[..., 2] / mom[..., 0] + eps)


def emulate_apply(x, mean, rstd, gamma, beta, R, silu, *, gamma_shift=0, sample_shift=0):
    """gn_apply: sc = rstd gamma, sh = beta - mean sc, r16(x sc + sh), SiLU in fp32 on the rounded value, one more rounding.  Defects:
    gamma indexed `gamma_shift` channels off / sample s with the statistics of sample s - sample_shift."""
    ns, G = mean.shape
    c = x.shape[1]
    g = torch.roll(gamma, -gamma_shift) if gamma_shift else gamma
    if sample_shift:
        mean, rstd = torch.roll(mean, sample_shift, 0), torch.roll(rstd, sample_shift, 0)
    sc = _per_channel(rstd, c // G)[:, None, :] * g.to(F32)
    sh = beta.to(F32) - _per_channel(mean, c // G)[:, None, :] * sc
    y = r16(x.to(F32).reshape(ns, R, c) * sc + sh)
    if silu:
        y = y * (1.0 / (1.0 + torch.exp(-y)))
    return y.to(H16).reshape(ns * R, c)


def emulate_row_stats(x, eps, gen):
    """two passes over a row in a random channel order: (mean, rstd) fp32"""
    v = x.to(F32)[:, torch.randperm(x.shape[1], generator=gen)]
    mean = v.sum(1) / x.shape[1]
    d = v - mean[:, None]
    return mean, torch.rsqrt((d * d).sum(1) / x.shape[1] + eps)


def emulate_layernorm(x, gamma, beta, eps, gen):
    mean, rstd = emulate_row_stats(x, eps, gen)
    return ((x.to(F32) - mean[:, None]) * rstd[:, None] * gamma.to(F32) + beta.to(F32)).to(H16)


def emulate_tiles(mom, n, tile_w, eps, *, full_last=False):
    """row_stats_from_moments_kernel: per tile (count, sum / count, q - s mean), merged in tile order: [rows, 2] fp32.  Defect
    `full_last`: the partial last tile counted as tile_w."""
    acc = tuple(torch.zeros(mom.shape[0]) for _ in range(3))
    for t, cnt in enumerate(tile_counts(n, tile_w)):
        nb = torch.full((mom.shape[0],), float(tile_w if full_last else cnt))
        mb = mom[:, t, 0] / nb
        acc = chan_merge32(acc, nb, mb, (mom[:, t, 1] - mom[:, t, 0] * mb).clamp_min(0))
    return torch.stack([acc[1], torch.rsqrt(acc[2] / acc[0] + eps)], 1)


def emulate_fold(w, bias, gamma, beta, mean, rstd, cpg):
    """gn_fold_xs_kernel: W' = r16(W (gamma rstd)), c' = sum (W beta - W' mean) + bias in fp32: ([nsample, n, k] fp16, [nsample, n] fp32)"""
    r, m = _per_channel(rstd, cpg)[:, None, :], _per_channel(mean, cpg)[:, None, :]
    wk = (w.to(F32)[None] * (gamma.to(F32) * r)).to(H16)
    ck = (w.to(F32)[None] * beta.to(F32) - wk.to(F32) * m).sum(-1)
    return wk, ck + (bias.to(F32) if bias is not None else 0.0)


# ---- poisoned allocations and descriptors (GPU test) ---------------------------------------------------------------------------------
def poisoned32(numel, device):
    """fp32 twin of attn_contract.poisoned / sentinel: `numel` elements inside a larger allocation, all NAN32"""
    v = alloc(numel, F32, 128, device)
    v.base_alloc.view(I32).fill_(NAN32)
    return v


def put(v, x):
    v.copy_(x.reshape(-1))
    return v


def intact32(t, keep=0):
    """elements of the allocation around the fp32 view `t` -- and of `t` itself from element `keep` on -- that lost the NAN32 fill"""
    b = t.base_alloc.view(I32)
    off = (t.data_ptr() - t.base_alloc.data_ptr()) // 4
    return int((b[:off] != NAN32).sum()) + int((b[off + keep:] != NAN32).sum())


def check_out16(buf, what):
    """an fp16 output in a sentinel allocation: every element written, none NaN, nothing written around it"""
    unw, nanc, stray = LC.unwritten(buf), int(torch.isnan(buf).sum()), LC.stray_writes(buf)
    assert unw == 0, f"{what}: {unw} output elements were never written"
    assert nanc == 0, f"{what}: {nanc} output elements are NaN (poison -- an undescribed input element or stale workspace -- reached a result)"
    assert stray == 0, f"{what}: {stray} elements outside the output's extent were written"
    return buf


def check_out32(buf, what):
    unw = int((buf.view(I32) == NAN32).sum())
    assert unw == 0, f"{what}: {unw} fp32 output elements were never written"
    assert not bool(torch.isnan(buf).any()), f"{what}: NaN in an fp32 output (poison reached a result)"
    stray = intact32(buf, buf.numel())
    assert stray == 0, f"{what}: {stray} fp32 elements outside the output's extent were written"
    return buf


class GnLayout:
    """mvoc_gn_desc of a case, every operand in an allocation of its own: inputs poisoned (fp16 NaN / NAN32), `out` in sentinels, the
    workspace WS_EXCESS bytes larger than `need` and NAN32 all over.  sums: chan_sums(2) from launch_census.chan_sums64 of each source."""

    def __init__(self, case, device, need, *, silu=0, sums=False, affine=True, out=True):
        from mvoc_amd._ffi import GnDesc
        self.case, self.need = case, need
        c1, c2, rows = case.c1, case.c - case.c1, case.nsample * case.R
        self.T = T = {"x": put(poisoned(rows * c1, device), case.x[:, :c1].contiguous())}
        if c2:
            T["x2"] = put(poisoned(rows * c2, device), case.x[:, c1:].contiguous())
        if affine:
            T["gamma"], T["beta"] = put(poisoned(case.c, device), case.gamma), put(poisoned(case.c, device), case.beta)
        if out:
            T["out"] = sentinel(rows * case.c, device)
        if sums:
            T["chan_sums"] = put(poisoned32(rows // 256 * c1 * 2, device), LC.chan_sums64(case.x[:, :c1]).to(F32))
            if c2:
                T["chan_sums2"] = put(poisoned32(rows // 256 * c2 * 2, device), LC.chan_sums64(case.x[:, c1:]).to(F32))
        T["workspace"] = poisoned32(need // 4 + WS_EXCESS // 4, device)
        d = self.d = GnDesc()
        for name, t in T.items():
            setattr(d, name, t.data_ptr())
        d.workspace_bytes = need
        d.nsample, d.rows_per_sample, d.c, d.c1, d.groups, d.silu, d.eps = case.nsample, case.R, case.c, c1, case.G, silu, case.eps

    def reset(self):
        """before EVERY call: stale workspace contents are NaN, the output holds sentinels"""
        self.T["workspace"].base_alloc.view(I32).fill_(NAN32)
        if "out" in self.T:
            self.T["out"].base_alloc.view(I16).fill_(OUT_SENTINEL)

    def check_workspace(self, what):
        bad = intact32(self.T["workspace"], self.need // 4)
        assert bad == 0, f"{what}: {bad} workspace elements beyond mvoc_groupnorm_workspace_bytes (or in front of the workspace) were written"

    def out(self, what):
        self.check_workspace(what)
        return check_out16(self.T["out"], what).reshape(-1, self.case.c)
