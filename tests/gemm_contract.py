"""Constructors, checkers and runners of the GEMM contract tests (helper module, not collected by pytest).

What include/mvoc_hip.h promises about mvoc_gemm_f16, held on inputs whose answer is known, on every tile id, at the shapes where the
kernels' hand-counted waits, clamped rows and guarded columns can go wrong (one to five K tiles, one row to two blocks and a row, widths
below, at and above a tile's), inside poisoned allocations:
  * ``GemmLayout``: a mvoc_gemm_desc with every operand inside an allocation the test owns.  Every input element the descriptor does
    not describe holds fp16 NaN (fp32 operands: a NaN bit pattern): the lead and tail of each operand, the columns of a / a2 at and
    past c1 / cin - c1 at pitch lda / lda2, the residual's and the row-add's columns at and past cols and their row gaps, whatever
    follows w[n][k], bias[n], ln_rowsum[n], ln_bias[n], ln_stats[m][2], and the whole workspace.  The allocations of out, chan_sums and
    row_moments hold a sentinel.  Conv weights with k > 9 cin: the columns at and past 9 cin are DESCRIBED and hold the zeros
    pack_conv3x3 writes -- the kernels zero the activation side there and still multiply, so NaN would reach the result.
  * ``walk(family)``: the deterministic list of cases of one tile family.  tests/test_gemm_contract_cpu.py asserts what it covers.
  * ``draw``: the constructions A (integers, exact), L (LayerNorm fold with dyadic statistics, exact), C (activations on integer draws,
    held to launch_census.gemm_epilogue's derived bound), D (random against fp64, rel-L2 per 32-row group).
  * ``emulate``: the documented rounding chain in torch fp32 / fp16 with the K axis accumulated in a shuffled order.
  * ``run_case``: one code path for the GPU tests and the CPU test: `kernel` is the library's entry or ``emulate_into``.
Everything is pure torch and works on CPU and GPU; every draw is made on the CPU from a generator seeded by the case's parameters.
"""
import ctypes as C

import torch
import torch.nn.functional as F

import launch_census as LC
from attn_contract import NAN16, _LayoutBase, gen_of
from launch_census import OUT_SENTINEL, alloc, stray_writes, unwritten  # noqa: F401  (re-exported for the tests)
from mvoc_amd._ffi import A_CONV3X3, A_PLAIN, A_TEMPORAL3, ACT_GEGLU, ACT_GELU, ACT_NONE, ACT_SILU, GemmDesc

H16, F32, F64, I16, I32 = torch.float16, torch.float32, torch.float64, torch.int16, torch.int32
LEAD = 128           # poisoned (outputs: sentinel) elements in front of every operand
NAN32 = 0x7FC0A5A5   # the fp32 poison: a quiet NaN with a payload no arithmetic produces
SENT32 = int.from_bytes(bytes([LC.U8_SENTINEL] * 4), "little", signed=True)  # launch_census.fill_sentinel's bytes as one int32
RC = (0, -1, -2, -3)  # the header's return codes
EXACT_LIMIT = 2048

# ---- the walk's lists (the GPU file's docstring and the CPU file's coverage assertions say the same) ---------------------------------
FAMILIES = ("GENERAL", "GLDS", "G8", "AUTO")
TILES = {"GENERAL": (1, 2, 3, 4), "GLDS": (11, 12, 13, 61, 62, 64), "G8": (81, 82), "AUTO": (0,)}
FAMILY_K = {"GENERAL": (32, 64, 96, 128), "GLDS": (64, 128, 192, 256, 320), "G8": (64, 128, 192, 256, 320)}
K_STEP = {"GENERAL": 32, "GLDS": 64, "G8": 64}   # K per tile of the pipelined loop (tiles 61 / 62 / 64 step 32: twice the count)
RING = {"GENERAL": 2, "GLDS": 2, "G8": 2}        # stages of the loop: every K-tile count from 1 to RING + 2 is walked
BN = {1: 128, 2: 160, 3: 64, 4: 64, 11: 128, 12: 160, 13: 64, 61: 128, 62: 160, 64: 160, 81: 256, 82: 320}
NO_GEGLU = (2, 12, 62, 64, 82)
M = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513)
TRIMS = (0, 8, 24)
GENERAL_TAIL_TRIM = 6  # n_store % 4 == 2: the scalar tail of the general epilogue's store
N_CAP = 704
ROWADD_DIV = (1, 64, 100, "m")
ADDR = (0, 16, 128)
MAX_M, MAX_N, MAX_K = 2048, 704, 1728  # the workload cap; the deepest K is the two-source conv, 9 (64 + 128)
CONV_GEO = ((1, 1, 1), (2, 3, 5), (3, 9, 7), (5, 8, 8))           # (nimg, h, w)
TEMPORAL_GEO = ((2, 1, 5), (3, 2, 1), (2, 3, 21), (1, 16, 16))    # (nvid, frames, hw)
SUBPIXEL_SRC = ((1, 16, 16), (2, 16, 16))                         # source grids of 256 and 512 pixels: m = 1024, 2048
SUBPIXEL_N = (32, 256, 288)
CHUNK_MAJOR = (("conv", (2, 23, 23)), ("temporal", (2, 3, 171)))  # m = 1058 and 1026: ragged above 1024
STATS_M, STATS_N = (256, 512), (256, 288, 320, 352)
SECTIONS = ("A", "L", "C", "D")
ACT_NAME = {ACT_NONE: "none", ACT_SILU: "silu", ACT_GELU: "gelu", ACT_GEGLU: "geglu"}
# section D's bounds, rel-L2 per 32-row group, from the tests of the same form in tests/test_ops_gpu.py
D_BOUND = {"plain": 1e-3,    # test_linear_random
           "act": 2e-3,      # test_linear_concat_and_acts (SiLU), test_linear_geglu
           "ln": 2e-3,       # test_linear_layernorm_fold
           "gather": 1.5e-3,  # test_conv3x3, test_tconv3, test_conv3x3_upsample
           "split": 1.5e-3}  # test_split_k


def n_classes(bn):
    """below, at and above a tile's width, and two tiles and a bit (capped)"""
    return tuple(dict.fromkeys((32, bn - 32, bn, bn + 32, min(2 * bn + 32, N_CAP))))


def geglu_n(bn):
    return tuple(dict.fromkeys((64, bn, bn + 64)))


def placements(family):
    """(ldo - cols, ldr / lda pad, a as an inner column block, address mod 256 of the operands, of out)"""
    ldo = (0, 8) if family == "G8" else (0, 8, 4)
    out_addr = ADDR if family == "G8" else ADDR + (8,)
    return tuple((ldo[i % len(ldo)], (0, 16)[(i // 2) % 2], bool((i // 3) % 2), ADDR[i % 3], out_addr[i % len(out_addr)])
                 for i in range(12))


def cols_of(p):
    return p["n"] // 2 if p["act"] == ACT_GEGLU else p["n"] - p["trim"]


def g8_epi(p):
    """launch8's epilogue form (gemm8.hip): 1 plain, 2 LayerNorm fold, 3 GEGLU + LayerNorm fold, 0 everything else"""
    if p["act"] == ACT_NONE:
        return (0 if p["rowadd_div"] else 2) if p["ln"] else 1
    return 3 if (p["act"] == ACT_GEGLU and p["ln"]) else 0


def epilogue_name(p):
    parts = [ACT_NAME[p["act"]]] + [k for k in ("bias", "resid", "ln") if p[k]] + (["rowadd"] if p["rowadd_div"] else [])
    return "+".join(parts)


# (name, fields): the epilogue forms of the K and M loops; LayerNorm forms only where the library folds (tile 0 or >= 11)
EPILOGUES = (("none", {}), ("bias", dict(bias=True)), ("bias+resid", dict(bias=True, resid=True)),
             ("rowadd", dict(bias=True, rowadd_div=64)), ("silu", dict(bias=True, act=ACT_SILU)),
             ("gelu+resid", dict(bias=True, act=ACT_GELU, resid=True)), ("ln", dict(ln=True)),
             ("ln+rowadd", dict(ln=True, rowadd_div=64)), ("silu+rowadd+resid", dict(bias=True, act=ACT_SILU, rowadd_div=64, resid=True)))


def _geometry(p):
    """fills m / k / cin from the gather's geometry"""
    if p["mode"] == "conv":
        nimg, h, w = p["geo"]
        hup, wup = p["up"] if p["up"] else (h, w)
        s = p["stride"]
        if p["pad_mode"] == 0:
            ho, wo = (hup - 1) // s + 1, (wup - 1) // s + 1
        else:
            ho, wo = (hup - 2) // s + 1, (wup - 2) // s + 1
        p["hout"], p["wout"], p["m"] = ho, wo, nimg * ho * wo
        if not p["k"]:
            p["k"] = 4 * p["cin"] if p["upsample"] == 2 else -(-9 * p["cin"] // 32) * 32  # (pack_conv3x3 pads K to a multiple of 32)
    elif p["mode"] == "temporal":
        nvid, frames, hw = p["geo"]
        p["m"], p["k"] = nvid * frames * hw, 3 * p["cin"]
    else:
        p["cin"] = p["k"]
    if not p["c1"]:
        p["c1"] = p["cin"]
    return p


def _case(out, family, tile, **kw):
    i = len(out)
    ldo_pad, pad, inner, addr, out_addr = placements(family)[i % 12]
    p = dict(family=family, tile=tile, i=i, mode="plain", m=0, n=64, k=0, cin=0, c1=0, act=ACT_NONE, bias=False, resid=False,
             rowadd_div=0, ln=False, trim=0, ldo_pad=ldo_pad, ldr_pad=pad, lda_pad=pad, inner=inner, addr=addr, out_addr=out_addr,
             split_k=1, workspace=False, chan_sums=False, row_moments=False, geo=None, stride=1, pad_mode=0, upsample=0, up=None,
             k_order=0, sections=None)
    p.update(kw)
    _geometry(p)
    if p["rowadd_div"] == "m":
        p["rowadd_div"] = p["m"]
    if p["act"] == ACT_GEGLU:
        p["trim"] = 0
    if (family == "G8" or p["tile"] in (81, 82) or p["upsample"] == 2 or p["k_order"]) and p["ldo_pad"] == 4:
        p["ldo_pad"] = 8
    if p["k_order"] or p["upsample"] == 2 or p["tile"] in (81, 82):
        p["out_addr"] = p["addr"]
    out.append(p)
    return p


def _tile_walk(out, family, tile, ks, bn, fold):
    """the cases of one tile; the other options cycle with the case index"""
    def add(**kw):
        return _case(out, family, tile, **kw)

    ns = n_classes(bn)
    epis = [e for e in EPILOGUES if fold or "ln" not in e[1]]
    g8 = tile in (81, 82)
    # 1. every K with every epilogue form
    for k in ks:
        for name, e in epis:
            if e.get("ln") and k % 64:
                continue
            add(m=M[(3 * len(out) + 1) % len(M)], n=ns[len(out) % len(ns)], k=k, **e)
    # 2. every M with and without bias + residual (section A sees every M)
    for m in M:
        for e in ({}, dict(bias=True, resid=True)):
            add(m=m, n=ns[len(out) % len(ns)], k=ks[len(out) % len(ks)], **e)
    # 3. every N class with every n_store trim, with and without residual
    for n in ns:
        for t in TRIMS + ((GENERAL_TAIL_TRIM,) if family == "GENERAL" else ()):
            add(m=M[(5 * len(out) + 2) % len(M)], n=n, k=ks[len(out) % len(ks)], bias=True, resid=bool(len(out) % 2), trim=t,
                rowadd_div=(64 if len(out) % 3 == 0 else 0))
    # 4. row-add divisors; one 256-row tile over five row-add rows (m = 513, div 65: rows 256 .. 511 lie on row-add rows 3 .. 7)
    for div in ROWADD_DIV:
        if g8 and div == 1:
            continue  # section E: refused on a forced 81 / 82; the automatic family runs it
        add(m=257, n=ns[len(out) % len(ns)], k=ks[-1], bias=True, rowadd_div=div, resid=bool(len(out) % 2))
    add(m=513, n=bn, k=ks[0], bias=True, rowadd_div=65, five_rows=True)
    if g8:
        add(m=513, n=bn + 32, k=ks[1], bias=True, rowadd_div=100, resid=True)
    # 5. GEGLU
    if tile not in NO_GEGLU:
        for n in geglu_n(bn):
            for e in (dict(bias=True), dict(bias=True, resid=True)) + ((dict(ln=True),) if fold else ()):
                add(m=M[(7 * len(out)) % len(M)], n=n, k=ks[len(out) % len(ks)] if not e.get("ln") else 64 * (1 + len(out) % 3),
                    act=ACT_GEGLU, **e)
    # 6. gathers
    cin = 8 if family == "GENERAL" else 64
    for geo in CONV_GEO:
        nimg, h, w = geo
        add(mode="conv", geo=geo, cin=cin, n=ns[len(out) % len(ns)], bias=True, resid=bool(len(out) % 2))
        if h % 2 and h > 1:
            add(mode="conv", geo=geo, cin=cin, n=ns[len(out) % len(ns)], bias=True, stride=2)
        if h > 1:
            add(mode="conv", geo=geo, cin=cin, n=ns[len(out) % len(ns)], bias=True, stride=2, pad_mode=1, rowadd_div=64)
    add(mode="conv", geo=(3, 8, 8), cin=cin, n=ns[len(out) % len(ns)], bias=True, upsample=1, up=(11, 7))
    add(mode="conv", geo=(2, 8, 8), cin=cin, n=ns[len(out) % len(ns)], bias=True, upsample=1, up=(16, 16))
    c1, c2 = (8, 24) if family == "GENERAL" else (64, 128)
    add(mode="conv", geo=(3, 9, 7), cin=c1 + c2, c1=c1, n=ns[len(out) % len(ns)], bias=True, resid=True)
    if g8:
        add(mode="conv", geo=(5, 8, 8), cin=c1 + c2, c1=c1, n=bn, bias=True, rowadd_div=64)
    else:
        add(mode="conv", geo=(2, 3, 5), cin=c1 + c2, c1=c1, n=bn, bias=True, rowadd_div=15)
    add(mode="plain", m=129, n=ns[len(out) % len(ns)], k=c1 + c2 if family != "GENERAL" else 96, c1=c1 if family != "GENERAL" else 32,
        bias=True)
    if family == "GENERAL":
        add(mode="conv", geo=(3, 9, 7), cin=8, k=96, n=ns[len(out) % len(ns)], bias=True)  # the padded K of the small-channel convs
    for geo in TEMPORAL_GEO:
        add(mode="temporal", geo=geo, cin=max(cin, 32), n=ns[len(out) % len(ns)], bias=True, resid=bool(len(out) % 2))
    add(mode="temporal", geo=(2, 3, 21), cin=c1 + c2, c1=c1, n=bn, bias=True)
    # 7. forced split-K inside an exactly sized workspace (direct-to-LDS and eight-phase tiles)
    if family in ("GLDS", "G8"):
        for split in (2, 4):
            for mult in (1, 2):
                add(m=(257, 129, 512, 256)[len(out) % 4], n=ns[len(out) % len(ns)], k=64 * split * mult, bias=True, split_k=split,
                    workspace=True, resid=bool(mult - 1), rowadd_div=(64 if split == 4 else 0))
        add(m=256, n=bn, k=128, bias=True, split_k=2, workspace=True, chan_sums=True, row_moments=True)  # chan_sums via the reduce
        add(m=129, n=bn, k=128, bias=True, act=ACT_SILU, split_k=2, workspace=True)
    # 8. statistics requests on the eight-phase tiles, honoured and not
    if g8:
        for m in STATS_M:
            for n in STATS_N:
                add(m=m, n=n, k=ks[len(out) % len(ks)], bias=True, resid=bool(len(out) % 2), chan_sums=True, row_moments=True,
                    rowadd_div=(64 if len(out) % 3 == 0 else 0))
        add(m=257, n=256, k=128, bias=True, chan_sums=True, row_moments=True)
        add(m=256, n=288, k=64, bias=True, act=ACT_SILU, chan_sums=True, row_moments=True)
        add(m=512, n=320, k=128, bias=True, trim=8, chan_sums=True, row_moments=True)
        add(m=256, n=320, k=192, ln=True, chan_sums=True, row_moments=True)
    # 9. the forms of the eight-phase tiles alone: sub-pixel upsample (81), chunk-major K (82)
    if tile == 81:
        for src in SUBPIXEL_SRC:
            for n in SUBPIXEL_N:
                add(mode="conv", geo=src, cin=64, n=n, bias=True, upsample=2, up=(2 * src[1], 2 * src[2]), sections=("A",))
    if tile == 82:
        for mode, geo in CHUNK_MAJOR:
            for cin_ in (64, 128):
                for e in (dict(bias=True), dict(bias=True, resid=True, rowadd_div=(529 if mode == "conv" else 513))):
                    add(mode=mode, geo=geo, cin=cin_, n=320, k_order=1, **e)


def walk(family):
    """the cases of one family.  AUTO: the cases of tiles 3, 13 and 81 (K = 32 .. 320, every M, the widths about 64 and 256, every
    gather, the sub-pixel form, the forced splits, the statistics requests) and the chunk-major cases of tile 82 with tile = 0 (the
    route mvoc_amd.ops takes to both forms), a row-add divisor below 64 at a shape the eight-phase tiles would otherwise take, and
    one case the automatic policy splits (see auto_split_case)."""
    out = []
    if family == "AUTO":
        for fam, tile in (("GENERAL", 3), ("GLDS", 13), ("G8", 81), ("G8", 82)):
            sub = []
            _tile_walk(sub, fam, tile, FAMILY_K[fam], BN[tile], fam != "GENERAL")
            for p in sub:
                if tile == 82 and not p["k_order"]:
                    continue
                out.append(dict(p, family="AUTO", tile=0, i=len(out), via=fam))
        _case(out, "AUTO", 0, m=1025, n=256, k=256, bias=True, rowadd_div=1, via="G8")
        out.append(dict(auto_split_case(), i=len(out)))
        return out
    for tile in TILES[family]:
        _tile_walk(out, family, tile, FAMILY_K[family], BN[tile], family != "GENERAL")
    return out


def auto_split_case():
    """the automatic split-K policy, chosen from gemm.hip: tile 0, m <= 2048 and k < 2048 take tile 13; with a workspace and
    split_k = 0 its 5 x 1 = 5 blocks (< 384) are split while k % (128 sk) == 0 and k / (2 sk) >= 512: k = 1024 gives two slices.
    run_case asserts that both slabs of the exactly sized workspace were written."""
    out = []
    return _case(out, "AUTO", 0, m=513, n=64, k=1024, bias=True, resid=True, split_k=0, workspace=True, expect_split=2, via="GLDS")


def section_of(p):
    if p["act"] != ACT_NONE:
        return "C"
    return "L" if p["ln"] else "A"


def section_cases(section, family, tile=None):
    w = [p for p in walk(family) if tile is None or p["tile"] == tile]
    if section == "D":
        # random data: the K loop, GEGLU and the gathers (every third of the rest); the sub-pixel form's summed weights are rounded
        # once more than the logical conv's (its packed weights are not the logical ones): exact section only
        return [p for p in w if (p["sections"] is None or "D" in p["sections"]) and not p["chan_sums"] and not p["row_moments"]
                and (p["mode"] != "plain" or p["act"] == ACT_GEGLU or p["i"] % 3 == 0)]
    return [p for p in w if section_of(p) == section and (p["sections"] is None or section in p["sections"])]


def case_key(section, p):
    return f"{section}_{p['family']}_t{p['tile']}_{p['i']}"


def describe(section, p):
    return (f"{case_key(section, p)} {p['mode']} m {p['m']} n {p['n']} k {p['k']} cin {p['cin']} c1 {p['c1']} {epilogue_name(p)} div "
            f"{p['rowadd_div']} trim {p['trim']} split {p['split_k']} geo {p['geo']} stride {p['stride']} pad {p['pad_mode']} up "
            f"{p['upsample']}{p['up']} ko {p['k_order']} ldo +{p['ldo_pad']} ld +{p['ldr_pad']} inner {p['inner']} addr {p['addr']}/"
            f"{p['out_addr']}")


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
def _region(numel, dtype, addr_mod, device, fill, lead=LEAD):
    es = 2 if dtype == H16 else 4
    v = alloc(lead + numel, dtype, addr_mod, device)
    v.base_alloc.view(I16 if dtype == H16 else I32).fill_(fill)
    t = v[lead:]
    t.base_alloc = v.base_alloc
    assert (t.data_ptr() - lead * es) % 256 == addr_mod
    return t


def _ceil4(x):
    return -(-x // 4) * 4


class GemmLayout(_LayoutBase):
    """mvoc_gemm_desc + operands, an allocation each.  a [rows_a][c1] at pitch lda (inner: a column block of a matrix 64 wider),
    a2 likewise, w [w_rows][k], bias [n], rowadd [ceil(m / div)][cols] at pitch ld_rowadd, resid [m][cols] at pitch ldr, the fp32
    vectors, out [m][cols] at pitch ldo, chan_sums [m / 256][cols][2], row_moments [m][ld][2], workspace split * m * n fp32."""

    def __init__(self, device, p):
        self.device = dev = torch.device(device)
        self.p = p
        m, n, k = p["m"], p["n"], p["k"]
        self.m, self.n, self.k = m, n, k
        self.cols = cols = cols_of(p)
        c1, c2 = p["c1"], p["cin"] - p["c1"]
        if p["mode"] == "conv":
            self.rows_a = p["geo"][0] * p["geo"][1] * p["geo"][2]
        else:
            self.rows_a = m
        wide = 64 if p["inner"] else 0
        self.lda, self.lda2 = c1 + p["lda_pad"] + wide, c2 + p["lda_pad"] + wide
        self.a_lead = LEAD + (32 if p["inner"] else 0)
        self.ldo, self.ldr = _ceil4(cols) + p["ldo_pad"], _ceil4(cols) + p["ldr_pad"]
        self.ld_rowadd = _ceil4(cols) + p["ldr_pad"]
        self.ra_rows = -(-m // p["rowadd_div"]) if p["rowadd_div"] else 0
        self.w_rows = 4 * n if p["upsample"] == 2 else n
        self.rm_ld = -(-n // 256) + 1
        self.split = p["split_k"] if p["split_k"] > 1 else p.get("expect_split", 0)
        self.shapes = {"a": ((self.rows_a, c1), (self.lda, 1)), "w": ((self.w_rows, k), (k, 1)), "out": ((m, cols), (self.ldo, 1))}
        self.dtypes = {"a": H16, "w": H16, "out": H16}
        if c2:
            self.shapes["a2"], self.dtypes["a2"] = ((self.rows_a, c2), (self.lda2, 1)), H16
        if p["bias"]:
            self.shapes["bias"], self.dtypes["bias"] = ((n,), (1,)), H16
        if p["rowadd_div"]:
            self.shapes["rowadd"], self.dtypes["rowadd"] = ((self.ra_rows, cols), (self.ld_rowadd, 1)), H16
        if p["resid"]:
            self.shapes["resid"], self.dtypes["resid"] = ((m, cols), (self.ldr, 1)), H16
        if p["ln"]:
            for name, shape in (("ln_rowsum", (n,)), ("ln_bias", (n,)), ("ln_stats", (m, 2))):
                self.shapes[name], self.dtypes[name] = (shape, (2, 1) if len(shape) == 2 else (1,)), F32
        if p["workspace"]:
            self.shapes["workspace"], self.dtypes["workspace"] = ((self.split * m * n,), (1,)), F32
        if p["chan_sums"]:
            self.shapes["chan_sums"], self.dtypes["chan_sums"] = ((max(m // 256, 1), cols, 2), (cols * 2, 2, 1)), F32
        if p["row_moments"]:
            self.shapes["row_moments"], self.dtypes["row_moments"] = ((m, self.rm_ld, 2), (self.rm_ld * 2, 2, 1)), F32
        self.outputs = tuple(nm for nm in ("out", "chan_sums", "row_moments") if nm in self.shapes)
        self.inputs = tuple(nm for nm in self.shapes if nm not in self.outputs)
        self.T, self.views = {}, {}
        for name, (shape, strides) in self.shapes.items():
            dt = self.dtypes[name]
            numel = sum((s - 1) * st for s, st in zip(shape, strides)) + 1
            if name in self.outputs:
                fill = OUT_SENTINEL if dt == H16 else SENT32
                addr = p["out_addr"] if name == "out" else p["addr"]
            else:
                fill, addr = (NAN16 if dt == H16 else NAN32), p["addr"]
            lead = self.a_lead if name in ("a", "a2") else LEAD
            self.T[name] = _region(numel, dt, addr, dev, fill, lead)
            self.views[name] = (lambda b, shape=shape, strides=strides: b.as_strided(shape, strides, b.storage_offset()))

    # -- the descriptor
    def desc(self):
        p, d = self.p, GemmDesc()
        for name in ("a", "a2", "w", "out", "bias", "rowadd", "resid", "ln_rowsum", "ln_bias", "ln_stats", "chan_sums", "row_moments",
                     "workspace"):
            setattr(d, name, self.T[name].data_ptr() if name in self.T else None)
        d.m, d.n, d.k = self.m, self.n, self.k
        d.n_store = 0 if (p["act"] == ACT_GEGLU or (p["trim"] == 0 and p["i"] % 2)) else self.cols
        d.ldo, d.ldr = self.ldo, (self.ldr if p["resid"] else 0)
        d.ld_rowadd, d.rowadd_div = (self.ld_rowadd, p["rowadd_div"]) if p["rowadd_div"] else (0, 1)
        d.a_mode = {"plain": A_PLAIN, "conv": A_CONV3X3, "temporal": A_TEMPORAL3}[p["mode"]]
        d.lda, d.lda2, d.c1, d.cin = self.lda, (self.lda2 if "a2" in self.T else 0), p["c1"], p["cin"]
        if p["mode"] == "conv":
            d.nimg, d.hsrc, d.wsrc = p["geo"]
            d.hout, d.wout, d.stride, d.upsample, d.pad_mode = p["hout"], p["wout"], p["stride"], p["upsample"], p["pad_mode"]
            d.hup, d.wup = p["up"] if p["up"] else (0, 0)
        elif p["mode"] == "temporal":
            d.frames, d.hw = p["geo"][1], p["geo"][2]
        d.act, d.tile, d.split_k = p["act"], p["tile"], p["split_k"]
        d.workspace_bytes = self.split * self.m * self.n * 4 if p["workspace"] else 0
        d.ln_eps, d.row_moments_ld, d.k_order = 1e-5, (self.rm_ld if p["row_moments"] else 0), p["k_order"]
        return d

    # -- poison bookkeeping (an allocation per operand, as xs_contract.XsLayout)
    def described(self, name):
        buf = self.T[name]
        mask = torch.zeros(buf.base_alloc.numel(), dtype=torch.bool, device=self.device)
        self.views[name](mask[buf.storage_offset():]).fill_(True)
        return mask

    def _raw(self, name):
        b = self.T[name].base_alloc
        return b.view(I16 if b.dtype == H16 else I32)

    def check_poison(self):
        """no described input element is NaN, every other element of the input allocations is poison; the output allocations hold
        their sentinel; the workspace is poison throughout"""
        for name in self.inputs:
            mask, raw = self.described(name), self._raw(name)
            poison = NAN16 if self.dtypes[name] == H16 else NAN32
            if name == "workspace":
                assert bool((raw == poison).all()), "workspace: not poisoned throughout"
                continue
            assert bool((raw[~mask] == poison).all()), f"{name}: an undescribed element lost its poison"
            assert int((~mask).sum()) >= LEAD + LC.SLACK_BYTES // 4
            assert not bool(torch.isnan(self.T[name].base_alloc[mask]).any()), f"{name}: a described element is NaN"
        for name in self.outputs:
            sent = OUT_SENTINEL if self.dtypes[name] == H16 else SENT32
            assert bool((self._raw(name) == sent).all()), f"{name}: the allocation does not hold its sentinel"

    def untouched(self, name):
        """the whole allocation of an output still holds its sentinel"""
        return bool((self._raw(name) == (OUT_SENTINEL if self.dtypes[name] == H16 else SENT32)).all())

    def check_out(self, name="out"):
        vals = super().check_out(name)
        bad = int((~torch.isfinite(vals)).sum())
        assert bad == 0, f"{name}: {bad} described elements are not finite (a poisoned, undescribed input element reached a result)"
        return vals

    def check_f32_out(self, name, shape):
        """an fp32 output: every element of [shape] (a leading block of the operand's view) written and finite, nothing else of the
        allocation touched.  Returns the block."""
        buf, raw = self.T[name], self._raw(name)
        mask = torch.zeros(raw.numel(), dtype=torch.bool, device=self.device)
        sl = tuple(slice(0, s) for s in shape)
        self.views[name](mask[buf.storage_offset():])[sl].fill_(True)
        stray = int((raw[~mask] != SENT32).sum())
        assert stray == 0, f"{name}: {stray} elements outside the described extent were written"
        vals = self.views[name](buf)[sl].contiguous()
        unw = int((vals.view(I32) == SENT32).sum())
        assert unw == 0, f"{name}: {unw} described elements were never written"
        assert bool(torch.isfinite(vals).all()), f"{name}: a described element is not finite"
        return vals

    def check_workspace(self):
        """nothing outside the split * m * n floats of the workspace changed; returns how many of them were written"""
        if "workspace" not in self.T:
            return 0
        mask, raw = self.described("workspace"), self._raw("workspace")
        stray = int((raw[~mask] != NAN32).sum())
        assert stray == 0, f"workspace: {stray} elements outside split_k * m * n * 4 bytes were written"
        return int((raw[mask] != NAN32).sum())

    # -- filling
    def fill(self, case):
        for name in ("a", "a2", "rowadd", "resid"):
            if name in self.T:
                self.put(name, case[name])
        for name in ("w", "bias"):
            if name in self.T:
                self.put(name, case["packed"][name])
        for name in ("ln_rowsum", "ln_bias"):
            if name in self.T:
                self.views[name](self.T[name]).copy_(case["packed"][name].to(self.device, F32))
        if "ln_stats" in self.T:
            self.views["ln_stats"](self.T["ln_stats"]).copy_(case["ln_stats"].to(self.device, F32))
        self.logical = {k: v.to(self.device) for k, v in case["logical"].items()}

    def ref_buffers(self):
        """what launch_census.gemm_ref reads: each strided operand as rows of its full pitch (the last row's padding lies in the
        allocation's slack)"""
        bufs = {}
        for name, rows, ld in (("a", self.rows_a, self.lda), ("a2", self.rows_a, self.lda2), ("resid", self.m, self.ldr),
                               ("rowadd", self.ra_rows, self.ld_rowadd)):
            if name in self.T:
                t = self.T[name]
                bufs[name] = t.base_alloc[t.storage_offset():t.storage_offset() + rows * ld]
        if "ln_stats" in self.T:
            bufs["ln_stats"] = self.T["ln_stats"]
        return bufs

    def reference(self):
        """launch_census.gemm_ref on the layout's own buffers and the case's logical weights: (fp64 stored values, bound) [m, cols]"""
        d = self.desc()
        ref, bound = LC.gemm_ref(d, self.ref_buffers(), self.logical)
        return ref[:, :self.cols], bound[:, :self.cols]


# ---- constructions -------------------------------------------------------------------------------------------------------------------
def _ints(gen, lo, hi, shape, dtype=H16):
    return LC._ints(shape, gen, "cpu", lo, hi, dtype)


def geglu_perm(n):
    """mvoc_amd.unet.pack_geglu's row order: packed row -> logical row"""
    idx = torch.arange(n)
    return ((idx // 32) % 2) * (n // 2) + (idx // 64) * 32 + idx % 32


def pack_weights(p, wl):
    """the logical weights in the form `w` holds, through the product's packers"""
    from mvoc_amd.unet import pack_conv3x3, pack_conv3x3_subpixel, pack_tconv
    if p["mode"] == "plain":
        return wl[geglu_perm(p["n"])].contiguous() if p["act"] == ACT_GEGLU else wl
    if p["mode"] == "conv":
        if p["upsample"] == 2:
            return pack_conv3x3_subpixel(wl)
        wp = pack_conv3x3(wl)
        if p["k"] > wp.shape[1]:  # the padded K of the small-channel convs: zeros, as the packer writes below a multiple of 32
            wp = F.pad(wp, (0, p["k"] - wp.shape[1]))
        return LC.chunk_major_ref(wp, 9) if p["k_order"] else wp
    wp = pack_tconv(wl)
    return LC.chunk_major_ref(wp, 3) if p["k_order"] else wp


def _w_shape(p):
    return {"plain": (p["n"], p["k"]), "conv": (p["n"], p["cin"], 3, 3), "temporal": (p["n"], p["cin"], 3, 1, 1)}[p["mode"]]


def draw(section, p):
    """the operands of a case, drawn on the CPU from a generator seeded by the case's own parameters"""
    gen = gen_of(section, sorted((k, str(v)) for k, v in p.items()))
    m, n, cols = p["m"], p["n"], cols_of(p)
    rows_a = p["geo"][0] * p["geo"][1] * p["geo"][2] if p["mode"] == "conv" else m
    c1, c2 = p["c1"], p["cin"] - p["c1"]
    ra_rows = -(-m // p["rowadd_div"]) if p["rowadd_div"] else 0
    ktot = p["cin"] * {"plain": 1, "conv": 9, "temporal": 3}[p["mode"]]
    if section != "D":
        a, a2 = _ints(gen, -1, 1, (rows_a, c1)), _ints(gen, -1, 1, (rows_a, c2))
        wl = LC._ints_sparse(_w_shape(p), gen, "cpu")
        bias, ra, r = _ints(gen, -4, 4, (n,)), _ints(gen, -4, 4, (ra_rows, cols)), _ints(gen, -4, 4, (m, cols))
        ln_rowsum, ln_bias = wl.reshape(n, -1).double().sum(1).to(F32), _ints(gen, -4, 4, (n,), F32)
        ln_stats = torch.stack([_ints(gen, -2, 2, (m,), F32) * 0.5, torch.exp2(-_ints(gen, 0, 2, (m,), F32))], 1)  # dyadic (build_gemm)
    else:
        a, a2 = torch.randn(rows_a, c1, generator=gen).to(H16), torch.randn(rows_a, c2, generator=gen).to(H16)
        wl = (torch.randn(_w_shape(p), generator=gen) / ktot ** 0.5).to(H16)
        bias = (0.5 * torch.randn(n, generator=gen)).to(H16)
        ra, r = (0.5 * torch.randn(ra_rows, cols, generator=gen)).to(H16), (0.5 * torch.randn(m, cols, generator=gen)).to(H16)
        ln_rowsum, ln_bias = wl.reshape(n, -1).double().sum(1).to(F32), (0.5 * torch.randn(n, generator=gen)).to(F32)
        x = torch.cat([a, a2], 1).double()  # the rows' own statistics (plain mode only), as mvoc_row_stats_f16 hands them over
        mean, rstd = LC.row_stats64(x, 1e-5)
        ln_stats = torch.stack([mean, rstd], 1).to(F32)
    logical = {"w": wl, "bias": bias}
    packed = {"w": pack_weights(p, wl), "bias": bias}
    if p["ln"]:
        logical.update(ln_rowsum=ln_rowsum, ln_bias=ln_bias)
        packed.update(ln_rowsum=ln_rowsum, ln_bias=ln_bias)
    if p["act"] == ACT_GEGLU:
        perm = geglu_perm(n)
        packed = {k: (v if k == "w" else v[perm].contiguous()) for k, v in packed.items()}
    assert tuple(packed["w"].shape) == ((4 * n if p["upsample"] == 2 else n), p["k"]), (packed["w"].shape, p["k"])
    return {"a": a, "a2": a2, "rowadd": ra, "resid": r, "ln_stats": ln_stats, "logical": logical, "packed": packed}


# ---- the documented rounding chain ---------------------------------------------------------------------------------------------------
def _r16(x):
    return x.to(H16).to(F32)


def gather(p, a, a2):
    """A(m, k) of include/mvoc_hip.h, tap-major: [m, ntaps * cin]"""
    x = torch.cat([a, a2], 1) if a2 is not None and a2.shape[1] else a
    cin = x.shape[1]
    if p["mode"] == "plain":
        return x
    if p["mode"] == "temporal":
        nvid, frames, hw = p["geo"]
        xp = F.pad(x.reshape(nvid, frames, hw, cin), (0, 0, 0, 0, 1, 1))
        return torch.cat([xp[:, t:t + frames].reshape(-1, cin) for t in range(3)], 1)
    nimg, h, w = p["geo"]
    x = x.reshape(nimg, h, w, cin)
    if p["upsample"]:
        x = x.index_select(1, LC.nearest_index(p["up"][0], h, x.device)).index_select(2, LC.nearest_index(p["up"][1], w, x.device))
    xp = F.pad(x, (0, 0, 1, 1, 1, 1)) if p["pad_mode"] == 0 else F.pad(x, (0, 0, 0, 1, 0, 1))
    s, ho, wo = p["stride"], p["hout"], p["wout"]
    return torch.cat([xp[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s].reshape(-1, cin) for ky in range(3)
                      for kx in range(3)], 1)


def logical_matrix(p, wl):
    """the logical weights as [n, ntaps * cin], tap-major"""
    n = wl.shape[0]
    if p["mode"] == "conv":
        return wl.permute(0, 2, 3, 1).reshape(n, -1)
    if p["mode"] == "temporal":
        return wl.reshape(n, -1, 3).permute(0, 2, 1).reshape(n, -1)
    return wl


def accumulate32(A, W, order):
    """sum_k A W in fp32, the K axis permuted by `order` (a seed) and added up in pieces of 32"""
    k = A.shape[1]
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(order))
    A, W = A.to(F32)[:, perm], W.to(F32)[:, perm]
    acc = torch.zeros(A.shape[0], W.shape[0])
    for k0 in range(0, k, 32):
        acc = acc + A[:, k0:k0 + 32] @ W[:, k0:k0 + 32].t()
    return acc


def emulate(p, ops, order=0):
    """the chain of include/mvoc_hip.h, gemm.hip and gemm8.hip in torch fp32 / fp16 on the CPU: fp16 [m, cols].  ops: a, a2, w (logical),
    bias, rowadd [ra_rows, cols], resid [m, cols], ln_rowsum, ln_bias, ln_stats (logical order; absent ones None)"""
    return epilogue32(p, ops, accumulate32(gather(p, ops["a"], ops["a2"]), logical_matrix(p, ops["w"]), order))


def epilogue32(p, ops, acc):
    """the epilogue's rounding points on an fp32 accumulator"""
    if p["ln"]:
        st = ops["ln_stats"].to(F32)
        y = st[:, 1:2] * (acc - st[:, 0:1] * ops["ln_rowsum"].to(F32)[None]) + ops["ln_bias"].to(F32)[None]
    else:
        y = acc + (ops["bias"].to(F32)[None] if p["bias"] else 0)
    cols = cols_of(p)
    if p["act"] == ACT_GEGLU:
        inner = p["n"] // 2
        v = _r16(_r16(y[:, :inner]) * _r16(F.gelu(_r16(y[:, inner:]))))
    else:
        v = _r16(y)[:, :cols]
        if p["rowadd_div"]:
            v = _r16(v + ops["rowadd"].to(F32)[torch.arange(p["m"]) // p["rowadd_div"]])
        if p["act"] == ACT_SILU:
            v = _r16(F.silu(v))
        elif p["act"] == ACT_GELU:
            v = _r16(F.gelu(v))
    if p["resid"]:
        v = _r16(v + ops["resid"].to(F32))
    return v.to(H16)


def honoured(p):
    """what the header lets a launch honour of its statistics requests, and what the library honours today where the tile is forced
    (gemm.hip): (chan_sums, row_moments tile width or 0).  The CPU stand-in answers this; on the GPU run_case holds the library's
    query functions to it on forced tiles 81 / 82 and on the forced split-K of a forced tile (must_honour), so that a library which
    stopped honouring the requests altogether does not pass the statistics cases vacuously"""
    g8 = p["tile"] in (81, 82)
    split = p["split_k"] > 1 and p["workspace"] and p["act"] != ACT_GEGLU and not p["ln"]
    if split:
        return bool(p["chan_sums"] and p["act"] == ACT_NONE and p["m"] % 256 == 0 and p["trim"] == 0), 0
    if not g8:
        return False, 0
    cs = bool(p["chan_sums"] and p["act"] == ACT_NONE and p["m"] % 256 == 0)
    wide = p["tile"] == 82 and p["act"] == ACT_NONE and not (p["ln"] and p["rowadd_div"]) and p["mode"] != "conv"
    rm = (320 if wide else 256) if (p["row_moments"] and p["act"] != ACT_GEGLU and p["trim"] == 0) else 0
    return cs, rm


def must_honour(p):
    """the cases whose statistics answers are decided by the descriptor alone: a forced eight-phase tile, or a forced split-K on a
    forced direct-to-LDS tile (the reduce pass).  With tile = 0 the answer follows the dispatch, which is not under test."""
    return p["tile"] in (81, 82) or (p["tile"] >= 11 and p["split_k"] > 1 and p["workspace"])


def emulate_into(L, order=0, defect=None):
    """the CPU stand-in for the kernel: reads the layout's buffers (the weights: the case's logical ones), writes the described output
    elements and the honoured statistics.  Returns (rc, chan_sums written, row_moments tile width) as library_kernel does.
    `defect`: a planted fault (tests/test_gemm_contract_cpu.py: each must trip the check named there)"""
    p = L.p

    def get(name):
        return L.views[name](L.T[name]).cpu() if name in L.T else None

    ops = {name: get(name) for name in ("a", "a2", "bias", "rowadd", "resid", "ln_rowsum", "ln_bias", "ln_stats")}
    if p["act"] == ACT_GEGLU:  # packed -> logical order
        inv = torch.argsort(geglu_perm(p["n"]))
        for name in ("bias", "ln_rowsum", "ln_bias"):
            if ops[name] is not None:
                ops[name] = ops[name][inv]
    ops["w"] = L.logical["w"].cpu()
    if defect == "a_padding_column":  # one column too many of `a`: the first undescribed one
        t = L.T["a"]
        ops["a"] = t.as_strided((L.rows_a, p["c1"]), (L.lda, 1), t.storage_offset() + 1).cpu()
    elif defect == "resid_row_gap":
        t = L.T["resid"]
        ops["resid"] = t.as_strided((L.m, L.cols), (L.ldr, 1), t.storage_offset() + 8).cpu()
    elif defect == "rowadd_next_row":
        ops["rowadd"] = torch.roll(ops["rowadd"], -1, 0)
    elif defect == "bias_past_n":
        t = L.T["bias"]
        ops["bias"] = t.as_strided((p["n"],), (1,), t.storage_offset() + 16).cpu()
    out = emulate(p, ops, order)
    if defect == "row_copies_neighbour":
        out[L.m // 2] = out[L.m // 2 - 1]
    elif defect == "last_k_tile_dropped":
        A = gather(p, ops["a"], ops["a2"]).clone()
        A[:, -32:] = 0
        out = epilogue32(p, ops, accumulate32(A, logical_matrix(p, ops["w"]), order))
    view = L.views["out"](L.T["out"])
    view.copy_(out.to(L.device))
    flat, off = L.T["out"].base_alloc, L.T["out"].storage_offset()
    if defect == "row_m_written":
        flat[off + L.m * L.ldo] = 1.0
    elif defect == "columns_past_n_store":
        flat[off + (L.m // 2) * L.ldo + L.cols:off + (L.m // 2) * L.ldo + L.cols + 2] = 1.0
    cs, rm = (False, 0) if defect == "stats_never_honoured" else honoured(p)
    stored = out.to(F32)
    if defect == "input_written":  # a described element of an input
        L.T["bias"][0] += 1.0
    if defect == "stats_when_unhonoured" and "chan_sums" in L.T:
        L.views["chan_sums"](L.T["chan_sums"])[0, 0, 0] = 1.0
    if cs:
        xs = stored.reshape(-1, 256, L.cols)
        L.views["chan_sums"](L.T["chan_sums"]).copy_(torch.stack([xs.sum(1), (xs * xs).sum(1)], -1).to(L.device))
    if rm:
        mom = LC.row_moments64(stored, rm, L.rm_ld).to(F32)
        nt = -(-p["n"] // rm)
        if defect == "row_moments_padding":
            nt = L.rm_ld
        L.views["row_moments"](L.T["row_moments"])[:, :nt].copy_(mom[:, :nt].to(L.device))
    if p["workspace"] and L.split > 1:  # the slabs are scratch: written, whatever they held
        L.views["workspace"](L.T["workspace"]).zero_()
        if defect == "workspace_overrun":
            L.T["workspace"].base_alloc[L.T["workspace"].storage_offset() + L.split * L.m * L.n] = 0.0
    return 0, int(cs), rm


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
    """rel-L2 per 32-row group: [ceil(m / 32)]"""
    out, ref = out.to(F64), ref.to(F64)
    pad = -out.shape[0] % 32
    num = F.pad(((out - ref) ** 2).sum(1), (0, pad)).reshape(-1, 32).sum(1).sqrt()
    den = F.pad((ref ** 2).sum(1), (0, pad)).reshape(-1, 32).sum(1).sqrt()
    return torch.where(den > 0, num / den.clamp_min(1e-300), num)


def d_bound(p):
    """the project's bound of the case's form: the widest of the forms it combines (each from the test named at D_BOUND)"""
    forms = ["plain"] + (["act"] if p["act"] != ACT_NONE else []) + (["ln"] if p["ln"] else []) + \
            (["gather"] if p["mode"] != "plain" else []) + (["split"] if p["workspace"] else [])
    return max(D_BOUND[f] for f in forms)


def check_stats(L, out, cs_written, rm_width, exact, what):
    """chan_sums / row_moments: honoured (the query answers non-zero): the described extent fully written and right -- equal to the
    fp64 sums of the STORED output where those are sums of small integers (exact), else within the fp32 summation bound
    count * 2^-24 * sum |terms|; not honoured: the whole allocation still holds its sentinel"""
    p = L.p
    stored = out.to(F64)
    for name, on in (("chan_sums", cs_written), ("row_moments", rm_width)):
        if name not in L.T:
            assert not on, f"{what}: {name} reported written without a request"
            continue
        if not on:
            assert L.untouched(name), f"{what}: {name} was written although the query function answers 0"
            continue
        if name == "chan_sums":
            assert p["m"] % 256 == 0, f"{what}: chan_sums honoured although m is no multiple of 256"
            got = L.check_f32_out(name, (p["m"] // 256, L.cols, 2)).to(F64)
            want = LC.chan_sums64(stored, 256)
            mag = LC.chan_sums64(stored.abs(), 256)
            count = 256
        else:
            assert rm_width in (256, 320) and L.cols == p["n"], f"{what}: row_moments width {rm_width}, cols {L.cols}"
            nt = -(-p["n"] // rm_width)
            got = L.check_f32_out(name, (p["m"], nt, 2)).to(F64)
            want = LC.row_moments64(stored, rm_width, L.rm_ld)[:, :nt]
            mag = LC.row_moments64(stored.abs(), rm_width, L.rm_ld)[:, :nt]
            count = rm_width
        if exact:
            assert torch.equal(got, want), f"{what}: {name} differs from the sums of the stored output, worst {float((got - want).abs().max())}"
        else:
            lim = count * 2.0 ** -24 * mag + 1e-30
            assert bool(((got - want).abs() <= lim).all()), f"{what}: {name} beyond the fp32 summation bound"


# ---- runners: one code path for the GPU tests and the CPU test -----------------------------------------------------------------------
def library_kernel(lib, stream_fn, sync):
    def kernel(L):
        rc = lib.mvoc_gemm_f16(C.byref(L.desc()), stream_fn())
        cs, rm = lib.mvoc_gemm_chan_sums_written(), lib.mvoc_gemm_row_moments_written()
        sync()
        return rc, cs, rm
    return kernel


def run_case(section, p, device, kernel, figures=None, err=lambda: ""):
    """draw, lay out, check_poison, launch, the checks of every case, the section's comparison: the described output's bits"""
    what = describe(section, p)
    case = draw(section, p)
    L = GemmLayout(device, p)
    L.fill(case)
    L.check_poison()
    ref, bound = L.reference()
    exact = section in ("A", "L")
    if exact:
        assert bool((ref.abs() < EXACT_LIMIT).all()) and torch.equal(ref.to(H16).to(F64), ref + 0.0), what  # before launching
    before = {name: L._raw(name).clone() for name in L.inputs if name != "workspace"}
    rc, cs, rm = kernel(L)
    assert rc in RC, f"{what}: return code {rc} is none of the header's"
    assert rc == 0, f"{what}: refused with {rc}: {err()}"
    out = L.check_out("out")
    written = L.check_workspace()
    if "expect_split" in p:
        assert written == L.split * L.m * L.n, f"{what}: the automatic policy wrote {written} workspace floats, not {L.split} slabs"
    if must_honour(p):
        want_cs, want_rm = honoured(p)
        assert (bool(cs), bool(rm)) == (want_cs, bool(want_rm)), \
            f"{what}: the query functions answer ({cs}, {rm}), the header's conditions give ({int(want_cs)}, {want_rm})"
    check_stats(L, out, cs, rm, exact, what)
    for name in L.inputs:  # the inputs are inputs: neither their described elements nor the poison around them changed
        if name != "workspace":
            assert torch.equal(L._raw(name), before[name]), f"{what}: {name} was written"
    if exact:
        assert_equal_bits(out, ref, what)
    elif section == "C":
        assert_within_bound(out, ref, bound, what)
    else:
        lim = d_bound(p)
        worst = float(group_errors(out, ref).max())
        if figures is not None:
            figures.append((what, worst, lim))
        assert worst < lim, f"{what}: a 32-row group has rel-L2 {worst:.3g} (bound {lim})"
    return out.cpu().view(I16).clone()
