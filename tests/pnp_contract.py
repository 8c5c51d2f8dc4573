"""Constructions and references of the blend-scatter / plane / loop-glue contract set (tests/test_pnp_contract_cpu.py shows them
sound without a GPU, tests/test_pnp_contract_gpu.py launches them through the C ABI).  numpy only: nothing here loads the library.

ONE reference for every mvoc_pnp_blend_scatter_* entry (blend_reference): numpy float16 arithmetic, one correctly rounded fp16
operation per +, - and *, restating include/mvoc_hip.h and not the kernels.  It works on the LOGICAL batch X[T][chunk][F][H][W][C]
(T tensors: x, and x2 when given); a layout (tokens with any strides / pitch / gap, NCHW) is nothing but the table of element
offsets that pack() derives from the descriptor's own formula, so the same case runs on both layouts and the whole allocation --
guards, pitch columns, chunk gaps, sources, the chunks of idle variants -- is compared after the call: the reference at the
described destination elements, the bytes from before the call everywhere else.  Everything the contract says is not read holds
fp16 NaN before the call (table rows: INT32_MIN).

The loop glue (ddim_reference, fusion_reference) forms every scalar product as a numpy float32 product cast to float16 -- two
roundings, as the header says; `once` names the product sites a MUTATED reference rounds once (the exact product in float64, one
cast), which is what a contracted mixed-precision fma computes.

The walk is a covering walk: per entry a greedy pairwise array over the factors that apply to it (walk_cases), then the work-item
totals 255 / 256 / 257 / 513 per item geometry, the special-value atlas and the nearest-rule index masks per load form."""
import itertools

import numpy as np

F16 = np.float16
NAN_BITS = 0x7E00
I32MIN, I32MAX = -(2 ** 31), 2 ** 31 - 1
ONE = F16(1.0)

ENTRIES = ("pos", "mapped", "variants", "sel", "placed", "placed_variants", "resampled", "resampled_variants")
LAYOUTS = ("tokens", "nchw")
SRC_RULE = {"pos": "direct", "mapped": "direct", "variants": "direct", "sel": "direct", "placed": "shift", "placed_variants": "shift",
            "resampled": "map", "resampled_variants": "map"}
PER_VARIANT = ("placed_variants", "resampled_variants")
SYMBOL = {"pos": "", "mapped": "_mapped", "variants": "_variants", "sel": "_variants_sel", "placed": "_placed",
          "placed_variants": "_placed_variants", "resampled": "_resampled", "resampled_variants": "_resampled_variants"}


def symbol(layout, entry):
    return f"mvoc_pnp_blend_scatter_{layout}{SYMBOL[entry]}"


def bits(a):
    return np.ascontiguousarray(a).view(np.int16)


def f16_from_bits(b):
    return np.asarray(b, dtype=np.uint16).view(F16)


# the 16 special values: +-0, +-1, +-65504, +-inf, NaN, the smallest subnormal of both signs, the normal just above 2^-14, the
# (negative) largest subnormal just below it, three ordinary values
SPECIALS = f16_from_bits([0x0000, 0x8000, 0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x0001, 0x8001, 0x0401, 0x83FF,
                          0x3555, 0xC248, 0x2E66])
ATLAS_MASKS = np.array([0.0, -0.0, 1.0, np.float32(1) / 255, np.float32(128) / 255, np.float32(254) / 255], dtype=np.float32).astype(F16)


# ---- the nearest rule ------------------------------------------------------------------------------------------------------------
def near(out_size, in_size, rule="float"):
    """source index of every destination index: min(floor(f32(d) * (f32(in) / f32(out))), in - 1) -- F.interpolate's rule, float
    rounding included.  rule = "ceil" / "exact" are the mutations of tests/test_pnp_contract_cpu.py"""
    d = np.arange(out_size)
    if rule == "exact":
        idx = d * in_size // out_size
    else:
        scale = np.float32(in_size) / np.float32(out_size)
        prod = d.astype(np.float32) * scale
        idx = (np.ceil(prod) if rule == "ceil" else np.floor(prod)).astype(np.int64)
    return np.minimum(idx, in_size - 1)


def float_rule_differs(in_size, out_size):
    return not np.array_equal(near(out_size, in_size), near(out_size, in_size, "exact"))


# ---- a blend case ----------------------------------------------------------------------------------------------------------------
class Case:
    """one launch.  fac: the factor levels it was built from (the coverage check reads them); the rest is what the launch needs"""

    def __init__(self, layout, entry, geom, C, nobj, ndst, base, srcmap, var, table, mask, x2, strides="spatial", pitch=1, gap=0,
                 lead=256, seed=0, kind="random"):
        self.layout, self.entry, self.kind, self.seed = layout, entry, kind, seed
        self.F, self.H, self.W, self.mh, self.mw = geom
        self.C, self.nobj, self.ndst, self.base = C, nobj, ndst, base
        self.nd = 2 if ndst == 0 else ndst
        self.nvar, self.active = var
        self.T = 2 if x2 else 1
        self.strides, self.pitch, self.gap, self.lead = strides, pitch, gap, lead
        self.table_kind, self.mask_kind, self.srcmap = table, mask, srcmap
        self.rule = SRC_RULE[entry]
        self.nm = self.nvar if entry in PER_VARIANT else 1  # table / mask sets
        if base == -1:  # no background chunk: the positional tokens entry alone
            self.nsrc, self.obj_chunk = nobj, list(range(nobj))
        elif srcmap == "ident":
            self.nsrc, self.obj_chunk = nobj + 1, list(range(1, nobj + 1))
        elif srcmap == "reversed":
            self.nsrc, self.obj_chunk = nobj + 1, list(range(nobj, 0, -1))
        elif srcmap == "shared":  # two (or more) objects on one chunk
            self.nsrc, self.obj_chunk = 2, [1] * nobj
        else:  # "chunk0": an object on the background's chunk
            self.nsrc, self.obj_chunk = nobj + 1, [0] + list(range(2, nobj + 1))
        self.nchunk = self.nsrc + self.nd * self.nvar
        self.fac = dict(geom=geom, C=C, nobj=nobj, ndst=ndst, base=base, srcmap=srcmap, var=var, table=table, mask=mask, x2=x2,
                        strides=strides, pitch=pitch, gap=gap, lead=lead)
        self._built = False

    def __repr__(self):
        return (f"{self.layout}/{self.entry}/{self.kind} F{self.F} H{self.H} W{self.W} m{self.mh}x{self.mw} C{self.C} nobj{self.nobj} "
                f"ndst{self.ndst} base{self.base} {self.srcmap} nvar{self.nvar} active{self.active:#x} {self.table_kind} {self.mask_kind} "
                f"T{self.T} {self.strides} pitch{self.pitch} gap{self.gap} lead{self.lead}")

    # chunk numbering of the header: u_k = nsrc + k, c_k = nsrc + (ndst - 1) * nvar + k
    def u_chunk(self, k):
        return self.nsrc + k

    def c_chunk(self, k):
        return self.nsrc + (self.nd - 1) * self.nvar + k

    def on(self, k):
        return (self.active >> k) & 1

    def work_items(self):
        px = self.F * self.H * self.W
        if self.layout == "tokens":
            return px * self.C // 8
        return px * self.C // 8 if (self.H * self.W) % 8 == 0 and self.lead % 16 == 0 else px * self.C

    def build(self):
        """draw X, the masks and the table (deterministic in the seed)"""
        if self._built:
            return self
        rng = np.random.default_rng(1000 + self.seed)
        shape = (self.T, self.nchunk, self.F, self.H, self.W, self.C)
        if self.kind == "atlas":
            X = np.broadcast_to(atlas_values(self)[0], shape).copy()
            for j, ch in enumerate(self.obj_chunk):
                X[:, ch] = atlas_values(self)[1]
            self.masks = np.broadcast_to(atlas_values(self)[2], (self.nm, self.nobj, self.F, self.mh, self.mw)).copy()
        elif self.kind == "index":  # base 0, object 1.0, mask cell (my, mx) a distinct small integer: the result IS the sampled cell
            X = np.zeros(shape, F16)
            for ch in self.obj_chunk:
                X[:, ch] = ONE
            cells = (1 + np.arange(self.mh * self.mw)).reshape(self.mh, self.mw).astype(F16)
            assert self.mh * self.mw <= 2048
            self.masks = np.broadcast_to(cells, (self.nm, self.nobj, self.F, self.mh, self.mw)).copy()
        else:
            X = rng.standard_normal(shape).astype(F16)
            u8 = rng.integers(0, 256, (self.nm, self.nobj, self.F, self.mh, self.mw))
            self.masks = (u8 > 127).astype(F16) if self.mask_kind == "hard" else (u8.astype(np.float32) / np.float32(255)).astype(F16)
        # what the contract says is not read holds NaN
        nan = f16_from_bits([NAN_BITS])[0]
        read = set(self.obj_chunk) | ({0} if self.base == 1 else set())
        for ch in range(self.nsrc):
            if ch not in read:
                X[:, ch] = nan
        for k in range(self.nvar):
            if self.nd == 2:
                X[:, self.u_chunk(k)] = nan
            if self.base == 1 or not self.on(k):
                X[:, self.c_chunk(k)] = nan
            if self.nm > 1 and not self.on(k):
                self.masks[k] = nan
        self.X = X
        self.table = make_table(self)
        self._built = True
        return self


def atlas_values(c):
    """(base, object, mask) of the special-value atlas on [F][H = 4][W = 6][C = 64]: pixel p has mask ATLAS_MASKS[p % 6] and its 64
    channels hold base SPECIALS[(p // 6) * 4 + ch // 16] against object SPECIALS[ch % 16] -- the 16 x 16 x 6 cross product per frame"""
    assert (c.H, c.W, c.C, c.mh, c.mw) == (4, 6, 64, 4, 6)
    p = np.arange(24).reshape(4, 6)
    ch = np.arange(64)
    base = SPECIALS[(p[:, :, None] // 6) * 4 + ch[None, None, :] // 16]
    obj = np.broadcast_to(SPECIALS[ch % 16], (4, 6, 64))
    mask = ATLAS_MASKS[p % 6]
    return base, obj, mask


def make_table(c):
    """shift: int32 [nm][nobj][F][2] = (dfy, dfx); map: int32 [nm][nobj][F][H + W] (ymap, then xmap); direct: None"""
    if c.rule == "direct":
        return None
    H, W, kind = c.H, c.W, c.table_kind
    rng = np.random.default_rng(77 + c.seed)
    if c.rule == "shift":
        t = np.zeros((c.nm, c.nobj, c.F, 2), np.int64)
        extreme = [(I32MIN, 0), (0, I32MAX), (H, 0), (0, W), (I32MAX, I32MIN), (0, 0), (1, 0), (-H, 0), (0, -W)]
        for s, j, f in itertools.product(range(c.nm), range(c.nobj), range(c.F)):
            if kind in ("small", "absent"):
                t[s, j, f] = ((j + f + s) % 3 - 1, (2 * j + f + s) % 5 - 2)
            elif kind == "extreme":
                t[s, j, f] = extreme[((s * c.nobj + j) * c.F + f) % len(extreme)]
        if kind == "absent":
            t[:, 0, 0] = (H, 0)  # object 0 has left frame 0
        if kind == "atlas":  # frame 0 unmoved; the others lose row 0 and the last two columns
            t[:, :, 1:] = (1, -2)
        return t.astype(np.int32)
    t = np.zeros((c.nm, c.nobj, c.F, H + W), np.int64)
    for s, j, f in itertools.product(range(c.nm), range(c.nobj), range(c.F)):
        y, x = np.arange(H), np.arange(W)
        if kind in ("small", "absent"):
            y, x = y - ((j + f + s) % 3 - 1), x - ((2 * j + f + s) % 5 - 2)
        elif kind == "up":  # the object at 3/2 of its size: nearest on pixel centres
            y, x = (2 * y + 1) // 3, (2 * x + 1) // 3
        elif kind == "down" or (kind == "atlas" and f > 0):  # at 1/2: the far half of the grid has no source
            y, x = 2 * y + 1 + s, 2 * x + 1
        elif kind == "mirror":
            y, x = H - 1 - y, (W - 1 - x) if (j + s) % 2 == 0 else x
        elif kind == "extreme":
            y, x = rng.integers(0, H, H), rng.integers(0, W, W)
            odd = [I32MIN, I32MAX, H, W, -1]
            y[rng.integers(0, H)] = odd[(s + j + f) % 5]
            x[rng.integers(0, W)] = odd[(s + j + f + 2) % 5]
        t[s, j, f, :H], t[s, j, f, H:] = y, x
    if kind == "absent":
        t[:, 0, 0] = -1
    return t.astype(np.int32)


# ---- THE reference ---------------------------------------------------------------------------------------------------------------
def _ftz(a):
    a = a.copy()
    a[(np.abs(a) < F16(2.0 ** -14)) & ~np.isnan(a)] *= F16(0)  # keeps the sign, as a flushing unit does
    return a


def blend_reference(c, mut=()):
    """-> X after the call.  For every tensor, every variant k whose bit is set and every (f, py, px, ch):
         inj = base (chunk 0 if base_chunk0 == 1, else variant k's cond chunk)
         for j in object order: (present, sy, sx) by the source rule; v = chunk S_j at (f, sy, sx, ch) if present else +0;
                                m = masks[f][near(py)][near(px)] if present else +0;  inj = f16(f16(inj * f16(1 - m)) + f16(v * m))
         c_k = inj; u_k = inj when ndst == 2
    mut: names of deliberate mistakes (tests/test_pnp_contract_cpu.py), none of them the contract"""
    c.build()
    X0, X = c.X, c.X.copy()
    rule = "ceil" if "near_ceil" in mut else "exact" if "near_exact" in mut else "float"
    ny, nx = near(c.H, c.mh, rule), near(c.W, c.mw, rule)
    py, px = np.meshgrid(np.arange(c.H, dtype=np.int64), np.arange(c.W, dtype=np.int64), indexing="ij")
    fi = np.arange(c.F)[:, None, None]
    order = range(c.nobj - 1, -1, -1) if "reverse_objects" in mut else range(c.nobj)
    with np.errstate(all="ignore"):
        for k in range(c.nvar):
            if not c.on(k):
                continue
            s = k if c.nm > 1 and "table0" not in mut else 0
            u, cc = c.u_chunk(k), c.c_chunk(k)
            if "swap_blocks" in mut and c.nd == 2:
                u, cc = cc, u
            loads = []
            for j in order:
                if c.rule == "direct":
                    sy, sx = np.broadcast_to(py, (c.F, c.H, c.W)), np.broadcast_to(px, (c.F, c.H, c.W))
                elif c.rule == "shift":
                    off = c.table[s, j].astype(np.int64)  # [F][2]
                    sy, sx = py[None] - off[:, 0, None, None], px[None] - off[:, 1, None, None]
                else:
                    tab = c.table[s, j].astype(np.int64)  # [F][H + W]
                    sy, sx = np.broadcast_to(tab[:, :c.H, None], (c.F, c.H, c.W)), np.broadcast_to(tab[:, None, c.H:], (c.F, c.H, c.W))
                present = (sy >= 0) & (sy < c.H) & (sx >= 0) & (sx < c.W)
                m = np.where(present, c.masks[s, j][:, ny][:, :, nx], F16(0))[..., None]
                loads.append((present[..., None], np.clip(sy, 0, c.H - 1), np.clip(sx, 0, c.W - 1), m, c.obj_chunk[j]))
            for t in range(c.T):
                inj = X0[t, 0] if c.base == 1 or "base_chunk0" in mut else X0[t, cc]
                for present, sy, sx, m, ch in loads:
                    v = np.where(present, X0[t, ch][fi, sy, sx], F16(0))
                    if "flush" in mut:
                        new = _ftz(_ftz(_ftz(inj) * _ftz(ONE - _ftz(m))) + _ftz(_ftz(v) * _ftz(m)))
                    else:
                        new = (inj * (ONE - m)) + (v * m)
                    if "product_plus_zero" in mut:  # obj * m formed as an fma onto +0.0: a -0.0 product comes out as +0.0
                        new = (inj * (ONE - m)) + ((v * m) + F16(0))
                    if "select" in mut:  # the two ends of the mask taken as a select
                        new = np.where(m == ONE, v, np.where(m == F16(0), inj, new))
                    if "skip_absent" in mut:
                        new = np.where(present, new, inj)
                    inj = new
                if c.nd == 2:
                    X[t, u] = inj
                X[t, cc] = inj
    return X


def dest_chunks(c):
    """boolean [nchunk]: the chunks the call is described to write"""
    d = np.zeros(c.nchunk, bool)
    for k in range(c.nvar):
        if c.on(k):
            d[c.c_chunk(k)] = True
            if c.nd == 2:
                d[c.u_chunk(k)] = True
    return d


def compare(got_bits, ref_bits, dest):
    """-> (elements that differ, destination elements compared as NaN).  Raw bits everywhere; at a DESTINATION element whose
    reference is NaN the result must be NaN, sign and payload not compared (tests/test_variants_gpu.py has the reason)"""
    got_bits, ref_bits = np.asarray(got_bits).view(np.int16), np.asarray(ref_bits).view(np.int16)
    ref_nan = np.isnan(ref_bits.view(F16)) & dest
    ok = np.where(ref_nan, np.isnan(got_bits.view(F16)), got_bits == ref_bits)
    return int((~ok).sum()), int(ref_nan.sum())


# ---- layouts: the descriptor and the offset of every logical element ---------------------------------------------------------------
GUARD = 128  # elements of NaN in front of and behind every operand


class Packed:
    pass


def pack(c):
    """-> the allocations before the call (int16 / int32), the descriptor fields, and the allocation the call must leave"""
    c.build()
    P = Packed()
    F, H, W, C, HW = c.F, c.H, c.W, c.C, c.H * c.W
    ch, f, y, x, e = np.meshgrid(np.arange(c.nchunk), np.arange(F), np.arange(H), np.arange(W), np.arange(C), indexing="ij", sparse=True)
    if c.layout == "tokens":
        ld = C * c.pitch
        if c.strides == "spatial":  # [chunks * F, HW, ld]
            P.f_stride, P.p_stride, P.chunk_stride = HW * ld, ld, F * HW * ld + c.gap * ld
        else:  # temporal: [chunks * HW, F, ld]
            P.f_stride, P.p_stride, P.chunk_stride = ld, F * ld, HW * F * ld + c.gap * ld
        rel = ch * P.chunk_stride + f * P.f_stride + (y * W + x) * P.p_stride + e
        region = c.nchunk * P.chunk_stride
        x2_off = C if c.pitch > 1 else region + 64
    else:
        P.f_stride = P.p_stride = P.chunk_stride = 0  # not read by the nchw entries
        rel = ((ch * F + f) * C + e) * HW + y * W + x
        region = c.nchunk * F * C * HW
        x2_off = (region + 7) // 8 * 8 + 64
    rel = np.broadcast_to(rel, (c.nchunk, F, H, W, C))
    lead = GUARD + c.lead // 2  # c.lead bytes past a 256-byte boundary
    P.x_off = [lead, lead + x2_off][:c.T]
    size = lead + (x2_off if c.T == 2 and c.pitch == 1 else 0) + region + GUARD
    P.offs = np.stack([rel + o for o in P.x_off])  # [T][nchunk][F][H][W][C]
    assert GUARD <= P.offs.min() and P.offs.max() < size - GUARD
    assert len(np.unique(P.offs)) == P.offs.size, "two logical elements at one address"
    P.feat = np.full(size, NAN_BITS, np.int16)
    P.feat[P.offs] = bits(c.X)
    P.expect = P.feat.copy()
    P.expect[P.offs] = bits(blend_reference(c))
    P.dest = np.zeros(size, bool)
    P.dest[P.offs[:, dest_chunks(c)]] = True
    P.masks = np.full(2 * GUARD + c.masks.size, NAN_BITS, np.int16)
    P.masks[GUARD:GUARD + c.masks.size] = bits(c.masks).ravel()
    P.m_off = GUARD
    P.table, P.t_off = None, 0
    if c.table is not None:
        tab = c.table.copy()
        for k in range(c.nvar if c.nm > 1 else 0):
            if not c.on(k):
                tab[k] = I32MIN  # rows of a variant whose bit is clear
        P.table = np.full(2 * 16 + tab.size, I32MIN, np.int32)
        P.table[16:16 + tab.size] = tab.ravel()
        P.t_off = 16
    return P


# ---- the walk ----------------------------------------------------------------------------------------------------------------------
GEOMS = [(1, 1, 1, 1, 1), (3, 3, 5, 5, 9), (2, 4, 6, 8, 12), (2, 4, 6, 2, 3), (3, 8, 8, 8, 8),
         (1, 22, 4, 26, 4), (1, 4, 22, 4, 26), (1, 46, 1, 14, 1), (1, 1, 33, 1, 39)]
FLOAT_RULE_GEOMS = GEOMS[5:]
CHANNELS = {"tokens": (8, 24, 64), "nchw": (1, 3, 20)}
VARS = [(1, 1), (2, 3), (3, 0b101), (8, 0xFF), (8, 0x80)]
TABLES = {"direct": ("none",), "shift": ("zero", "small", "absent", "extreme"),
          "map": ("ident", "small", "absent", "up", "down", "mirror", "extreme")}
BAD_PAIRS = {frozenset({("nobj", 1), ("srcmap", "shared")})}
# (F, H, W, C) whose work-item total per tensor is 255, 256, 257 and 513, per item geometry
TOTALS = {"tokens": [(1, 15, 17, 8), (1, 16, 16, 8), (1, 1, 257, 8), (3, 9, 19, 8)],
          "nchw8": [(1, 20, 34, 3), (2, 32, 32, 1), (1, 8, 257, 1), (1, 36, 38, 3)],
          "nchw1": [(1, 5, 17, 3), (64, 2, 2, 1), (1, 1, 257, 1), (1, 9, 19, 3)]}
TOTAL_TARGETS = (255, 256, 257, 513)


def factors(layout, entry):
    """the factors that apply to an entry and their levels"""
    f = dict(geom=GEOMS, C=CHANNELS[layout], nobj=(1, 2, 3, 4), ndst=(0, 1, 2), mask=("hard", "soft"), x2=(True, False))
    f["base"] = (-1, 0, 1) if (layout, entry) == ("tokens", "pos") else (0, 1)
    if entry != "pos":
        f["srcmap"] = ("ident", "reversed", "shared", "chunk0")
    if entry == "variants":
        f["var"] = [v for v in VARS if v[1] == (1 << v[0]) - 1]
    elif entry not in ("pos", "mapped"):
        f["var"] = VARS
    if SRC_RULE[entry] != "direct":
        f["table"] = TABLES[SRC_RULE[entry]]
    if layout == "tokens":
        f.update(strides=("spatial", "temporal"), pitch=(1, 3), gap=(0, 8), lead=(16, 128))
    return f


def pairs_of(fac, names):
    return {frozenset({(a, fac[a]), (b, fac[b])}) for a, b in itertools.combinations(names, 2)}


def required_pairs(layout, entry):
    f = factors(layout, entry)
    need = set()
    for a, b in itertools.combinations(sorted(f), 2):
        for la, lb in itertools.product(f[a], f[b]):
            need.add(frozenset({(a, la), (b, lb)}))
    return need - BAD_PAIRS


def _pairwise(layout, entry):
    """greedy covering array: every remaining pair seeds an assignment, the other factors take the level that covers most"""
    f = factors(layout, entry)
    names = sorted(f)
    need = required_pairs(layout, entry)
    out, turn = [], 0
    while need:
        seed = min(need, key=lambda p: sorted(map(repr, p)))
        fac = dict(seed)
        for a in names:
            if a in fac:
                continue
            best, best_n = None, -1
            for i in range(len(f[a])):
                lv = f[a][(i + turn) % len(f[a])]
                pr = {frozenset({(a, lv), (b, fac[b])}) for b in fac}
                if pr & BAD_PAIRS:
                    continue
                n = len(pr & need)
                if n > best_n:
                    best, best_n = lv, n
            fac[a] = best
        need -= pairs_of(fac, names)
        out.append(fac)
        turn += 1
    return out


def _case(layout, entry, fac, seed, kind="random"):
    d = dict(srcmap="ident", var=(1, 1), table="none", strides="spatial", pitch=1, gap=0, lead=256)
    d.update(fac)
    if layout == "nchw":
        d["lead"] = fac.get("lead", 256)
    return Case(layout, entry, d["geom"], d["C"], d["nobj"], d["ndst"], d["base"], d["srcmap"], d["var"], d["table"], d["mask"],
                d["x2"], d["strides"], d["pitch"], d["gap"], d["lead"], seed=seed, kind=kind)


_WALK = {}


def walk_cases(layout, entry):
    """-> {"pairs": [...], "totals": [...], "index": [...], "atlas": [...]} of one entry on one layout"""
    key = (layout, entry)
    if key in _WALK:
        return _WALK[key]
    base_seed = 10000 * (LAYOUTS.index(layout) * len(ENTRIES) + ENTRIES.index(entry))
    pw = _pairwise(layout, entry)
    w = {"pairs": [_case(layout, entry, fac, base_seed + i) for i, fac in enumerate(pw)]}
    # work-item totals: the shapes of TOTALS with the other factors rotated through the pairwise rows
    tot, i = [], 0
    for group in (("tokens",) if layout == "tokens" else ("nchw8", "nchw1")):
        for (F, H, W, C) in TOTALS[group]:
            fac = dict(pw[(7 * i + 3) % len(pw)])
            fac.update(geom=(F, H, W, max(1, (H + 1) // 2), max(1, (W + 2) // 3)), C=C, x2=i % 2 == 0)
            if layout == "tokens":
                fac.update(pitch=1 + 2 * (i % 2))
            tot.append(_case(layout, entry, fac, base_seed + 5000 + i))
            i += 1
    w["totals"] = tot
    # the nearest rule made visible: float-rule geometries under an index mask, identity tables
    idx = []
    for i, g in enumerate(FLOAT_RULE_GEOMS):
        fac = dict(pw[(5 * i + 1) % len(pw)])
        fac.update(geom=g, C=CHANNELS[layout][0], nobj=1, mask="index", table={"direct": "none", "shift": "zero", "map": "ident"}[SRC_RULE[entry]])
        if "srcmap" in fac:
            fac.update(srcmap="ident")
        idx.append(_case(layout, entry, fac, base_seed + 6000 + i, kind="index"))
    w["index"] = idx
    # the special-value atlas: one per entry (so each of the six load forms has several); frame 0 is the cross product unmoved,
    # in frame 1 the table takes the object away from some pixels (a -0.0 base among them)
    fac = dict(pw[0])
    fac.update(geom=(2, 4, 6, 4, 6), C=64, nobj=1, mask="atlas", srcmap="ident", base=1,
               table={"direct": "none", "shift": "atlas", "map": "atlas"}[SRC_RULE[entry]])
    if layout == "tokens":
        fac.update(lead=16)
    w["atlas"] = [_case(layout, entry, fac, base_seed + 7000, kind="atlas")]
    _WALK[key] = w
    return w


def all_cases(layout, entry):
    w = walk_cases(layout, entry)
    return w["pairs"] + w["totals"] + w["index"] + w["atlas"]


def nchw_misaligned_case():
    """the alignment fix: x two bytes past an aligned address, H * W = 24 -- bit-exact through the 1-wide form"""
    fac = dict(geom=(2, 4, 6, 8, 12), C=3, nobj=2, ndst=2, base=1, mask="soft", x2=False, lead=258)
    return _case("nchw", "pos", fac, 424242)


# ---- planes ------------------------------------------------------------------------------------------------------------------------
def shift_planes_reference(src, offsets):
    """dst[pl][f][y][x] = src[pl][f][y - dy_f][x - dx_f] or +0; src [nplane][F][h][w] fp16, offsets [F][2] int32"""
    npl, F, h, w = src.shape
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    off = offsets.astype(np.int64)
    sy, sx = y[None] - off[:, 0, None, None], x[None] - off[:, 1, None, None]
    return _gather(src, sy, sx)


def gather_planes_reference(src, maps):
    """dst[pl][f][y][x] = src[pl][f][ymap_f[y]][xmap_f[x]] or +0; maps [F][h + w] int32"""
    npl, F, h, w = src.shape
    m = maps.astype(np.int64)
    sy, sx = np.broadcast_to(m[:, :h, None], (F, h, w)), np.broadcast_to(m[:, None, h:], (F, h, w))
    return _gather(src, sy, sx)


def _gather(src, sy, sx):
    npl, F, h, w = src.shape
    ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    v = src[:, np.arange(F)[:, None, None], np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
    return np.where(ok[None], v, F16(0))


def plane_cases():
    """(kind, nplane, F, h, w, table kind, seed): every int32 entry, and totals of 255, 256, 257 and 513 elements"""
    shapes = [(1, 1, 1, 1), (1, 3, 5, 9), (4, 2, 4, 6), (1, 1, 15, 17), (1, 1, 16, 16), (1, 1, 1, 257), (1, 3, 9, 19), (2, 2, 22, 4)]
    out = []
    for i, (npl, F, h, w) in enumerate(shapes):
        for kind, tabs in (("shift", TABLES["shift"]), ("gather", TABLES["map"])):
            for j, tk in enumerate(tabs):
                if (i + j) % 2 == 0 or tk == "extreme":
                    out.append((kind, npl, F, h, w, tk, 100 * i + j))
    return out


def plane_case(kind, npl, F, h, w, tk, seed, special=False):
    """-> (src fp16 [npl][F][h][w], table int32, reference dst)"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((npl, F, h, w)).astype(F16)
    if special:
        src = SPECIALS[rng.integers(0, 16, (npl, F, h, w))]
    c = Case("nchw", "placed" if kind == "shift" else "resampled", (F, h, w, h, w), 1, 1, 2, 1, "ident", (1, 1), tk, "hard", False,
             seed=seed)
    table = make_table(c)[0, 0]
    ref = shift_planes_reference(src, table) if kind == "shift" else gather_planes_reference(src, table)
    return src, table, ref


# ---- loop glue ---------------------------------------------------------------------------------------------------------------------
DDIM_SITES = ("g_dv", "sa_x", "sb_v", "sa_v", "sb_x", "sq_eps", "sp_x0")
FUSION_SITES = ("mix_lat", "omix_bg", "mix_fg", "omix_inv")


def smul(scalar, x, once=False):
    """fp32 scalar x fp16 tensor: the fp32 product, ROUNDED to fp32, then rounded to fp16.  once: the mutation -- the exact product
    (35 significant bits, exact in float64) rounded to fp16 in one step"""
    if once:
        return (np.float64(np.float32(scalar)) * x.astype(np.float64)).astype(F16)
    return (np.float32(scalar) * x.astype(np.float32)).astype(F16)


def flips(scalar):
    """number of the 65 536 fp16 operands on which one rounding and two give different bits"""
    allx = f16_from_bits(np.arange(65536))
    with np.errstate(all="ignore"):
        a, b = smul(scalar, allx), smul(scalar, allx, True)
    return int(((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))).sum())


def ddim_reference(x, vu, vc, coef, once=()):
    """x / vu / vc fp16 [n] (vu may be None), coef = (sa, sb, sp, sq, g) fp32:
         v = vu + g * (vc - vu);  x0 = sa * x - sb * v;  eps = sa * v + sb * x;  out = sp * x0 + sq * eps"""
    sa, sb, sp, sq, g = (np.float32(t) for t in coef)
    with np.errstate(all="ignore"):
        v = vc
        if vu is not None:
            v = vu + smul(g, vc - vu, "g_dv" in once)
        x0 = smul(sa, x, "sa_x" in once) - smul(sb, v, "sb_v" in once)
        eps = smul(sa, v, "sa_v" in once) + smul(sb, x, "sb_x" in once)
        return smul(sp, x0, "sp_x0" in once) + smul(sq, eps, "sq_eps" in once)


def ddim_variants_reference(x, vu, vc, coef, once=(), row0=False):
    """x / vu / vc fp16 [nvar][n_per], coef fp32 [nvar][5]; row0: the mutation that gives every variant row 0"""
    return np.stack([ddim_reference(x[k], None if vu is None else vu[k], vc[k], coef[0 if row0 else k], once) for k in range(len(x))])


def fusion_reference(lat, bg, objs, masks, mix, rnf, once=(), omix_f32=False):
    """lat / bg fp16 [n], objs / masks fp16 [nobj][n], mix a python float; the factors are f32(mix) and f32(1.0 - mix), the
    subtraction in double (omix_f32: the mutation 1.0f - f32(mix))"""
    mixf = np.float32(mix)
    omix = np.float32(1.0) - mixf if omix_f32 else np.float32(1.0 - float(mix))
    with np.errstate(all="ignore"):
        l = smul(mixf, lat, "mix_lat" in once) + smul(omix, bg, "omix_bg" in once)
        for obj, m in zip(objs, masks):
            inv_obj = obj * m
            background = l * (ONE - m)
            fusion = inv_obj
            if rnf:
                fusion = smul(mixf, l * m, "mix_fg" in once) + smul(omix, inv_obj, "omix_inv" in once)
            l = background + fusion
        return l


def fusion_variants_reference(lat, bg, objs, masks, mix, rnf, once=(), omix_f32=False):
    return np.stack([fusion_reference(lat[k], bg, objs, masks, mix, rnf, once, omix_f32) for k in range(len(lat))])


GLUE_N = (1, 100, 255, 256, 257, 513)
GLUE_NVAR = (1, 2, 3, 8)
# scalars of the isolating cases, chosen by flips(): 0.3 -> 126, 0.99 -> 310 operands (test_pnp_contract_cpu asserts >= 32 per site)
S_ISO, S_ISO2 = 0.3, 0.99
MIX_ISO = {"mix_lat": 0.3, "mix_fg": 0.3, "omix_bg": 0.01, "omix_inv": 0.01}
MIX_OMIX_FORM = 0.65  # f32(1.0 - 0.65) = 0.35 and 1.0f - f32(0.65) = 0.35000002 differ: fusion_isolating_case("omix_form")
HAND_ROWS = [(0.3, 0.99, 0.99, 0.3, 7.3), (0.99, 0.0447, 0.01, 0.3, 0.3), (1.0, 0.0, 1.0, 0.0, 1.0), (0.6, 0.8, 0.8, 0.6, 9.0)]


def all_patterns():
    return f16_from_bits(np.arange(65536))


def ddim_isolating_case(site):
    """-> (x, vu, vc, coef): the 65 536 fp16 patterns in the free operand of ONE product, every other product by 0 or 1"""
    a, z = all_patterns(), np.zeros(65536, F16)
    s = S_ISO
    return {"sp_x0": (a, None, z, (1, 0, s, 0, 1)), "sa_x": (a, None, z, (s, 0, 1, 0, 1)), "sb_x": (a, None, z, (0, s, 0, 1, 1)),
            "sa_v": (z, None, a, (s, 0, 0, 1, 1)), "sb_v": (z, None, a, (0, s, 1, 0, 1)), "sq_eps": (z, None, a, (1, 0, 0, s, 1)),
            "g_dv": (z, z, a, (1, 0, 0, 1, s))}[site]


def fusion_isolating_case(site):
    """-> (lat, bg, objs, masks, mix, rnf)"""
    a, z, one = all_patterns(), np.zeros(65536, F16), np.ones(65536, F16)
    none = np.zeros((0, 65536), F16)
    mix = MIX_ISO.get(site, MIX_OMIX_FORM)
    return {"mix_lat": (a, z, none, none, mix, 0), "omix_bg": (z, a, none, none, mix, 0), "omix_form": (z, a, none, none, mix, 0),
            "mix_fg": (a, z, z[None], one[None], mix, 1), "omix_inv": (z, z, a[None], one[None], mix, 1)}[site]


def scheduler_rows():
    """three timesteps each of mvoc_amd.schedulers' DDIM and inverse tables (guidance 9.0 / 7.5), then the hand-made rows"""
    from mvoc_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    rows = []
    for cls, gs in ((DDIMScheduler, 9.0), (DDIMInverseScheduler, 7.5)):
        s = cls()
        s.set_timesteps(50)
        for t in (s.timesteps[0], s.timesteps[17], s.timesteps[-1]):
            rows.append(tuple(s.coefficients(int(t), gs)))
    return rows + HAND_ROWS


def ddim_cases(rows):
    """-> list of (name, x, vu, vc, coef [nvar][5]) with x [nvar][n_per]; nvar = 0 marks the single-tensor entry"""
    out, i = [], 0
    for n in GLUE_N:
        for nvar in (0,) + GLUE_NVAR:
            for uncond in (False, True):
                rng = np.random.default_rng(500 + i)
                K = max(nvar, 1)
                x, vc, vu = (rng.standard_normal((K, n)).astype(F16) for _ in range(3))
                coef = np.array([rows[(i + 3 * k) % len(rows)] for k in range(K)], np.float32)
                out.append((f"n{n}_nvar{nvar}_u{int(uncond)}", nvar, x, vu if uncond else None, vc, coef))
                i += 1
    # the 16 special values in x, v and the uncond prediction: 16 x 16 x 16 elements
    rng = np.random.default_rng(7)
    for nvar in (0, 3):
        K = max(nvar, 1)
        x = np.stack([SPECIALS[np.arange(4096) % 16]] * K)
        vc = np.stack([SPECIALS[(np.arange(4096) // 16) % 16]] * K)
        vu = np.stack([SPECIALS[(np.arange(4096) // 256) % 16]] * K)
        coef = np.array([rows[(k + 1) % len(rows)] for k in range(K)], np.float32)
        out.append((f"special_nvar{nvar}", nvar, x, vu, vc, coef))
        out.append((f"special_nvar{nvar}_nou", nvar, x, None, vc, coef))
    return out


def fusion_cases():
    """-> list of (name, nvar, lat [nvar][n], bg [n], objs [nobj][n], masks [nobj][n], mix, rnf)"""
    out, i = [], 0
    mixes = (0.3, 0.01, 0.99, 0.0, 0.65, 0.0447, 0.9)
    for n in GLUE_N:
        for nvar in (0,) + GLUE_NVAR:
            for nobj, rnf in itertools.product((0, 1, 2, 4), (0, 1)):
                rng = np.random.default_rng(900 + i)
                K = max(nvar, 1)
                lat, bg = rng.standard_normal((K, n)).astype(F16), rng.standard_normal(n).astype(F16)
                objs = rng.standard_normal((nobj, n)).astype(F16)
                u8 = rng.integers(0, 256, (nobj, n))
                hard = (i // 2 + i // 8) % 2
                masks = (u8 > 127).astype(F16) if hard else (u8.astype(np.float32) / np.float32(255)).astype(F16)
                out.append((f"n{n}_nvar{nvar}_nobj{nobj}_rnf{rnf}_{'hard' if hard else 'soft'}", nvar, lat, bg, objs, masks,
                            mixes[i % len(mixes)], rnf))
                i += 1
    for nvar in (0, 2):  # the special values in the latents, the background and the objects, under the six atlas masks
        for rnf in (0, 1):
            K, n = max(nvar, 1), 1536
            e = np.arange(n)
            lat = np.stack([SPECIALS[(e + k) % 16] for k in range(K)])
            bg = SPECIALS[(e // 16) % 16]
            objs = np.stack([SPECIALS[(e * 7 + 3) % 16], SPECIALS[(e // 4) % 16]])
            masks = np.stack([ATLAS_MASKS[e // 256], ATLAS_MASKS[(e // 256 + 2) % 6]])
            out.append((f"special_nvar{nvar}_rnf{rnf}", nvar, lat, bg, objs, masks, 0.3, rnf))
    return out
