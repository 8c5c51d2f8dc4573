"""CPU: the host side of the blend-scatter family and its plane movers -- every refusal of the twenty ``mvoc_pnp_blend_scatter_*``
entries and the four ``mvoc_*_planes*_f16`` movers, its return code, its exact text and its place in the order of the checks.

A refusal returns before the library makes any HIP call, so this needs no device: the descriptors are filled by hand and the
pointers are made up (nothing is ever read through them).  EVERY call here commits at least one fault -- a call that passed its
checks would launch a kernel on made-up pointers -- and the table ``EXPECTED`` says what comes back: (case, return code, text,
layouts, suffixes) for the entries mvoc_pnp_blend_scatter_<layout><suffix> of the two lists (with "planes": the movers
mvoc_<name>_f16).  ``{entry}`` in a text stands for the entry's name, ``{mover}`` for the name a mover speaks under.  The order of
the checks of an entry that takes variants is

    no-background, null table, nvar, active, the descriptor (null operand, nobj, dims, ndst), the source map, the table form's
    limits (height * width, 16-bit tap fields), the layout's preconditions (multiples of 8, alignment, grid)

and for every adjacent pair one case commits both faults: the earlier one is reported.  The table was recorded from the library
before its sixteen variant entries and four movers were folded into one body each; it holds for both.
"""
import ctypes as C

import pytest

X, X2, MASKS, TABLE, DST = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # made up, 16-byte aligned, never dereferenced
LAYOUTS = ("tokens", "nchw")
# suffix -> (signature, table form); signatures: pos (d), mapped (+ nsrc, obj_chunk), variants (+ nvar), sel (+ active), table (+ table)
SUFFIXES = {"": ("pos", None), "_mapped": ("mapped", None), "_variants": ("variants", None), "_variants_sel": ("sel", None),
            "_placed": ("table", "shift"), "_placed_variants": ("table", "shift"), "_resampled": ("table", "map"),
            "_resampled_variants": ("table", "map"), "_warped": ("table", "map2"), "_bilinear": ("table", "taps")}
ENTRIES = [f"mvoc_pnp_blend_scatter_{layout}{suffix}" for suffix in SUFFIXES for layout in LAYOUTS]
MOVER_FORMS = {"shift_planes": "shift", "gather_planes": "map", "gather_planes_warped": "map2", "gather_planes_bilinear": "taps"}
MOVERS = {f"mvoc_{name}_f16": form for name, form in MOVER_FORMS.items()}
# the suffixes by what their entries take, for the table below
ALL = tuple(SUFFIXES)
MAPPED, VARIANTS, SEL, TABLES = ALL[1:], ALL[2:], ALL[3:], ALL[4:]
PLACED, WARPS = ("_placed", "_placed_variants"), ("_warped", "_bilinear")
NO_LIMITS = ALL[1:8]  # a map, no limits of a table form
PLANES = tuple(MOVER_FORMS)

# nobj = 2, one frame of 2 x 2 pixels, 8 channels; two variants, both injecting
BASE = dict(x=X, x2=0, masks=MASKS, chunk_stride=32, f_stride=32, p_stride=8, nobj=2, frames=1, height=2, width=2, channels=8,
            mask_h=2, mask_w=2, base_chunk0=0, ndst=2, nsrc=3, obj_chunk=(1, 2), nvar=2, active=3, table=TABLE)
MOVER_BASE = dict(src=X, dst=DST, nplane=1, frames=1, h=2, w=2, table=TABLE)

NO_BG = dict(base_chunk0=-1)
NULL_TABLE = dict(table=0)
NVAR_9 = dict(nvar=9)
ACTIVE_0 = dict(active=0)
NULL_X = dict(x=0)
NOBJ_5 = dict(nobj=5)
HEIGHT_0 = dict(height=0)
NDST_3 = dict(ndst=3)
NULL_CHUNKS = dict(obj_chunk=None)
CHUNK_HIGH = dict(obj_chunk=(1, 3))
HW_31 = dict(height=65536, width=32768)      # height * width = 2^31
TAP_ROWS = dict(height=65535, width=2)       # one row too many for the 16-bit tap fields
CHANNELS_4 = dict(channels=4)
ODD_X = dict(x=X + 2)
GRID = dict(frames=1 << 20, height=1024, width=1024)  # 2^40 work items per tensor: 2^32 blocks
TAP_GRID = dict(frames=1 << 20, height=65535, width=2)


def _is(sig, form):
    return lambda layout, s, f: (sig is None or s in sig) and (form is None or f in form)


MAPPED_UP, VARIANTS_UP, SEL_UP = ("mapped", "variants", "sel", "table"), ("variants", "sel", "table"), ("sel", "table")
# (case, the entries it applies to (layout, signature, form) -> bool, the faults it commits)
CASES = [
    ("no_background", lambda layout, s, f: (layout, s) != ("tokens", "pos"), NO_BG),
    ("null_desc", _is(None, None), dict(null_desc=True)),
    ("null_table", _is(("table",), None), NULL_TABLE),
    ("nvar_0", _is(VARIANTS_UP, None), dict(nvar=0)),
    ("nvar_9", _is(VARIANTS_UP, None), NVAR_9),
    ("active_0", _is(SEL_UP, None), ACTIVE_0),
    ("active_2^nvar", _is(SEL_UP, None), dict(active=4)),
    ("null_x", _is(None, None), NULL_X),
    ("null_masks", _is(None, None), dict(masks=0)),
    ("nobj_0", _is(None, None), dict(nobj=0)),
    ("nobj_5", _is(None, None), NOBJ_5),
    ("frames_0", _is(None, None), dict(frames=0)),
    ("height_0", _is(None, None), HEIGHT_0),
    ("width_0", _is(None, None), dict(width=0)),
    ("channels_0", _is(None, None), dict(channels=0)),
    ("mask_h_0", _is(None, None), dict(mask_h=0)),
    ("mask_w_0", _is(None, None), dict(mask_w=0)),
    ("ndst_3", _is(None, None), NDST_3),
    ("ndst_-1", _is(None, None), dict(ndst=-1)),
    ("null_obj_chunk", _is(MAPPED_UP, None), NULL_CHUNKS),
    ("nsrc_0", _is(MAPPED_UP, None), dict(nsrc=0)),
    ("nsrc_nobj+2", _is(MAPPED_UP, None), dict(nsrc=4)),
    ("obj_chunk_-1", _is(MAPPED_UP, None), dict(obj_chunk=(-1, 2))),
    ("obj_chunk_nsrc", _is(MAPPED_UP, None), CHUNK_HIGH),
    ("hw_2^31", _is(None, ("map2", "taps")), HW_31),
    ("tap_rows_65535", _is(None, ("taps",)), TAP_ROWS),
    ("tap_cols_65535", _is(None, ("taps",)), dict(height=2, width=65535)),
    ("channels_4", lambda layout, s, f: layout == "tokens", CHANNELS_4),
    ("chunk_stride_4", lambda layout, s, f: layout == "tokens", dict(chunk_stride=4)),
    ("f_stride_4", lambda layout, s, f: layout == "tokens", dict(f_stride=4)),
    ("p_stride_4", lambda layout, s, f: layout == "tokens", dict(p_stride=4)),
    ("odd_x", lambda layout, s, f: layout == "tokens", ODD_X),
    ("odd_x2", lambda layout, s, f: layout == "tokens", dict(x2=X2 + 8)),
    ("grid", _is(None, None), GRID),
    # ---- two faults: the earlier check speaks ----
    ("no_background+null_table", _is(("table",), None), {**NO_BG, **NULL_TABLE}),
    ("no_background+nvar_9", _is(VARIANTS_UP, None), {**NO_BG, **NVAR_9}),
    ("no_background+null_x", lambda layout, s, f: s in ("pos", "mapped") and (layout, s) != ("tokens", "pos"), {**NO_BG, **NULL_X}),
    ("null_table+nvar_9", _is(("table",), None), {**NULL_TABLE, **NVAR_9}),
    ("nvar_9+active_0", _is(SEL_UP, None), {**NVAR_9, **ACTIVE_0}),
    ("nvar_9+null_x", _is(("variants",), None), {**NVAR_9, **NULL_X}),
    ("active_0+null_x", _is(SEL_UP, None), {**ACTIVE_0, **NULL_X}),
    ("null_x+nobj_5", _is(None, None), {**NULL_X, **NOBJ_5}),
    ("nobj_5+height_0", _is(None, None), {**NOBJ_5, **HEIGHT_0}),
    ("height_0+ndst_3", _is(None, None), {**HEIGHT_0, **NDST_3}),
    ("ndst_3+null_obj_chunk", _is(MAPPED_UP, None), {**NDST_3, **NULL_CHUNKS}),
    ("ndst_3+channels_4", lambda layout, s, f: (layout, s) == ("tokens", "pos"), {**NDST_3, **CHANNELS_4}),
    ("ndst_3+grid", lambda layout, s, f: (layout, s) == ("nchw", "pos"), {**NDST_3, **GRID}),
    ("null_obj_chunk+nsrc_0", _is(MAPPED_UP, None), {**NULL_CHUNKS, "nsrc": 0}),
    ("nsrc_0+obj_chunk_nsrc", _is(MAPPED_UP, None), {"nsrc": 0, **CHUNK_HIGH}),
    ("obj_chunk_nsrc+hw_2^31", _is(None, ("map2", "taps")), {**CHUNK_HIGH, **HW_31}),
    ("obj_chunk_nsrc+channels_4", lambda layout, s, f: layout == "tokens" and s != "pos" and f not in ("map2", "taps"),
     {**CHUNK_HIGH, **CHANNELS_4}),
    ("obj_chunk_nsrc+grid", lambda layout, s, f: layout == "nchw" and s != "pos" and f not in ("map2", "taps"), {**CHUNK_HIGH, **GRID}),
    ("hw_2^31+tap_cols_65535", _is(None, ("taps",)), dict(height=65536, width=65535)),
    ("hw_2^31+channels_4", lambda layout, s, f: layout == "tokens" and f in ("map2", "taps"), {**HW_31, **CHANNELS_4}),
    ("hw_2^31+grid", lambda layout, s, f: layout == "nchw" and f in ("map2", "taps"), {**HW_31, "frames": 1 << 20}),
    ("tap_rows_65535+channels_4", lambda layout, s, f: layout == "tokens" and f == "taps", {**TAP_ROWS, **CHANNELS_4}),
    ("tap_rows_65535+grid", lambda layout, s, f: layout == "nchw" and f == "taps", TAP_GRID),
    ("channels_4+odd_x", lambda layout, s, f: layout == "tokens", {**CHANNELS_4, **ODD_X}),
    ("odd_x+grid", lambda layout, s, f: layout == "tokens", {**ODD_X, **GRID}),
]

MOVER_GRID = dict(nplane=1 << 20, frames=1 << 10, h=1024, w=1024)  # 2^50 elements
MOVER_CASES = [
    ("null_src", _is(None, None), dict(src=0)),
    ("null_dst", _is(None, None), dict(dst=0)),
    ("null_table", _is(None, None), dict(table=0)),
    ("src_is_dst", _is(None, None), dict(dst=X)),
    ("nplane_0", _is(None, None), dict(nplane=0)),
    ("frames_0", _is(None, None), dict(frames=0)),
    ("h_0", _is(None, None), dict(h=0)),
    ("w_0", _is(None, None), dict(w=0)),
    ("hw_2^31", _is(None, ("map2", "taps")), dict(h=65536, w=32768)),
    ("tap_rows_65535", _is(None, ("taps",)), dict(h=65535, w=2)),
    ("tap_cols_65535", _is(None, ("taps",)), dict(h=2, w=65535)),
    ("grid", _is(None, None), MOVER_GRID),
    # ---- two faults: the earlier check speaks ----
    ("null_table+src_is_dst", _is(None, None), dict(table=0, dst=X)),
    ("src_is_dst+nplane_0", _is(None, None), dict(dst=X, nplane=0)),
    ("nplane_0+hw_2^31", _is(None, ("map2", "taps")), dict(nplane=0, h=65536, w=32768)),
    ("negative_dims+grid", _is(None, None), dict(nplane=-(1 << 20), frames=-(1 << 10), h=1024, w=1024)),
    ("hw_2^31+tap_cols_65535", _is(None, ("taps",)), dict(h=65536, w=65535)),
    ("hw_2^31+grid", _is(None, ("map2", "taps")), dict(nplane=1 << 20, h=65536, w=32768)),
    ("tap_rows_65535+grid", _is(None, ("taps",)), dict(nplane=1 << 20, frames=1 << 10, h=65535, w=64)),
]

NO_BACKGROUND = ("{entry}: base_chunk0 = -1 (no background chunk) is taken by mvoc_pnp_blend_scatter_tokens only (a mapped entry "
                 "expresses the layout as nsrc = nobj, obj_chunk[j] = j; the nchw entries need chunk 0)")
TAP_FIELDS = "does not fit the 16-bit tap fields (< 65535)"
BOTH = "tokens nchw"
EXPECTED = [
    ('no_background', -1, NO_BACKGROUND, 'nchw', ALL),
    ('no_background', -1, NO_BACKGROUND, 'tokens', MAPPED),
    ('null_desc', -1, 'pnp: null operand', BOTH, ALL),
    ('null_table', -1, 'pnp placed: null offset table', BOTH, PLACED),
    ('null_table', -1, 'pnp resampled: null map table', BOTH, ('_resampled',)),
    ('null_table', -1, 'pnp resampled variants: null map table', BOTH, ('_resampled_variants',)),
    ('null_table', -1, 'pnp warped: null map table', BOTH, ('_warped',)),
    ('null_table', -1, 'pnp bilinear: null tap table', BOTH, ('_bilinear',)),
    ('nvar_0', -1, 'pnp variants: nvar 0 not in [1, 8]', BOTH, VARIANTS),
    ('nvar_9', -1, 'pnp variants: nvar 9 not in [1, 8]', BOTH, VARIANTS),
    ('active_0', -1, 'pnp variants: active mask 0x0 not in [1, 2^nvar = 4)', BOTH, SEL),
    ('active_2^nvar', -1, 'pnp variants: active mask 0x4 not in [1, 2^nvar = 4)', BOTH, SEL),
    ('null_x', -1, 'pnp: null operand', BOTH, ALL),
    ('null_masks', -1, 'pnp: null operand', BOTH, ALL),
    ('nobj_0', -2, 'pnp: nobj 0 not in [1,4]', BOTH, ALL),
    ('nobj_5', -2, 'pnp: nobj 5 not in [1,4]', BOTH, ALL),
    ('frames_0', -1, 'pnp: bad dims', BOTH, ALL),
    ('height_0', -1, 'pnp: bad dims', BOTH, ALL),
    ('width_0', -1, 'pnp: bad dims', BOTH, ALL),
    ('channels_0', -1, 'pnp: bad dims', BOTH, ALL),
    ('mask_h_0', -1, 'pnp: bad dims', BOTH, ALL),
    ('mask_w_0', -1, 'pnp: bad dims', BOTH, ALL),
    ('ndst_3', -1, 'pnp: ndst 3 not in {0 (= 2), 1, 2}', BOTH, ALL),
    ('ndst_-1', -1, 'pnp: ndst -1 not in {0 (= 2), 1, 2}', BOTH, ALL),
    ('null_obj_chunk', -1, 'pnp mapped: null obj_chunk', BOTH, MAPPED),
    ('nsrc_0', -1, 'pnp mapped: nsrc 0 not in [1, nobj + 1 = 3]', BOTH, MAPPED),
    ('nsrc_nobj+2', -1, 'pnp mapped: nsrc 4 not in [1, nobj + 1 = 3]', BOTH, MAPPED),
    ('obj_chunk_-1', -1, 'pnp mapped: obj_chunk[0] = -1 not in [0, nsrc = 3)', BOTH, MAPPED),
    ('obj_chunk_nsrc', -1, 'pnp mapped: obj_chunk[1] = 3 not in [0, nsrc = 3)', BOTH, MAPPED),
    ('hw_2^31', -2, 'pnp warped: height * width does not fit the int32 map entries', BOTH, ('_warped',)),
    ('hw_2^31', -2, 'pnp bilinear: height * width does not fit an int', BOTH, ('_bilinear',)),
    ('tap_rows_65535', -2, 'pnp bilinear: height 65535 or width 2 ' + TAP_FIELDS, BOTH, ('_bilinear',)),
    ('tap_cols_65535', -2, 'pnp bilinear: height 2 or width 65535 ' + TAP_FIELDS, BOTH, ('_bilinear',)),
    ('channels_4', -2, 'pnp tokens: channels/strides must be multiples of 8', 'tokens', ALL),
    ('chunk_stride_4', -2, 'pnp tokens: channels/strides must be multiples of 8', 'tokens', ALL),
    ('f_stride_4', -2, 'pnp tokens: channels/strides must be multiples of 8', 'tokens', ALL),
    ('p_stride_4', -2, 'pnp tokens: channels/strides must be multiples of 8', 'tokens', ALL),
    ('odd_x', -2, 'pnp tokens: x and x2 must be 16-byte aligned', 'tokens', ALL),
    ('odd_x2', -2, 'pnp tokens: x and x2 must be 16-byte aligned', 'tokens', ALL),
    ('grid', -2, 'pnp tokens: grid too large', 'tokens', ALL),
    ('grid', -2, 'pnp nchw: grid too large', 'nchw', ALL),
    ('no_background+null_table', -1, NO_BACKGROUND, BOTH, TABLES),
    ('no_background+nvar_9', -1, NO_BACKGROUND, BOTH, VARIANTS),
    ('no_background+null_x', -1, NO_BACKGROUND, 'nchw', ('', '_mapped')),
    ('no_background+null_x', -1, NO_BACKGROUND, 'tokens', ('_mapped',)),
    ('null_table+nvar_9', -1, 'pnp placed: null offset table', BOTH, PLACED),
    ('null_table+nvar_9', -1, 'pnp resampled: null map table', BOTH, ('_resampled',)),
    ('null_table+nvar_9', -1, 'pnp resampled variants: null map table', BOTH, ('_resampled_variants',)),
    ('null_table+nvar_9', -1, 'pnp warped: null map table', BOTH, ('_warped',)),
    ('null_table+nvar_9', -1, 'pnp bilinear: null tap table', BOTH, ('_bilinear',)),
    ('nvar_9+active_0', -1, 'pnp variants: nvar 9 not in [1, 8]', BOTH, SEL),
    ('nvar_9+null_x', -1, 'pnp variants: nvar 9 not in [1, 8]', BOTH, ('_variants',)),
    ('active_0+null_x', -1, 'pnp variants: active mask 0x0 not in [1, 2^nvar = 4)', BOTH, SEL),
    ('null_x+nobj_5', -1, 'pnp: null operand', BOTH, ALL),
    ('nobj_5+height_0', -2, 'pnp: nobj 5 not in [1,4]', BOTH, ALL),
    ('height_0+ndst_3', -1, 'pnp: bad dims', BOTH, ALL),
    ('ndst_3+null_obj_chunk', -1, 'pnp: ndst 3 not in {0 (= 2), 1, 2}', BOTH, MAPPED),
    ('ndst_3+channels_4', -1, 'pnp: ndst 3 not in {0 (= 2), 1, 2}', 'tokens', ('',)),
    ('ndst_3+grid', -1, 'pnp: ndst 3 not in {0 (= 2), 1, 2}', 'nchw', ('',)),
    ('null_obj_chunk+nsrc_0', -1, 'pnp mapped: null obj_chunk', BOTH, MAPPED),
    ('nsrc_0+obj_chunk_nsrc', -1, 'pnp mapped: nsrc 0 not in [1, nobj + 1 = 3]', BOTH, MAPPED),
    ('obj_chunk_nsrc+hw_2^31', -1, 'pnp mapped: obj_chunk[1] = 3 not in [0, nsrc = 3)', BOTH, WARPS),
    ('obj_chunk_nsrc+channels_4', -1, 'pnp mapped: obj_chunk[1] = 3 not in [0, nsrc = 3)', 'tokens', NO_LIMITS),
    ('obj_chunk_nsrc+grid', -1, 'pnp mapped: obj_chunk[1] = 3 not in [0, nsrc = 3)', 'nchw', NO_LIMITS),
    ('hw_2^31+tap_cols_65535', -2, 'pnp bilinear: height * width does not fit an int', BOTH, ('_bilinear',)),
    ('hw_2^31+channels_4', -2, 'pnp warped: height * width does not fit the int32 map entries', 'tokens', ('_warped',)),
    ('hw_2^31+channels_4', -2, 'pnp bilinear: height * width does not fit an int', 'tokens', ('_bilinear',)),
    ('hw_2^31+grid', -2, 'pnp warped: height * width does not fit the int32 map entries', 'nchw', ('_warped',)),
    ('hw_2^31+grid', -2, 'pnp bilinear: height * width does not fit an int', 'nchw', ('_bilinear',)),
    ('tap_rows_65535+channels_4', -2, 'pnp bilinear: height 65535 or width 2 ' + TAP_FIELDS, 'tokens', ('_bilinear',)),
    ('tap_rows_65535+grid', -2, 'pnp bilinear: height 65535 or width 2 ' + TAP_FIELDS, 'nchw', ('_bilinear',)),
    ('channels_4+odd_x', -2, 'pnp tokens: channels/strides must be multiples of 8', 'tokens', ALL),
    ('odd_x+grid', -2, 'pnp tokens: x and x2 must be 16-byte aligned', 'tokens', ALL),
    ('null_src', -1, '{mover}: null operand', 'planes', PLANES),
    ('null_dst', -1, '{mover}: null operand', 'planes', PLANES),
    ('null_table', -1, '{mover}: null operand', 'planes', PLANES),
    ('src_is_dst', -1, '{mover}: in place (src == dst) is not supported', 'planes', PLANES),
    ('nplane_0', -1, '{mover}: bad dims', 'planes', PLANES),
    ('frames_0', -1, '{mover}: bad dims', 'planes', PLANES),
    ('h_0', -1, '{mover}: bad dims', 'planes', PLANES),
    ('w_0', -1, '{mover}: bad dims', 'planes', PLANES),
    ('hw_2^31', -2, '{mover}: h * w does not fit the int32 map entries', 'planes', ('gather_planes_warped',)),
    ('hw_2^31', -2, '{mover}: h * w does not fit an int', 'planes', ('gather_planes_bilinear',)),
    ('tap_rows_65535', -2, '{mover}: h 65535 or w 2 ' + TAP_FIELDS, 'planes', ('gather_planes_bilinear',)),
    ('tap_cols_65535', -2, '{mover}: h 2 or w 65535 ' + TAP_FIELDS, 'planes', ('gather_planes_bilinear',)),
    ('grid', -2, '{mover}: grid too large', 'planes', PLANES),
    ('null_table+src_is_dst', -1, '{mover}: null operand', 'planes', PLANES),
    ('src_is_dst+nplane_0', -1, '{mover}: in place (src == dst) is not supported', 'planes', PLANES),
    ('nplane_0+hw_2^31', -1, '{mover}: bad dims', 'planes', ('gather_planes_warped', 'gather_planes_bilinear')),
    ('negative_dims+grid', -1, '{mover}: bad dims', 'planes', PLANES),
    ('hw_2^31+tap_cols_65535', -2, '{mover}: h * w does not fit an int', 'planes', ('gather_planes_bilinear',)),
    ('hw_2^31+grid', -2, '{mover}: h * w does not fit the int32 map entries', 'planes', ('gather_planes_warped',)),
    ('hw_2^31+grid', -2, '{mover}: h * w does not fit an int', 'planes', ('gather_planes_bilinear',)),
    ('tap_rows_65535+grid', -2, '{mover}: h 65535 or w 64 ' + TAP_FIELDS, 'planes', ('gather_planes_bilinear',)),
]


def _kind(entry):
    """(layout, signature, form) of an entry's name"""
    if entry in MOVERS:
        return "planes", "mover", MOVERS[entry]
    layout, _, suffix = entry[len("mvoc_pnp_blend_scatter_"):].partition("_")
    return (layout,) + SUFFIXES["_" + suffix if suffix else ""]


def cases_of(entry):
    """the (case, faults) pairs that apply to an entry"""
    kind = _kind(entry)
    return [(name, faults) for name, applies, faults in (MOVER_CASES if entry in MOVERS else CASES) if applies(*kind)]


def call(entry, faults):
    """one call of ``entry`` on the base arguments with ``faults`` laid over them -> (return code, mvoc_last_error())"""
    from mvoc_amd._ffi import PnpDesc, lib
    fn = getattr(lib, entry)
    if entry in MOVERS:
        a = {**MOVER_BASE, **faults}
        rc = fn(a["src"], a["dst"], a["nplane"], a["frames"], a["h"], a["w"], a["table"], None)
        return rc, lib.mvoc_last_error().decode()
    a = {**BASE, **faults}
    d = PnpDesc()
    for field, _ in PnpDesc._fields_:
        setattr(d, field, a[field])
    sig = _kind(entry)[1]
    chunks = None if a["obj_chunk"] is None else (C.c_int32 * len(a["obj_chunk"]))(*a["obj_chunk"])
    args = {"pos": (), "mapped": (a["nsrc"], chunks), "variants": (a["nsrc"], chunks, a["nvar"]),
            "sel": (a["nsrc"], chunks, a["nvar"], a["active"]), "table": (a["nsrc"], chunks, a["nvar"], a["active"], a["table"])}[sig]
    rc = fn(None if a.get("null_desc") else C.byref(d), *args, None)
    return rc, lib.mvoc_last_error().decode()


def _expected():
    want = {}
    for case, rc, text, layouts, suffixes in EXPECTED:
        for layout in layouts.split():
            for suffix in suffixes:
                entry = f"mvoc_{suffix}_f16" if layout == "planes" else f"mvoc_pnp_blend_scatter_{layout}{suffix}"
                assert (entry, case) not in want, f"{entry} / {case} is listed twice"
                want[entry, case] = (rc, text.replace("{entry}", entry).replace("{mover}", suffix))
    return want


def test_the_table_lists_every_case_of_every_entry_once_and_nothing_else():
    from mvoc_amd import _ffi
    bound = [n for n in _ffi.SIGNATURES if n.startswith("mvoc_pnp_blend_scatter_") or "_planes" in n]
    assert sorted(bound) == sorted(ENTRIES + list(MOVERS)) and len(ENTRIES) == 20 and len(MOVERS) == 4
    assert sorted(_expected()) == sorted((entry, case) for entry in ENTRIES + list(MOVERS) for case, _ in cases_of(entry))


@pytest.mark.parametrize("entry", ENTRIES + list(MOVERS))
def test_every_refusal_keeps_its_code_its_text_and_its_place(entry):
    want = _expected()
    wrong = []
    for case, faults in cases_of(entry):
        got = call(entry, faults)
        assert got[0] in (-1, -2), f"{entry} / {case}: not refused ({got})"  # anything else went on to HIP
        if got != want[entry, case]:
            wrong.append((case, got, want[entry, case]))
    assert not wrong, "\n".join(f"{entry} / {case}: got {got}, expected {exp}" for case, got, exp in wrong)
