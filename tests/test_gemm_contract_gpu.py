"""What include/mvoc_hip.h promises about mvoc_gemm_f16, through the C ABI (mvoc_amd._ffi: pitches, offsets and n_store cannot all be said
through mvoc_amd.ops), on every tile id at the shapes no other test launches.  Constructions and checks are tests/gemm_contract.py's,
shown sound on the CPU by tests/test_gemm_contract_cpu.py, which also asserts what the walk covers:

  families  GENERAL tiles 1, 2, 3, 4 at K = 32, 64, 96, 128 (one to four steps of the two-stage loop); GLDS tiles 11, 12, 13, 61, 62, 64 at
            K = 64, 128, 192, 256, 320 (one to five 64-deep steps; 61 / 62 / 64 step 32); G8 tiles 81, 82 at the same K (nk = 1, 2, 3, 4
            take the four arms of G8_KTILE, 5 the trailing odd tile behind a pair); AUTO tile 0 on the cases of tiles 3, 13 and 81, the
            sub-pixel form included, and on the chunk-major cases of tile 82 (the route mvoc_amd.ops takes to both forms)
            Every loop here has two stages (gemm_contract.RING), so "ring depth + 2" is four K tiles; the fifth (K = 320) is walked
            because the families' K lists hold it, not because a ring asks for it.
            A forced tile 82 runs the 320-wide kernel only without activation, without LayerNorm fold + row-add, and on plain,
            temporal3 or same-size stride-1 conv launches; every other case "on 82" (launch8's epi 0, the stride-2 / pad_mode /
            upsampled / odd-size convs) is sent to the 256-wide kernel by mvoc_launch_gemm8 and exercises tile 81's code from
            tile 82's host path.
  shapes    M = 1, 31 .. 33, 127 .. 129, 255 .. 257, 513; N = 32, bn - 32, bn, bn + 32, 2 bn + 32 per tile width bn (GEGLU: 64, bn,
            bn + 64 on the tiles that carry it); n_store trims 0, 8, 24 (GENERAL also 6: n_store % 4 == 2, the scalar store tail)
  epilogues none, bias, bias + residual, row-add (divisors 1, 64, 100, m; 65 puts one 256-row tile on five row-add rows), SiLU, GELU,
            GEGLU with and without residual, the LayerNorm fold with and without row-add and under GEGLU (launch8's epi 1, 0, 2, 3)
  places    ldo - cols 0 / 8 (/ 4: epi_lds off), ldr / ld_rowadd / lda pads 0 / 16, a as the inner column block of a wider matrix,
            operands at 0 / 16 / 128 mod 256 (out also 8)
  gathers   conv3x3 on (1, 1, 1), (2, 3, 5), (3, 9, 7), (5, 8, 8): stride 1, stride 2 on the odd sizes, pad_mode 1 with stride 2,
            nearest upsample (8, 8) -> (11, 7) and 2 x; two sources 64 + 128 (GENERAL 8 + 24) in every mode; cin = 8 in k = 96 (GENERAL);
            temporal3 on (2, 1, 5), (3, 2, 1), (2, 3, 21), (1, 16, 16); the sub-pixel form at m = 1024 / 2048, n = 32, 256, 288 (81); the
            chunk-major form on conv (2, 23, 23) and temporal (2, 3, 171), cin 64 / 128, with and without residual + row-add (82)
  split-K   forced 2 and 4 at k = 64 split {1, 2} in a workspace of exactly split m n 4 bytes; the automatic policy once (m 513, n 64,
            k 1024: gemm.hip's final rule gives two slices to tile 13; the test sees both slabs written)
  stats     chan_sums and row_moments (ld = ceil(n / 256) + 1) requested on 81 / 82 at m = 256, 512, n = 256 .. 352, and where they are
            not honoured: m = 257, an activation, n_store < n, split-K (chan_sums through the reduce pass is honoured)

  A  integer operands: the output EQUALS the fp64 answer as bits; chan_sums / row_moments EQUAL the sums of the stored output
  L  the LayerNorm fold with dyadic {mean, rstd}: exact likewise
  C  SiLU / GELU / GEGLU on integer draws: per element within launch_census.gemm_epilogue's derived bound
  D  random data against launch_census.gemm_ref (fp64 with the chain's rounding points), rel-L2 per 32-row group under the bound of the
     test of the same form in tests/test_ops_gpu.py (gemm_contract.D_BOUND names them); the K loop, GEGLU, every gather, a third of
     the rest.  The sub-pixel form is held in A only: its packed weights are sums rounded once more than the logical conv's.
  in EVERY case: the return code is one of 0, -1, -2, -3 (and 0); undescribed input elements are NaN and none reaches a result; every
     described output element is written and finite; no other element of the out, chan_sums, row_moments and workspace allocations
     changes; statistics are either reported by the query functions and right over their described extent, or wholly untouched
  E  refusals: the documented negative code, an error text that names the entry, no output byte changed, both queries answer 0; the
     corrected descriptor then runs

Every launch is at most 2 048 rows by 704 columns by K = 1 728.  What this file cannot hold: which tile the automatic choice takes
(dispatch policy), launches beyond 2^31 bytes, and speed.

Conv weights with k > 9 cin keep ZEROS in the columns at and past 9 cin (they are described): the kernels zero the activation side and
still multiply.

Worst section-D figures measured on an MI355X (per family the case closest to its bound, rel-L2 of its worst 32-row group; printed
by the tests):
  GENERAL 2.9e-5 (bound 1.5e-3: upsampled conv (2, 8, 8) -> (16, 16), cin 8 in k 96, tile 2); 2.7e-5 (bound 1e-3: plain, tile 1)
  GLDS    4.2e-5 (bound 1e-3: m 127, n 192, k 128, bias + row-add, tile 62); 3.1e-5 (bound 1.5e-3: temporal (2, 1, 5), tile 12)
  G8      2.4e-5 (bound 1e-3: m 513, n 224, k 320, tile 81); 4.1e-5 (bound 1.5e-3: chunk-major temporal (2, 3, 171), tile 82)
  AUTO    9.9e-5 (bound 2e-3: m 128, n 320, k 192, GEGLU under the LayerNorm fold)
The reference carries the chain's own rounding points, so what is left is rounding flips of another accumulation order; the CPU
emulation stays under 7 % of every bound.

Kernel perturbations tried on an MI355X against this file, on a scratch copy of the tree (never committed; each reads or waits on the
block's own LDS and registers, or reads inside the test's own allocations: wrong data at most):
  * gemm.hip, the direct-to-LDS ring: the barrier's drain of the LDS-DMA (vmcnt(0)) weakened to vmcnt(1).  TRIPPED A, L, C and D on
    every GLDS tile it could (23 of 48 functions, AUTO included: 2 364 of 65 664 elements of an integer case wrong, C 56 over its
    bound); G8 and GENERAL passed, as they must.
  * gemm8.hip, the epilogue table: the bias chunk read one 8-channel chunk further inside the table.  TRIPPED A, C and D on tiles 81
    and 82 (25 273 of 28 448 elements; rel-L2 0.58 in a row group); L passed: the LayerNorm fold takes no bias.
  * gemm8.hip, G8_KTILE: the counted per-tile wait (wait_tile: vmcnt 6 / 7) raised by one.  NOT seen, all passed.  Likewise the wait
    of the last-but-one tile ((t) + 2 == nk: vmcnt(0)) raised to vmcnt(1): NOT seen.  The piece such a wait no longer covers was
    issued a phase and two barriers earlier; at K <= 320 with the operands in L2 it has always landed.  What this file holds of the
    eight-phase loop is that every arm of G8_KTILE (nk = 1 .. 5) multiplies the right tiles; a count too LARGE by one is beyond a
    functional test of this size (as tests/test_xs_contract_gpu.py found for xslin.hip's steady state).
  * gemm.hip, the general kernel: the w row guard `n0 + row < p.N` removed (run on the GENERAL cases whose rows past n stay inside
    the 64 KB the test owns behind w: 530 cases).  NOT seen, all passed: the rows past n feed accumulators of channels >= n, which
    no epilogue stores.  The guard keeps the kernel inside w; it does not change a result, and no test of results can hold it.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_contract as GC  # noqa: E402
from mvoc_amd._ffi import ACT_GEGLU, lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _err():
    return lib.mvoc_last_error().decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


KERNEL = GC.library_kernel(lib, _stream, torch.cuda.synchronize)
TILE_PARAMS = [(f, t) for f in GC.FAMILIES for t in GC.TILES[f]]
TILE_IDS = [f"{f}-{t}" for f, t in TILE_PARAMS]


def _section(section, family, tile):
    figures = []
    cases = GC.section_cases(section, family, tile)
    for p in cases:
        GC.run_case(section, p, DEV, KERNEL, figures, _err)
    if figures:
        what, worst, lim = max(figures, key=lambda f: f[1] / f[2])
        print(f"section D {family} tile {tile}: {len(figures)} cases, worst 32-row group rel-L2 {worst:.3g} (bound {lim}) at {what}")
    return len(cases)


# ---- A, L, C, D ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,tile", TILE_PARAMS, ids=TILE_IDS)
def test_integers_exact(family, tile):
    assert _section("A", family, tile) > 0


@pytest.mark.parametrize("family,tile", [ft for ft in TILE_PARAMS if ft[0] != "GENERAL"], ids=[i for i in TILE_IDS if not i.startswith("GENERAL")])
def test_layernorm_fold_exact(family, tile):
    assert _section("L", family, tile) > 0


@pytest.mark.parametrize("family,tile", TILE_PARAMS, ids=TILE_IDS)
def test_activations_within_the_derived_bound(family, tile):
    assert _section("C", family, tile) > 0


@pytest.mark.parametrize("family,tile", TILE_PARAMS, ids=TILE_IDS)
def test_random_per_row_group(family, tile):
    assert _section("D", family, tile) > 0


# ---- E: refusals ---------------------------------------------------------------------------------------------------------------------
def _set(**kw):
    def change(d, L):
        for name, v in kw.items():
            setattr(d, name, v)
    return change


PLAIN = dict(m=129, n=128, k=64, bias=True, resid=True)
CONV = dict(mode="conv", geo=(3, 9, 7), cin=64, n=64, bias=True)
TEMPORAL = dict(mode="temporal", geo=(2, 3, 21), cin=64, n=64, bias=True)
STATS = dict(m=256, n=512, k=128, bias=True, chan_sums=True, row_moments=True)
# (what, family, tile, base case, change, code, words of the error text that only this refusal sets)
REFUSALS = [
    ("n 48", "GLDS", 13, PLAIN, _set(n=48), -2, "n (48) must be a multiple of 32"),
    ("k 48", "GLDS", 13, PLAIN, _set(k=48, cin=48, c1=48), -2, "k (48) of 32"),
    ("cin 12", "GENERAL", 3, dict(CONV, cin=8, k=96), _set(cin=12, c1=12), -2, "cin (12)"),
    ("c1 below cin without a2", "GLDS", 13, PLAIN, _set(c1=32), -1, "second source"),
    ("ldo not a multiple of 4", "GLDS", 13, PLAIN, lambda d, L: setattr(d, "ldo", d.ldo + 2), -2, "ldo/ldr"),
    ("conv m", "GLDS", 13, CONV, lambda d, L: setattr(d, "m", d.m - 1), -1, "conv m != nimg"),
    ("temporal k", "GLDS", 13, TEMPORAL, _set(cin=32, c1=32), -1, "temporal k != 3*cin"),
    ("GEGLU n 96", "GLDS", 13, dict(PLAIN, n=96, resid=False), _set(act=ACT_GEGLU, n_store=0), -2, "GEGLU needs n"),
    ("GEGLU tile 2", "GENERAL", 2, PLAIN, _set(act=ACT_GEGLU, n_store=0), -2, "tile 2 cannot do GEGLU"),
    ("GEGLU tile 12", "GLDS", 12, PLAIN, _set(act=ACT_GEGLU, n_store=0), -2, "tile 12 needs"),
    ("GEGLU tile 62", "GLDS", 62, PLAIN, _set(act=ACT_GEGLU, n_store=0), -2, "tile 62 needs"),
    ("GEGLU tile 64", "GLDS", 64, PLAIN, _set(act=ACT_GEGLU, n_store=0), -2, "tile 64 needs"),
    ("GEGLU tile 82", "G8", 82, PLAIN, _set(act=ACT_GEGLU, n_store=0), -2, "82: no GEGLU"),
    ("LayerNorm fold without ln_stats", "GLDS", 13, dict(PLAIN, ln=True, bias=False), _set(ln_stats=None), -2, "LayerNorm folding needs"),
    ("k_order 1 on a plain launch", "G8", 82, dict(PLAIN, m=1025, n=320, k=64), _set(k_order=1), -2, "k_order = 1"),
    ("k_order 1 below 1024 rows", "G8", 82, dict(CONV, geo=(5, 8, 8), n=320), _set(k_order=1), -2, "k_order = 1"),
    ("sub-pixel below 1024 rows", "G8", 81, dict(CONV, geo=(2, 8, 8), upsample=1, up=(16, 16)), _set(upsample=2, k=256), -2, "sub-pixel"),
    ("sub-pixel with a residual", "G8", 81, dict(CONV, geo=(1, 16, 16), upsample=2, up=(32, 32), resid=False),
     lambda d, L: (setattr(d, "resid", d.out), setattr(d, "ldr", d.ldo)), -2, "sub-pixel"),
    ("row_moments_ld 1 at n 512", "G8", 81, STATS, _set(row_moments_ld=1), -2, "row_moments_ld 1 <"),
    ("tile 7", "GLDS", 13, PLAIN, _set(tile=7), -1, "unknown tile 7"),
    ("tile 14 with split-K and chan_sums", "GLDS", 13, dict(m=256, n=128, k=128, bias=True, split_k=2, workspace=True, chan_sums=True),
     _set(tile=14), -1, "unknown tile 14"),
    ("row-add divisor 1 on tile 81", "G8", 81, dict(PLAIN, rowadd_div=64), _set(rowadd_div=1), -2, "tiles 81 / 82 need"),
    ("row-add divisor 63 on tile 82", "G8", 82, dict(PLAIN, rowadd_div=64), _set(rowadd_div=63), -2, "tiles 81 / 82 need"),
]


@pytest.mark.parametrize("what,family,tile,base,change,code,words", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals(what, family, tile, base, change, code, words):
    p = GC._case([], family, tile, **base)
    section = GC.section_of(p)
    L = GC.GemmLayout(DEV, p)
    L.fill(GC.draw(section, p))
    L.check_poison()
    d = L.desc()
    change(d, L)
    rc = lib.mvoc_gemm_f16(C.byref(d), _stream())
    text = _err()
    queries = (lib.mvoc_gemm_chan_sums_written(), lib.mvoc_gemm_row_moments_written())
    torch.cuda.synchronize()
    assert rc == code, (what, rc, text)
    assert "gemm" in text and words in text, (what, text)  # (a refusal that set no text would leave an earlier call's)
    assert queries == (0, 0), (what, queries)
    for name in L.outputs:
        assert L.untouched(name), f"{what}: {name} was written by a refused call"
    assert L.check_workspace() == 0
    GC.run_case(section, p, DEV, KERNEL, err=_err)  # the corrected descriptor is accepted and right
