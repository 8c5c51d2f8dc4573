"""What include/mvoc_hip.h promises about mvoc_xs_linear_f16, through the C ABI (mvoc_amd._ffi: pitches, offsets and n_store cannot all
be said through mvoc_amd.ops), at the shapes no other test launches: T = n / 32 = 1..5 stages (below T = 4 the steady-state wait of
xslin.hip is never taken and every stage runs through the hand-counted special cases), m = 1 .. 257 rows (every lane clamped to row 0;
one partly filled block; a block and a row), K = 64, 128 and 320 (5, 9 and 21 DMA pieces per stage: wave 0 carries one more than waves
1..3).  Constructions and checks are tests/xs_contract.py's, shown sound on the CPU by tests/test_xs_contract_cpu.py:

  A  integer operands: the output EQUALS the fp64 answer, as bits (bias, residual, trimmed store, wide pitches)
  B  balanced rows under the folded LayerNorm: every normalised value is exactly +-1, the output EQUALS the integer answer -- also
     about a mean of +-1000, where a one-pass variance is lost
  C  SiLU / GELU (with and without residual) / GEGLU on sparse integer draws: per element within launch_census.xs_ref's derived bound
  D  random data against fp64 at the project's bounds (1.5e-3; 2.5e-3 with LayerNorm), rel-L2 per 32-row group; rows of large offset
  S  a weight set per 256 rows, two and three sets, exact
  in EVERY case: undescribed input elements are NaN (the lead and tail of x and wp, bytes 128..1023 of every constants piece, the
  residual's padding columns, row gaps and slack) and none reaches a result; every described output element is written; no other
  element of the output allocation is (rows >= m, columns >= n_store, the lead, the slack)
  E  refusals: the documented negative code, an error text that names the entry, nothing written; the unchanged descriptor then runs
  F  the forms only the environment selects, in one child process (tests/xs_forced_worker.py: MVOC_XS_RG=2, MVOC_TFUSED_WAVES=8): all
     of A-D and S again on the two-row-group kernels, the tfused cases of the attention contract set and sections A, B and L of the
     fused kernel's own set (tests/tfused_contract.py; compared by the SHA-256 of their bits) on the 8-wave kernels, and every output bit-equal to the default forms' (both xs forms chain the same MFMAs over s = 0 .. K/16 - 1 in the same order per output
     element and share the epilogue; the 4- and 8-wave tfused kernels differ in scheduling only)

Every launch is at most 768 rows by 192 columns.  Nothing is launched with a misaligned pointer.

Kernel perturbations tried on an MI355X against this file (A-D, S and F; never committed; each only reads LDS of the block's own ring
or residual slots at another time or place, so wrong data at most):
  * every special-case count of wait_stage (st == 0, st == 1, the last stage) raised by one: tripped A at K = 64 and 128 (m = 1, n = 64:
    32 of 64 elements wrong; m = 1, n = 32 with residual: all 24), C and D at K = 64 (m = 1, GELU: rel-L2 1 in the one row group) and
    F.  Only one-row launches saw it: there the awaited DMA is recent.  K = 320 and sections B and S passed.
  * cvec4 one quad further (constants of channels c + 4; the last quad from the poisoned tail): all of A, B, C, D, S and F tripped,
    A / D / S by the not-finite check (124 elements of the first case), B by equality (all 1 032), C by the bound.
  * the residual read from the other parity slot (one row group per wave): all of A, B, C, D, S and F tripped -- equality (725 of 744),
    the bound, rel-L2 0.53 to 0.76 per row group, and where the slot had never been filled the not-finite check.
  * every steady-state count raised by one: NOT seen, all passed.  The piece such a wait no longer covers was issued two stages, two
    barriers, earlier; at these sizes it has always landed.  What this file holds of the steady state is that its counts do not
    corrupt T = 4 and 5 (GEGLU: 6 stages); a count that is too LARGE by one there is beyond a functional test of this size."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402
import xs_contract as XC  # noqa: E402
import xs_forced_worker as FW  # noqa: E402
from mvoc_amd._ffi import ACT_GEGLU, ACT_NONE, lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
I16 = torch.int16
_BITS = {}  # case key -> output bits of the default forms, kept for section F (a section that has not run yet is run there)


def _err():
    return lib.mvoc_last_error().decode()


def _section(section, k):
    figures = []
    bits = FW.xs_bits(k, (section,), figures)
    assert len(bits) == len(XC.section_cases(section, k))
    for what, rel, lim in figures:
        print(f"{what}: worst 32-row group rel-L2 {rel:.3g} (bound {lim})")
    _BITS.update(bits)


# ---- A, B, C, D, S -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", XC.K)
def test_integers_exact(k):
    _section("A", k)


@pytest.mark.parametrize("k", XC.K)
def test_layernorm_fold_exact(k):
    """the census adds 2 ulp to its normalize replays; this set does not: the balanced rows leave the kernel nothing to round"""
    _section("B", k)


@pytest.mark.parametrize("k", XC.K)
def test_activations_within_the_derived_bound(k):
    _section("C", k)


@pytest.mark.parametrize("k", XC.K)
def test_random_per_row_group(k):
    _section("D", k)


@pytest.mark.parametrize("k", XC.K)
def test_weight_sets_exact(k):
    _section("S", k)


# ---- E: refusals ---------------------------------------------------------------------------------------------------------------------
def _set(**kw):
    def change(d, L):
        for name, v in kw.items():
            setattr(d, name, v)
    return change


def _shift(name, nbytes):
    def change(d, L):
        setattr(d, name, getattr(d, name) + nbytes)
    return change


def _rel(**kw):
    """fields relative to the layout's columns / n"""
    def change(d, L):
        for name, (base, off) in kw.items():
            setattr(d, name, {"cols": L.cols, "n": L.n}[base] + off)
    return change


# (what, residual in the base descriptor, change, code): the base is m = 384, n = 96, k = 64, act none, tight pitches
REFUSALS = [
    ("null x", True, _set(x=None), -1),
    ("null wp", True, _set(wp=None), -1),
    ("null out", True, _set(out=None), -1),
    ("m 0", True, _set(m=0), -1),
    ("n 48", True, _set(n=48), -1),
    ("k 96", True, _set(k=96), -2),
    ("act 4", True, _set(act=4), -1),
    ("act -1", True, _set(act=-1), -1),
    ("residual with GEGLU", True, _set(act=ACT_GEGLU, n=128), -2),
    ("GEGLU with n 96", False, _set(act=ACT_GEGLU), -2),
    ("n_store n - 32", True, _rel(n_store=("n", -32)), -2),
    ("n_store n - 4", True, _rel(n_store=("n", -4)), -2),
    ("ldo cols + 4", True, _rel(ldo=("cols", 4)), -2),
    ("out 8 bytes off", True, _shift("out", 8), -2),
    ("resid 8 bytes off", True, _shift("resid", 8), -2),
    ("ldr cols + 4", True, _rel(ldr=("cols", 4)), -2),
    ("wp_set_rows 64", True, _set(wp_set_rows=64), -2),
    ("wp_set_rows 256, m 384", True, _set(wp_set_rows=256), -2),
    ("x 8 bytes off", True, _shift("x", 8), -2),
    ("wp 8 bytes off", True, _shift("wp", 8), -2),
]


@pytest.mark.parametrize("what,resid,change,code", REFUSALS, ids=[r[0].replace(" ", "_").replace(",", "") for r in REFUSALS])
def test_refusals(what, resid, change, code):
    p = XC._case(0, 64, 384, 96, ACT_NONE, resid, 0, 0)
    case = XC.draw("A", p)
    L = XC.XsLayout(DEV, p)
    L.fill(case)
    L.check_poison()
    d = L.desc()
    change(d, L)
    assert lib.mvoc_xs_linear_f16(C.byref(d), FW.stream()) == code, (what, _err())
    assert "xs_linear" in _err(), _err()
    torch.cuda.synchronize()
    assert bool((L.T["out"].base_alloc.view(I16) == LC.OUT_SENTINEL).all()), what
    FW.KERNEL(L)  # the unchanged descriptor is accepted
    XC.assert_equal_bits(L.check_out("out"), L.reference()[0], what)


# ---- F: the forms the environment selects, in a process of their own -----------------------------------------------------------------
def test_forced_forms_return_the_same_bits(tmp_path):
    for name in FW.FORCED_ENV:
        assert name not in os.environ, f"{name} is set: this process does not run the default forms"
    assert FW.rows_per_block() == 128
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xs_forced_worker.py")
    run = subprocess.run([sys.executable, worker, str(tmp_path)], timeout=300, env=dict(os.environ, **FW.FORCED_ENV),
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    for k in XC.K:  # the default forms' bits: kept by the tests above, run here where they have not
        for section in XC.SECTIONS:
            if not all(XC.case_key(section, p) in _BITS for p in XC.section_cases(section, k)):
                _BITS.update(FW.xs_bits(k, (section,)))
    own = dict(_BITS)
    own.update(FW.tfused_bits(check=False))  # held to the fp64 reference by tests/test_attention_contract_gpu.py
    files = {f[:-3] for f in os.listdir(tmp_path) if f.endswith(".pt")}
    assert files == set(own), sorted(files ^ set(own))[:8]
    differ = [key for key in sorted(own) if not torch.equal(torch.load(os.path.join(tmp_path, key + ".pt")), own[key])]
    assert not differ, f"{len(differ)} of {len(own)} outputs differ between the default and the forced forms, first {differ[:8]}"
