"""What include/mvoc_hip.h promises about mvoc_temporal_qkv_attn_f16, through the C ABI (mvoc_amd._ffi), on the constructions of
tests/tfused_contract.py (shown sound on the CPU by tests/test_tfused_contract_cpu.py):

  A  exact selection: the output row EQUALS the selected integer value row, small scores and the large-score twin
  B  uniform attention within one fp16 ulp of the exact frame mean; all-zero rows EQUAL fp16(ln_bias) of the value channels
  L  section A at every (B, u) pair -- LayerNorm is the only thing that varies -- and the inexact edges (constant rows, narrow rows)
  R  three random distributions against fp64 per (sample, head) at tfused_contract.HEAD_BOUND and per sample at TFUSED_BOUND
  D  in EVERY case: operands at 0 / 16 / 128 mod 256 inside all-NaN allocations, every described output element written, no other
  T  the unfused twin: every case of A and L through mvoc_row_stats_f16 -> mvoc_gemm_f16 (ln_rowsum / ln_bias / ln_stats, the same folded
     weights) -> mvoc_temporal_attn_f16, the chain unet.py takes on injected sites: the same integers wherever its single late rounding
     can return them (tfused_contract.twin_failure says where, and why not everywhere), one fp16 ulp of its documented value elsewhere
  E  refusals: -2, an error text that names the entry, nothing written, and the unchanged descriptor accepted afterwards

hw walks below, at and above the block edges of the 4- and the 8-wave form and three blocks of either; the 8-wave form itself needs a
process of its own (tests/xs_forced_worker.py, started by tests/test_xs_contract_gpu.py, runs A, B and L there and compares the bits).
Every case is one launch of at most a few thousand rows.

Kernel perturbations tried on an MI355X against this file (A/B libraries, never committed; arithmetic only, no address changed):
  * the block-diagonal mask always true (a row sees its whole wave): A, B, L, R, the refusals' accepted run and the eps test tripped
    (A at c 64, hw 2: 1 956 of 3 072 elements, -24 != -29; R: rel-L2 0.58 per head);
  * the dm^2 correction of the variance dropped: ONLY section L tripped, at the pair (1024, 1) (c 64: 495 of 512 elements, -7.3125 !=
    -12); A, B and R passed;
  * the value constant of the neighbouring channel (ln_bias index r ^ 1): A, B, L and R tripped (A at c 128: all 1 024 elements)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_contract as AC  # noqa: E402
import launch_census as LC  # noqa: E402
import tfused_contract as TC  # noqa: E402
from mvoc_amd import ops  # noqa: E402
from mvoc_amd._ffi import lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return lib.mvoc_last_error().decode()


def run_case(case, check=True):
    """one launch on the case's layout, section D, then (check) the case's own check: the described output elements [ns, F, hw, c]"""
    L = TC.TFLayout(DEV, case)
    L.check_poison()
    rc = lib.mvoc_temporal_qkv_attn_f16(C.byref(L.desc()), _stream())
    assert rc == 0, _err()
    out = L.check_out()
    if check:
        ref = None
        if case["check"] == "random":
            ref = TC.fp64_reference(dict(case, x=L.T["x"].reshape(L.shape)))
        why = TC.failure(case, out, ref, AC.TFUSED_BOUND)
        assert why is None, why
    return out


def run_section(section, c):
    n = 0
    for case in TC.section_cases(section, c):
        run_case(case)
        n += 1
    return n


@pytest.mark.parametrize("c", TC.C_ALL)
def test_exact_selection(c):
    assert run_section("A", c) == 2 * len(TC.section_geometries("A", c))


@pytest.mark.parametrize("c", TC.C_ALL)
def test_uniform_attention_and_zero_rows(c):
    assert run_section("B", c) == 2 * len(TC.section_geometries("B", c))


@pytest.mark.parametrize("c", TC.C_ALL)
def test_layernorm_edges(c):
    assert run_section("L", c) == (len(TC.L_PAIRS) + 2) * len(TC.section_geometries("L", c))


@pytest.mark.parametrize("c", TC.C_ALL)
def test_random_per_head(c):
    assert run_section("R", c) == len(TC.DISTRIBUTIONS) * len(TC.section_geometries("R", c))


# ---- T: the unfused three-launch chain -------------------------------------------------------------------------------------------------
# The chain carries LayerNorm's (1 - delta) = 1 / sqrt(1 + 4 eps / u^2) in fp32 up to the addition of the channel's constant, where the
# fused kernel has rounded it away with x^: wherever the normalised term t and the constant cancel, the residue delta t survives the
# single rounding to fp16 (r = 0 comes out as -1.5e-4 for t = 30 at u = 2), at every (B, u) pair but (8192, 32), whose delta = 2e-8
# vanishes in fp32.  So no other pair can be bit-exact on this chain, and that one only with an rsqrt that returns 1 / 16 itself; tests/tfused_contract.py: twin_failure derives from the chain's documented arithmetic on which elements the integer itself is
# due (98.6 % of them at the least, 88 % at u = 0.5) and holds the rest to one fp16 ulp of t (1 - delta) + c plus the fp32 evaluation
# error.  tests/test_tfused_contract_cpu.py shows the chain's CPU model to meet exactly that, and to miss plain equality.
def _device_weights(W):
    if "dev" not in W:
        c = W["c"]
        W["dev"] = {"w_ln": W["lin"].w_ln.to(DEV), "ln": (W["ln_rowsum"].to(DEV), W["ln_bias"].to(DEV), TC.LN_EPS), "n": 3 * c}
    return W["dev"]


def run_twin(case):
    i, c, frames, hw, ns = case["geo"]
    Wd = _device_weights(case["W"])
    x = case["x"].to(DEV).reshape(-1, c).contiguous()
    stats = ops.row_stats(x, TC.LN_EPS)
    qkv = ops.linear(x, Wd["w_ln"], None, n_store=Wd["n"], ln=Wd["ln"] + (stats,))
    out = ops.temporal_attn(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:3 * c], nsample=ns, frames=frames, hw=hw, heads=c // 64)
    return out.reshape(ns, frames, hw, c)


@pytest.mark.parametrize("c", TC.C_ALL)
def test_unfused_twin_returns_the_same_integers(c):
    """the same integers wherever the chain's arithmetic can return them, one fp16 ulp of its documented value elsewhere (above)"""
    n = 0
    for section in ("A", "L"):
        for case in TC.section_cases(section, c):
            if case["check"] != "equal":
                continue  # the inexact edges of L belong to section R's bound, not to this comparison
            why = TC.twin_failure(case, run_twin(case))
            assert why is None, "unfused chain: " + why
            n += 1
    assert n == 2 * len(TC.section_geometries("A", c)) + len(TC.L_PAIRS) * len(TC.section_geometries("L", c))


# ---- E: refusals -----------------------------------------------------------------------------------------------------------------------
def _shift(field, nbytes):
    def change(d):
        setattr(d, field, getattr(d, field) + nbytes)
    return change


def _nsample_65536(d):
    d.nsample = 65536


REFUSALS = [("x off 16 bytes", _shift("x", 8)), ("x off by one element", _shift("x", 2)), ("wp off 16 bytes", _shift("wp", 8)),
            ("out off 16 bytes", _shift("out", 8)), ("ln_rowsum off 4 bytes", _shift("ln_rowsum", 2)),
            ("ln_bias off 4 bytes", _shift("ln_bias", 2)), ("nsample 65536", _nsample_65536)]


@pytest.mark.parametrize("what,change", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals(what, change):
    """a refused call launches nothing: the host entry returns before it forms the kernel's arguments"""
    geo = next(g for g in TC.geometries() if g[1:] == (320, 8, 7, 1))
    case = TC.exact_case(geo, TC.PAIRS[0])
    for shift in range(3):  # the operands at each of the contract's addresses
        L = TC.TFLayout(DEV, case, shift)
        d = L.desc()
        change(d)
        assert lib.mvoc_temporal_qkv_attn_f16(C.byref(d), _stream()) == -2, (what, _err())
        assert "temporal_qkv_attn" in _err(), _err()
        torch.cuda.synchronize()
        assert L.untouched(), what
        assert lib.mvoc_temporal_qkv_attn_f16(C.byref(L.desc()), _stream()) == 0, _err()  # the unchanged descriptor is accepted
        why = TC.failure(case, L.check_out())
        assert why is None, why


def test_ln_eps_is_honoured_as_given():
    """rows of variance 2^-8 (u = 2^-3): x^ = +-1 / sqrt(1 + 256 eps); two values of eps must give the two different fp64 answers"""
    geo = next(g for g in TC.geometries() if g[1:] == (128, 16, 9, 3))
    base = TC.random_case(geo, "wide")
    s = TC._exact_base(geo)[0]
    case = dict(base, x=(1 + 0.125 * (1 + s) / 2).to(torch.float16), key="tfE_eps")
    outs = []
    for eps in (1e-5, 1e-3):
        L = TC.TFLayout(DEV, case)
        d = L.desc()
        d.ln_eps = eps
        assert lib.mvoc_temporal_qkv_attn_f16(C.byref(d), _stream()) == 0, _err()
        out = L.check_out()
        W = case["W"]
        ref = LC.tfused_ref(d, {"x": L.T["x"]}, {"w": W["w"].to(DEV), "gamma": W["gamma"].to(DEV), "beta": W["beta"].to(DEV)})
        rel, mab = TC.head_errors(out, ref.reshape(L.shape))
        assert rel < TC.HEAD_BOUND[0] and mab < TC.HEAD_BOUND[1], (eps, rel, mab)
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])
