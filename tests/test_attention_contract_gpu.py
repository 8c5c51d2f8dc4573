"""What include/mvoc_hip.h promises about mvoc_flash_attn_f16, mvoc_temporal_attn_f16 and mvoc_temporal_qkv_attn_f16, through the C ABI
(mvoc_amd._ffi: padded batch strides cannot be said through mvoc_amd.ops), on constructions whose answer is known without a softmax
(tests/attn_contract.py; shown sound on the CPU by tests/test_attention_contract_cpu.py):

  A  one-hot selection: the output row EQUALS the selected integer value row (torch.equal)
  B  uniform attention: within one fp16 ulp of the exact integer mean (causal: of the prefix mean of every row)
  C  random data against fp64 at the project's own bounds, rel-L2 per (batch entry, head) / per sample; every grid size 1..9
  D  in EVERY case of A-C: undescribed input elements are NaN and none reaches a result, every described output element is written,
     no other element of the output allocations is (Layout.check_out)
  E  refusals: the documented negative code, an error text that names the entry, nothing written
  F  the default kernel choice returns the bits of the explicit ones

Flash cases run the phase kernel (pipelined = 1) and the software-pipelined kernel (pipelined = 2) and compare the two bit for bit.
Where the pipelined kernel does not apply the phase kernel runs alone, and nothing is skipped: the head_dim 96 cases (2 in A, 2 in B)
and the causal cases (3 + 3 in A, 3 in B).  Every case is one launch of at most a few thousand rows."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_contract as AC  # noqa: E402
import launch_census as LC  # noqa: E402
from mvoc_amd._ffi import TFusedDesc, lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
I16 = torch.int16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return lib.mvoc_last_error().decode()


def run_flash(L, modes=None):
    """launch the layout once per kernel that applies, section D on every output of every launch, the kernels' results bit-equal:
    name -> described output elements [nbatch, tq, heads, hd]"""
    modes = modes or ((1, 2) if L.hd == 64 and not L.causal else (1,))
    first = None
    for mode in modes:
        L.reset_outputs()
        d = L.desc(mode)
        rc = lib.mvoc_flash_attn_f16(C.byref(d), _stream())
        assert rc == 0, _err()
        vals = {name: L.check_out(name) for name in L.outputs}
        if first is None:
            first = vals
        else:
            for name in L.outputs:
                assert torch.equal(first[name].view(I16), vals[name].view(I16)), f"{name}: pipelined = {mode} differs from pipelined = {modes[0]}"
    return first


def run_temporal(L):
    rc = lib.mvoc_temporal_attn_f16(C.byref(L.desc()), _stream())
    assert rc == 0, _err()
    return L.check_out("out")


def flash_layout(i, nbatch, heads, kv_bdiv, tq, tk, **kw):
    """the i-th case of a walk: fused column views with 2 padding rows and 8 padding columns / contiguous operands with 3 padding rows"""
    return AC.Layout(DEV, nbatch, heads, tq, tk, kv_bdiv=kv_bdiv, fused=i % 2 == 0, pad_rows=2 + i % 2, **kw)


def check_exact(L, case, what):
    L.fill(case)
    out = run_flash(L)
    AC.assert_equal_rows(out["out"], L.expected(case), what)
    if L.pair:
        AC.assert_equal_rows(out["out2"], L.expected(case, "exp2"), what + " (out2)")


def check_ulp(L, case, what):
    L.fill(case)
    out = run_flash(L)
    AC.assert_within_ulp(out["out"], L.expected(case), what)
    if L.pair:
        AC.assert_within_ulp(out["out2"], L.expected(case, "exp2"), what + " (out2)")


SMALL = [(tq, tk) for tq in AC.FLASH_TQ for tk in AC.FLASH_TK]
FORM_IDS = ["-".join(map(str, f)) for f in AC.FORMS]


# ---- A: one-hot selection, exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pair"])
@pytest.mark.parametrize("form", AC.FORMS, ids=FORM_IDS)
def test_flash_onehot_exact(form, pair):
    nbatch, heads, kv_bdiv = form
    for i, (tq, tk) in enumerate(SMALL):
        L = flash_layout(i, nbatch, heads, kv_bdiv, tq, tk, pair=pair)
        case = AC.onehot_case(tk, tq, 64, AC.gen_of("A", form, pair, tq, tk), groups=L.nkv * heads, nqb=kv_bdiv)
        check_exact(L, case, f"one-hot {form} {tq}x{tk}")


@pytest.mark.parametrize("tk", AC.HD96_TK)
def test_flash_onehot_exact_head_dim_96(tk):
    """CLIP ViT-H's form: 80 real dims, 16 zero dims, scale 1 / sqrt(80); the phase kernel only"""
    nbatch, heads, kv_bdiv = 3, 2, 1
    L = flash_layout(tk, nbatch, heads, kv_bdiv, 33, tk, hd=96, scale=1.0 / math.sqrt(80.0))
    check_exact(L, AC.onehot_case(tk, 33, 80, AC.gen_of("A96", tk), hd=96, groups=L.nkv * heads), f"one-hot head_dim 96 33x{tk}")


@pytest.mark.parametrize("t", AC.CAUSAL_ONEHOT_T)
def test_flash_onehot_exact_causal(t):
    """every query selects a random key <= itself; and the boundary form (twin keys 2m / 2m + 1 with one code) in which an even row is
    wrong by whole halves if key i + 1 is visible and an odd row if key i is not.  The phase kernel only."""
    nbatch, heads = 3, 2
    L = flash_layout(t, nbatch, heads, 1, t, t, causal=1)
    check_exact(L, AC.onehot_case(t, t, 64, AC.gen_of("Ac", t), causal=True, groups=nbatch * heads), f"causal one-hot {t}")
    L = flash_layout(t + 1, nbatch, heads, 1, t, t, causal=1)
    check_exact(L, AC.causal_boundary_case(t, AC.gen_of("Ab", t), groups=nbatch * heads), f"causal boundary {t}")


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pair"])
@pytest.mark.parametrize("tk", AC.LONG_TK)
def test_flash_onehot_exact_long_rows(tk, pair):
    """3 to 65 key tiles: the pipelined kernel's stage ring wraps; selected keys uniform over all tiles (the running maximum jumps by
    > 200 log2 units wherever a better key appears), then the staircases: a maximum that grows by 2.9 log2 units per tile (deferred,
    probabilities up to 2^8 against the stale maximum, then rescaled) and by 23 (a kernel that defers that overflows fp16)"""
    L = flash_layout(tk, 1, 1, 1, AC.LONG_TQ, tk, pair=pair)
    check_exact(L, AC.onehot_case(tk, AC.LONG_TQ, 64, AC.gen_of("Al", tk, pair)), f"one-hot long row {tk}")
    for step in AC.STAIR_STEPS:
        L = flash_layout(tk + step, 1, 1, 1, AC.LONG_TQ, tk, pair=pair)
        check_exact(L, AC.staircase_case(tk, AC.LONG_TQ, step, AC.gen_of("As", tk, pair, step)), f"staircase {tk} step {step}")


def temporal_layout(i, nsample, hw, frames, heads):
    return AC.TLayout(DEV, nsample, hw, frames, heads, fused=i % 2 == 0, pad_pix=1 + i % 3, pad_frames=1 + i % 2)


@pytest.mark.parametrize("heads", AC.T_HEADS)
def test_temporal_onehot_exact(heads):
    """every frames value 1..32 x hw below, at and above the pixels of a 32-row tile (4 at 8 frames, 2 at 16); codes of the frame index
    over 5 dims; padded pixel, frame and sample strides"""
    for frames in AC.T_FRAMES:
        for hw in AC.T_HW:
            L = temporal_layout(frames + hw, 2, hw, frames, heads)
            case = AC.onehot_case(frames, frames, 64, AC.gen_of("At", heads, frames, hw), ndims=5, groups=2 * hw * heads)
            L.fill(case)
            AC.assert_equal_rows(run_temporal(L), L.expected(case), f"temporal one-hot frames {frames} hw {hw}")


# ---- B: uniform attention, within one fp16 ulp of the exact mean ---------------------------------------------------------------------
@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pair"])
@pytest.mark.parametrize("form", AC.FORMS, ids=FORM_IDS)
def test_flash_uniform_mean(form, pair):
    nbatch, heads, kv_bdiv = form
    for i, (tq, tk) in enumerate(SMALL):
        L = flash_layout(i + 1, nbatch, heads, kv_bdiv, tq, tk, pair=pair)
        case = AC.uniform_case(tk, tq, AC.gen_of("B", form, pair, tq, tk), groups=L.nkv * heads, nqb=kv_bdiv)
        check_ulp(L, case, f"uniform {form} {tq}x{tk}")


@pytest.mark.parametrize("tk", AC.HD96_TK)
def test_flash_uniform_mean_head_dim_96(tk):
    L = flash_layout(tk, 3, 2, 1, 33, tk, hd=96, scale=1.0 / math.sqrt(80.0))
    check_ulp(L, AC.uniform_case(tk, 33, AC.gen_of("B96", tk), hd=96, hd_real=80, groups=6), f"uniform head_dim 96 33x{tk}")


@pytest.mark.parametrize("t", AC.CAUSAL_UNIFORM_T)
def test_flash_uniform_prefix_mean_causal(t):
    """row i is the mean of keys 0..i: the mask boundary of every row"""
    L = flash_layout(t, 3, 2, 1, t, t, causal=1)
    check_ulp(L, AC.uniform_case(t, t, AC.gen_of("Bc", t), causal=True, groups=6), f"causal prefix mean {t}")


@pytest.mark.parametrize("tq,tk", [(AC.LONG_TQ, tk) for tk in AC.LONG_TK] + [(AC.HUGE_TQ, AC.HUGE_TK)])
def test_flash_uniform_mean_long_rows(tq, tk):
    for pair in (False, True):
        L = flash_layout(tk + pair, 1, 1, 1, tq, tk, pair=pair)
        check_ulp(L, AC.uniform_case(tk, tq, AC.gen_of("Bl", tk, pair)), f"uniform long row {tq}x{tk}")


@pytest.mark.parametrize("heads", AC.T_HEADS)
def test_temporal_uniform_mean(heads):
    for frames in AC.T_FRAMES:
        for hw in AC.T_HW:
            L = temporal_layout(frames + hw + 1, 2, hw, frames, heads)
            case = AC.uniform_case(frames, frames, AC.gen_of("Bt", heads, frames, hw), groups=2 * hw * heads)
            L.fill(case)
            AC.assert_within_ulp(run_temporal(L), L.expected(case), f"temporal uniform frames {frames} hw {hw}")


# ---- C: random data against fp64 at the project's bounds -----------------------------------------------------------------------------
def check_random(i, nbatch, heads, kv_bdiv, tq, tk):
    pair = i % 3 == 2
    L = flash_layout(i, nbatch, heads, kv_bdiv, tq, tk, pair=pair)
    L.fill(AC.random_case(tk, tq, AC.gen_of("C", nbatch, heads, kv_bdiv, tq, tk), groups=L.nkv * heads, nqb=kv_bdiv))
    out = run_flash(L)
    d = L.desc()
    for name in L.outputs:  # rel-L2 per (batch entry, head) slice
        AC.assert_close_slices(out[name], LC.attn_ref(d, L.T, name), (0, 2), LC.FLASH_BOUND, f"random {(nbatch, heads, kv_bdiv)} {tq}x{tk} {name}")
    return AC.flash_grid(nbatch, heads, tq)


@pytest.mark.parametrize("form", AC.RAND_FORMS, ids=["3-2-1", "6-1-3"])
def test_flash_random_per_slice(form):
    grids = set()
    for i, (tq, tk) in enumerate((tq, tk) for tq in AC.RAND_TQ for tk in AC.RAND_TK):
        grids.add(check_random(i, *form, tq, tk))
    assert grids == {6, 12, 18}


def test_flash_random_every_small_grid():
    """grids of 1 to 9 blocks (the XCD remap of fewer blocks than XCDs, and of a count that is no multiple of 8), with the 6 / 12 / 18
    of the walk above: every grid size from 1 through 9 is launched"""
    grids = {check_random(i, *case) for i, case in enumerate(AC.GRID_EXTRA)}
    grids |= {AC.flash_grid(nb, h, tq) for nb, h, _ in AC.RAND_FORMS for tq in AC.RAND_TQ}
    assert set(range(1, 10)) <= grids, sorted(grids)


@pytest.mark.parametrize("hw", AC.RAND_T_HW)
def test_temporal_random_per_sample(hw):
    nsample, heads = 3, 2
    for frames in AC.T_FRAMES:
        L = temporal_layout(frames + hw, nsample, hw, frames, heads)
        L.fill(AC.random_case(frames, frames, AC.gen_of("Ct", frames, hw), groups=nsample * hw * heads))
        out = run_temporal(L)
        AC.assert_close_slices(out, LC.tattn_ref(L.desc(), L.T), (0,), AC.TATTN_BOUND, f"temporal random frames {frames} hw {hw}")


def build_tfused(c, frames, hw, nsample, seed, zero_qk=False):
    """a hand-filled mvoc_tfused_desc through launch_census.build_tfused (the pointer fields only say "set" and an alignment there);
    the slack around every input is then poisoned.  zero_qk: Wq = Wk = 0, re-packed by the product's own packers."""
    d0 = TFusedDesc()
    d0.x, d0.wp, d0.ln_rowsum, d0.ln_bias, d0.out = 256, 512, 768, 1024, 1280
    d0.nsample, d0.frames, d0.hw, d0.c, d0.heads, d0.ln_eps = nsample, frames, hw, c, c // 64, 1e-5
    d, bufs, Lg = LC.build_tfused(d0, DEV, seed)
    if zero_qk:
        from mvoc_amd.unet import Linear, pack_tfused_weights
        Lg["w"] = Lg["w"].clone()
        Lg["w"][:2 * c] = 0
        lin = Linear(Lg["w"]).fold_layernorm(Lg["gamma"], Lg["beta"], d.ln_eps)
        bufs["wp"].copy_(pack_tfused_weights(lin.w_ln, d.heads).reshape(-1))
        bufs["ln_rowsum"].copy_(lin.ln[0])
        bufs["ln_bias"].copy_(lin.ln[1])
    for name in ("x", "wp", "ln_rowsum", "ln_bias"):
        keep = bufs[name].clone()
        bufs[name].base_alloc.fill_(float("nan"))
        bufs[name].copy_(keep)
    return d, bufs, Lg


def run_tfused(d, bufs):
    rc = lib.mvoc_temporal_qkv_attn_f16(C.byref(d), _stream())
    assert rc == 0, _err()
    out = bufs["out"]
    assert LC.unwritten(out) == 0 and not bool(torch.isnan(out).any())
    assert LC.stray_writes(out) == 0
    return out.reshape(d.nsample, -1)


@pytest.mark.parametrize("c", AC.TF_C)
def test_tfused_random_per_sample(c):
    """hw below, at and above one block's pixels (4 waves x 32 / frames pixels: 16 / 8 / 4 at 8 / 16 / 32 frames); the
    MVOC_TFUSED_WAVES=8 instantiations need a process of their own and are not run here"""
    for frames in AC.TF_FRAMES:
        for hw in AC.TF_HW:
            for nsample in AC.TF_NS:
                d, bufs, Lg = build_tfused(c, frames, hw, nsample, 1000 * c + 10 * frames + hw + nsample)
                out = run_tfused(d, bufs)
                ref = LC.tfused_ref(d, bufs, Lg).reshape(nsample, -1)
                AC.assert_close_slices(out, ref, (0,), AC.TFUSED_BOUND, f"tfused c {c} frames {frames} hw {hw} nsample {nsample}")


@pytest.mark.parametrize("c", AC.TF_C)
def test_tfused_zero_qk_is_the_frame_mean(c):
    """Wq = Wk = 0: every score is 0, the output of every frame is the mean over the frames of the fp16-rounded value projections"""
    frames, hw, nsample = 16, 9, 3
    d, bufs, Lg = build_tfused(c, frames, hw, nsample, c, zero_qk=True)
    out = run_tfused(d, bufs)
    x = bufs["x"].reshape(-1, c)
    v = LC.r16(LC.r16(LC.layernorm64(x, Lg["gamma"], Lg["beta"], d.ln_eps)) @ Lg["w"][2 * c:].to(torch.float64).t())
    ref = v.reshape(nsample, frames, hw, c).mean(1, keepdim=True).expand(nsample, frames, hw, c).reshape(nsample, -1)
    AC.assert_close_slices(out, ref, (0,), AC.TFUSED_BOUND, f"tfused zero q/k c {c}")


# ---- E: refusals ---------------------------------------------------------------------------------------------------------------------
def _all_sentinel(bufs):
    torch.cuda.synchronize()
    return all(bool((b.base_alloc.view(I16) == LC.OUT_SENTINEL).all()) for b in bufs)


def _set(**kw):
    def change(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return change


def _shift_v2(d):
    d.v2 = d.v2 + 8  # 4 elements off a 16-byte boundary


FLASH_REFUSALS = [
    ("head_dim 80", False, _set(head_dim=80), -2),
    ("causal, tq != tk", False, _set(causal=1), -2),
    ("v2 with head_dim 96", True, _set(head_dim=96), -2),
    ("v2 without out2", True, _set(out2=None), -2),
    ("pipelined 3", False, _set(pipelined=3), -1),
    ("q_ts 68", False, _set(q_ts=68), -2),
    ("o_ts 66", False, _set(o_ts=66), -2),
    ("v2 off 16 bytes", True, _shift_v2, -2),
    ("nbatch 0", False, _set(nbatch=0), -1),
    ("null k", False, _set(k=None), -1),
]


@pytest.mark.parametrize("what,pair,change,code", FLASH_REFUSALS, ids=[r[0].replace(" ", "_").replace(",", "") for r in FLASH_REFUSALS])
def test_flash_refusals(what, pair, change, code):
    L = AC.Layout(DEV, 2, 1, 33, 77, pair=pair)
    L.fill(AC.random_case(77, 33, AC.gen_of("E"), groups=2))
    d = L.desc()
    change(d)
    assert lib.mvoc_flash_attn_f16(C.byref(d), _stream()) == code, (what, _err())
    assert "flash_attn" in _err(), _err()
    assert _all_sentinel([L.T[n] for n in L.outputs]), what
    d = L.desc()  # the unchanged descriptor is accepted
    assert lib.mvoc_flash_attn_f16(C.byref(d), _stream()) == 0, _err()
    L.check_out("out")


@pytest.mark.parametrize("what,change,code", [("frames 0", _set(frames=0), -2), ("frames 33", _set(frames=33), -2),
                                              ("k_ps 68", _set(k_ps=68), -2), ("hw 0", _set(hw=0), -1)],
                         ids=["frames_0", "frames_33", "k_ps_68", "hw_0"])
def test_temporal_refusals(what, change, code):
    L = AC.TLayout(DEV, 2, 3, 8, 1)
    L.fill(AC.random_case(8, 8, AC.gen_of("Et"), groups=6))
    d = LC.copy_desc(L.desc())
    change(d)
    assert lib.mvoc_temporal_attn_f16(C.byref(d), _stream()) == code, (what, _err())
    assert "temporal_attn" in _err(), _err()
    assert _all_sentinel([L.T["out"]]), what
    run_temporal(L)


@pytest.mark.parametrize("what,change,code", [("frames 4", _set(frames=4), -2), ("c 192, 3 heads", _set(c=192, heads=3), -2),
                                              ("c 128, 3 heads", _set(c=128, heads=3), -1), ("null wp", _set(wp=None), -1)],
                         ids=["frames_4", "c_192", "c_128_3_heads", "null_wp"])
def test_tfused_refusals(what, change, code):
    d0, bufs, _ = build_tfused(320, 8, 5, 1, 7)
    d = LC.copy_desc(d0)
    change(d)
    assert lib.mvoc_temporal_qkv_attn_f16(C.byref(d), _stream()) == code, (what, _err())
    assert "temporal_qkv_attn" in _err(), _err()
    assert _all_sentinel([bufs["out"]]), what
    run_tfused(d0, bufs)


# ---- F: the default kernel choice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tk", [257, 2049])
def test_flash_default_choice_returns_the_same_bits(tk):
    """pipelined = 0 picks a kernel by key count (below / from 2 048 keys): whichever it picks, the bits are those of pipelined = 1 and 2"""
    for pair in (False, True):
        L = flash_layout(tk, 2, 2, 1, 130, tk, pair=pair)
        L.fill(AC.random_case(tk, 130, AC.gen_of("F", tk, pair), groups=4, amp=1.5))
        out = run_flash(L, modes=(0, 1, 2))
        d = L.desc()
        for name in L.outputs:
            AC.assert_close_slices(out[name], LC.attn_ref(d, L.T, name), (0, 2), LC.FLASH_BOUND, f"default choice {tk} {name}")
