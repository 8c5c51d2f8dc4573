"""The constructions of the attention contract tests (tests/attn_contract.py) are sound: shown on the CPU, with the documented
rounding chain restated in torch (``emulate``), before any kernel is blamed.  For every (tq, tk, head_dim, causal) that sections A and
B of tests/test_attention_contract_gpu.py launch: the one-hot cases select exactly, the uniform cases sit within one fp16 ulp of the
exact mean and SEE a dropped key, the random cases of section C leave the emulated chain well inside the project's bounds, and the
layouts poison exactly what their descriptors do not describe."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_contract as AC  # noqa: E402
import launch_census as LC  # noqa: E402

CPU = torch.device("cpu")

# (tq, tk, head_dim, real dims, causal) of sections A and B
FLASH_AB = [(tq, tk, 64, 64, False) for tq in AC.FLASH_TQ for tk in AC.FLASH_TK]
FLASH_AB += [(33, tk, 96, 80, False) for tk in AC.HD96_TK]
LONG_AB = [(AC.LONG_TQ, tk, 64, 64, False) for tk in AC.LONG_TK]
ONEHOT_SHAPES = FLASH_AB + LONG_AB + [(t, t, 64, 64, True) for t in AC.CAUSAL_ONEHOT_T]
UNIFORM_SHAPES = FLASH_AB + LONG_AB + [(AC.HUGE_TQ, AC.HUGE_TK, 64, 64, False)] + [(t, t, 64, 64, True) for t in AC.CAUSAL_UNIFORM_T]


_gen = AC.gen_of


def test_onehot_cases_select_exactly():
    for tq, tk, hd, real, causal in ONEHOT_SHAPES:
        case = AC.onehot_case(tk, tq, real, _gen("onehot", tq, tk, hd, causal), hd=hd, causal=causal, groups=2, nqb=2)
        if causal:
            assert bool((case["sel"] <= torch.arange(tq)).all())
        o, o2 = AC.emulate_case(case, AC.default_scale(hd, real), causal)
        AC.assert_equal_rows(o, case["exp"], f"onehot {tq}x{tk} hd {hd} causal {causal}")
        AC.assert_equal_rows(o2, case["exp2"], f"onehot v2 {tq}x{tk} hd {hd} causal {causal}")
    for frames in AC.T_FRAMES:  # the temporal form: codes of the frame index over 5 dims
        case = AC.onehot_case(frames, frames, 64, _gen("t", frames), ndims=5, groups=6)
        AC.assert_equal_rows(AC.emulate_case(case, 0.125)[0], case["exp"], f"temporal onehot {frames}")


def test_staircase_and_boundary_cases_select_exactly():
    for tk in AC.LONG_TK:
        for step in AC.STAIR_STEPS:
            case = AC.staircase_case(tk, AC.LONG_TQ, step, _gen("stair", tk, step), groups=2)
            assert bool((case["sel"] >= 64 * ((tk - 1) // 64)).all())
            AC.assert_equal_rows(AC.emulate_case(case, 0.125)[0], case["exp"], f"staircase {tk} step {step}")
            # the staircase is what it says: the best score of tile t exceeds tile t - 1's by 2 * step natural units (all but the last)
            s = (case["q"][0, 0, 0].float() @ case["k"][0].float().t()) * 0.125
            tops = torch.stack([s[64 * t:64 * t + 64].max() for t in range((tk - 1) // 64)] or [s.max()])
            if len(tops) > 1:
                assert torch.equal(tops[1:] - tops[:-1], torch.full((len(tops) - 1,), 2.0 * step))
    for t in AC.CAUSAL_ONEHOT_T:
        case = AC.causal_boundary_case(t, _gen("bound", t), groups=2)
        AC.assert_equal_rows(AC.emulate_case(case, 0.125, True)[0], case["exp"], f"causal boundary {t}")
        if t > 1:  # ... and it does pin the boundary: one key more, or one key less, changes rows
            q, k, v = case["q"][0, 0].float(), case["k"][0].float(), case["v"][0].float()
            s = q @ k.t() * 0.125
            for shift in (1, -1):
                vis = torch.arange(t)[None, :] <= (torch.arange(t)[:, None] + shift).clamp(min=0)
                p = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
                assert int(((p @ v).double() != case["exp"][0, 0]).any(1).sum()) >= (t - 1) // 2


def test_uniform_cases_within_one_ulp_and_see_a_dropped_key():
    for tq, tk, hd, real, causal in UNIFORM_SHAPES:
        what = f"uniform {tq}x{tk} hd {hd} causal {causal}"
        case = AC.uniform_case(tk, tq, _gen("uniform", tq, tk, hd, causal), hd=hd, hd_real=real, causal=causal, groups=2)
        s = torch.matmul(case["q"].float(), case["k"][:, None].float().transpose(-1, -2))
        assert not bool(s.any()), what  # every score is exactly 0
        o, o2 = AC.emulate_case(case, AC.default_scale(hd, real), causal)
        AC.assert_within_ulp(o, case["exp"], what)
        AC.assert_within_ulp(o2, case["exp2"], what + " v2")
        if tk < 2 or causal:
            continue
        # one key less (the last one: what a ragged-tile mask off by one does; and a random one) moves the mean by >= 1 ulp in at least
        # half of the 64 columns
        v = case["v"][0].double()
        for j in (tk - 1, int(torch.randint(0, tk, (1,), generator=_gen("drop", tk)))):
            less = (v.sum(0) - v[j]) / (tk - 1)
            full = case["exp"][0, 0, 0]
            moved = ((less - full).abs() >= AC.ulp16(full))[:min(real, 64)]
            assert int(moved.sum()) >= 32, (what, j, int(moved.sum()))
    for frames in AC.T_FRAMES:
        case = AC.uniform_case(frames, frames, _gen("tu", frames), groups=6)
        AC.assert_within_ulp(AC.emulate_case(case, 0.125)[0], case["exp"], f"temporal uniform {frames}")


def test_emulated_chain_on_the_random_inputs_is_inside_the_bounds():
    """per (batch entry, head) slice, every (tq, tk) of section C: the chain itself uses about a seventh of the rel-L2 bound, so a
    kernel that keeps the chain passes with room and the bound says something about a kernel that does not"""
    worst = [0.0, 0.0]
    for tq in AC.RAND_TQ:
        for tk in AC.RAND_TK:
            case = AC.random_case(tk, tq, _gen("rand", tq, tk), groups=4, nqb=3)
            o = AC.emulate_case(case, 0.125)[0].double()
            p = torch.softmax(torch.matmul(case["q"].double(), case["k"][:, None].double().transpose(-1, -2)) * 0.125, -1)
            ref = torch.matmul(p, case["v"][:, None].double())
            rel, mab = AC.slice_errors(o, ref, (0, 1))
            worst = [max(worst[0], rel), max(worst[1], mab)]
    print(f"emulated chain, section C inputs: worst slice rel-L2 {worst[0]:.3g}, max abs {worst[1]:.3g}")
    assert worst[0] < LC.FLASH_BOUND[0] and worst[1] < LC.FLASH_BOUND[1], worst


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("pair", [False, True])
def test_flash_layout_extents_and_poison(fused, pair):
    for (nbatch, heads, kv_bdiv), tq, tk, hd in [((1, 1, 1), 1, 1, 64), ((3, 2, 1), 33, 77, 64), ((6, 1, 3), 130, 145, 64), ((2, 5, 2), 33, 2, 64),
                                                 ((3, 2, 1), 33, 17, 96)]:
        if pair and hd == 96:
            continue
        L = AC.Layout(CPU, nbatch, heads, tq, tk, kv_bdiv=kv_bdiv, hd=hd, pair=pair, fused=fused, pad_rows=0 if (not fused and tq == 1) else 2)
        d = L.desc()
        ext = LC.attn_extents(d)
        for name in L.inputs + L.outputs:
            assert L.extent_of(name) == ext[name] == L.T[name].numel(), name
            assert L.T[name].data_ptr() % 16 == 0
        for p, t in (("q", tq), ("k", tk), ("v", tk), ("o", tq)):
            assert getattr(d, p + "_ts") % 8 == 0 and getattr(d, p + "_ts") >= heads * hd
            assert getattr(d, p + "_bs") >= t * getattr(d, p + "_ts")
        L.fill(AC.random_case(tk, tq, _gen("lay", tq, tk), hd=hd, groups=L.nkv * heads, nqb=kv_bdiv))
        L.check_poison()
        # the logical views see what was put, and launch_census.attn_ref reads the layout as the kernel is told to
        ref = LC.attn_ref(d, L.T)
        assert ref.shape == (nbatch, tq, heads, hd) and not bool(torch.isnan(ref).any())
        for name in L.outputs:  # untouched outputs: all sentinel, and the checker says so
            assert LC.stray_writes(L.T[name]) == 0 and LC.unwritten(L.views[name](L.T[name]).contiguous()) == nbatch * tq * heads * hd
            with pytest.raises(AssertionError, match="never written"):
                L.check_out(name)
        # the checker catches a write into a padding column, and a NaN in a described element
        o = L.T["out"]
        L.views["out"](o).fill_(1.0)
        L.check_out("out")
        pad = o.base_alloc[o.storage_offset() + heads * hd:]  # the first padding column of row 0 (with one row: the slack)
        pad[0] = 3.0
        with pytest.raises(AssertionError, match="written"):
            L.check_out("out")
        pad.view(torch.int16)[0] = LC.OUT_SENTINEL
        L.check_out("out")
        o[0] = float("nan")
        with pytest.raises(AssertionError, match="NaN"):
            L.check_out("out")


@pytest.mark.parametrize("fused", [True, False])
def test_temporal_layout_extents_and_poison(fused):
    for nsample, hw, frames, heads in [(2, 1, 1, 1), (2, 3, 7, 5), (2, 5, 32, 1), (3, 4, 16, 2)]:
        L = AC.TLayout(CPU, nsample, hw, frames, heads, fused=fused)
        d = L.desc()
        ext = LC.tattn_extents(d)
        for name in L.inputs + L.outputs:
            assert L.extent_of(name) == ext[name] == L.T[name].numel(), name
            assert L.T[name].data_ptr() % 16 == 0
        for p in "qkvo":
            ps, ts, bs = (getattr(d, p + s) for s in ("_ps", "_ts", "_bs"))
            assert ps % 8 == 0 and ps >= heads * 64 and ts > hw * ps - 1 and bs > frames * ts - 1 and ts % 8 == 0
        case = AC.onehot_case(frames, frames, 64, _gen("tl", frames), ndims=5, groups=nsample * hw * heads)
        L.fill(case)
        L.check_poison()
        # the expectation in logical order is what the fp64 reference computes from the filled layout
        assert float((LC.tattn_ref(d, L.T) - L.expected(case)).abs().max()) < 1e-30  # (fp64: the other keys weigh e^-144, not 0)
        with pytest.raises(AssertionError, match="never written"):
            L.check_out("out")


def test_flash_fill_and_expected_agree_with_the_reference():
    """Layout.fill / Layout.expected put every (kv batch entry, head) draw where launch_census.attn_ref finds it: the fp64 reference
    of a filled one-hot layout is the expectation (kv_bdiv, several heads, the pair form)"""
    for nbatch, heads, kv_bdiv in AC.FORMS:
        L = AC.Layout(CPU, nbatch, heads, 33, 77, kv_bdiv=kv_bdiv, pair=True)
        case = AC.onehot_case(77, 33, 64, _gen("fill", nbatch), groups=L.nkv * heads, nqb=kv_bdiv)
        L.fill(case)
        d = L.desc()
        assert float((LC.attn_ref(d, L.T) - L.expected(case)).abs().max()) < 1e-30  # (fp64: the other keys weigh e^-144, not 0)
        assert float((LC.attn_ref(d, L.T, "out2") - L.expected(case, "exp2")).abs().max()) < 1e-30


def test_grid_sizes_of_section_c():
    sizes = {AC.flash_grid(nb, h, tq) for nb, h, _ in AC.RAND_FORMS for tq in AC.RAND_TQ}
    sizes |= {AC.flash_grid(nb, h, tq) for nb, h, _, tq, _ in AC.GRID_EXTRA}
    assert set(range(1, 10)) <= sizes and max(sizes) == 18, sorted(sizes)
