"""The constructions of tests/stem_contract.py are sound (no GPU, the library is never called):

  * every reference agrees with an independent formulation on EVERY case of the walk (test_references_agree_with_independent_formulations:
    the emulation of an entry is that formulation -- F.conv2d, F.adaptive_avg_pool2d, the oracle's float32 timestep chain, torch permutes
    for the layout entries and permute_rows, integer passes over the PIL tables against PIL itself for mask_resize_u8, transformers'
    embedding lookup + position_ids / class-token concatenation for clip_embed, F.unfold for clip_patches, float32 torch for the
    elementwise entries, F.linear for conv1x1_small, the encoder written out in float32 for temporal_encoder4), inside the same poisoned
    allocations and through the same checker the GPU file uses;
  * the walk covers the work-item totals 1, 255, 256, 257, 513 (or the nearest reachable ones) and the per-entry lists of the issue;
  * every checker rejects a mutated emulation (test_mutation_is_rejected).  The cases that reject each mutation (first of them named):
      cos_sin_swapped         every timestep_embedding case (nb=1 dim=2 t=0: cos 1, sin 0)
      half_minus_1            40 of the 42 timestep_embedding cases (dim=6 nb=1 t=1 is the issue's; dim=2 divides by zero); the two
                              one-row cases with t = 0 and dim >= 4 cannot see it (every angle is 0)
      window_end_floored      adaptive_avgpool 7x9 -> 4x5, 3x2 -> 5x4, 1x1 -> 3x2 and the ragged totals; not the equal / divisible ones
      ky_kx_swapped           conv3x3_small at every size but 1x1 (1x5 stride 1 cin 3 cout 1: a one-row image reads one kernel ROW)
      stride2_origin_shifted  conv3x3_small stride 2 at every size (1x1: the shifted window reads x[0] with tap (0, 0), not (1, 1))
      coff_ignored            ncfhw_to_tokens and temporal_encoder4 at coff != 0: (8, 4), (11, 5), (9, 3)
      sibling_written         ncfhw_to_tokens and temporal_encoder4 at ldo > c: (8, 0), (8, 4), (11, 5), (9, 3)
      c_f_swapped             ncfhw_to_tokens / tokens_to_ncfhw wherever c != f and both exceed 1 (b=2 c=4 f=5 hw=7)
      py_px_swapped           clip_patches at patch >= 2: (4, 2), (6, 3), (28, 14)
      pos_row_div_t           clip_embed at t >= 2 with more than one row per sequence (text nb=1 t=2 c=8)
      class_row_last          clip_embed vision form at t >= 2 (vision nb=1 t=2 c=8)
      heads_swapped, residual_dropped, softmax_over_pixels
                              all seven temporal_encoder4 cases (f = 1 hw = 33 first); softmax_over_pixels also breaks the relayout
                              invariance wherever hw > 1 and f > 1
      score_scale_dropped     temporal_encoder4 f = 2, 5, 16, 32 and the constant-row case; not f = 1 (one key) and not the dominant
                              case (its softmax is saturated either way)
      threshold_ge_10         mask_finish whenever the byte 10 occurs: the atlas of all 256 values, the random n = 255, 256, 513
  * the measured bound of temporal_encoder4 (twice the eager-fp16 yardstick) stays under the 3e-3 of test_ops_gpu.py, the dominant case
    leads by 30 in both heads, the constant rows have variance 0;
  * the timestep bound holds for the reference's own float32 chain on t = 0..999 and fps = 1..64 at dim 320, and the GELU term for a
    float32 erf evaluation over every fp16 pattern.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402
import stem_contract as S  # noqa: E402

torch.set_grad_enabled(False)
F32, F64, H16 = torch.float32, torch.float64, torch.float16


@pytest.mark.parametrize("entry", S.ENTRIES)
def test_references_agree_with_independent_formulations(entry):
    for i, c in enumerate(S.cases(entry)):
        pl = S.Placed(S.problem(c), i)
        pl.emulate()
        assert pl.verify(repr(c)) <= 1.0


@pytest.mark.parametrize("entry", S.ENTRIES)
def test_walk_covers_the_totals(entry):
    if entry == "temporal_encoder4":
        works = {b * f * hw for b, f, hw, _ in S.enc_relayout_cases()}
        per_total = {t: sum(1 for b, f, hw, _ in S.enc_relayout_cases() if b * f * hw == t) for t in S.TOTALS}
    else:
        tot = [S.problem(c).work for c in S.cases(entry) if c.kind == "totals"]
        works, per_total = set(tot), {t: tot.count(t) for t in set(tot)}
    want = S.REACHABLE.get(entry, S.TOTALS)
    assert set(want) <= works, (entry, sorted(works))
    if entry not in ("act", "add", "scale", "gaussian_sample", "mask_finish"):  # (one extent: nothing to factorise)
        assert all(per_total[t] >= 2 for t in want if t >= 254), per_total


def test_factorisations_have_pairwise_different_extents():
    for table in (S.FACT2, S.FACT3, S.FACT4):
        assert set(table) == set(S.TOTALS)
        for total, facts in table.items():
            assert len(set(facts)) == len(facts) and all(math.prod(f) == total for f in facts)
            if total in (255, 256, 513):  # 1 and the prime 257 have no such factorisation
                assert len(facts) >= 3 and all(len(set(f)) == len(f) for f in facts), (total, facts)
                assert len({f[0] for f in facts}) == len(facts)  # no extent keeps its place


def test_walk_holds_the_per_entry_lists():
    P = lambda e, kind=None: [c.p for c in S.cases(e) if kind is None or c.kind == kind]
    conv = P("conv3x3_small", "entry")
    assert {(p["h"], p["w"]) for p in conv} == {(1, 1), (1, 5), (2, 3), (5, 4), (7, 9)} and len(conv) == 5 * 2 * 3 * 3 * 2 * 2
    assert {(p["cin"], p["cout"], p["stride"], p["bias"], p["silu"]) for p in conv} >= {(3, 1, 1, True, False), (8, 32, 2, False, True)}
    pool = {((p["h"], p["w"]), (p["oh"], p["ow"])) for p in P("adaptive_avgpool", "entry")}
    assert pool >= {((7, 9), (4, 5)), ((3, 2), (5, 4)), ((1, 1), (1, 1)), ((4, 4), (4, 4)), ((8, 6), (4, 2))}
    sm = P("softmax_rows", "entry")
    assert {(p["rows"], p["cols"]) for p in sm} == {(r, c) for r in (1, 3, 4, 5, 9) for c in (8, 504, 512, 520, 1032)}
    assert {p["shift"] % 4 for p in sm if p["rows"] == 1} >= {0, 1, 2}  # a one-row matrix of each special kind
    te = P("timestep_embedding", "entry")
    assert {(p["nb"], p["dim"]) for p in te} == {(nb, d) for nb in (1, 5) for d in (2, 6, 320)}
    assert {p["t0"] for p in te if p["nb"] == 1} == set(range(len(S.T_VALUES))) and set(S.T_VALUES) >= {0.0, 1.0, 8.0, 16.0, 500.0, 981.0, 999.0}
    assert any(t != int(t) for t in S.T_VALUES)
    for c in (4, 3):
        assert {(p["ldo"], p["coff"]) for p in P("ncfhw_to_tokens") if p["c"] == c} == {(c, 0), (8, 0), (8, 4), (11, 5)}
    assert {(p["ldo"], p["coff"]) for p in P("temporal_encoder4")} | {pt for *_, pt in S.enc_relayout_cases()} == {(4, 0), (8, 4), (9, 3)}
    assert {p["f"] for p in P("temporal_encoder4", "accuracy")} == {1, 2, 5, 16, 32}
    for e in ("tokens_to_ncfhw", "tokens_to_image"):
        assert {p["ld"] - p["c"] for p in P(e, "totals")} == {0, 3}
    cp = P("clip_patches", "entry")
    assert {(p["size"], p["patch"]) for p in cp} == {(4, 2), (6, 3), (28, 14)}
    assert all({p["kpad"] == 3 * p["patch"] ** 2 for p in cp if p["patch"] == pt} == {True, False} for pt in (2, 3, 14))
    ce = P("clip_embed", "entry")
    assert {(p["form"], p["t"], p["c"]) for p in ce} == {(fm, t, c) for fm in ("text", "vision") for t in (1, 2, 5) for c in (8, 24)}
    pr = P("permute_rows", "orders")
    assert len({p["perm"] for p in pr if p["c"] == 8 and p["shape4"] == (2, 3, 4, 5)}) == 24
    assert sum(p["c"] == 24 for p in pr) == 2 and any(1 in p["shape4"] for p in pr)
    mr = P("mask_resize_u8", "entry")
    assert {((p["H"], p["W"]), (p["h"], p["w"])) for p in mr} == {((8, 8), (1, 1)), ((16, 24), (2, 3)), ((17, 23), (2, 2)), ((40, 72), (5, 9))}
    fr = S.mask_frames(5, 8, 8, torch.Generator().manual_seed(0))
    assert int(fr[1].max()) == 0 and int(fr[2].min()) == 255 and set(fr[3].unique().tolist()) == {0, 255}
    assert {c.kind for e in ("act", "add", "scale", "gaussian_sample", "mask_finish") for c in S.cases(e)} == {"totals", "atlas"}
    assert {p["scale"] for p in P("scale")} == set(S.SCALES) and min(S.SCALES) < 0
    assert sorted(S.problem(S.Case("mask_finish", "atlas", n=256)).ins["v"].tolist()) == list(range(256))
    lv = S.problem(S.Case("gaussian_sample", "atlas", n=0)).ins["logvar"].to(F32)
    assert float(lv[lv.isfinite()].max()) > 20 and float(lv[lv.isfinite()].min()) < -30 and bool((lv == 20).any()) and bool((lv == -30).any())


def test_clip_and_resize_cases_drive_the_edges():
    """the checkerboard reaches both clips of the resize, the pad columns of clip_patches exist, a vision table is never read at t = 1"""
    pr = S.problem(S.Case("mask_resize_u8", "entry", n=5, H=16, W=24, h=2, w=3))
    assert 0 in pr.outs["tmp"].ref.tolist() and 255 in pr.outs["tmp"].ref.tolist()
    pc = S.problem(S.Case("clip_patches", "entry", nimg=2, size=4, patch=2, kpad=17))
    assert int((pc.outs["out"].ref.reshape(-1, 17)[:, 12:] == 0).all()) and not bool((pc.outs["out"].ref.reshape(-1, 17)[:, :12] == 0).any())
    pe = S.problem(S.Case("clip_embed", "entry", form="vision", nb=3, t=1, c=8))
    assert bool(pe.ins["table"].isnan().all()) and not bool(pe.outs["out"].ref.isnan().any())
    pt = S.problem(S.Case("clip_embed", "entry", form="text", nb=3, t=5, c=8))
    ids = pt.ins["ids"].tolist()
    assert 0 in ids and S.VOCAB - 1 in ids and len(set(ids)) < len(ids)


@pytest.mark.parametrize("mutation", sorted(S.MUTATIONS))
def test_mutation_is_rejected(mutation):
    for entry in S.MUTATIONS[mutation]:
        rejected = []
        for i, c in enumerate(S.cases(entry)):
            pl = S.Placed(S.problem(c), i)
            pl.emulate(mutation)
            if S.fails(pl):
                rejected.append(repr(c))
        assert rejected, f"no case of {entry} rejects the mutation {mutation}"


def test_relayout_invariance_holds_for_the_emulation_and_breaks_when_pixels_mix():
    seen = 0
    for b, f, hw, pitch in S.enc_relayout_cases():
        pa, pb, index, dest = S.enc_relayout_pair(b, f, hw, pitch)
        A, B = S.Placed(pa, 1), S.Placed(pb, 2)
        A.emulate()
        B.emulate()
        S.relayout_equal(A, B, index, dest, f"{b}x{f}x{hw}")
        if hw > 1 and f > 1:
            A2, B2 = S.Placed(pa, 0), S.Placed(pb, 0)
            A2.emulate("softmax_over_pixels")
            B2.emulate("softmax_over_pixels")
            with pytest.raises(AssertionError):
                S.relayout_equal(A2, B2, index, dest)
            seen += 1
    assert seen >= 6


def test_encoder_bound_and_special_cases():
    """twice the eager-fp16 yardstick stays under the 3e-3 of test_ops_gpu.py::test_temporal_encoder4_and_layout; one frame leads by 30
    in both heads of the dominant case; the constant rows have no variance"""
    for c in S.cases("temporal_encoder4"):
        rel, mx = S.enc_yardstick(c)
        assert 0 < 2 * rel <= 3e-3, (repr(c), rel)
        assert 0 < mx < 0.05, (repr(c), mx)
        x, W = S.enc_data(c)
        b, f, hw, _ = x.shape
        if c.kind == "dominant":
            s = S.enc_scores64(x.permute(0, 2, 1, 3).reshape(b * hw, f, 4), W)  # [s, head, query, key]
            top = s.sort(-1).values
            assert float((top[..., -1] - top[..., -2]).min()) >= 30.0
        if c.kind == "constant_row":
            assert int((x.to(F32).var(-1, unbiased=False) == 0).sum()) >= b * hw
        blob = S.enc_blob(W)
        assert blob.numel() == 288 and blob.dtype == H16


def test_timestep_chain_matches_the_oracle_and_stays_inside_the_bound():
    from oracle.unet_ref import timestep_embedding
    t = torch.cat([torch.arange(1000, dtype=F32), torch.arange(1, 65, dtype=F32)])
    chain = S.timestep_embedding_f32(t, 320)
    assert torch.equal(chain, timestep_embedding(t, 320))
    got = chain.to(H16)
    ref, bound, bound3 = S.timestep_embedding64(t, 320)
    dev = (got.to(F64) - ref).abs()
    assert float((dev / bound3).max()) <= 1.0              # the issue's `+ 3` form holds for torch's own float32 chain
    assert bool((bound >= bound3).all()) and float((bound / bound3).max()) < 1.01  # the device term adds under 1 %
    assert float((got == ref.to(H16)).double().mean()) > 0.98
    assert float(dev.max()) < 3e-4
    # the dim = 6 divisor: half - 1 moves k = 1 by a factor 10000^(1/6)
    a, b = S.timestep_embedding_f32(torch.tensor([1.0]), 6), S.timestep_embedding_f32(torch.tensor([1.0]), 6, "half_minus_1")
    assert float((a - b).abs().max()) > 0.01


def test_gelu_term_covers_a_float32_erf_evaluation():
    x = S.ALL_F16[S.ALL_F16.isfinite()]
    g64 = S.gelu_erf64(x)
    xf = x.to(F32)
    g32 = (0.5 * xf * (1.0 + torch.special.erf(xf * math.sqrt(0.5)))).to(F64)
    assert float(((g32 - g64).abs() / (S.GELU_ERF_ABS * x.to(F64).abs()).clamp_min(1e-300)).max()) <= 1.0
    ref, bound = S.act64(x, S.ACT_GELU)
    assert bool(((g32.to(H16).to(F64) - ref).abs() <= bound).all())


def test_checker_sees_what_the_layout_promises():
    """a write past the operand, a write into the lead, an unwritten element and a changed input are each reported"""
    c = S.Case("ncfhw_to_tokens", "pitch", b=2, c=4, f=5, hw=7, ldo=8, coff=4)
    for damage in ("behind", "lead", "unwritten", "input", None):
        # where the host allocator puts a block decides how many elements lie in front of a view (none when the block's own address
        # mod 256 is the lead asked for): cycle through the leads until a placement's output has some
        held = []
        for li in range(12):
            pl = S.Placed(S.problem(c), li)
            held.append(pl)  # (kept, so that the next placement gets other blocks)
            out, x = pl.T["out"], pl.T["x"]
            off = (out.data_ptr() - out.base_alloc.data_ptr()) // 2
            if off > 0:
                break
        pl.emulate()
        if damage == "behind":
            out.base_alloc[off + out.numel()] = 0.0
        elif damage == "lead":
            assert off > 0, "no placement with elements in front of the output"
            out.base_alloc[off - 1] = 0.0
        elif damage == "unwritten":
            out.view(torch.int16)[4] = LC.OUT_SENTINEL
        elif damage == "input":
            x.base_alloc[-1] = 1.0
        assert S.fails(pl) == (damage is not None), damage
