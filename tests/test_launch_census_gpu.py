"""Launch census of the headline step: every descriptor the benchmark's launch set sends through the C ABI, recorded, deduplicated,
replayed on fresh test-filled buffers and compared with a float64 restatement of include/mvoc_hip.h (tests/launch_census.py; the
references are pinned against torch primitives in test_launch_census_cpu.py).

Two recordings: the headline job (bench.Job 16 x 64 x 64 with graphs and the concurrent inversions, 40 mix steps = 10 composition
steps, both captured composition variants) and the reference's native size (16 x 90 x 160 latents: ragged 23 x 40 level, GEGLU
output past 2 GB).  Integer operands make every plain GEMM and xs_linear replay bit-exact; the other families are held to the
bounds of their per-op tests in test_ops_gpu.py."""
import ctypes as C
import gc
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F64, H16 = torch.float64, torch.float16
TESTS = os.path.dirname(os.path.abspath(__file__))

# entry points the UNet path calls that the census does not replay: the exact test that covers each.  A recorded entry point that is
# neither replayed nor listed here fails test_census_entry_points_are_all_covered.
NOT_REPLAYED = {
    "mvoc_ddim_step_f16": "test_ops_gpu.py::test_ddim_step_bit_exact",
    "mvoc_latent_fusion_f16": "test_ops_gpu.py::test_latent_fusion_bit_exact",
    "mvoc_pnp_blend_scatter_tokens": "test_ops_gpu.py::test_pnp_tokens_spatial_bit_exact",
    "mvoc_pnp_blend_scatter_nchw": "test_ops_gpu.py::test_pnp_nchw_bit_exact",
    "mvoc_timestep_embedding_f16": "test_stem_contract_gpu.py::test_walk",
    "mvoc_conv3x3_small_f16": "test_stem_contract_gpu.py::test_walk",
    "mvoc_adaptive_avgpool_f16": "test_stem_contract_gpu.py::test_walk",
    "mvoc_ncfhw_to_tokens_f16": "test_stem_contract_gpu.py::test_walk",
    "mvoc_tokens_to_ncfhw_f16": "test_stem_contract_gpu.py::test_walk",
    "mvoc_temporal_encoder4_f16": "test_stem_contract_gpu.py::test_temporal_encoder4_accuracy",
    "mvoc_act_f16": "test_stem_contract_gpu.py::test_walk",
    "mvoc_add_f16": "test_stem_contract_gpu.py::test_walk",
    "mvoc_groupnorm_moments_f16": "test_frame_shard_gpu.py::test_groupnorm_moments_pair_is_bit_exact",
    "mvoc_groupnorm_apply_moments_f16": "test_frame_shard_gpu.py::test_groupnorm_moments_pair_is_bit_exact",
}
# host-side queries (no launch)
HOST_QUERIES = {"mvoc_gemm_chan_sums_written", "mvoc_gemm_row_moments_written", "mvoc_gemm_workspace_bytes",
                "mvoc_groupnorm_workspace_bytes", "mvoc_last_error", "mvoc_version"}

CONFIGS = (("headline", dict(latent=64, latent_w=None)), ("native", dict(latent=90, latent_w=160)))


def _lib():
    from mvoc_amd._ffi import lib
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib().mvoc_last_error().decode()


@pytest.fixture(scope="module")
def census():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import bench
    from mvoc_amd import ops
    dev = torch.device("cuda:0")
    recs, times = {}, {}
    for cfg, kw in CONFIGS:
        t0 = time.time()
        rec = LC.Recorder()
        rec.install()  # before the Job: _make_stock_step captures the unhinted B = 1 inversion in its __init__
        try:
            job = bench.Job(dev, 16, kw["latent"], True, latent_w=kw["latent_w"])
            job.enable_concurrent_inversions()  # captured under gemm_concurrency(3)
            for k in range(40):  # 10 composition steps: the feature-injection variant (j % 10 == 9) and the Q/K-only one
                job.step(k)
            torch.cuda.synchronize()
        finally:
            rec.uninstall()
        del job
        ops._CHUNK_CACHE.clear()  # (holds the job's conv weights alive)
        gc.collect()
        torch.cuda.empty_cache()
        recs[cfg] = rec
        times[cfg] = time.time() - t0
    line = "; ".join(f"{cfg}: " + ", ".join(f"{fam} {len(v)}" for fam, v in sorted(rec.by_family().items())) +
                     f" ({sum(c for _, c in rec.launches.values())} calls, {times[cfg]:.0f} s)" for cfg, rec in recs.items())
    print(f"\n[census] unique descriptors per family -- {line}", flush=True)
    return recs


def _launches(census, family):
    for cfg, rec in census.items():
        for i, (ln, cnt) in enumerate(rec.by_family().get(family, [])):
            yield cfg, i, ln, cnt


def _report(family, fails, n):
    print(f"[census] {family}: {n} replays, {len(fails)} failing", flush=True)
    assert not fails, f"{family}: {len(fails)} of {n} replays fail:\n" + "\n".join(fails)


def _seed(cfg, i):
    return 7919 * (1 + [c for c, _ in CONFIGS].index(cfg)) + i


def _sentinel_count(t):
    return int((t.base_alloc.view(torch.int16) != LC.OUT_SENTINEL).sum())


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def test_census_coverage(census):
    """a census that silently recorded little fails here"""
    head = census["headline"].by_family()
    g = [ln.desc for ln, _ in head["gemm"]]
    need = {
        "k_order = 1": any(d.k_order == 1 for d in g),
        "upsample = 2": any(d.upsample == 2 for d in g),
        "split-K workspace under the unhinted inversion": any(d.workspace and d.concurrency <= 1 for d in g),
        "two-source plain GEMM (proj_out fold)": any(d.a_mode == LC.A_PLAIN and d.a2 for d in g),
        # (the step issues no two-source conv: a decoder resnet's skip concat enters through GroupNorm's x2 and conv_shortcut's a2)
        "two-source GroupNorm": any(ln.desc.x2 for ln, _ in head.get("groupnorm", [])),
        "ln_rowsum": any(d.ln_rowsum for d in g),
        "rowadd": any(d.rowadd for d in g),
        "GEGLU": any(d.act == LC.ACT_GEGLU for d in g),
        "chan_sums": any(d.chan_sums for d in g),
        "row_moments": any(d.row_moments for d in g),
        "concurrency = 3": any(d.concurrency == 3 for d in g),
        "paired flash": any(ln.desc.v2 for ln, _ in head.get("flash_attn", [])),
        "flash tk >= 2048": any(ln.desc.tk >= 2048 for ln, _ in head.get("flash_attn", [])),
        "xs_linear wp_set_rows": any(ln.desc.wp_set_rows for ln, _ in head.get("xs_linear", [])),
        "xs_linear m >= 131072": any(ln.desc.m >= 131072 for ln, _ in head.get("xs_linear", [])),
        "tfused": bool(head.get("tfused")),
    }
    nat = [ln.desc for ln, _ in census["native"].by_family()["gemm"]]
    need["native: GEMM m % 256 != 0 at n >= 640"] = any(d.m % 256 and d.n >= 640 for d in nat)
    missing = [k for k, ok in need.items() if not ok]
    assert not missing, f"the census lacks: {missing}"


def test_census_entry_points_are_all_covered(census):
    """every mvoc_* entry point the step calls is replayed here, is a host query, or names the exact test that covers it"""
    for name, where in NOT_REPLAYED.items():
        mod, fn = where.split("::")
        src = open(os.path.join(TESTS, mod)).read()
        assert f"def {fn}(" in src, f"{name}: {where} does not exist"
    stray = {}
    for cfg, rec in census.items():
        for name, cnt in rec.calls.items():
            if name not in LC.RECORDED and name not in NOT_REPLAYED and name not in HOST_QUERIES:
                stray[name] = stray.get(name, 0) + cnt
    assert not stray, f"entry points neither replayed nor covered by a listed exact test: {stray}"


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
def _check_gemm(ln, seed, fails):
    lib = _lib()
    d, bufs, L = LC.build_gemm(ln.desc, torch.device("cuda:0"), seed)
    rc = lib.mvoc_gemm_f16(C.byref(d), _stream())
    if rc:
        fails.append(f"rc {rc} ({_err()}): {LC.describe(ln)}")
        return
    cs_written, rm_w = lib.mvoc_gemm_chan_sums_written(), lib.mvoc_gemm_row_moments_written()
    cols = LC.gemm_out_cols(d)
    exact = d.act == LC.ACT_NONE and not d.ln_rowsum
    bad, worst, ratio = 0, 0.0, 0.0
    for r0, r1 in LC.gemm_blocks(d):
        ref, bound = LC.gemm_ref(d, bufs, L, r0, r1)
        got = LC.stored_rows(d, bufs, r0, r1).to(F64)
        if exact:
            assert ref.abs().max() < 2048  # every product and sum exact in fp32, the result exact in fp16
            wrong = got != ref
        else:
            if d.ln_rowsum:
                bound = bound + 2 * LC.ulp16(ref)
            wrong = ~((got - ref).abs() <= bound)
            worst = max(worst, float(((got - ref).abs() / LC.ulp16(ref)).nan_to_num(1e9).max()))
            ratio = max(ratio, float(((got - ref).abs() / bound.clamp_min(1e-300)).nan_to_num(1e9).max()))
        bad += int(wrong.sum())
    msg = []
    if bad:
        msg.append(f"{bad} wrong of {d.m * cols}" + ("" if exact else f" (worst {worst:.1f} ulp)"))
    touched = _sentinel_count(bufs["out"])
    if touched != d.m * cols:
        msg.append(f"{touched - d.m * cols} output elements written outside the stored [m, n_store] block")
    out = bufs["out"].reshape(d.m, d.ldo)[:, :cols]
    step = 256 * 256  # rows per block of the statistics checks
    if cs_written and not d.chan_sums:
        msg.append("chan_sums written without a request")
    elif cs_written:
        cs = bufs["chan_sums"].reshape(d.m // 256, cols, 2)
        for r0 in range(0, d.m, step):
            r1 = min(d.m, r0 + step)
            ref = LC.chan_sums64(out[r0:r1])
            if not torch.allclose(cs[r0 // 256:r1 // 256].to(F64), ref, rtol=1e-5, atol=1e-3):
                msg.append(f"chan_sums differ from the sums of the stored values (rows {r0}..{r1})")
                break
    if rm_w and not d.row_moments:
        msg.append("row_moments written without a request")
    elif rm_w:
        mom = bufs["row_moments"].reshape(d.m, d.row_moments_ld, 2)
        nt = -(-d.n // rm_w)
        for r0 in range(0, d.m, step):
            r1 = min(d.m, r0 + step)
            ref = LC.row_moments64(out[r0:r1], rm_w, d.row_moments_ld)
            if not torch.allclose(mom[r0:r1, :nt].to(F64), ref[:, :nt], rtol=1e-5, atol=2e-3):
                msg.append(f"row_moments (tile {rm_w}) differ from the sums of the stored values (rows {r0}..{r1})")
                break
    if msg:
        fails.append("; ".join(msg) + f" -- {LC.describe(ln)}")
    return ratio  # worst deviation in units of the bound (0.0: a bit-exact replay)


def test_census_gemm(census):
    from mvoc_amd import ops
    fails, n = [], 0
    for cfg, i, ln, cnt in _launches(census, "gemm"):
        n += 1
        try:
            _check_gemm(ln, _seed(cfg, i), fails)
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
        finally:
            ops._CHUNK_CACHE.clear()  # (would keep every replay's chunk-major weights alive)
    _report("gemm", fails, n)


# ---- xs_linear ------------------------------------------------------------------------------------------------------------------------
def test_census_xs_linear(census):
    lib = _lib()
    fails, n = [], 0
    for cfg, i, ln, cnt in _launches(census, "xs_linear"):
        n += 1
        try:
            d, bufs, L = LC.build_xs(ln.desc, torch.device("cuda:0"), _seed(cfg, i))
            rc = lib.mvoc_xs_linear_f16(C.byref(d), _stream())
            if rc:
                fails.append(f"rc {rc} ({_err()}): {LC.describe(ln)}")
                continue
            _, cols = LC.xs_extents(d)
            exact = d.act == LC.ACT_NONE
            bad = 0
            for r0, r1 in LC.xs_blocks(d):
                ref, bound = LC.xs_ref(d, bufs, L, r0, r1)
                got = bufs["out"].reshape(-1)[r0 * d.ldo:r1 * d.ldo].reshape(r1 - r0, d.ldo)[:, :cols].to(F64)
                if d.normalize:
                    bound = bound + 2 * LC.ulp16(ref)
                wrong = (got != ref) if (exact and not d.normalize) else ~((got - ref).abs() <= bound)
                bad += int(wrong.sum())
            touched = _sentinel_count(bufs["out"])
            if bad or touched != d.m * cols:
                fails.append(f"{bad} wrong of {d.m * cols}, {touched - d.m * cols} written outside -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("xs_linear", fails, n)


# ---- attention ------------------------------------------------------------------------------------------------------------------------
ATTN_FULL_WORK = 1 << 33  # nbatch * heads * tq * tk above this: every 7th query row and the last 64 are compared (the native size)


def _attn_compare(d, T, which):
    """(rel-L2, max abs) of output `which` against fp64, in blocks of batches / queries"""
    hd = LC.attn_hd(d)
    got_all = LC.attn_out_view(d, T, which)
    sample = d.nbatch * d.heads * d.tq * d.tk > ATTN_FULL_WORK
    qidx = torch.cat([torch.arange(0, d.tq, 7), torch.arange(max(0, d.tq - 64), d.tq)]).unique() if sample else None
    num = den = 0.0
    mx = 0.0
    qb = max(64, (1 << 27) // (d.heads * d.tk))
    for b in range(d.nbatch):
        for q0 in range(0, d.tq, qb):
            q1 = min(d.tq, q0 + qb)
            if sample:
                sel = qidx[(qidx >= q0) & (qidx < q1)]
                if not len(sel):
                    continue
            ref = LC.attn_ref(d, T, which, b, b + 1, q0, q1)
            got = got_all[b:b + 1, q0:q1].to(F64)
            if sample:
                loc = (sel - q0).to(ref.device)
                ref, got = ref[:, loc], got[:, loc]
            num += float(((got - ref) ** 2).sum())
            den += float((ref ** 2).sum())
            mx = max(mx, float((got - ref).abs().max()))
    return (num / max(den, 1e-300)) ** 0.5, mx


def test_census_flash_attn(census):
    """against fp64 at the bounds of test_flash_attn (rel-L2 2e-3, max 1e-2); at every descriptor the phase kernel (pipelined = 1) and
    the pipelined kernel (= 2) return the same bits, and the recorded choice returns them too"""
    lib = _lib()
    fails, n = [], 0
    for cfg, i, ln, cnt in _launches(census, "flash_attn"):
        n += 1
        try:
            d, T = LC.build_attn(ln.desc, torch.device("cuda:0"), _seed(cfg, i))
            outs = [w for w in ("out", "out2") if w in T]
            res = {}
            for mode in (ln.desc.pipelined, 1, 2):
                d.pipelined = mode
                for w in outs:
                    T[w].base_alloc.view(torch.int16).fill_(LC.OUT_SENTINEL)
                rc = lib.mvoc_flash_attn_f16(C.byref(d), _stream())
                if rc:
                    raise RuntimeError(f"rc {rc} ({_err()}) at pipelined = {mode}")
                res[mode] = [LC.attn_out_view(d, T, w).clone() for w in outs]
                if mode == ln.desc.pipelined:
                    for w in outs:
                        rl, mx = _attn_compare(d, T, w)
                        if not (rl < LC.FLASH_BOUND[0] and mx < LC.FLASH_BOUND[1]):
                            fails.append(f"{cfg} {w}: rel-L2 {rl:.2e}, max {mx:.2e} -- {LC.describe(ln)}")
            for a, b in zip(res[1], res[2]):
                if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
                    fails.append(f"{cfg}: pipelined 1 and 2 differ in {int((a.view(torch.int16) != b.view(torch.int16)).sum())} elements -- {LC.describe(ln)}")
            for a, b in zip(res[ln.desc.pipelined], res[1 if ln.desc.pipelined == 1 else 2]):
                if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
                    fails.append(f"{cfg}: the recorded kernel choice differs from both explicit ones -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("flash_attn", fails, n)


def test_census_temporal_attn_and_tfused(census):
    """temporal attention at the bounds of test_temporal_attn (rel-L2 2e-3, max 1e-2); the fused LN -> QKV -> attention at those of
    test_temporal_qkv_attn_fused (3e-3, 2e-2)"""
    lib = _lib()
    fails, n = [], 0
    for cfg, i, ln, cnt in _launches(census, "temporal_attn"):
        n += 1
        try:
            d, T = LC.build_tattn(ln.desc, torch.device("cuda:0"), _seed(cfg, i))
            rc = lib.mvoc_temporal_attn_f16(C.byref(d), _stream())
            if rc:
                raise RuntimeError(f"rc {rc} ({_err()})")
            num = den = mx = 0.0
            for s in range(d.nsample):
                ref = LC.tattn_ref(d, T, s, s + 1)
                got = LC.tattn_view(d, T["out"], "o")[s:s + 1].to(F64)
                num += float(((got - ref) ** 2).sum())
                den += float((ref ** 2).sum())
                mx = max(mx, float((got - ref).abs().max()))
            rl = (num / den) ** 0.5
            if not (rl < 2e-3 and mx < 1e-2):
                fails.append(f"{cfg}: rel-L2 {rl:.2e}, max {mx:.2e} -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    for cfg, i, ln, cnt in _launches(census, "tfused"):
        n += 1
        try:
            d, T, L = LC.build_tfused(ln.desc, torch.device("cuda:0"), _seed(cfg, i))
            rc = lib.mvoc_temporal_qkv_attn_f16(C.byref(d), _stream())
            if rc:
                raise RuntimeError(f"rc {rc} ({_err()})")
            per = d.frames * d.hw
            num = den = mx = 0.0
            for s in range(d.nsample):
                ref = LC.tfused_ref(d, T, L, s, s + 1)
                got = T["out"].reshape(-1, d.c)[s * per:(s + 1) * per].to(F64)
                num += float(((got - ref) ** 2).sum())
                den += float((ref ** 2).sum())
                mx = max(mx, float((got - ref).abs().max()))
            rl = (num / den) ** 0.5
            if not (rl < 3e-3 and mx < 2e-2) or _sentinel_count(T["out"]) != d.nsample * per * d.c:
                fails.append(f"{cfg}: rel-L2 {rl:.2e}, max {mx:.2e} -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("temporal_attn + tfused", fails, n)


# ---- norms ------------------------------------------------------------------------------------------------------------------------------
def _gn_run(d, T, L, ln, cfg, fails, tag):
    lib = _lib()
    T["out"].base_alloc.view(torch.int16).fill_(LC.OUT_SENTINEL)
    rc = lib.mvoc_groupnorm_f16(C.byref(d), _stream())
    if rc:
        raise RuntimeError(f"rc {rc} ({_err()})")
    num = den = mx = 0.0
    for s in range(d.nsample):
        ref = LC.gn_ref(d, L, s, s + 1)
        got = T["out"].reshape(-1, d.c)[s * d.rows_per_sample:(s + 1) * d.rows_per_sample].to(F64)
        num += float(((got - ref) ** 2).sum())
        den += float((ref ** 2).sum())
        mx = max(mx, float((got - ref).abs().max()))
    rl = (num / den) ** 0.5
    if not (rl < LC.GN_BOUND[0] and mx < LC.GN_BOUND[1]):  # test_groupnorm's bounds
        fails.append(f"{cfg} {tag}: rel-L2 {rl:.2e}, max {mx:.2e} -- {LC.describe(ln)}")


def test_census_groupnorm(census):
    """GroupNorm (+ SiLU, + second source) at test_groupnorm's bounds, with the producer's chan_sums supplied from fp64 sums where the
    recorded call had them and without them too; the fold into per-sample xs weights at test_groupnorm_folded_into_xs_linear's"""
    lib = _lib()
    fails, n = [], 0
    for cfg, i, ln, cnt in _launches(census, "groupnorm"):
        n += 1
        try:
            d, T, L, _ = LC.build_gn(ln.desc, torch.device("cuda:0"), _seed(cfg, i))
            _gn_run(d, T, L, ln, cfg, fails, "as recorded")
            if d.chan_sums:
                d.chan_sums = d.chan_sums2 = None
                _gn_run(d, T, L, ln, cfg, fails, "own statistics")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    for cfg, i, ln, cnt in _launches(census, "groupnorm_fold_xs"):
        n += 1
        try:
            d, T, L, fa = LC.build_gn(ln.desc, torch.device("cuda:0"), _seed(cfg, i), ln.args)
            rc = lib.mvoc_groupnorm_fold_xs_f16(C.byref(d), fa["w"].data_ptr(), fa["bias"].data_ptr() if fa["bias"] is not None else None,
                                                fa["n"], fa["k"], fa["wp_sets"].data_ptr(), _stream())
            if rc:
                raise RuntimeError(f"rc {rc} ({_err()})")
            nn_, k = fa["n"], fa["k"]
            sets = fa["wp_sets"].reshape(d.nsample, -1)
            num = den = 0.0
            for s in range(d.nsample):
                w_s, c_s = LC.unpack_xs_weights(sets[s], nn_, k)
                x = L["x"][s * d.rows_per_sample:(s + 1) * d.rows_per_sample].to(F64)
                got = x @ w_s.to(F64).t() + c_s.to(F64)
                ref = LC.gn_fold_ref(d, L, s, s + 1)
                num += float(((got - ref) ** 2).sum())
                den += float((ref ** 2).sum())
            rl = (num / den) ** 0.5
            if not rl < 1.5e-3:
                fails.append(f"{cfg}: folded weights give rel-L2 {rl:.2e} -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("groupnorm", fails, n)


def test_census_row_stats_and_layernorm(census):
    """row statistics (and from a producer's row moments) at test_gemm_row_moments_and_layernorm_statistics_from_them's bounds,
    LayerNorm at test_layernorm's"""
    lib = _lib()
    dev = torch.device("cuda:0")
    fails, n = [], 0

    def stats_ok(st, x, eps):
        return LC.row_stats_ratio(st, x, eps) <= 1.0

    for fam in ("row_stats", "row_stats_from_moments", "layernorm"):
        for cfg, i, ln, cnt in _launches(census, fam):
            n += 1
            a = ln.args
            try:
                gen = torch.Generator(device=dev).manual_seed(_seed(cfg, i))
                rows = a["rows"]
                c = a["c"] if "c" in a else a["n"]
                x = (torch.randn(rows, c, generator=gen, device=dev) * 1.5 + 0.3).to(H16)
                if fam == "row_stats":
                    xb = LC.alloc(rows * c, H16, a["x"] % 256, dev)
                    xb.copy_(x.reshape(-1))
                    st = LC.alloc(rows * 2, torch.float32, a["stats"] % 256, dev)
                    rc = lib.mvoc_row_stats_f16(xb.data_ptr(), st.data_ptr(), rows, c, a["eps"], _stream())
                    ok = rc == 0 and stats_ok(st.reshape(rows, 2), x, a["eps"])
                elif fam == "row_stats_from_moments":
                    mom = LC.alloc(rows * a["ld"] * 2, torch.float32, a["moments"] % 256, dev)
                    mom.copy_(LC.row_moments64(x, a["tile_w"], a["ld"]).to(torch.float32).reshape(-1))
                    st = LC.alloc(rows * 2, torch.float32, a["out"] % 256, dev)
                    rc = lib.mvoc_row_stats_from_moments_f32(mom.data_ptr(), rows, a["ld"], c, a["tile_w"], a["eps"], st.data_ptr(), _stream())
                    ok = rc == 0 and stats_ok(st.reshape(rows, 2), x, a["eps"])
                else:
                    gm = (1 + 0.2 * torch.randn(c, generator=gen, device=dev)).to(H16)
                    bt = (0.2 * torch.randn(c, generator=gen, device=dev)).to(H16)
                    xb, gb, bb = (LC.alloc(t.numel(), H16, a[nm] % 256, dev) for t, nm in ((x, "x"), (gm, "gamma"), (bt, "beta")))
                    xb.copy_(x.reshape(-1)), gb.copy_(gm), bb.copy_(bt)
                    ob = LC.alloc(rows * c, H16, a["out"] % 256, dev)
                    rc = lib.mvoc_layernorm_f16(xb.data_ptr(), gb.data_ptr(), bb.data_ptr(), ob.data_ptr(), rows, c, a["eps"], _stream())
                    ref = LC.layernorm64(x, gm, bt, a["eps"])
                    got = ob.reshape(rows, c).to(F64)
                    ok = rc == 0 and float((got - ref).abs().max()) < LC.LN_BOUND[1] and LC.rel_l2(got, ref) < LC.LN_BOUND[0]
                if rc:
                    fails.append(f"{cfg}: rc {rc} ({_err()}) -- {LC.describe(ln)}")
                elif not ok:
                    fails.append(f"{cfg}: outside the bounds -- {LC.describe(ln)}")
            except (RuntimeError, AssertionError) as e:
                fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("row_stats + layernorm", fails, n)


def test_act_and_add_exact():
    """the step's elementwise SiLU and add (time embedding): add is one fp16 rounding of the exact sum, SiLU within one fp16 ulp of
    fp64 (v_exp + v_rcp: a few fp32 ulps)"""
    from mvoc_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    a = (torch.randn(5 * 1280 + 3, generator=g, device="cuda") * 4).to(H16)
    b = (torch.randn(5 * 1280 + 3, generator=g, device="cuda") * 4).to(H16)
    assert torch.equal(ops.add(a, b), (a.to(F64) + b.to(F64)).to(H16))
    y = ops.act(a, ops.ACT_SILU).to(F64)
    ref = LC.silu64(a.to(F64))
    assert ((y - ref).abs() <= LC.ulp16(ref)).all()


# ---- the Python mirrors of the library's gates ------------------------------------------------------------------------------------------
def _conv_case(m, stride):
    """(nimg, h, w) with nimg * hout * wout == m"""
    if stride == 1:
        return {1023: (3, 11, 31), 1024: (4, 16, 16), 2048: (8, 16, 16)}[m]
    return {1023: (3, 21, 61), 1024: (4, 32, 32), 2048: (8, 32, 32)}[m]


def test_python_mirrors_of_the_library_gates():
    """ops._chunk_ok true => the library takes the k_order = 1 request (rc 0) and the result is exact; the sub-pixel gate of
    ops.conv3x3 true => the upsample = 2 launch is taken and exact.  The other direction (the library would take a request Python
    does not make: the grid-fill rule is a deliberate extra condition on the Python side) is counted and printed, not asserted."""
    from mvoc_amd import ops
    from mvoc_amd._ffi import GemmDesc
    from mvoc_amd.unet import pack_conv3x3, pack_conv3x3_subpixel, pack_tconv
    lib = _lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    fails, py_yes, lib_only, total = [], 0, 0, 0
    import itertools
    # a sample of the whole grid, and one of its corner where every alignment rule holds (tile 0: the grid-fill rule decides;
    # tile 82: the Python gate skips it, so the k_order = 1 request is made at these small m too)
    grid = list(itertools.product((1023, 1024, 2048), (320, 1280, 352), (64, 96), (1, 2), (0, 2, 16), ((0, 0), (8, 0), (4, 4)),
                                  (32, 64), (1, 3, 9), ("conv", "tconv"), (0, 82)))
    aligned = list(itertools.product((1024, 2048), (320, 640, 1280), (64, 128), (1,), (0, 16), ((0, 0), (8, 0)), (64,), (1, 3, 9),
                                     ("conv", "tconv"), (0, 82)))
    rng = torch.Generator().manual_seed(3)
    cases = [grid[i] for i in torch.randperm(len(grid), generator=rng)[:140].tolist()]
    cases += [aligned[i] for i in torch.randperm(len(aligned), generator=rng)[:100].tolist()]
    for m, n, cin, stride, off, (ldo_pad, ns_cut), rdiv, conc, mode, tile in cases:
        if mode == "tconv" and stride == 2:
            stride = 1
        total += 1
        ntaps = 9 if mode == "conv" else 3
        if mode == "conv":
            nimg, h, w = _conv_case(m, stride)
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            rows_a = nimg * h * w
            wl = LC._ints_sparse((n, cin, 3, 3), gen, dev)
            wt = pack_conv3x3(wl)
        else:
            frames = 16 if m % 16 == 0 else 1
            nimg, rows_a = 1, m
            wl = LC._ints_sparse((n, cin, 3, 1, 1), gen, dev)
            wt = pack_tconv(wl)
        ns = n - ns_cut
        ldo = ns + ldo_pad
        x = LC.alloc(rows_a * cin, H16, 0, dev)
        x.copy_(LC._ints((rows_a * cin,), gen, dev))
        outb = LC.alloc(m * ldo, H16, off, dev)
        bias = LC.alloc(n, H16, off, dev)
        bias.copy_(LC._ints((n,), gen, dev, -4, 4))
        res = LC.alloc(m * ldo, H16, off, dev)
        res.copy_(LC._ints((m * ldo,), gen, dev, -4, 4))
        rowadd = LC.alloc(-(-m // rdiv) * ns, H16, 0, dev) if mode == "conv" else None
        if rowadd is not None:
            rowadd.copy_(LC._ints(rowadd.shape, gen, dev, -4, 4))
        out2, res2 = outb.as_strided((m, ns), (ldo, 1)), res.as_strided((m, ns), (ldo, 1))
        ra2 = rowadd.view(-1, ns) if rowadd is not None else None
        d = GemmDesc()
        d.a, d.w, d.out, d.bias, d.resid = x.data_ptr(), wt.data_ptr(), outb.data_ptr(), bias.data_ptr(), res.data_ptr()
        d.rowadd = ra2.data_ptr() if ra2 is not None else None
        d.m, d.n, d.k, d.n_store, d.ldo, d.ldr = m, n, wt.shape[1], ns, ldo, ldo
        d.ld_rowadd, d.rowadd_div = (ns, rdiv) if ra2 is not None else (0, 1)
        d.lda, d.c1, d.cin, d.concurrency, d.tile = cin, cin, cin, conc, tile
        if mode == "conv":
            d.a_mode, d.nimg, d.hout, d.wout, d.hsrc, d.wsrc, d.stride, d.hup, d.wup = LC.A_CONV3X3, nimg, ho, wo, h, w, stride, h, w
        else:
            d.a_mode, d.frames, d.hw = LC.A_TEMPORAL3, frames, m // frames
        xv = x.view(rows_a, cin)
        with ops.gemm_concurrency(conc):
            ok = ops._chunk_ok(d, xv, None, wt, out2, bias, res2, ra2, ntaps, rows_a)
        if cin % 64:  # no chunk-major form of these weights exists
            if ok:
                fails.append(f"_chunk_ok true at cin = {cin}")
            continue
        d.w, d.k_order, d.split_k = ops.chunk_major_weights(wt, ntaps).data_ptr(), 1, 1
        outb.base_alloc.view(torch.int16).fill_(LC.OUT_SENTINEL)
        rc = lib.mvoc_gemm_f16(C.byref(d), _stream())
        tag = f"{mode} m={m} n={n} cin={cin} stride={stride} off={off} ldo={ldo} ns={ns} rowadd_div={rdiv} conc={conc} tile={tile}"
        if ok:
            py_yes += 1
            if rc:
                fails.append(f"_chunk_ok true, library rc {rc} ({_err()}): {tag}")
                continue
            L = {"w": wl, "bias": bias}
            T = {"a": x, "resid": res, "rowadd": rowadd}
            ref, _ = LC.gemm_ref(d, T, L)
            got = out2.to(F64)
            if not torch.equal(got, ref):
                fails.append(f"_chunk_ok true, {int((got != ref).sum())} wrong: {tag}")
        elif rc == 0:
            lib_only += 1
    # the sub-pixel gate, through ops.conv3x3 itself (what it requested is read back with the recorder)
    sp_yes = sp_lib_only = 0
    for (nimg, h, w, cin, n, conc, tiles_min) in ((16, 16, 16, 64, 320, 1, None), (16, 16, 16, 64, 640, 3, None), (8, 16, 16, 128, 320, 9, None),
                                                   (4, 8, 8, 64, 320, 1, None), (4, 8, 8, 64, 320, 9, None), (4, 16, 16, 64, 352, 1, 0),
                                                   (2, 16, 16, 96, 640, 3, 0), (5, 12, 20, 64, 352, 1, 0), (3, 11, 31, 64, 320, 1, 0),
                                                   (16, 16, 16, 64, 320, 1, 10 ** 6)):
        wl = LC._ints_sparse((n, cin, 3, 3), gen, dev)
        wt, wsp = pack_conv3x3(wl), pack_conv3x3_subpixel(wl)
        x = LC._ints((nimg * h * w, cin), gen, dev)
        b = LC._ints((n,), gen, dev, -4, 4)
        saved = ops.SUBPIXEL_MIN_TILES
        rec = LC.Recorder()
        try:
            if tiles_min is not None:
                ops.SUBPIXEL_MIN_TILES = tiles_min
            rec.install()
            try:
                with ops.gemm_concurrency(conc):
                    out, ho, wo = ops.conv3x3(x, wt, b, nimg=nimg, h=h, wd=w, upsample_to=(2 * h, 2 * w), w_subpixel=wsp)
            finally:
                rec.uninstall()
        finally:
            ops.SUBPIXEL_MIN_TILES = saved
        (lnr, _), = rec.by_family()["gemm"]
        d = LC.copy_desc(lnr.desc)
        tag = f"subpixel nimg={nimg} {h}x{w} cin={cin} n={n} conc={conc} min_tiles={tiles_min}"
        T = {"a": x.reshape(-1)}
        ref, _ = LC.gemm_ref(d, T, {"w": wl, "bias": b})
        if d.upsample == 2:
            sp_yes += 1
            if not torch.equal(out.to(F64), ref):
                fails.append(f"sub-pixel gate true, {int((out.to(F64) != ref).sum())} wrong: {tag}")
        else:
            d2 = LC.copy_desc(d)
            d2.upsample, d2.w, d2.k, d2.split_k, d2.concurrency = 2, wsp.data_ptr(), 4 * cin, 1, conc
            o2 = torch.empty_like(out)
            d2.out = o2.data_ptr()
            d2.workspace, d2.workspace_bytes, d2.chan_sums = None, 0, None
            if lib.mvoc_gemm_f16(C.byref(d2), _stream()) == 0:
                sp_lib_only += 1
                if not torch.equal(o2.to(F64), ref):
                    fails.append(f"library-accepted sub-pixel launch wrong: {tag}")
    print(f"\n[mirror] k_order = 1: {total} cases, Python requests {py_yes}, library-only acceptances {lib_only}; "
          f"sub-pixel: Python requests {sp_yes}, library-only acceptances {sp_lib_only}", flush=True)
    assert py_yes and sp_yes, "the sweep never reached the requested forms"
    assert not fails, "\n".join(fails)
