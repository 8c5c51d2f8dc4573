"""Launch census of the stages either side of the denoising loop: every descriptor and every stem call the VAE (encode + decode), the
two CLIP towers and the mask path send through the C ABI, recorded on seeded weights of the real architectures, deduplicated by
(scalars, pointer alignment), replayed on fresh test-filled buffers and compared with the float64 restatements of
tests/launch_census.py (pinned against torch in test_stage_census_cpu.py and test_launch_census_cpu.py).

Integer operands make every GEMM / conv / xs_linear replay without an activation bit-exact -- the VAE's score GEMM q k^T, P v + b and
the small convs included; GroupNorm, LayerNorm, row statistics and flash attention are held to the bounds of the UNet census
(launch_census.FLASH_BOUND / GN_BOUND / LN_BOUND / row_stats_ratio); softmax and the Gaussian sampler to bounds derived there.

The last group runs the four launches that meet the decoder's 256-channel 512 x 512 tensor at the extents VaeCodec produces
(20 and 36 frames: past 2^31 bytes, past 2^32 bytes and 2^31 elements), with image i = image 0 times a small integer.

Addressing of those extents, read from the kernels before the group first ran:
  * gemm.hip: an operand of 2^31 bytes or more fails g8_ok (and the same test in ops.conv3x3 / ops._chunk_ok), so neither the
    eight-phase tiles of gemm8.hip, whose buffer offsets are 32-bit, nor the sub-pixel and chunk-major forms are chosen: the convs go
    to gemm_glds_kernel as tile 11, the K = 256 GEMM as tile 61.  There rows are ints (the entry refuses m >= 2^31; 9.4e6 here), the
    source row of a tap is a long, every byte offset is size_t / long on flat 64-bit pointers (global_load_lds, no buffer
    resource), and the grid is m_tiles * n_tiles = 147 456 blocks at most against the 2^31 - 1 the launcher refuses.
    mvoc_gemm_workspace_bytes is 0 for m > 8192, so no split-K slab is involved.
  * norm.hip: gn_partial / gn_apply form rowbase = (long)sample * rows and index x and out with long * int; rows within a sample
    (262 144) and chunks are ints; the grid is (nchunk, nsample) with nsample <= 65 535 refused beyond; the non-temporal variant is
    picked by a long byte count.  No buffer resources.
Nothing had to be fixed or refused.

Measured on an MI355X (worst deviation / bound per family): gemm 127 unique keys, 121 of them bit-exact integer replays, the six with
GELU / a LayerNorm fold 0.22; xs_linear 2, exact; flash_attn 3, 0.14; groupnorm 36, 0.26; row_stats + layernorm 8, 0.21; the nine
data-movement / integer stem entries exact; softmax_rows 166 elements on the accepted neighbouring fp16 value, every other one
exact; gaussian_sample exact.  The large-extent cases take 0.1 - 0.4 s each (one pays ~4 s for the allocator's first 5 GB block);
GroupNorm there: rel-L2 3.2e-4, max 4.0e-3.  The whole file: 9 s, beside 47 s of test_launch_census_gpu.py on the same machine.

That the census can fail (scratch perturbations, one at a time): pad_mode forced to 0 in the encoder's downsamplers, and causal
dropped in clip.py -> test_stage_form_coverage (1 form each); ky / kx swapped in pack_conv3x3_small -> test_stage_stem[conv3x3_small],
8 of 8 keys; the softmax replay's input rolled by one column -> test_stage_stem[softmax_rows], 3 of 3; one image's multiplier
changed on the reference side -> test_vae_forms_at_codec_extents (gemm: 31 776 159 elements of that image; groupnorm: image 7 != 3)."""
import ctypes as C
import gc
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402
import test_launch_census_gpu as G  # noqa: E402  (the UNet census: its GEMM and attention checks are reused as they are)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F64, F32, H16 = torch.float64, torch.float32, torch.float16
TESTS = os.path.dirname(os.path.abspath(__file__))

# entry points the stages call that this census does not replay: the exact test that covers each (none today: everything the three
# stages call is replayed).  A called entry point that is neither replayed nor listed fails test_stage_entry_points_are_all_covered.
NOT_REPLAYED = {}

REPLAYED_FAMILIES = {"gemm", "xs_linear", "flash_attn", "groupnorm", "row_stats", "row_stats_from_moments", "layernorm"} | \
    {LC.FAMILY[n] for n in LC.STEM_ENTRIES}
VAE_SIZES = ((2, 64, 64), (1, 256, 256), (1, 192, 320))  # smallest legal; every level % 256 rows; ragged 24 x 40 / 48 x 80 levels
VISION_BATCHES = (2, 5)                                  # 514 and 1285 rows
TEXT_SHAPE = (2, 77)


def _dev():
    return torch.device("cuda:0")


def _record(fn):
    rec = LC.Recorder()
    rec.install()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        rec.uninstall()
    return rec


def _vae_pass(vae, n, h, w, seed):
    from mvoc_amd.vae import VaeCodec
    codec = VaeCodec(vae)
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, h, w, generator=g) * 2 - 1).half()
    lat = codec._scaled(vae.encode_sample(x, generator=torch.Generator().manual_seed(seed)))  # encode_video's device half
    video = codec.decode(lat[None].permute(0, 2, 1, 3, 4).contiguous())
    assert tuple(video.shape) == (1, 3, n, h, w) and torch.isfinite(video).all()


@pytest.fixture(scope="module")
def stages(golden_dir):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mvoc_amd import ops
    from mvoc_amd.clip import CLIPTextModel, CLIPVisionModelWithProjection, ClipTextConfig, ClipVisionConfig
    from mvoc_amd.utils import mask_preprocess
    from mvoc_amd.vae import AutoencoderKL, VaeConfig
    recs = {}
    t0 = time.time()
    vae = AutoencoderKL(device=_dev()).init_random(1234)
    for n, h, w in VAE_SIZES:
        recs[f"vae {n}x{h}x{w}"] = _record(lambda: _vae_pass(vae, n, h, w, h + w))
    del vae
    # (the checkpoint's decoder upsamples at 512, 512 and 256 channels; an upsampler at 128 exists only in a narrower configuration,
    # recorded here at the smallest size so that the folded-upsample conv is replayed at cin = 128 too)
    narrow = AutoencoderKL(VaeConfig(block_out_channels=(128, 128, 256, 512)), device=_dev()).init_random(77)
    recs["vae (128, 128, 256, 512) 1x64x64"] = _record(lambda: _vae_pass(narrow, 1, 64, 64, 9))
    del narrow
    for layers in (2, 3):
        vis = CLIPVisionModelWithProjection(ClipVisionConfig(num_hidden_layers=layers), device=_dev()).init_random(4321)
        for b in (VISION_BATCHES if layers == 2 else VISION_BATCHES[:1]):
            px = torch.randn(b, 3, 224, 224, generator=torch.Generator().manual_seed(b))
            recs[f"vision b={b}" + ("" if layers == 2 else " (3 layers)")] = _record(lambda: vis(px))
        del vis
        txt = CLIPTextModel(ClipTextConfig(num_hidden_layers=layers), device=_dev()).init_random(4322)
        ids = torch.randint(0, 49408, TEXT_SHAPE, generator=torch.Generator().manual_seed(3))
        recs["text" + ("" if layers == 2 else " (3 layers)")] = _record(lambda: txt(ids))
        del txt
    mdir = os.path.join(golden_dir, "boat_surf_masks")
    recs["mask"] = _record(lambda: [mask_preprocess(os.path.join(mdir, m), "cuda:0", H16, 1, 4, 16, downscale=8) for m in ("boat_mask", "surf_mask")])
    ops._CHUNK_CACHE.clear()
    gc.collect()
    torch.cuda.empty_cache()
    print(f"\n[stages] recorded in {time.time() - t0:.0f} s: " +
          "; ".join(f"{k}: {len(r.launches)} unique / {sum(c for _, c in r.launches.values())} calls" for k, r in recs.items()), flush=True)
    return recs


def _unique(stages, family):
    """the unique descriptors of a family over all recordings (a key two recordings share is replayed once), with a stable seed"""
    seen = {}
    for cfg, rec in stages.items():
        for ln, cnt in rec.by_family().get(family, []):
            seen.setdefault(ln.key, (cfg, ln))
    return [(cfg, 104729 + 31 * i, ln) for i, (cfg, ln) in enumerate(seen.values())]


def _report(family, fails, n, worst=None):
    print(f"[stages] {family}: {n} replays, {len(fails)} failing" + (f", worst deviation / bound = {worst:.3f}" if worst is not None else ""), flush=True)
    assert n, f"{family}: nothing recorded"
    assert not fails, f"{family}: {len(fails)} of {n} replays fail:\n" + "\n".join(fails)


def _gemm_descs(stages, prefix=""):
    return [ln.desc for cfg, rec in stages.items() if cfg.startswith(prefix) for ln, _ in rec.by_family().get("gemm", [])]


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def test_stage_entry_points_are_all_covered(stages):
    """every mvoc_* entry point the three stages call is replayed here, is a host query, or names the exact test that covers it"""
    for name, where in NOT_REPLAYED.items():
        mod, fn = where.split("::")
        assert f"def {fn}(" in open(os.path.join(TESTS, mod)).read(), f"{name}: {where} does not exist"
    stray, called = {}, set()
    for cfg, rec in stages.items():
        for name, cnt in rec.calls.items():
            called.add(name)
            if name not in LC.RECORDED and name not in NOT_REPLAYED and name not in G.HOST_QUERIES:
                stray[name] = stray.get(name, 0) + cnt
    assert not stray, f"entry points neither replayed nor covered by a listed exact test: {stray}"
    missing = [n for n in LC.STEM_ENTRIES if n not in called]
    assert not missing, f"stem entries the recordings never called: {missing}"
    # every recorded family has a replay test below
    fams = {LC.FAMILY[ln.name] for rec in stages.values() for ln, _ in rec.launches.values()}
    assert fams <= REPLAYED_FAMILIES, f"recorded families without a replay: {fams - REPLAYED_FAMILIES}"


def test_stage_form_coverage(stages):
    """the forms this census exists for are in the recordings (a refactor that routes them elsewhere fails here, not silently)"""
    g = _gemm_descs(stages)
    vae_g = _gemm_descs(stages, "vae")
    clip_g = _gemm_descs(stages, "vision") + _gemm_descs(stages, "text")
    mid_tokens = {(h // 8) * (w // 8) for _, h, w in VAE_SIZES}
    flash = [ln.desc for rec in stages.values() for ln, _ in rec.by_family().get("flash_attn", [])]
    gn = [ln.desc for rec in stages.values() for ln, _ in rec.by_family().get("groupnorm", [])]
    need = {
        "pad_mode = 1 (stride 2)": any(d.pad_mode == 1 and d.stride == 2 for d in vae_g),
        "n_store < n": any(d.n_store and d.n_store < d.n for d in vae_g),
        "n_store < n with ldo > n_store (decoder conv_out)": any(d.n_store == 3 and d.ldo == 4 for d in vae_g),
        "n_store = 8 (encoder conv_out)": any(d.n_store == 8 for d in vae_g),
        "causal = 1": any(d.causal == 1 for d in flash),
        "head_dim = 96": any(d.head_dim == 96 and not d.causal for d in flash),
        "explicit attention scale": any(d.scale for d in flash),
        "257 and 77 tokens": {257, 77} <= {d.tq for d in flash},
        "GroupNorm eps = 1e-6": any(abs(d.eps - 1e-6) < 1e-9 for d in gn),
        "GroupNorm rows not a multiple of 256": any(d.rows_per_sample % 256 for d in gn),
        "ragged CLIP rows (2 * 257, 5 * 257)": {514, 1285} <= {d.m for d in clip_g},
        "xs_linear in the VAE": any(rec.by_family().get("xs_linear") for cfg, rec in stages.items() if cfg.startswith("vae")),
    }
    for cin in (512, 256, 128):
        need[f"upsample != 0 at cin = {cin}"] = any(d.upsample and d.cin == cin for d in vae_g)
    for t in mid_tokens:
        need[f"plain GEMM with n = {t} mid-block tokens"] = any(d.a_mode == LC.A_PLAIN and d.n == t and d.k == 512 for d in vae_g)
        need[f"P v + b over {t} tokens"] = any(d.a_mode == LC.A_PLAIN and d.k == t and d.n == 512 and d.bias for d in vae_g)
    for k in (1280, 1024):
        need[f"LayerNorm fold with GELU at K = {k}"] = any(d.ln_rowsum and d.act == LC.ACT_GELU and d.k == k for d in g)
    missing = [k for k, ok in need.items() if not ok]
    assert not missing, f"the stage recordings lack: {missing}"


def test_deeper_towers_add_no_descriptor(stages):
    """the key deduplicates layers: a 3-layer tower records the key set of the 2-layer one"""
    for two, three in ((f"vision b={VISION_BATCHES[0]}", f"vision b={VISION_BATCHES[0]} (3 layers)"), ("text", "text (3 layers)")):
        a, b = set(stages[two].launches), set(stages[three].launches)
        assert a == b, f"{two}: {len(a - b)} keys only at 2 layers, {len(b - a)} only at 3"


# ---- replays ------------------------------------------------------------------------------------------------------------------------
def test_stage_gemm(stages):
    from mvoc_amd import ops
    fails, worst, exact = [], 0.0, 0
    todo = _unique(stages, "gemm")
    for cfg, seed, ln in todo:
        try:
            r = G._check_gemm(ln, seed, fails)
            worst = max(worst, r or 0.0)
            exact += ln.desc.act == LC.ACT_NONE and not ln.desc.ln_rowsum
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
        finally:
            ops._CHUNK_CACHE.clear()
    print(f"[stages] gemm: {exact} of {len(todo)} replays are bit-exact integer replays", flush=True)
    _report("gemm", fails, len(todo), worst)


def test_stage_xs_linear(stages):
    lib = G._lib()
    fails, todo = [], _unique(stages, "xs_linear")
    for cfg, seed, ln in todo:
        try:
            d, bufs, L = LC.build_xs(ln.desc, _dev(), seed)
            rc = lib.mvoc_xs_linear_f16(C.byref(d), G._stream())
            if rc:
                raise RuntimeError(f"rc {rc} ({G._err()})")
            _, cols = LC.xs_extents(d)
            assert d.act == LC.ACT_NONE and not d.normalize, "the stages' xs_linear calls are plain: bit-exact"
            bad = 0
            for r0, r1 in LC.xs_blocks(d):
                ref, _ = LC.xs_ref(d, bufs, L, r0, r1)
                got = bufs["out"].reshape(-1)[r0 * d.ldo:r1 * d.ldo].reshape(r1 - r0, d.ldo)[:, :cols].to(F64)
                bad += int((got != ref).sum())
            touched = G._sentinel_count(bufs["out"])
            if bad or touched != d.m * cols:
                fails.append(f"{bad} wrong of {d.m * cols}, {touched - d.m * cols} written outside -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("xs_linear", fails, len(todo), 0.0)


def test_stage_flash_attn(stages):
    """head_dim 96 / explicit scale / causal through the production dispatch, at LC.FLASH_BOUND; the phase kernel and the pipelined
    one return the same bits, and so does the recorded choice"""
    lib = G._lib()
    fails, worst, todo = [], 0.0, _unique(stages, "flash_attn")
    for cfg, seed, ln in todo:
        try:
            d, T = LC.build_attn(ln.desc, _dev(), seed)
            res = {}
            for mode in (ln.desc.pipelined, 1, 2):
                d.pipelined = mode
                T["out"].base_alloc.view(torch.int16).fill_(LC.OUT_SENTINEL)
                rc = lib.mvoc_flash_attn_f16(C.byref(d), G._stream())
                if rc:
                    raise RuntimeError(f"rc {rc} ({G._err()}) at pipelined = {mode}")
                res[mode] = LC.attn_out_view(d, T, "out").clone()
                if mode == ln.desc.pipelined:
                    rl, mx = G._attn_compare(d, T, "out")
                    ratio = max(rl / LC.FLASH_BOUND[0], mx / LC.FLASH_BOUND[1])
                    worst = max(worst, ratio)
                    if not ratio < 1:
                        fails.append(f"{cfg}: rel-L2 {rl:.2e}, max {mx:.2e} -- {LC.describe(ln)}")
                    hd = LC.attn_hd(d)
                    if G._sentinel_count(T["out"]) != d.nbatch * d.tq * d.heads * hd:
                        fails.append(f"{cfg}: wrote {G._sentinel_count(T['out'])} elements, the output has {d.nbatch * d.tq * d.heads * hd} -- {LC.describe(ln)}")
            if not (torch.equal(res[1].view(torch.int16), res[2].view(torch.int16)) and
                    torch.equal(res[ln.desc.pipelined].view(torch.int16), res[1].view(torch.int16))):
                fails.append(f"{cfg}: the kernel choices differ in bits -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("flash_attn", fails, len(todo), worst)


def test_stage_groupnorm(stages):
    """GroupNorm (+ SiLU) at eps = 1e-6 over 4-channel and 16-channel groups, at LC.GN_BOUND"""
    lib = G._lib()
    fails, worst, todo = [], 0.0, _unique(stages, "groupnorm")
    for cfg, seed, ln in todo:
        try:
            d, T, L, _ = LC.build_gn(ln.desc, _dev(), seed)
            rc = lib.mvoc_groupnorm_f16(C.byref(d), G._stream())
            if rc:
                raise RuntimeError(f"rc {rc} ({G._err()})")
            num = den = mx = 0.0
            for s in range(d.nsample):
                ref = LC.gn_ref(d, L, s, s + 1)
                got = T["out"].reshape(-1, d.c)[s * d.rows_per_sample:(s + 1) * d.rows_per_sample].to(F64)
                num += float(((got - ref) ** 2).sum())
                den += float((ref ** 2).sum())
                mx = max(mx, float((got - ref).abs().max()))
            ratio = max((num / den) ** 0.5 / LC.GN_BOUND[0], mx / LC.GN_BOUND[1])
            worst = max(worst, ratio)
            if not ratio < 1 or G._sentinel_count(T["out"]) != d.nsample * d.rows_per_sample * d.c:
                fails.append(f"{cfg}: rel-L2 {(num / den) ** 0.5:.2e}, max {mx:.2e} -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("groupnorm", fails, len(todo), worst)


def test_stage_row_stats_and_layernorm(stages):
    lib = G._lib()
    dev = _dev()
    fails, worst, n = [], 0.0, 0
    for fam in ("row_stats", "row_stats_from_moments", "layernorm"):
        for cfg, seed, ln in _unique(stages, fam):
            n += 1
            a = ln.args
            try:
                gen = torch.Generator(device=dev).manual_seed(seed)
                rows = a["rows"]
                c = a["c"] if "c" in a else a["n"]
                x = (torch.randn(rows, c, generator=gen, device=dev) * 1.5 + 0.3).to(H16)
                if fam == "row_stats":
                    xb = LC.alloc(rows * c, H16, a["x"] % 256, dev)
                    xb.copy_(x.reshape(-1))
                    st = LC.alloc(rows * 2, F32, a["stats"] % 256, dev)
                    rc = lib.mvoc_row_stats_f16(xb.data_ptr(), st.data_ptr(), rows, c, a["eps"], G._stream())
                    ratio = LC.row_stats_ratio(st.reshape(rows, 2), x, a["eps"])
                elif fam == "row_stats_from_moments":
                    mom = LC.alloc(rows * a["ld"] * 2, F32, a["moments"] % 256, dev)
                    mom.copy_(LC.row_moments64(x, a["tile_w"], a["ld"]).to(F32).reshape(-1))
                    st = LC.alloc(rows * 2, F32, a["out"] % 256, dev)
                    rc = lib.mvoc_row_stats_from_moments_f32(mom.data_ptr(), rows, a["ld"], c, a["tile_w"], a["eps"], st.data_ptr(), G._stream())
                    ratio = LC.row_stats_ratio(st.reshape(rows, 2), x, a["eps"])
                else:
                    gm = (1 + 0.2 * torch.randn(c, generator=gen, device=dev)).to(H16)
                    bt = (0.2 * torch.randn(c, generator=gen, device=dev)).to(H16)
                    xb, gb, bb = (LC.alloc(t.numel(), H16, a[nm] % 256, dev) for t, nm in ((x, "x"), (gm, "gamma"), (bt, "beta")))
                    xb.copy_(x.reshape(-1)), gb.copy_(gm), bb.copy_(bt)
                    ob = LC.alloc(rows * c, H16, a["out"] % 256, dev)
                    LC.fill_sentinel(ob)
                    rc = lib.mvoc_layernorm_f16(xb.data_ptr(), gb.data_ptr(), bb.data_ptr(), ob.data_ptr(), rows, c, a["eps"], G._stream())
                    ref = LC.layernorm64(x, gm, bt, a["eps"])
                    got = ob.reshape(rows, c).to(F64)
                    ratio = max(float((got - ref).abs().max()) / LC.LN_BOUND[1], LC.rel_l2(got, ref) / LC.LN_BOUND[0])
                    if LC.stray_writes(ob):
                        fails.append(f"{cfg}: {LC.stray_writes(ob)} elements written outside the output -- {LC.describe(ln)}")
                worst = max(worst, ratio)
                if rc:
                    fails.append(f"{cfg}: rc {rc} ({G._err()}) -- {LC.describe(ln)}")
                elif not ratio <= 1:
                    fails.append(f"{cfg}: {ratio:.2f} x the bound -- {LC.describe(ln)}")
            except (RuntimeError, AssertionError) as e:
                fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    _report("row_stats + layernorm", fails, n, worst)


@pytest.mark.parametrize("name", LC.STEM_ENTRIES)
def test_stage_stem(stages, name):
    """the eleven stem entries: bit for bit, except softmax and the Gaussian sampler, where the neighbouring fp16 value is accepted
    at the elements whose fp32 exponential / quotient sits within its derived error of a rounding boundary"""
    lib = G._lib()
    fam = LC.FAMILY[name]
    fails, worst, alts, todo = [], 0.0, 0, _unique(stages, fam)
    for cfg, seed, ln in todo:
        try:
            args, T = LC.build_stem(ln, _dev(), seed)
            rc = getattr(lib, name)(*args, G._stream())
            if rc:
                raise RuntimeError(f"rc {rc} ({G._err()})")
            bad, ratio, alt = LC.stem_compare(ln, T)
            worst, alts = max(worst, ratio), alts + alt
            stray = sum(LC.stray_writes(T[k]) for k in LC.STEM_OUTPUTS[name])
            left = sum(LC.unwritten(T[k]) for k in LC.STEM_OUTPUTS[name] if T[k].dtype == H16)
            if bad or stray or left:
                fails.append(f"{cfg}: {bad} wrong (worst {ratio:.2f} x the bound), {stray} written outside, {left} not written -- {LC.describe(ln)}")
        except (RuntimeError, AssertionError) as e:
            fails.append(f"{cfg}: {type(e).__name__}: {e} -- {LC.describe(ln)}")
    if name in ("mvoc_softmax_rows_f16", "mvoc_gaussian_sample_f16"):
        print(f"[stages] {fam}: {alts} elements hold the accepted neighbouring value, every other one is bit-exact", flush=True)
    _report(fam, fails, len(todo), worst)


# ---- the VAE forms at the extents VaeCodec produces -------------------------------------------------------------------------------------
SIDE, CH = 512, 256  # the decoder's last level: 256 channels at 512 x 512 after the last upsampler


def _record_large(which, nimg):
    """the descriptor ops.* would send for `which` at nimg frames: recorded dry (nothing launched on the uninitialised buffers)"""
    from mvoc_amd import ops
    from mvoc_amd.unet import Linear
    from mvoc_amd.vae import _Conv3
    dev = _dev()
    z = lambda *s: torch.zeros(s, dtype=H16, device=dev)
    rec = LC.Recorder(dry=True)
    rec.install()
    try:
        if which == "upsample":
            x = torch.empty((nimg * (SIDE // 2) ** 2, CH), dtype=H16, device=dev)
            _Conv3({"c.weight": z(CH, CH, 3, 3), "c.bias": z(CH)}, "c")(x, nimg, SIDE // 2, SIDE // 2, upsample_to=(SIDE, SIDE))
        else:
            x = torch.empty((nimg * SIDE * SIDE, CH), dtype=H16, device=dev)
            if which == "groupnorm":
                ops.groupnorm(x, z(CH), z(CH), nsample=nimg, rows_per_sample=SIDE * SIDE, groups=32, eps=1e-6, silu=True)
            elif which == "conv":
                _Conv3({"c.weight": z(CH // 2, CH, 3, 3), "c.bias": z(CH // 2)}, "c")(x, nimg, SIDE, SIDE)
            else:
                Linear(z(CH // 2, CH), z(CH // 2))(x)
    finally:
        rec.uninstall()
        ops._CHUNK_CACHE.clear()
    (ln, cnt), = rec.launches.values()
    del x
    gc.collect()
    torch.cuda.empty_cache()
    return ln


@pytest.mark.parametrize("nimg", [20, 36])
@pytest.mark.parametrize("which", ["upsample", "groupnorm", "conv", "gemm"])
def test_vae_forms_at_codec_extents(which, nimg):
    """nimg = 20: the 256-channel tensor holds 1.34e9 elements = 2.68e9 bytes (past 2^31 bytes); nimg = 36: 2.4e9 elements = 4.8e9
    bytes (past 2^31 elements and 2^32 bytes).  Image i of the input is image 0 times s_i in {1, -1, 2, -2}, neighbours differing.
    GEMM / conv: image 0 against fp64 in full, bit-exact; image i = s_i * image 0 exactly (test_stage_census_cpu:
    test_multiplier_pattern_keeps_every_image_exact).  GroupNorm + SiLU (beta = 0): eps and SiLU do not commute with the
    multiplier, so images 0..3 (one per multiplier) are held to LC.GN_BOUND against fp64 and image i >= 4 must equal image i % 4
    bit for bit.  A read from the wrong image, a wrapped offset or a dropped tail block breaks the equalities; the sentinel past the
    end and in the slack must survive."""
    lib = G._lib()
    t0 = time.time()
    ln = _record_large(which, nimg)
    mult = LC.image_multipliers(nimg)
    d0 = ln.desc
    print(f"\n[extent] {which} nimg={nimg}: {LC.describe(ln)}", flush=True)
    if which == "groupnorm":
        assert d0.nsample == nimg and d0.rows_per_sample == SIDE * SIDE and d0.c == CH and abs(d0.eps - 1e-6) < 1e-9 and d0.silu
        d, T, L, _ = LC.build_gn(d0, _dev(), 5 + nimg, mult=mult)
        rc = lib.mvoc_groupnorm_f16(C.byref(d), G._stream())
        assert rc == 0, f"rc {rc} ({G._err()})"
        out = T["out"].reshape(nimg, SIDE * SIDE, CH)
        x0 = L["x"]
        for i in range(4):
            Li = {"x": (x0 * mult[i]), "gamma": L["gamma"], "beta": L["beta"]}
            d1 = LC.copy_desc(d)
            d1.nsample = 1
            ref = LC.gn_ref(d1, Li)
            got = out[i].to(F64)
            rl, mx = LC.rel_l2(got, ref), float((got - ref).abs().max())
            print(f"[extent] groupnorm image {i} (x {mult[i]}): rel-L2 {rl:.2e}, max {mx:.2e}", flush=True)
            assert rl < LC.GN_BOUND[0] and mx < LC.GN_BOUND[1], (i, rl, mx)
            del ref, got
        for i in range(4, nimg):
            assert torch.equal(out[i].view(torch.int16), out[i % 4].view(torch.int16)), f"image {i} differs from image {i % 4}"
        assert G._sentinel_count(T["out"]) == nimg * SIDE * SIDE * CH
    else:
        assert d0.m == nimg * SIDE * SIDE and d0.cin == CH and d0.n_store == (CH if which == "upsample" else CH // 2)
        assert (d0.upsample != 0) == (which == "upsample") and (d0.a_mode == LC.A_PLAIN) == (which == "gemm")
        d, T, L = LC.build_gemm(d0, _dev(), 5 + nimg)
        LC.apply_image_multipliers(d, T, L, mult)
        rc = lib.mvoc_gemm_f16(C.byref(d), G._stream())
        assert rc == 0, f"rc {rc} ({G._err()})"
        per, cols = d.m // nimg, LC.gemm_out_cols(d)
        for r0, r1 in LC.gemm_blocks(d):
            if r0 >= per:
                break
            ref, bound = LC.gemm_ref(d, T, L, r0, min(r1, per))
            assert not bound.any() and float(ref.abs().max()) * 2 < 2048 and torch.isfinite(ref).all()
            got = LC.stored_rows(d, T, r0, min(r1, per)).to(F64)
            assert torch.equal(got, ref), f"image 0: {int((got != ref).sum())} wrong of {got.numel()}"
            del ref, got
        out = T["out"].reshape(nimg, per, d.ldo)[:, :, :cols]
        for i in range(1, nimg):
            # (values, not bits: -1 * 0 is -0 in the scaled image and +0 in the kernel's sum)
            assert torch.equal(out[i], out[0] * mult[i]), f"image {i} is not {mult[i]} x image 0: {int((out[i] != out[0] * mult[i]).sum())} differ"
        assert G._sentinel_count(T["out"]) == d.m * cols
    torch.cuda.synchronize()
    print(f"[extent] {which} nimg={nimg}: {time.time() - t0:.1f} s", flush=True)
