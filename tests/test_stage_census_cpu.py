"""CPU pins of the stage census (tests/launch_census.py, the VAE / CLIP / mask-path part): every new float64 reference against the
torch primitive it restates, the derivations of the two bounds that are not "bit for bit" measured, the extent functions against
the bytes the torch formulation touches, and the per-image multiplier pattern of the large-extent cases.  A mismatch of
test_stage_census_gpu.py can then only point at a kernel, a packer or the dispatch."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402
from mvoc_amd._ffi import A_CONV3X3, A_PLAIN, ACT_NONE, AttnDesc, GemmDesc  # noqa: E402

F64, F32, H16 = torch.float64, torch.float32, torch.float16
CPU = torch.device("cpu")


def _launch(name, **args):
    """a recorded stem call: pointers are the values given as LC._Ptr"""
    names = LC.ARG_ENTRIES[name]
    assert tuple(args) == names, (tuple(args), names)
    return LC.Launch(name, None, args)


P = LC._Ptr


def _nhwc(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c)


# ---- references against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(8, 8), (7, 10), (6, 5)])
def test_pad_mode_1_conv_reference_is_pad_bottom_right_plus_stride_2(h, w):
    """the encoder's Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) + conv2d(stride=2, padding=0), with n_store < n and a padded
    output pitch; the replay leaves the sentinel in the pitch's tail"""
    nimg, cin, n, ns, ldo = 2, 32, 32, 5, 8
    ho, wo = (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1
    d = GemmDesc()
    d.a, d.w, d.out, d.bias = 0x100, 0x200, 0x310, 0x400
    d.m, d.n, d.k, d.n_store, d.ldo, d.rowadd_div = nimg * ho * wo, n, 9 * cin, ns, ldo, 1
    d.a_mode, d.lda, d.c1, d.cin, d.nimg, d.hout, d.wout, d.hsrc, d.wsrc = A_CONV3X3, cin, cin, cin, nimg, ho, wo, h, w
    d.stride, d.hup, d.wup, d.pad_mode = 2, h, w, 1
    dd, bufs, L = LC.build_gemm(d, CPU, 3)
    out, bound = LC.gemm_ref(dd, bufs, L)
    x = bufs["a"].reshape(nimg, h, w, cin).permute(0, 3, 1, 2).double()
    ref = _nhwc(F.conv2d(F.pad(x, (0, 1, 0, 1)), L["w"].double(), L["bias"].double(), stride=2, padding=0))
    assert tuple(ref.shape) == (d.m, n) and torch.equal(out, ref[:, :ns]) and not bound.any()
    assert LC.gemm_extents(dd)["out"][0] == d.m * ldo and LC.stored_rows(dd, bufs, 0, d.m).shape == (d.m, ns)
    assert int((bufs["out"].base_alloc.view(torch.int16) != LC.OUT_SENTINEL).sum()) == 0  # nothing written yet: all sentinel


def test_causal_scaled_head_dim_96_attention_reference_matches_sdpa():
    nb, heads, t, hd = 2, 3, 21, 96
    c = heads * hd
    d = AttnDesc()
    d.q_ts = d.k_ts = d.v_ts = 3 * c
    d.o_ts = c
    d.q_bs = d.k_bs = d.v_bs = t * 3 * c
    d.o_bs = t * c
    d.nbatch, d.heads, d.tq, d.tk, d.kv_bdiv, d.head_dim, d.causal, d.scale = nb, heads, t, t, 1, hd, 1, 1.0 / math.sqrt(80.0)
    d.q, d.k, d.v, d.out = 0x100, 0x200, 0x300, 0x400
    dd, T = LC.build_attn(d, CPU, 5)
    q, k, v = (LC.attn_view(T[n_], nb, t * 3 * c, t, 3 * c, heads, hd).double().transpose(1, 2) for n_ in "qkv")
    ref = F.scaled_dot_product_attention(q, k, v, is_causal=True, scale=float(d.scale)).transpose(1, 2)
    assert LC.attn_hd(dd) == 96 and abs(LC.attn_scale(dd) - 1 / math.sqrt(80)) < 1e-7
    assert torch.allclose(LC.attn_ref(dd, T), ref, rtol=1e-12, atol=1e-12)
    assert torch.allclose(LC.attn_ref(dd, T, "out", 1, 2, 5, 17), ref[1:, 5:17], rtol=1e-12, atol=1e-12)  # the mask follows q0
    full = F.scaled_dot_product_attention(q, k, v, scale=float(d.scale)).transpose(1, 2)
    assert not torch.allclose(LC.attn_ref(dd, T), full, atol=1e-3)  # (the mask matters on this data)
    # extents: the last element a [nb, t, heads, hd] view of the fused buffer reaches
    ext = LC.attn_extents(dd)
    assert ext["q"] == (nb - 1) * d.q_bs + (t - 1) * d.q_ts + heads * hd and ext["out"] == nb * t * c
    with pytest.raises(RuntimeError, match="no buffer for the recorded pointer field `out`"):  # every pointer field is rewritten
        LC.rewrite(LC.copy_desc(d), {k_: T[k_] for k_ in "qkv"})


@pytest.mark.parametrize("stride,silu,cin,cout", [(1, 0, 3, 8), (2, 0, 4, 6), (1, 1, 4, 5), (2, 1, 3, 7)])
def test_conv3x3_small_reference_and_packer(stride, silu, cin, cout):
    """conv3x3_small: logical integer weights through the product's pack_conv3x3_small into the header's [cout][3][3][cin]"""
    ln = _launch("mvoc_conv3x3_small_f16", x=P(0x100), w=P(0x210), bias=P(0x300), out=P(0x402), nimg=2, h=7, wd=6, cin=cin, cout=cout,
                 stride=stride, silu=silu)
    args, T = LC.build_stem(ln, CPU, 1)
    ref = LC.stem_ref(ln, T)["out"]
    x = T["x"].reshape(2, 7, 6, cin).permute(0, 3, 1, 2).double()
    y = LC.r16(_nhwc(F.conv2d(x, T["W"].double(), T["bias"].double(), stride=stride, padding=1)))
    if silu:
        y = LC.r16(F.silu(y))
    assert torch.equal(ref[0], y.reshape(-1)) and (ref[1] is None) == (not silu)
    assert torch.equal(T["w"].reshape(cout, 3, 3, cin), T["W"].permute(0, 2, 3, 1))  # w[co][ky][kx][c]
    assert T["out"].data_ptr() % 256 == 2 and args[3] == T["out"].data_ptr() and args[4:] == [2, 7, 6, cin, cout, stride, silu]


def test_softmax_reference_matches_torch():
    ln = _launch("mvoc_softmax_rows_f16", x=P(0x100), rows=9, cols=64)
    _, T = LC.build_stem(ln, CPU, 2)
    v, (lo, hi) = LC.stem_ref(ln, T)["x"]
    ref = torch.softmax(T["X"].double(), -1)
    assert torch.equal(v.reshape(9, 64), ref.half().double()) and torch.equal(T["x"].reshape(9, 64), T["X"])
    for alt in (lo, hi):  # the alternatives: the same value almost everywhere, never more than the neighbouring fp16 value
        assert ((alt - v).abs() <= LC.ulp16(v)).all() and float((alt != v).double().mean()) < 0.02
    T["x"].copy_(torch.softmax(T["X"].float(), -1).half().reshape(-1))  # an fp32 evaluation passes; one ulp off everywhere does not
    assert LC.stem_compare(ln, T)[0] == 0
    T["x"].copy_((v + LC.ulp16(v)).half())
    assert LC.stem_compare(ln, T)[0] > 500
    assert float(T["X"].max()) == 40.0 and (T["X"][0] == T["X"][0, 0]).all()  # a dominant score and a constant row are in the data


def test_small_references_match_torch():
    g = torch.Generator().manual_seed(4)
    # conv1x1_small
    ln = _launch("mvoc_conv1x1_small_f16", x=P(0x100), w=P(0x200), bias=P(0x300), out=P(0x400), rows=37, cin=8, cout=5)
    _, T = LC.build_stem(ln, CPU, 1)
    y = F.conv2d(T["x"].reshape(1, 37, 1, 8).permute(0, 3, 1, 2).double(), T["w"].reshape(5, 8, 1, 1).double(), T["bias"].double())
    assert torch.equal(LC.stem_ref(ln, T)["out"][0], _nhwc(y).reshape(-1)) and float(y.abs().max()) < 2048
    # layouts
    ln = _launch("mvoc_image_to_tokens_f16", x=P(0x100), out=P(0x200), n=3, c=5, hw=42)
    _, T = LC.build_stem(ln, CPU, 1)
    assert torch.equal(LC.stem_ref(ln, T)["out"][0], _nhwc(T["x"].reshape(3, 5, 6, 7)).reshape(-1))
    ln = _launch("mvoc_tokens_to_image_f16", x=P(0x100), out=P(0x200), n=3, c=3, hw=42, ld=4)
    _, T = LC.build_stem(ln, CPU, 1)
    rows = torch.cat([T["x"], T["x"].new_zeros(1)]).reshape(3 * 42, 4)
    assert torch.equal(LC.stem_ref(ln, T)["out"][0], rows[:, :3].reshape(3, 42, 3).permute(0, 2, 1).reshape(-1))
    # python float * fp16 tensor, as eager does it
    x = (torch.randn(4096, generator=g) * 4).half()
    for s in (0.18215, 1 / 0.18215):
        assert torch.equal(LC.scale64(x, s), x * s)
    # CLIP patches = unfold, embed = embedding lookups
    px = torch.randn(2, 3, 28, 28, generator=g).half()
    ref = F.unfold(px.float(), kernel_size=14, stride=14).transpose(1, 2).reshape(2 * 4, 3 * 14 * 14).half()
    got = LC.clip_patches_ref(px, 14, 640)
    assert torch.equal(got[:, :588], ref) and not got[:, 588:].any() and got.shape == (8, 640)
    tab, pos, cls = torch.randn(50, 16, generator=g).half(), torch.randn(5, 16, generator=g).half(), torch.randn(16, generator=g).half()
    ids = torch.randint(0, 50, (10,), generator=g, dtype=torch.int32)
    want = (F.embedding(ids.long(), tab.double()) + pos.double().repeat(2, 1)).half()
    assert torch.equal(LC.clip_embed_ref(tab, ids, None, pos, 10, 5), want)
    pe = torch.randn(2 * 4, 16, generator=g).half()
    want = (torch.cat([cls.expand(2, 1, 16), pe.reshape(2, 4, 16)], 1).double() + pos.double()[None]).half().reshape(10, 16)
    assert torch.equal(LC.clip_embed_ref(pe, None, cls, pos, 10, 5), want)
    # mask_finish: `.to(float32).div_(255.0).to(fp16)` and cv.threshold(v, 10, 255) / 255 -> bool
    ln = _launch("mvoc_mask_finish", v=P(0x100), float_mask=P(0x200), bool_mask=P(0x300), n=300)
    _, T = LC.build_stem(ln, CPU, 1)
    r = LC.stem_ref(ln, T)
    assert torch.equal(r["float_mask"][0], T["v"].to(F32).div_(255.0).half()) and torch.equal(r["bool_mask"][0].bool(), T["v"] > 10)
    assert len(T["v"].unique()) == 256


def test_mask_resize_reference_is_the_path_of_the_g9_fixture(golden_dir):
    """the reference of mask_resize_u8 is PIL's own resize; on the boat_surf masks it gives the recorded G9 arrays, its
    horizontal-only form is the kernel's intermediate, and the product's tables evaluated in numpy agree on noise"""
    from PIL import Image
    from mvoc_amd.utils import resize8_reference
    g = np.load(os.path.join(golden_dir, "g9_boat_surf_masks.npz"))
    for name in ("boat_mask", "surf_mask"):
        d = os.path.join(golden_dir, "boat_surf_masks", name)
        fr = torch.from_numpy(np.stack([np.asarray(Image.open(os.path.join(d, f"{i:05d}.png")).convert("L")) for i in range(16)]))
        out = LC.pil_resize_u8(fr, fr.shape[2] // 8, fr.shape[1] // 8)
        assert np.array_equal(out.numpy(), g[f"{name}_90x160_float_u8"])
        assert np.array_equal((out > 10).numpy(), g[f"{name}_90x160_bool"])
    noise = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 48, 64), dtype=np.uint8))
    assert np.array_equal(LC.pil_resize_u8(noise, 8, 6).numpy(), resize8_reference(noise.numpy(), (6, 8)))
    ln = _launch("mvoc_mask_resize_u8", **{"in": P(0x100), "tmp": P(0x200), "out": P(0x300), "n": 2, "H": 48, "W": 64, "h": 6, "w": 8,
                                           "bounds_h": P(0x400), "kk_h": P(0x500), "ksize_h": 33, "bounds_v": P(0x600), "kk_v": P(0x700),
                                           "ksize_v": 33})
    _, T = LC.build_stem(ln, CPU, 1)
    r = LC.stem_ref(ln, T)
    fr = T["in"].reshape(2, 48, 64).numpy()
    assert np.array_equal(r["out"][0].reshape(2, 6, 8).numpy(), resize8_reference(fr, (6, 8)))
    assert np.array_equal(r["tmp"][0].reshape(2, 48, 8).numpy(), resize8_reference(fr, (48, 8)))  # (a same-size pass is the identity)


def test_gaussian_sample_reference_is_the_eager_chain():
    """against torch's CPU half ops (fp32 compute, one rounding per op): equal, except where exp lands within its fp32 error of an
    fp16 rounding boundary -- there the neighbouring standard deviation's result is accepted, nothing else"""
    ln = _launch("mvoc_gaussian_sample_f16", mean=P(0x100), logvar=P(0x200), noise=P(0x300), out=P(0x400), n=1 << 16)
    _, T = LC.build_stem(ln, CPU, 7)
    mean, logvar, noise = T["mean"], T["logvar"], T["noise"]
    eager = (mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * noise).double()
    v, (lo, hi) = LC.stem_ref(ln, T)["out"]
    assert ((eager == v) | (eager == lo) | (eager == hi)).all()
    loose = float(((lo != v) | (hi != v)).double().mean())
    print(f"gaussian_sample: {loose:.2e} of the elements have an alternative")
    assert loose < 2e-2 and float((eager != v).double().mean()) < 1e-2
    assert float(logvar[:7].min()) == -40.0 and float(logvar[:7].max()) == 30.0


# ---- derived bounds, measured -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [64, 1024, 4096])
def test_softmax_bound_derivation(cols):
    """an fp32 evaluation of the kernel's chain (max, exp2((x - max) log2 e), sum, 1 / sum, product) against fp64 stays inside
    softmax_rel(cols) wherever the result does not round to zero, and such results have |x - max| < 17.4 as the derivation assumes"""
    g = torch.Generator().manual_seed(cols)
    x = (torch.randn(64, cols, generator=g) * 3).half()
    x[3, 5], x[7] = 40.0, x[7, 0]
    x[9] = (torch.randn(cols, generator=g) * 0.05).half()
    x32 = x.float()
    dlt = x32 - x32.max(1, keepdim=True).values
    e = torch.exp2(dlt * torch.tensor(1.4426950408889634, dtype=F32))
    # per-lane sequential sums over cols / 64 steps, then the butterfly, as the kernel adds them
    lanes = e.reshape(64, -1, 64)  # column c belongs to lane (c / 8) % 64: any fixed assignment measures the same rounding growth
    acc = torch.zeros(64, 64)
    for i in range(lanes.shape[1]):
        acc = acc + lanes[:, i]
    while acc.shape[1] > 1:
        acc = acc[:, ::2] + acc[:, 1::2]
    p32 = e * (torch.tensor(1.0) / acc)
    p64 = torch.softmax(x.double(), -1)
    live = p64 >= 2.0 ** -25
    rel = ((p32.double() - p64).abs() / p64)[live]
    print(f"softmax cols={cols}: measured fp32 error {float(rel.max()) * 2 ** 23:.1f} ulp32, bound {LC.softmax_rel(cols) * 2 ** 23:.1f}")
    assert float(rel.max()) <= LC.softmax_rel(cols)
    assert float(dlt.double()[live].abs().max()) < 17.4
    assert LC.softmax_rel(cols) < 2.0 ** -13  # far under half an fp16 ulp (2^-11 relative): the term only decides rounding flips


def test_exp32_bound_derivation():
    """both ways an fp32 exponential is evaluated, at every fp16 argument the sampler can produce, against exp32_rel"""
    h = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(H16)
    h = h[torch.isfinite(h) & (h >= -15) & (h <= 10)].float()
    e64 = torch.exp(h.double())
    worst = 0.0
    for e32 in (torch.exp(h), torch.exp2(h * torch.tensor(1.4426950408889634, dtype=F32))):
        r = (e32.double() - e64).abs() / e64 / LC.exp32_rel(h.double())
        worst = max(worst, float(r.max()))
    print(f"exp32: worst measured error / bound = {worst:.2f}")
    assert worst <= 1.0


# ---- extents = what the torch formulation touches --------------------------------------------------------------------------------------
def test_stem_extents_equal_the_torch_tensors():
    e = LC.stem_extents
    a = dict(nimg=2, h=7, wd=6, cin=3, cout=8, stride=2, silu=0)
    x, w = torch.empty(2, 3, 7, 6), torch.empty(8, 3, 3, 3)
    ext = e("mvoc_conv3x3_small_f16", a)
    assert ext["x"][0] == x.numel() and ext["w"][0] == w.numel() and ext["bias"][0] == 8
    assert ext["out"][0] == F.conv2d(x, w, stride=2, padding=1).numel()
    ext = e("mvoc_conv1x1_small_f16", dict(rows=37, cin=8, cout=5))
    assert (ext["x"][0], ext["w"][0], ext["bias"][0], ext["out"][0]) == (37 * 8, 40, 5, 37 * 5)
    assert e("mvoc_softmax_rows_f16", dict(rows=9, cols=64))["x"] == (9 * 64, H16)
    assert e("mvoc_image_to_tokens_f16", dict(n=3, c=5, hw=42)) == {"x": (630, H16), "out": (630, H16)}
    ext = e("mvoc_tokens_to_image_f16", dict(n=3, c=3, hw=42, ld=4))
    view = torch.empty(3 * 42 * 4).as_strided((3, 42, 3), (42 * 4, 4, 1))
    assert ext["x"][0] == sum((s - 1) * st for s, st in zip(view.shape, view.stride())) + 1 and ext["out"][0] == 3 * 3 * 42
    assert all(v == (77, H16) for v in e("mvoc_gaussian_sample_f16", dict(n=77)).values())
    assert e("mvoc_scale_f16", dict(n=77, scale=0.5)) == {"x": (77, H16), "out": (77, H16)}
    ext = e("mvoc_clip_patches_f16", dict(nimg=2, size=28, patch=14, kpad=640))
    assert ext["pixels"][0] == 2 * 3 * 28 * 28 and ext["out"][0] == F.unfold(torch.empty(2, 3, 28, 28), 14, stride=14).shape[2] * 2 * 640
    ext = e("mvoc_clip_embed_f16", dict(table=P(1), ids=P(0), cls=P(1), pos=P(1), out=P(1), rows=10, t=5, c=16))
    assert ext["table"][0] == 2 * 4 * 16 and ext["pos"][0] == 5 * 16 and ext["out"][0] == 160 and ext["cls"][0] == 16
    ext = e("mvoc_clip_embed_f16", dict(table=P(1), ids=P(1), cls=P(0), pos=P(1), out=P(1), rows=10, t=5, c=16))
    assert ext["table"][0] == LC.STEM_VOCAB * 16 and ext["ids"] == (10, torch.int32)
    ext = e("mvoc_mask_resize_u8", dict(n=2, H=48, W=64, h=6, w=8, ksize_h=33, ksize_v=33))
    assert (ext["in"][0], ext["tmp"][0], ext["out"][0]) == (2 * 48 * 64, 2 * 48 * 8, 2 * 6 * 8)
    assert (ext["bounds_h"][0], ext["kk_h"][0], ext["bounds_v"][0], ext["kk_v"][0]) == (16, 8 * 33, 12, 6 * 33)
    assert e("mvoc_mask_finish", dict(n=300)) == {"v": (300, torch.uint8), "float_mask": (300, H16), "bool_mask": (300, torch.uint8)}
    assert set(LC.STEM_ENTRIES) == set(LC.STEM_OUTPUTS) and all(n in LC.ARG_ENTRIES and n in LC.FAMILY for n in LC.STEM_ENTRIES)


def test_an_unknown_pointer_argument_fails_on_the_host():
    ln = LC.Launch("mvoc_scale_f16", None, {"x": P(0x100), "out": P(0x200), "n": 8, "scale": 0.5, "extra": P(0x300)})
    with pytest.raises(RuntimeError, match="extra"):
        LC.build_stem(ln, CPU, 0)
    ln = LC.Launch("mvoc_scale_f16", None, {"x": P(0x100), "out": P(0), "n": 8, "scale": 0.5})
    with pytest.raises(RuntimeError, match="out"):
        LC.build_stem(ln, CPU, 0)
    # the views sit at the recorded alignment, the outputs inside a sentinel-filled allocation
    ln = _launch("mvoc_scale_f16", x=P(0x10e), out=P(0x2f2), n=100, scale=0.5)
    args, T = LC.build_stem(ln, CPU, 0)
    assert args[0] % 256 == 0x0e and args[1] % 256 == 0xf2 and args[2:] == [100, 0.5]
    assert LC.unwritten(T["out"]) == 100 and LC.stray_writes(T["out"]) == 0
    T["out"].copy_(LC.stem_ref(ln, T)["out"][0])
    assert LC.stem_compare(ln, T) == (0, 0.0, 0) and LC.unwritten(T["out"]) == 0
    T["out"].base_alloc[0] = 1.0
    T["out"][3] += 1
    assert LC.stray_writes(T["out"]) == 1 and LC.stem_compare(ln, T)[0] == 1


def test_recorder_stands_in_for_every_holder_of_the_library():
    """vae.py, clip.py and utils.py (through _ffi) call stem entries on a `lib` of their own: all of them are recorded, restored
    afterwards, and a dry recorder launches nothing"""
    import importlib
    mods = [importlib.import_module(n) for n in LC.LIB_HOLDERS]
    before = [m.lib for m in mods]

    class Fake:
        def __init__(self):
            self.n = 0

        def mvoc_scale_f16(self, *a):
            self.n += 1
            return 0

        def mvoc_version(self):
            return 100

    fake = Fake()
    import mvoc_amd.vae as V
    V.lib = fake
    try:
        for dry in (False, True):
            rec = LC.Recorder(dry=dry)
            rec.install()
            try:
                assert V.lib.mvoc_scale_f16(0x100, 0x202, 5, 0.25, None) == 0 and V.lib.mvoc_version() == 100
            finally:
                rec.uninstall()
            (ln, cnt), = rec.by_family()["scale"]
            assert ln.args == {"x": 0x100, "out": 0x202, "n": 5, "scale": 0.25} and LC.ptr_key(ln.args["out"]) == (True, 2)
            assert rec.calls == {"mvoc_scale_f16": 1, "mvoc_version": 1} and V.lib is fake
        assert fake.n == 1
    finally:
        V.lib = before[LC.LIB_HOLDERS.index("mvoc_amd.vae")]
    assert [m.lib for m in mods] == before


# ---- the multiplier pattern of the large-extent cases ---------------------------------------------------------------------------------
def _vae_large_form(which, nimg, side):
    """the four launches that meet the decoder's 256-channel tensor, at a small side: descriptors as ops.* fills them"""
    d = GemmDesc()
    d.a, d.w, d.out, d.bias, d.rowadd_div = 0x100, 0x200, 0x300, 0x400, 1
    if which == "upsample":
        d.a_mode, d.n, d.k, d.cin, d.hsrc, d.wsrc, d.hup, d.wup, d.upsample = A_CONV3X3, 256, 9 * 256, 256, side // 2, side // 2, side, side, 1
    elif which == "conv":
        d.a_mode, d.n, d.k, d.cin, d.hsrc, d.wsrc, d.hup, d.wup = A_CONV3X3, 128, 9 * 256, 256, side, side, side, side
    else:
        d.a_mode, d.n, d.k, d.cin = A_PLAIN, 128, 256, 256
    d.c1 = d.lda = 256
    d.n_store = d.ldo = d.n
    d.nimg, d.hout, d.wout, d.stride = nimg, side, side, 1
    d.m = nimg * side * side
    return d


@pytest.mark.parametrize("which", ["upsample", "conv", "gemm"])
def test_multiplier_pattern_keeps_every_image_exact(which):
    """image i = image 0 * s_i: every value of image 0's fp64 reference times every multiplier is an integer below 2048 (exact in
    fp16, and every fp32 partial sum exact), neighbouring images differ, and the full reference of image i IS s_i times image 0's"""
    mult = LC.image_multipliers(7)
    assert mult[:5] == [1, -1, 2, -2, 1] and all(a != b for a, b in zip(mult, mult[1:])) and set(mult) == set(LC.IMAGE_MULT)
    d = _vae_large_form(which, 7, 12)
    dd, bufs, L = LC.build_gemm(d, CPU, 11)
    LC.apply_image_multipliers(dd, bufs, L, mult)
    per = d.m // 7
    ref0, bound = LC.gemm_ref(dd, bufs, L, 0, per)
    assert not bound.any() and torch.isfinite(ref0).all() and torch.equal(ref0, ref0.round())
    for s in LC.IMAGE_MULT:
        assert float((ref0 * s).abs().max()) < 2048 and torch.equal((ref0 * s).half().double(), ref0 * s)
    print(f"{which}: max |image 0| = {float(ref0.abs().max()):.0f} (x 2 must stay under 2048)")
    for i in range(1, 7):
        assert torch.equal(LC.gemm_ref(dd, bufs, L, i * per, (i + 1) * per)[0], ref0 * mult[i])
    with pytest.raises(RuntimeError):
        dd.resid = 0x500
        LC.apply_image_multipliers(dd, bufs, L, mult)


def test_groupnorm_images_with_equal_multipliers_are_equal_and_the_sign_carries_through():
    """GroupNorm of s * x: the statistics scale exactly for s in {1, -1, 2, -2}, but eps = 1e-6 does not (var + eps), and SiLU is not
    odd: so the large-extent GroupNorm case compares images with EQUAL multipliers bit for bit and checks one image per multiplier
    against fp64; without SiLU and with beta = 0 the output of -x is the negated output of x"""
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(2 * 64, 32, generator=g) * 2 + 0.5).half()
    xs = torch.cat([x[:64] * s for s in (1, -1, 2, -2)])
    gm = (1 + 0.2 * torch.randn(32, generator=g)).half()
    y = LC.groupnorm64(xs, 4, 8, 1e-6, gm, torch.zeros(32).half(), False).reshape(4, 64, 32)
    assert torch.equal(y[1], -y[0]) and torch.equal(y[3], -y[2]) and not torch.equal(y[2], y[0])
    assert torch.allclose(y[2], y[0], rtol=1e-6)  # eps: a relative 1e-7, enough to flip fp16 roundings in 1e9 elements
    ys = LC.groupnorm64(xs, 4, 8, 1e-6, gm, torch.zeros(32).half(), True).reshape(4, 64, 32)
    assert not torch.allclose(ys[1], -ys[0], atol=1e-2)
