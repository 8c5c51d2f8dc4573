"""CPU pins of the launch census (tests/launch_census.py): every float64 reference against the torch primitive it restates, the
product's weight packers against the references, the replay builders' buffer arithmetic and the dedup key.  A mismatch of the
GPU census can then only point at a kernel or at the dispatch."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_census as LC  # noqa: E402
from mvoc_amd._ffi import (A_CONV3X3, A_PLAIN, A_TEMPORAL3, ACT_GEGLU, ACT_NONE, ACT_SILU, AttnDesc, GemmDesc,  # noqa: E402
                           GnDesc, TAttnDesc, TFusedDesc, XsDesc)

F64 = torch.float64
CPU = torch.device("cpu")


def _gemm_desc(**kw):
    d = GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _nhwc(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c)


def _conv_desc(nimg, cin, c1, n, h, w, *, stride=1, up=None, pad_mode=0, two=False, act=ACT_NONE, n_store=0, ldo=None,
               resid=False, rowadd_div=0, k_order=0, subpixel=False):
    hup, wup = up if up else (h, w)
    pt = 2 if pad_mode == 0 else 1
    ho, wo = (hup + pt - 3) // stride + 1, (wup + pt - 3) // stride + 1
    cols = n_store or n
    k = 4 * cin if subpixel else -(-9 * cin // 32) * 32
    return _gemm_desc(a=256, a2=512 if two else None, w=768, out=1024, bias=1280, resid=1536 if resid else None,
                      rowadd=1792 if rowadd_div else None, m=nimg * ho * wo, n=n, k=k, n_store=cols, ldo=ldo or cols,
                      ldr=cols if resid else 0, ld_rowadd=cols if rowadd_div else 0, rowadd_div=rowadd_div or 1, a_mode=A_CONV3X3,
                      lda=c1, lda2=cin - c1 if two else 0, c1=c1, cin=cin, nimg=nimg, hout=ho, wout=wo, hsrc=h, wsrc=w, stride=stride,
                      upsample=2 if subpixel else (1 if up else 0), hup=hup, wup=wup, act=act, pad_mode=pad_mode, k_order=k_order)


def _replay_cpu(d, seed=0):
    dd, bufs, L = LC.build_gemm(d, CPU, seed)
    return dd, bufs, L


@pytest.mark.parametrize("case", [
    dict(nimg=2, cin=64, c1=64, n=64, h=6, w=5),
    dict(nimg=2, cin=96, c1=64, n=64, h=5, w=7, two=True, resid=True, rowadd_div=35),
    dict(nimg=3, cin=64, c1=64, n=96, h=7, w=6, stride=2),
    dict(nimg=2, cin=32, c1=32, n=64, h=7, w=8, stride=2, pad_mode=1),
    dict(nimg=2, cin=64, c1=64, n=64, h=5, w=4, up=(9, 7)),
    dict(nimg=2, cin=64, c1=64, n=64, h=4, w=3, up=(8, 6), act=ACT_SILU, n_store=40, ldo=48),
    dict(nimg=2, cin=64, c1=64, n=64, h=4, w=3, up=(8, 6), subpixel=True),
    dict(nimg=2, cin=128, c1=128, n=64, h=4, w=4, k_order=1),
])
def test_conv_reference_matches_torch(case):
    """the conv3x3 reference (nine shifted-slab matmuls, nearest upsample, stride, pad_mode, second source, row-add, residual,
    SiLU, n_store < n) against F.interpolate + F.pad + F.conv2d on the logical weights; the replay packs the weights through
    pack_conv3x3 / pack_conv3x3_subpixel / chunk_major_weights"""
    d = _conv_desc(**case)
    dd, bufs, L = _replay_cpu(d, seed=len(str(case)))
    out, bound = LC.gemm_ref(dd, bufs, L)
    nimg, h, w = d.nimg, d.hsrc, d.wsrc
    x = LC._a_rows_range(dd, bufs, 0, nimg * h * w).reshape(nimg, h, w, d.cin).permute(0, 3, 1, 2)
    if d.upsample:
        x = F.interpolate(x, size=(d.hup, d.wup), mode="nearest")
    x = F.pad(x, (1, 1, 1, 1)) if d.pad_mode == 0 else F.pad(x, (0, 1, 0, 1))
    y = _nhwc(F.conv2d(x, L["w"].double(), L["bias"].double(), stride=d.stride))
    if d.rowadd:
        y = LC.r16(y) + bufs["rowadd"].reshape(-1, d.ld_rowadd)[:, :d.n].double()[torch.arange(d.m) // d.rowadd_div]
    y = LC.r16(y)
    if d.act == ACT_SILU:
        y = LC.r16(F.silu(y))
    y = y[:, :LC.gemm_out_cols(d)]
    if d.resid:
        y = LC.r16(y + bufs["resid"].reshape(d.m, d.ldr)[:, :d.n_store].double())
    assert out.shape == y.shape and torch.equal(out, y)
    assert (bound == 0).all() == (d.act == ACT_NONE)
    if case.get("k_order"):
        from mvoc_amd.unet import pack_conv3x3
        assert torch.equal(bufs["w"].reshape(d.n, d.k), LC.chunk_major_ref(pack_conv3x3(L["w"]), 9))


def test_subpixel_packing_is_upsample_plus_conv():
    """pack_conv3x3_subpixel's four 2 x 2 parity kernels, applied as convs on the source image, equal nearest 2x + 3 x 3 conv"""
    from mvoc_amd.unet import pack_conv3x3_subpixel
    g = torch.Generator().manual_seed(3)
    n, cin, h, w = 32, 8, 5, 4
    wl = torch.randint(-2, 3, (n, cin, 3, 3), generator=g).half()
    x = torch.randint(-2, 3, (2, cin, h, w), generator=g).double()
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wl.double(), padding=1)
    wp = pack_conv3x3_subpixel(wl).double().reshape(4, n, 2, 2, cin).permute(0, 1, 4, 2, 3)
    out = torch.empty_like(ref)
    for a in (0, 1):
        for b in (0, 1):
            pad = (1 - b, b, 1 - a, a)  # parity a: source rows (i - 1, i) for a = 0, (i, i + 1) for a = 1
            out[:, :, a::2, b::2] = F.conv2d(F.pad(x, pad), wp[2 * a + b])
    assert torch.equal(out, ref)


def test_chunk_major_weights_is_the_header_permutation():
    from mvoc_amd import ops
    g = torch.Generator().manual_seed(1)
    for ntaps, cin in ((9, 192), (3, 128)):
        w = torch.randint(-8, 9, (64, ntaps * cin), generator=g).half()
        assert torch.equal(ops.chunk_major_weights(w, ntaps), LC.chunk_major_ref(w, ntaps))


def test_temporal_reference_matches_conv3d():
    d = _gemm_desc(a=0x100, w=0x200, out=0x300, bias=0x400, m=2 * 5 * 6, n=64, k=3 * 64, n_store=64, ldo=64, a_mode=A_TEMPORAL3,
                   lda=64, c1=64, cin=64, frames=5, hw=6, rowadd_div=1)
    dd, bufs, L = _replay_cpu(d, 4)
    out, _ = LC.gemm_ref(dd, bufs, L)
    x = bufs["a"].reshape(2, 5, 6, 64).permute(0, 3, 1, 2).double()[..., None]      # [nvid, c, frames, hw, 1]
    y = F.conv3d(x, L["w"].double(), L["bias"].double(), padding=(1, 0, 0))
    y = y[..., 0].permute(0, 2, 3, 1).reshape(-1, 64)
    assert torch.equal(out, LC.r16(y))
    for r0, r1 in LC.gemm_blocks(dd, budget=30 * 64 * 9):  # row blocks are whole videos and reproduce the full answer
        assert (r0 % 30, r1 % 30) == (0, 0)
        assert torch.equal(LC.gemm_ref(dd, bufs, L, r0, r1)[0], out[r0:r1])


def test_plain_two_source_geglu_and_layernorm_fold_match_torch():
    from oracle.unet_ref import GEGLU
    # two sources split at c1, narrower store into a wider pitch, residual
    d = _gemm_desc(a=0x100, a2=0x140, w=0x200, out=0x300, bias=0x400, resid=0x500, m=37, n=96, k=160, n_store=72, ldo=80, ldr=88,
                   a_mode=A_PLAIN, lda=70, lda2=100, c1=64, cin=160, rowadd_div=1)
    dd, bufs, L = _replay_cpu(d, 5)
    out, bound = LC.gemm_ref(dd, bufs, L)
    x = torch.cat([bufs["a"].reshape(37, 70)[:, :64], bufs["a2"].reshape(37, 100)[:, :96]], 1).double()
    ref = LC.r16(LC.r16(F.linear(x, L["w"].double(), L["bias"].double()))[:, :72] + bufs["resid"].reshape(37, 88)[:, :72].double())
    assert torch.equal(out, ref) and (bound == 0).all()
    # GEGLU: the oracle's chain (value * gelu(gate)) on the logical weights; the replay packed them with pack_geglu
    d = _gemm_desc(a=0x100, w=0x200, out=0x300, bias=0x400, m=41, n=128, k=64, n_store=0, ldo=64, a_mode=A_PLAIN, lda=64, c1=64,
                   cin=64, act=ACT_GEGLU, rowadd_div=1)
    dd, bufs, L = _replay_cpu(d, 6)
    from mvoc_amd.unet import pack_geglu
    assert torch.equal(bufs["w"].reshape(128, 64), pack_geglu(L["w"], L["bias"])[0])
    out, bound = LC.gemm_ref(dd, bufs, L)
    m = GEGLU(64, 64).double()
    with torch.no_grad():
        m.proj.weight.copy_(L["w"].double())
        m.proj.bias.copy_(L["bias"].double())
        ref = m(bufs["a"].reshape(41, 64).double())
    assert ((out - ref).abs() <= LC.ulp16(ref) * 1.5 + 1e-12).all()  # the eager chain's three fp16 roundings
    assert (bound > 0).any()
    # LayerNorm fold: rstd * (acc - mean * rowsum(W')) + (beta @ W^T + b) with W' = W * gamma is F.layer_norm -> F.linear
    g = torch.Generator().manual_seed(7)
    m_, k, n = 29, 64, 96
    x = torch.randn(m_, k, generator=g, dtype=F64) * 1.3 + 0.4
    w = torch.randn(n, k, generator=g, dtype=F64)
    b, gm, bt = (torch.randn(n, generator=g, dtype=F64), 1 + 0.2 * torch.randn(k, generator=g, dtype=F64),
                 0.2 * torch.randn(k, generator=g, dtype=F64))
    wg = w * gm
    mean, rstd = LC.row_stats64(x, 1e-5)
    d = _gemm_desc(m=m_, n=n, k=k, n_store=n, ldo=n, a_mode=A_PLAIN, lda=k, c1=k, cin=k, ln_rowsum=1, ln_bias=1, ln_stats=1,
                   rowadd_div=1)
    T = {"a": x.reshape(-1), "ln_stats": torch.stack([mean, rstd], 1).reshape(-1)}
    acc = LC.gemm_acc(d, T, {"w": wg}, 0, m_)
    y = rstd[:, None] * (acc - mean[:, None] * wg.sum(1)[None, :]) + (w @ bt + b)[None, :]
    assert torch.allclose(y, F.linear(F.layer_norm(x, (k,), gm, bt, 1e-5), w, b), rtol=1e-10, atol=1e-10)
    out, _ = LC.gemm_epilogue(d, acc, T, {"ln_rowsum": wg.sum(1), "ln_bias": w @ bt + b}, 0, m_)
    assert torch.equal(out, LC.r16(y))


def test_replay_builder_extents_alignment_and_pointer_rewrite():
    d = _conv_desc(2, 96, 64, 64, 5, 7, two=True, resid=True, rowadd_div=35)
    d.out, d.resid = 0x10002, 0x2010
    ext = LC.gemm_extents(d)
    assert ext["a"][0] == 2 * 5 * 7 * 64 and ext["a2"][0] == 2 * 5 * 7 * 32
    assert ext["w"][0] == 64 * d.k and ext["out"][0] == d.m * d.ldo and ext["rowadd"][0] == 2 * d.ld_rowadd
    assert LC.gemm_extents(_conv_desc(2, 64, 64, 64, 4, 3, up=(8, 6), subpixel=True))["w"][0] == 4 * 64 * 4 * 64
    assert LC.gemm_extents(_gemm_desc(m=1000, n=640, n_store=640, ldo=640, chan_sums=1))["chan_sums"][0] == 3 * 640 * 2
    assert LC.gemm_extents(_gemm_desc(m=300, n=1280, n_store=1280, ldo=1280, row_moments=1, row_moments_ld=5))["row_moments"][0] == 300 * 5 * 2
    dd, bufs, _ = _replay_cpu(d)
    assert dd.out % 256 == 2 and dd.resid % 256 == 0x10 and dd.out != 0x10002
    for name, t in bufs.items():
        assert getattr(dd, name) == t.data_ptr() and t.numel() == ext[name][0]
    # a pointer field the builder does not know fails before any launch
    bad = LC.copy_desc(d)
    bad.workspace, bad.workspace_bytes = 0x5000, 1 << 20
    with pytest.raises(RuntimeError, match="workspace"):  # a recorded workspace: the library's own size rule must agree
        LC.build_gemm(bad, CPU, 0, workspace_bytes_fn=lambda m, n, k: 0)
    with pytest.raises(RuntimeError, match="no buffer"):
        LC.rewrite(LC.copy_desc(d), {"a": bufs["a"]})
    # alignment of the views
    for mod in (0, 2, 16, 130, 254):
        v = LC.alloc(10, torch.float16, mod, CPU)
        assert v.data_ptr() % 256 == mod
    with pytest.raises(ValueError):
        LC.alloc(10, torch.float32, 6, CPU)


def test_dedup_key():
    a = _gemm_desc(a=0x10000, w=0x20000, out=0x30010, m=1024, n=320, k=320)
    b = _gemm_desc(a=0x70000, w=0x80000, out=0x90010, m=1024, n=320, k=320)   # other addresses, same alignment
    assert LC.desc_key(a) == LC.desc_key(b)
    c = LC.copy_desc(a)
    c.out = 0x30012                                                          # another alignment
    assert LC.desc_key(c) != LC.desc_key(a)
    c = LC.copy_desc(a)
    c.workspace = 0x40000                                                    # a workspace passed
    assert LC.desc_key(c) != LC.desc_key(a)
    c = LC.copy_desc(a)
    c.concurrency = 3                                                        # a scalar field
    assert LC.desc_key(c) != LC.desc_key(a)
    assert LC.ptr_key(None) == (False, 0) and LC.ptr_key(0x100) == (True, 0)


def test_recorder_copies_counts_and_restores():
    from mvoc_amd import ops

    class FakeLib:
        def __init__(self):
            self.seen = []

        def mvoc_gemm_f16(self, pd, stream):
            self.seen.append(pd._obj.m)
            pd._obj.m = -1  # what the callee does to the caller's struct later must not reach the record
            return 0

        def mvoc_add_f16(self, *a):
            return 0

        def mvoc_row_stats_f16(self, *a):
            return 0

    real = ops.lib
    fake = FakeLib()
    ops.lib = fake
    try:
        rec = LC.Recorder()
        rec.install()
        try:
            d = _gemm_desc(a=0x1000, out=0x2002, m=77, n=32, k=32)
            assert ops.lib.mvoc_gemm_f16(C.byref(d), None) == 0
            d2 = _gemm_desc(a=0x5000, out=0x6002, m=77, n=32, k=32)
            ops.lib.mvoc_gemm_f16(C.byref(d2), None)
            ops.lib.mvoc_add_f16(1, 2, 3, 4, None)
            ops.lib.mvoc_row_stats_f16(0x100, 0x204, 10, 64, 1e-5, None)
        finally:
            rec.uninstall()
        assert ops.lib is fake
    finally:
        ops.lib = real
    assert fake.seen == [77, 77]
    assert rec.calls == {"mvoc_gemm_f16": 2, "mvoc_add_f16": 1, "mvoc_row_stats_f16": 1}
    fam = rec.by_family()
    assert len(fam["gemm"]) == 1 and fam["gemm"][0][1] == 2 and fam["gemm"][0][0].desc.m == 77
    (ln, cnt), = fam["row_stats"]
    assert ln.args["rows"] == 10 and LC.ptr_key(ln.args["stats"]) == (True, 4)


def _attn_case(g, nb, heads, tq, tk, kv_bdiv, pair):
    c = heads * 64
    d = AttnDesc()
    d.q_ts, d.k_ts, d.v_ts, d.o_ts = 3 * c, 2 * c, 2 * c, c + 64      # q a slice of a fused buffer, a padded output pitch
    d.q_bs, d.k_bs, d.v_bs, d.o_bs = tq * d.q_ts, tk * d.k_ts, tk * d.v_ts, tq * d.o_ts
    d.nbatch, d.heads, d.tq, d.tk, d.kv_bdiv = nb, heads, tq, tk, kv_bdiv
    d.q, d.k, d.v, d.out = 0x100, 0x200, 0x300, 0x400
    if pair:
        d.v2, d.out2 = 0x500, 0x600
    dd, T = LC.build_attn(d, CPU, 11)
    q = LC.attn_view(T["q"], nb, d.q_bs, tq, d.q_ts, heads, 64).double().transpose(1, 2)
    nkv = nb // kv_bdiv
    kk = LC.attn_view(T["k"], nkv, d.k_bs, tk, d.k_ts, heads, 64).double().transpose(1, 2).repeat_interleave(kv_bdiv, 0)
    for which, vn in (("out", "v"), ("out2", "v2")) if pair else (("out", "v"),):
        vv = LC.attn_view(T[vn], nkv, d.v_bs, tk, d.v_ts, heads, 64).double().transpose(1, 2).repeat_interleave(kv_bdiv, 0)
        ref = F.scaled_dot_product_attention(q, kk, vv).transpose(1, 2)
        assert torch.allclose(LC.attn_ref(dd, T, which), ref, rtol=1e-12, atol=1e-12)
        assert torch.allclose(LC.attn_ref(dd, T, which, 1, nb, 3, tq - 2), ref[1:, 3:tq - 2], rtol=1e-12, atol=1e-12)
    ext = LC.attn_extents(dd)
    assert ext["q"] == (nb - 1) * d.q_bs + (tq - 1) * d.q_ts + c and ext["k"] == (nkv - 1) * d.k_bs + (tk - 1) * d.k_ts + c


def test_attention_references_match_sdpa():
    g = torch.Generator().manual_seed(2)
    _attn_case(g, 4, 2, 19, 13, 2, False)
    _attn_case(g, 3, 1, 16, 16, 1, True)
    # temporal attention over frames, per pixel
    d = TAttnDesc()
    ns, hw, heads, fr = 2, 5, 2, 7
    c = heads * 64
    for p, ld in (("q", 3 * c), ("k", 3 * c), ("v", 3 * c), ("o", c)):
        setattr(d, p + "_ps", ld)
        setattr(d, p + "_ts", hw * ld)
        setattr(d, p + "_bs", fr * hw * ld)
    d.nsample, d.hw, d.heads, d.frames = ns, hw, heads, fr
    d.q, d.k, d.v, d.out = 0x100, 0x200, 0x300, 0x400
    dd, T = LC.build_tattn(d, CPU, 3)

    def seq(name, p):
        full = ns * fr * hw * getattr(d, p + "_ps")
        t = torch.cat([T[name], T[name].new_zeros(full - T[name].numel())]).reshape(ns, fr, hw, -1)[..., :c].double()
        return t.reshape(ns, fr, hw, heads, 64).permute(0, 2, 3, 1, 4)

    ref = F.scaled_dot_product_attention(seq("q", "q"), seq("k", "k"), seq("v", "v"))       # [ns, hw, heads, fr, 64]
    assert torch.allclose(LC.tattn_ref(dd, T), ref.permute(0, 1, 3, 2, 4), rtol=1e-12, atol=1e-12)


def test_tfused_reference_matches_layernorm_linear_sdpa():
    """LN -> QKV with the fp16 rounding of the normalised rows and of q / k / v, as in test_temporal_qkv_attn_fused; the replay
    packs the gamma-folded weights with pack_tfused_weights"""
    from mvoc_amd.unet import pack_tfused_weights
    d = TFusedDesc()
    d.nsample, d.frames, d.hw, d.c, d.heads, d.ln_eps = 2, 8, 5, 128, 2, 1e-5
    d.x, d.wp, d.ln_rowsum, d.ln_bias, d.out = 0x100, 0x200, 0x300, 0x400, 0x500
    dd, T, L = LC.build_tfused(d, CPU, 9)
    rows, c = 2 * 8 * 5, 128
    x = T["x"].reshape(rows, c).float()
    qkv = (F.layer_norm(x, (c,), L["gamma"].float(), L["beta"].float(), 1e-5).half().float() @ L["w"].float().t()).half().double()

    def seq(t):
        return t.reshape(2, 8, 5, 2, 64).permute(0, 2, 3, 1, 4).reshape(10, 2, 8, 64)

    ref = F.scaled_dot_product_attention(seq(qkv[:, :c]), seq(qkv[:, c:2 * c]), seq(qkv[:, 2 * c:]))
    ref = ref.reshape(2, 5, 2, 8, 64).permute(0, 3, 1, 2, 4).reshape(rows, c)
    got = LC.tfused_ref(dd, T, L)
    assert LC.rel_l2(got, ref) < 2e-3  # fp32 vs fp64 LayerNorm can flip an fp16 rounding of q / k / v
    w_ln = (L["w"].float() * L["gamma"].float()[None, :]).half()
    assert torch.equal(T["wp"].reshape(-1), pack_tfused_weights(w_ln, 2).reshape(-1))


def test_groupnorm_references_match_torch():
    d = GnDesc()
    d.nsample, d.rows_per_sample, d.c, d.c1, d.groups, d.silu, d.eps = 2, 512, 96, 64, 8, 1, 1e-5
    d.x, d.x2, d.gamma, d.beta, d.out, d.workspace, d.workspace_bytes = 0x100, 0x200, 0x300, 0x400, 0x500, 0x600, 64
    d.chan_sums, d.chan_sums2 = 0x700, 0x800
    dd, T, L, _ = LC.build_gn(d, CPU, 4)
    x = torch.cat([L["x"], L["x2"]], 1).double()                                  # group 5 straddles the two sources
    ref = F.silu(F.group_norm(x.reshape(2, 512, 96).permute(0, 2, 1), 8, L["gamma"].double(), L["beta"].double(), 1e-5))
    assert torch.allclose(LC.gn_ref(dd, L), ref.permute(0, 2, 1).reshape(-1, 96), rtol=1e-10, atol=1e-10)
    cs = T["chan_sums"].reshape(4, 64, 2)
    assert torch.allclose(cs[1, :, 0].double(), L["x"][256:512].double().sum(0), rtol=1e-6)
    # the fold into xs weights: GN -> linear
    d.x2, d.out, d.silu, d.chan_sums2, d.c = None, None, 0, None, 64
    fa = {"w": LC._Ptr(0x900), "bias": LC._Ptr(0xa00), "n": 96, "k": 64, "wp_sets": LC._Ptr(0xb00)}
    dd, T, L, fa2 = LC.build_gn(d, CPU, 5, fa)
    y = F.group_norm(L["x"].double().reshape(2, 512, 64).permute(0, 2, 1), 8, L["gamma"].double(), L["beta"].double(), 1e-5)
    ref = F.linear(y.permute(0, 2, 1).reshape(-1, 64), L["w"].double(), L["bias"].double())
    assert torch.allclose(LC.gn_fold_ref(dd, L), ref, rtol=1e-10, atol=1e-10)
    assert fa2["wp_sets"].numel() == 2 * 3 * 5 * 512


def test_xs_pack_round_trip_and_reference():
    from mvoc_amd.unet import pack_xs_weights
    g = torch.Generator().manual_seed(8)
    w = torch.randint(-3, 4, (96, 64), generator=g).half()
    c = torch.randn(96, generator=g)
    w2, c2 = LC.unpack_xs_weights(pack_xs_weights(w, c), 96, 64)
    assert torch.equal(w2, w) and torch.equal(c2, c)
    # normalize: rows mu +- v round to exactly +-1 after the LayerNorm, whatever the fp32 rsqrt does
    d = XsDesc()
    d.x, d.wp, d.out, d.m, d.n, d.k, d.n_store, d.ldo, d.normalize, d.ln_eps = 0x100, 0x200, 0x300, 300, 64, 64, 64, 64, 1, 1e-5
    dd, T, L = LC.build_xs(d, CPU, 1)
    x = T["x"].reshape(300, 64).double()
    xn = F.layer_norm(x, (64,), eps=1e-5)
    assert torch.equal(LC.r16(xn).abs(), torch.ones_like(xn))
    out, bound = LC.xs_ref(dd, T, L)
    assert torch.equal(out, LC.r16(LC.r16(xn) @ L["W"][0].double().t() + L["c"][0].double()))
    # per-sample weight sets, GEGLU
    d = XsDesc()
    d.x, d.wp, d.out, d.m, d.n, d.k, d.ldo, d.act, d.wp_set_rows = 0x100, 0x200, 0x300, 512, 128, 64, 64, ACT_GEGLU, 256
    dd, T, L = LC.build_xs(d, CPU, 2)
    assert len(L["W"]) == 2
    for s, (r0, r1) in enumerate(LC.xs_blocks(dd)):
        assert r1 - r0 == 256
        out, _ = LC.xs_ref(dd, T, L, r0, r1)
        y = T["x"].reshape(512, 64)[r0:r1].double() @ L["W"][s].double().t() + L["c"][s].double()
        ref = LC.r16(LC.r16(y[:, :64]) * LC.r16(F.gelu(LC.r16(y[:, 64:]))))
        assert torch.equal(out, ref)


def test_row_stats_and_layernorm_references():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(50, 320, generator=g, dtype=F64) * 1.5 + 0.3
    mean, rstd = LC.row_stats64(x, 1e-5)
    assert torch.allclose(mean, x.mean(1)) and torch.allclose(rstd, 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5))
    gm, bt = torch.randn(320, generator=g, dtype=F64), torch.randn(320, generator=g, dtype=F64)
    assert torch.allclose(LC.layernorm64(x, gm, bt, 1e-5), F.layer_norm(x, (320,), gm, bt, 1e-5), rtol=1e-12, atol=1e-12)
    mom = LC.row_moments64(x, 256, 2)
    assert torch.allclose(mom[:, 0, 0] + mom[:, 1, 0], x.sum(1)) and torch.allclose(mom[:, 1, 1], (x[:, 256:] ** 2).sum(1))


def test_activation_bound_derivation():
    """the GELU term of the bound covers the fp32 A-S 7.1.26 erf evaluation the kernels use (common.h: gelu_fast_f), in its tail"""
    x = torch.linspace(-12, 12, 20001, dtype=torch.float32)
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    erf_abs = 1.0 - poly * torch.exp(-z * z)
    g32 = 0.5 * x * (1.0 + torch.copysign(erf_abs, x))
    g64 = LC.gelu64(x.double())
    assert ((g32.double() - g64).abs() <= LC.GELU_ABS * x.double().abs() + 1e-30).all()
