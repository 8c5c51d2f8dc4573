"""GPU checks of the folded transformer tail (mvoc_amd.unet._TransformerBase.ff_tail): the two-source plain GEMM that carries it
(every tile form, split-K slices that start in either source, residual and GroupNorm statistics), bit for bit on integer
operands, and the folded tail / network against the unfolded ff2 -> proj_out chain."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mvoc_amd import ops as _ops
    return _ops


def dev(t):
    return t.to("cuda", torch.float16).contiguous()


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("tile", [0, 11, 12, 13, 61, 62, 81, 82])
@pytest.mark.parametrize("m", [333, 2048])
def test_two_source_linear_exact_integers(ops, tile, m):
    """[x | x2] @ w.T + b + r on integer operands, every tile form (PLAIN = 2 for the general tiles)"""
    g = torch.Generator().manual_seed(tile * 100 + m)
    n, k1, k2 = 320, 256, 128
    x = torch.randint(-3, 4, (m, k1), generator=g).float()
    x2 = torch.randint(-3, 4, (m, k2), generator=g).float()
    w = torch.randint(-3, 4, (n, k1 + k2), generator=g).float()
    b = torch.randint(-8, 9, (n,), generator=g).float()
    r = torch.randint(-8, 9, (m, n), generator=g).float()
    out = ops.linear(dev(x), dev(w), dev(b), x2=dev(x2), resid=dev(r), tile=tile)
    ref = torch.cat([x, x2], 1) @ w.t() + b + r
    assert torch.equal(out.float().cpu(), ref)


@pytest.mark.parametrize("tile,split_k", [(11, 4), (11, 5), (13, 4), (61, 5), (0, 0)])
def test_two_source_split_k_exact(ops, tile, split_k):
    """K slices across the source boundary: with k = 2560, c1 = 2048 a 4-way split crosses it inside a slice, a 5-way split
    starts a slice exactly in the second source"""
    g = torch.Generator().manual_seed(7 + tile + split_k)
    m, n, k1, k2 = 512, 256, 2048, 512
    x = torch.randint(-2, 3, (m, k1), generator=g).float()
    x2 = torch.randint(-2, 3, (m, k2), generator=g).float()
    w = torch.randint(-2, 3, (n, k1 + k2), generator=g).float()
    out = ops.linear(dev(x), dev(w), None, x2=dev(x2), tile=tile, split_k=split_k)
    ref = torch.cat([x, x2], 1) @ w.t()
    assert torch.equal(out.float().cpu(), ref)


@pytest.mark.parametrize("n,tile", [(320, 82), (640, 81)])
def test_two_source_chan_sums(ops, n, tile):
    """the eight-phase tiles (256- and 320-wide) still emit the GroupNorm statistics of the stored tile with two sources"""
    g = torch.Generator().manual_seed(n)
    m, k1, k2 = 4096, 4 * n, n
    x = torch.randint(-1, 2, (m, k1), generator=g).float()
    x2 = torch.randint(-1, 2, (m, k2), generator=g).float()
    w = torch.randint(-1, 2, (n, k1 + k2), generator=g).float()
    r = torch.randint(-4, 5, (m, n), generator=g).float()
    out = ops.linear(dev(x), dev(w), None, x2=dev(x2), resid=dev(r), tile=tile, sums=True)
    ref = torch.cat([x, x2], 1) @ w.t() + r
    assert torch.equal(out.float().cpu(), ref)
    cs = getattr(out, "chan_sums", None)
    assert cs is not None, "the fused launch must still write chan_sums"
    o = ref.view(m // 256, 256, n)
    assert torch.equal(cs[..., 0].cpu(), o.sum(1))
    assert torch.equal(cs[..., 1].cpu(), (o * o).sum(1))


@pytest.mark.parametrize("c,m", [(320, 4096), (640, 2048), (1280, 1024), (1280, 5120)])
def test_folded_ff_tail_against_fp32_chain(ops, c, m):
    """proj_out(ff2(f1) + h) + x: folded and unfolded launches against fp32 torch of the unfolded chain, within the per-op
    linear tolerance of test_ops_gpu (rel-L2 1e-3, max-abs 2e-2)"""
    from mvoc_amd.unet import Linear, fold_proj_out
    g = torch.Generator().manual_seed(c + m)
    f1 = torch.randn(m, 4 * c, generator=g).half()
    h = torch.randn(m, c, generator=g).half()
    x = torch.randn(m, c, generator=g).half()
    w2 = (torch.randn(c, 4 * c, generator=g) / math.sqrt(4 * c)).half()
    b2 = (torch.randn(c, generator=g) * 0.1).half()
    wp = (torch.randn(c, c, generator=g) / math.sqrt(c)).half()
    bp = (torch.randn(c, generator=g) * 0.1).half()
    ref = (f1.float() @ w2.float().t() + b2.float() + h.float()) @ wp.float().t() + bp.float() + x.float()
    ff2, po = Linear(dev(w2), dev(b2)), Linear(dev(wp), dev(bp))
    unfolded = po(ff2(dev(f1), resid=dev(h)), resid=dev(x))
    folded = Linear(*fold_proj_out(dev(w2), dev(b2), dev(wp), dev(bp)))(dev(f1), x2=dev(h), resid=dev(x), sums=True)
    for out in (unfolded, folded):
        assert rel_l2(out, ref) < 1e-3
        assert (out.float().cpu() - ref).abs().max() < 2e-2
    assert rel_l2(folded, unfolded) < 1e-3


def test_folded_network_against_unfolded():
    """one UNet forward at the composition batch (B = 5) with the fold on and off: two fp16 evaluations of the same network"""
    from oracle import unet_ref as U
    from mvoc_amd.unet import I2VGenXLUNet, _TransformerBase
    o = U.I2VGenXLUNet(U.UNetConfig.small4())
    U.init_weights_(o, seed=11)
    eng = I2VGenXLUNet(o.config.to_dict())
    eng.load_state_dict(o.state_dict())
    sites = [m for m in _walk(eng) if isinstance(m, _TransformerBase)]
    assert sites and all(s.ff_out is not None for s in sites)
    g = torch.Generator().manual_seed(5)
    b, f, hh, ww = 5, 8, 8, 8
    cd = o.config.cross_attention_dim
    r = lambda *s_: torch.randn(*s_, generator=g).half().float()
    args = (r(b, 4, f, hh, ww), 301, torch.tensor([8] * b), r(b, 4, f, hh, ww), r(b, 4, f, hh, ww), r(b, f, cd), r(b, 7, cd))
    folded = eng.forward_ext(*args)[0]
    saved = [s.ff_out for s in sites]
    try:
        for s in sites:
            s.ff_out = None
        unfolded = eng.forward_ext(*args)[0]
    finally:
        for s, v in zip(sites, saved):
            s.ff_out = v
    rel = rel_l2(folded, unfolded)
    assert rel < 3e-3, rel


def _walk(eng):
    seen, out = set(), []

    def visit(v):
        if id(v) in seen or isinstance(v, (torch.Tensor, str, int, float, type(None))):
            return
        seen.add(id(v))
        out.append(v)
        items = v if isinstance(v, (list, tuple)) else (v.values() if isinstance(v, dict) else
                                                            (vars(v).values() if hasattr(v, "__dict__") else ()))
        for c in items:
            visit(c)
    visit(eng)
    return out
