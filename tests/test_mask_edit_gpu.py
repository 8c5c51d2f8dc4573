"""GPU: the mask filter kernels (mvoc_mask_filter_f16 / mvoc_mask_filter_u8) against the restatement of their rule in
tests/test_mask_edit_cpu.py (``ref_pass_f16`` in torch on the CPU, ``ref_pass_u8`` in numpy int64) -- exact equality everywhere,
bit for bit in fp16 -- and the sampling call's ``obj_mask_edit`` on the toy composition of tests/test_collage_gpu.py: the run
equals the run without the argument that is handed the reference's pre-edited masks and alphas."""
import numpy as np
import pytest
import torch

import test_collage_gpu as tcg
import test_mask_edit_cpu as tmc

pytestmark = pytest.mark.gpu
tv = tcg.tv
OPS = ("max", "min", "mean")
SENTINEL = 0x5A
PAD = 64


# ---- kernels against the rule ----------------------------------------------------------------------------------------------------
def _flush(t, fill):
    """``t`` copied to the device so that it ends where its allocation's tensor ends; the 37 elements in front of it hold ``fill``"""
    buf = torch.full((37 + t.numel(),), fill, dtype=t.dtype, device="cuda")
    view = buf[37:].view(t.shape)
    view.copy_(t)
    return view


def _run(src_dev, op, radius, axis):
    """one launch into an output with sentinels before and behind it -> the output on the host; the sentinels must survive"""
    from mvoc_amd import ops
    n = src_dev.numel()
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.uint8, device="cuda") if src_dev.dtype == torch.uint8 else \
        torch.full((PAD + n + PAD,), SENTINEL * 257, dtype=torch.int16, device="cuda").view(torch.float16)
    out = buf[PAD:PAD + n].view(src_dev.shape)
    assert ops.mask_filter(src_dev, op, radius, axis, out=out) is out
    torch.cuda.synchronize()
    host = buf.cpu()
    raw = host if host.dtype == torch.uint8 else host.view(torch.int16)
    want = SENTINEL if host.dtype == torch.uint8 else SENTINEL * 257
    assert (raw[:PAD] == want).all() and (raw[PAD + n:] == want).all(), (op, radius, axis)
    return host[PAD:PAD + n].view(src_dev.shape)


def _radii(h, w):
    return [0, 1, 2, 8] + ([64] if (h, w) == (1, 7) else [])  # 8 on 5 x 6 and 64 on 1 x 7: at least as large as the plane


@pytest.mark.parametrize("nplane", [1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 6), (4, 6), (1, 255), (1, 257), (16, 16), (1, 511), (1, 513)],
                         ids=lambda v: f"{v[0]}x{v[1]}")
def test_the_fp16_kernels_give_the_bits_of_the_rule(hw, nplane):
    h, w = hw
    for kind in ("k255", "any"):
        src = tmc._planes((nplane, h, w), 1000 * h + w + nplane, kind)
        dev = _flush(src, float("nan"))
        for op in OPS:
            for axis in (0, 1):
                for r in _radii(h, w):
                    got = _run(dev, op, r, axis)
                    assert tmc._same_bits(got, tmc.ref_pass_f16(src, op, r, axis)), (kind, op, axis, r)
    # a fresh output tensor: the same bits
    from mvoc_amd import ops
    assert tmc._same_bits(ops.mask_filter(dev, "mean", 2, 1).cpu(), tmc.ref_pass_f16(src, "mean", 2, 1))


@pytest.mark.parametrize("nplane", [1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 6), (4, 6), (1, 255), (1, 257), (16, 16), (1, 511), (1, 513)],
                         ids=lambda v: f"{v[0]}x{v[1]}")
def test_the_u8_kernels_give_the_bytes_of_the_rule(hw, nplane):
    h, w = hw
    src = np.random.default_rng(1000 * h + w + nplane).integers(0, 256, (nplane, h, w), dtype=np.uint8)
    src[:, : (h + 1) // 2] = np.where(src[:, : (h + 1) // 2] > 127, 255, 0)  # hard and soft alphas
    dev = _flush(torch.from_numpy(src), 0xC3)
    for op in OPS:
        for axis in (0, 1):
            for r in _radii(h, w):
                got = _run(dev, op, r, axis)
                assert np.array_equal(got.numpy(), tmc.ref_pass_u8(src, op, r, axis)), (op, axis, r)


def test_edit_planes_and_edit_obj_masks_are_the_pass_sequence_of_the_rule():
    from mvoc_amd import ops
    from mvoc_amd.pipeline import edit_obj_masks
    cpu, dev = tv._hook_masks(3, 8, 8)
    edit = ((1, 2), (-1, 0))
    got = edit_obj_masks(dev, edit)
    want = tmc.ref_edit_masks(cpu, edit)
    for (gs, gh), (ws, wh), (s, h) in zip(got, want, cpu):
        assert gs.dtype == torch.float16 and gh.dtype == torch.bool and gs.shape == s.shape and gh.shape == h.shape
        assert tmc._same_bits(gs.cpu(), ws) and torch.equal(gh.cpu(), wh)
        assert not torch.equal(ws, s) and not torch.equal(wh, h)
    kept = edit_obj_masks(dev, ((0, 0), (0, 3)))
    assert kept[0][0] is dev[0][0] and kept[0][1] is dev[0][1] and kept[1][1] is dev[1][1]  # feather leaves the hard mask
    assert tmc._same_bits(kept[1][0].cpu(), tmc.ref_edit(cpu[1][0], 0, 3))
    alpha = np.random.default_rng(7).integers(0, 256, (3, 64, 64), dtype=np.uint8)
    for grow, feather in [(1, 2), (-1, 0), (0, 8), (8, 8)]:  # the image site: radii times 8, up to 64
        got = ops.edit_planes(torch.from_numpy(alpha).cuda(), grow, feather, 8)
        assert np.array_equal(got.cpu().numpy(), tmc.ref_edit(alpha, grow, feather, 8)), (grow, feather)
    t = torch.from_numpy(alpha).cuda()
    assert ops.edit_planes(t, 0, 0, 8) is t


def test_mask_filter_checks_its_arguments():
    from mvoc_amd import ops
    f16 = torch.zeros(2, 4, 6, dtype=torch.float16, device="cuda")
    for bad, text in [(dict(src=f16.float()), "src must be torch.float16 or torch.uint8, got torch.float32"),
                      (dict(op="blur"), "op 'blur' is not one of 'max', 'min', 'mean'"),
                      (dict(axis=2), r"axis 2 is not 0 \(along y\) or 1 \(along x\)"),
                      (dict(radius=65), r"radius 65 is not an int in \[0, 64\]"),
                      (dict(radius=-1), r"radius -1 is not an int in \[0, 64\]"),
                      (dict(radius=1.0), r"radius 1.0 is not an int in \[0, 64\]"),
                      (dict(radius=True), r"radius True is not an int in \[0, 64\]"),
                      (dict(src=f16[:, :, ::2]), r"src must be contiguous \[..., h, w\] and not empty"),
                      (dict(src=f16[:0]), r"src must be contiguous \[..., h, w\] and not empty"),
                      (dict(src=f16[0, 0]), r"src must be contiguous \[..., h, w\] and not empty"),
                      (dict(out=f16.to(torch.uint8)), "`out` must be torch.float16"),
                      (dict(out=f16[:1]), "out must be contiguous and of src's shape"),
                      (dict(out=f16), "out overlaps src"),
                      (dict(src=f16.view(-1)[:24].view(1, 4, 6), out=f16.view(-1)[12:36].view(1, 4, 6)), "out overlaps src")]:
        with pytest.raises(RuntimeError, match=text):
            ops.mask_filter(**dict(dict(src=f16, op="max", radius=1, axis=0), **bad))


# ---- the sampling call ------------------------------------------------------------------------------------------------------------
EDIT = [{"grow": 1, "feather": 2}, {"grow": -1}]
NORMAL = ((1, 2), (-1, 0))
LATENT_LAUNCHES = (4 + 2) + (2 + 2)  # per object the soft mask's passes and the hard mask's grow passes
IMAGE_LAUNCHES = 4 + 2


def _main():
    clips, _ = tcg._sources()
    return dict(main_first_image=clips[0][0], main_image_list=clips[0])


def _pre_edited(monkeypatch):
    """from here on the toy job is handed the masks the CPU reference edited -> the numpy-pre-edited alphas that go with them"""
    cpu, _ = tv._hook_masks(tcg.F_, tcg.LAT, tcg.LAT)
    edited = tmc.ref_edit_masks(cpu, NORMAL)
    monkeypatch.setattr(tv, "_hook_masks", lambda F, h, w: (edited, None))
    _, alpha = tcg._sources()
    return [tmc.ref_edit(alpha[j], g, f, 8) for j, (g, f) in enumerate(NORMAL)]


def test_an_edited_call_without_placement_runs_as_if_handed_the_pre_edited_masks(monkeypatch):
    plain = tcg._job(**_main())
    got = tcg._job(obj_mask_edit=EDIT, **_main())
    assert got.mask_edit_info["launches"] == LATENT_LAUNCHES and got.mask_edit_info["seconds"] > 0
    _pre_edited(monkeypatch)
    want = tcg._job(**_main())
    assert torch.equal(got.frames, want.frames) and torch.isfinite(got.frames).all()
    assert not torch.equal(got.frames, plain.frames)  # the edit is seen by the composition
    assert want.mask_edit_info == {"launches": 0, "seconds": 0.0}


def test_an_edited_rotated_bilinear_composed_call_runs_as_if_handed_the_pre_edited_masks_and_alphas(monkeypatch):
    kw = dict(obj_transforms=tcg.ROTATED, obj_transform_filter="bilinear", compose_main_images=True)
    plain = tcg._job(**kw)
    got = tcg._job(obj_mask_edit=EDIT, **kw)
    assert got.mask_edit_info["launches"] == LATENT_LAUNCHES + IMAGE_LAUNCHES
    assert got.collage_info["mask_edit_launches"] == IMAGE_LAUNCHES and "mask_edit_launches" not in plain.collage_info
    alpha = _pre_edited(monkeypatch)
    want = tcg._job(obj_alpha=alpha, **kw)
    assert tcg._same_images(got.main_frames[0], want.main_frames[0]) and not tcg._same_images(got.main_frames[0], plain.main_frames[0])
    assert torch.equal(got.frames, want.frames) and not torch.equal(got.frames, plain.frames)


def test_two_variants_with_their_own_transforms_share_the_edited_masks(monkeypatch):
    kw = dict(K=2, variant_obj_transforms=tcg.VARIANT_TRANSFORMS, **_main())
    got = tcg._job(obj_mask_edit=EDIT, **kw)
    assert got.mask_edit_info["launches"] == LATENT_LAUNCHES
    _pre_edited(monkeypatch)
    want = tcg._job(**kw)
    assert got.frames.shape[0] == 2 and torch.equal(got.frames, want.frames) and not torch.equal(got.frames[0], got.frames[1])


def test_none_and_an_all_zero_edit_are_the_call_without_the_argument():
    plain = tcg._job(**_main())
    for value in (None, [None, None], {"grow": 0, "feather": 0}, [{}, {"feather": 0}]):
        got = tcg._job(obj_mask_edit=value, **_main())
        assert torch.equal(got.frames, plain.frames), value
        assert got.mask_edit_info == {"launches": 0, "seconds": 0.0} and got.collage_info is None
    with pytest.raises(ValueError, match=r"obj_mask_edit: object 1: feather = 9 is not in \[0, 8\] latent pixels"):
        tcg._job(obj_mask_edit=[None, {"feather": 9}], **_main())
