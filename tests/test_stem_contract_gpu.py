"""What include/mvoc_hip.h promises about the nineteen one-thread-per-output entries of mvoc_amd/csrc/stem.hip and norm.hip's
mvoc_softmax_rows_f16 ("Extents (enforced by tests/test_stem_contract_gpu.py)"), through the C ABI (mvoc_amd._ffi), one launch per case.
The walk, the poisoned layouts and the references are tests/stem_contract.py; tests/test_stem_contract_cpu.py shows them sound.

  W  the walk (test_walk[entry]): per entry the geometries whose work-item total is 1, 255, 256, 257 and 513 in several factorisations
     (timestep_embedding: 2, 254, 256, 258, 512, 514, its count is even; clip_patches from 3), every (ldo, coff) and ld the issue
     lists, and the per-entry lists: conv3x3_small over 5 image sizes x 2 strides x 3 cin x 3 cout x bias x SiLU on integers,
     adaptive_avgpool over equal / divisible / ragged / upsampling / 1x1 windows, softmax_rows over 5 x 5 (rows, cols) with constant,
     dominant and -65504 rows, timestep_embedding over dim 2 / 6 / 320 and eight t, the elementwise entries over EVERY fp16 pattern
     (act both forms, scale three factors), 16 x 16 special pairs and rounding ties (add), 16 x 25 x 16 special triples with logvar at
     and past both clamps (gaussian_sample), every byte (mask_finish), clip_patches with pad columns, clip_embed in both forms,
     permute_rows in all 24 orders, mask_resize_u8 against PIL with all-0, all-255 and checkerboard frames
  in EVERY case: the entry returns 0; every operand sits in an allocation of its own, 0, 16 or 128 bytes past a 256-byte boundary;
     every element the header says is not read holds fp16 NaN (INT32_MIN, the census byte); the described output elements are held
     to the reference, every other byte of every output allocation (the sibling channels of a pitched row, the lead, 64 KB behind)
     still holds the sentinel, no described element is left unwritten, and every input allocation keeps its bytes
  T  temporal_encoder4: relayout invariance bit for bit at the totals (a (b, f, hw) launch against the (b * hw, f, 1) launch on the
     same data), and accuracy against oracle.unet_ref.I2VGenXLTransformerTemporalEncoder(4, 2, 4, 16) in fp64 at f = 1, 2, 5, 16, 32, a
     dominant-score case and a constant-row case; the bound is TWICE the rel-L2 and max-abs of the same module run in fp16 on the CPU
  E  refusals (test_refusals[entry]): every precondition the header states, one at a time: -1, mvoc_last_error() names the entry, not
     one byte of any output allocation changed; then the same buffers with the described arguments run and verify.  Host-side
     refusals only: nothing is launched that could leave its allocation (an out-of-range id is not tested).

Bounds that are not bit for bit: timestep_embedding (derived: stem_contract.timestep_embedding64), act (ulp16 of fp64 + 2^-22 |x| for
the erff GELU), conv3x3_small with SiLU (ulp16 of fp64), softmax_rows and gaussian_sample (the census's accepted neighbours),
temporal_encoder4 (measured).  Everything else is bit for bit.

Measured on an MI355X (worst deviation / bound per entry; 0 = bit for bit or inside the accepted neighbours throughout):
  timestep_embedding 0.9987 (nb=1 dim=254, against the derived bound; 0.9992 against the issue's `+ 3` form, which the device also keeps);
  act 0.9942 (the GELU atlas: a rounding flip is a whole fp16 ulp by construction); conv3x3_small with SiLU, add, adaptive_avgpool,
  ncfhw_to_tokens, tokens_to_ncfhw, conv1x1_small, softmax_rows, gaussian_sample, scale, image_to_tokens, tokens_to_image, mask_resize_u8,
  mask_finish, clip_patches, clip_embed, permute_rows: 0.
  temporal_encoder4, yardstick (eager fp16 on the CPU against fp64) -> kernel, rel-L2 / max-abs; the bound is twice the yardstick:
    f = 1   3.575e-4 / 1.952e-3 -> 3.575e-4 / 1.952e-3        f = 2   3.333e-4 / 2.482e-3 -> 3.333e-4 / 2.482e-3
    f = 5   3.393e-4 / 2.908e-3 -> 3.404e-4 / 2.908e-3        f = 16  3.415e-4 / 3.158e-3 -> 3.430e-4 / 3.158e-3
    f = 32  3.416e-4 / 4.170e-3 -> 3.411e-4 / 4.170e-3        dominant 3.364e-4 / 2.030e-3 -> 3.364e-4 / 2.030e-3
    constant rows 3.278e-4 / 3.432e-3 -> 3.215e-4 / 3.432e-3
  (the kernel rounds where the eager chain rounds, so it sits at the yardstick, a factor 2 inside the bound; 2 x 3.6e-4 is far under the
  3e-3 of test_ops_gpu.py::test_temporal_encoder4_and_layout).
  The whole file: 41 tests, about 900 launches, 3.1 s; the slowest tests are test_walk[timestep_embedding] (the process's first
  launch) at 0.24 s and test_walk[conv3x3_small] (378 launches) at 0.21 s.

A defect the file found: mvoc_gaussian_sample_f16 clamped logvar with fmaxf / fminf, which drop a NaN, so a NaN logvar gave a finite
sample where the reference's torch.clamp gives NaN (gaussian_sample[atlas]: 223 of 6400 elements, the first at mean +0, logvar NaN:
got 0.0, want NaN).  The kernel now keeps the NaN.  The alignment checks of clip_embed and permute_rows and the coff >= 0 checks of
ncfhw_to_tokens and temporal_encoder4 are new with this file; nothing here launches what they refuse.
"""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_contract as S  # noqa: E402
from mvoc_amd._ffi import lib  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return lib.mvoc_last_error().decode()


def _fn(entry):
    return getattr(lib, S.SYMBOL[entry])


def _run(case, i):
    pl = S.Placed(S.problem(case), i, DEV)
    rc = _fn(case.entry)(*pl.c_args(), _stream())
    assert rc == 0, (repr(case), rc, _err())
    torch.cuda.synchronize()
    return pl.verify(repr(case))


@pytest.mark.parametrize("entry", [e for e in S.ENTRIES if e != "temporal_encoder4"])
def test_walk(entry):
    t0, worst, at = time.time(), 0.0, None
    cs = S.cases(entry)
    for i, c in enumerate(cs):
        r = _run(c, i)
        if r > worst:
            worst, at = r, repr(c)
    print(f"\n[stem contract] {entry}: {len(cs)} launches, worst deviation / bound {worst:.4f} ({at}), {time.time() - t0:.2f} s")


def test_timestep_embedding_against_the_issue_form_of_the_bound():
    """prints (does not assert) how far the device sits from the `+ 3` form, which leaves nothing for sinf / cosf; the assertion is
    test_walk[timestep_embedding] with the device term added"""
    worst = 0.0
    for i, c in enumerate(S.cases("timestep_embedding")):
        prob = S.problem(c)
        pl = S.Placed(prob, i, DEV)
        assert _fn("timestep_embedding")(*pl.c_args(), _stream()) == 0, _err()
        torch.cuda.synchronize()
        ref, _, bound3 = S.timestep_embedding64(prob.ins["t"], c.p["dim"])
        worst = max(worst, float(((pl.T["out"].cpu().to(torch.float64).reshape(ref.shape) - ref).abs() / bound3).max()))
    print(f"\n[stem contract] timestep_embedding against the `+ 3` form: worst deviation / bound {worst:.4f}")


def test_temporal_encoder4_accuracy():
    for i, c in enumerate(S.cases("temporal_encoder4")):
        prob = S.problem(c)
        pl = S.Placed(prob, i, DEV)
        assert _fn("temporal_encoder4")(*pl.c_args(), _stream()) == 0, (repr(c), _err())
        torch.cuda.synchronize()
        o = prob.outs["out"]
        got = pl.T["out"].cpu()[o.dest].to(torch.float64)
        rel, mx = float((got - o.ref).norm() / o.ref.norm()), float((got - o.ref).abs().max())
        print(f"\n[stem contract] {c!r}: yardstick rel-L2 {o.rule[1] / 2:.3e} max-abs {o.rule[2] / 2:.3e}; kernel rel-L2 {rel:.3e} max-abs {mx:.3e}")
        assert o.rule[1] <= 3e-3
        assert pl.verify(repr(c)) <= 1.0


def test_temporal_encoder4_relayout_invariance():
    for i, (b, f, hw, pitch) in enumerate(S.enc_relayout_cases()):
        pa, pb, index, dest = S.enc_relayout_pair(b, f, hw, pitch)
        A, B = S.Placed(pa, i, DEV), S.Placed(pb, i + 1, DEV)
        for pl in (A, B):
            assert _fn("temporal_encoder4")(*pl.c_args(), _stream()) == 0, _err()
        torch.cuda.synchronize()
        S.relayout_equal(A, B, index, dest, f"b={b} f={f} hw={hw} (ldo, coff)={pitch}")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _set(i, v):
    return lambda a: a.__setitem__(i, v)


def _off(i, n):
    return lambda a: a.__setitem__(i, a[i] + n)


def _nulls(*idx):
    return [(f"null argument {i}", _set(i, None)) for i in idx]


def _zeros(*idx):
    return [(f"argument {i} = 0", _set(i, 0)) for i in idx] + [(f"argument {idx[0]} = -1", _set(idx[0], -1))]


def _misaligned(*idx):
    return [(f"argument {i} + {n} bytes", _off(i, n)) for i in idx for n in (2, 8)]


def _dims_with(k, v):
    def change(a):
        d = list(a[2])
        d[k] = v
        a[2] = type(a[2])(*d)
    return change


# entry -> (the text mvoc_last_error must carry, a case, the refused changes of its argument list (stream excluded))
REFUSALS = {
    "timestep_embedding": ("timestep_embedding", S.Case("timestep_embedding", "entry", nb=5, dim=6, t0=0),
                           _nulls(0, 3) + _zeros(1, 2) + [("dim odd", _set(2, 5)), ("dim -2", _set(2, -2))]),
    "act": ("act", S.Case("act", "totals", n=257, act=S.ACT_GELU), _nulls(0, 1) + _zeros(2)),
    "add": ("add", S.Case("add", "totals", n=257), _nulls(0, 1, 2) + _zeros(3)),
    "conv3x3_small": ("conv3x3_small", S.Case("conv3x3_small", "entry", nimg=2, h=5, w=4, cin=3, cout=5, stride=2, bias=True, silu=True),
                      _nulls(0, 1, 3) + _zeros(4, 5, 6, 7, 8) + [("stride 0", _set(9, 0)), ("stride 3", _set(9, 3)), ("stride -1", _set(9, -1))]),
    "adaptive_avgpool": ("avgpool", S.Case("adaptive_avgpool", "entry", nimg=2, h=7, w=9, c=3, oh=4, ow=5), _nulls(0, 1) + _zeros(2, 3, 4, 5, 6, 7)),
    "ncfhw_to_tokens": ("ncfhw_to_tokens", S.Case("ncfhw_to_tokens", "pitch", b=2, c=3, f=5, hw=7, ldo=11, coff=5),
                        _nulls(0, 1) + _zeros(2, 3, 4, 5) + [("ldo < coff + c", _set(6, 7)), ("ldo 0", _set(6, 0)), ("coff < 0", _set(7, -1))]),
    "tokens_to_ncfhw": ("tokens_to_ncfhw", S.Case("tokens_to_ncfhw", "pitch", b=2, c=4, f=5, hw=7, ld=7),
                        _nulls(0, 1) + _zeros(2, 3, 4, 5) + [("ld < c", _set(6, 3)), ("ld 0", _set(6, 0))]),
    "temporal_encoder4": ("temporal_encoder4", S.Case("temporal_encoder4", "accuracy", b=2, f=5, hw=33, ldo=9, coff=3),
                          _nulls(0, 1, 2) + _zeros(3, 4, 5) + [("ldo < coff + 4", _set(6, 6)), ("coff < 0", _set(7, -1))]),
    "conv1x1_small": ("conv1x1_small", S.Case("conv1x1_small", "entry", rows=9, cin=8, cout=8, bias=True),
                      _nulls(0, 1, 3) + _zeros(4, 5, 6) + [("cin 65", _set(5, 65)), ("cout 65", _set(6, 65))]),
    "softmax_rows": ("softmax_rows", S.Case("softmax_rows", "entry", rows=5, cols=520, shift=0),
                     _nulls(0) + _zeros(1, 2) + [("cols % 8", _set(2, 516))] + _misaligned(0)),
    "gaussian_sample": ("gaussian_sample", S.Case("gaussian_sample", "totals", n=257), _nulls(0, 1, 2, 3) + _zeros(4)),
    "scale": ("scale", S.Case("scale", "totals", n=257, scale=S.SCALES[0]), _nulls(0, 1) + _zeros(2)),
    "image_to_tokens": ("image_to_tokens", S.Case("image_to_tokens", "totals", n=3, c=5, hw=17), _nulls(0, 1) + _zeros(2, 3, 4)),
    "tokens_to_image": ("tokens_to_image", S.Case("tokens_to_image", "totals", n=3, c=5, hw=17, ld=8),
                        _nulls(0, 1) + _zeros(2, 3, 4) + [("ld < c", _set(5, 4))]),
    "mask_resize_u8": ("mask_resize", S.Case("mask_resize_u8", "entry", n=5, H=16, W=24, h=2, w=3),
                       _nulls(0, 1, 2, 8, 9, 11, 12) + _zeros(3, 4, 5, 6, 7)),
    "mask_finish": ("mask_finish", S.Case("mask_finish", "totals", n=257), _nulls(0, 1, 2) + _zeros(3)),
    "clip_patches": ("clip_patches", S.Case("clip_patches", "entry", nimg=2, size=6, patch=3, kpad=32),
                     _nulls(0, 1) + _zeros(2, 3, 4) + [("size % patch", _set(3, 7)), ("kpad < 3 patch^2", _set(5, 26)), ("kpad 0", _set(5, 0))]),
    "clip_embed": ("clip_embed", S.Case("clip_embed", "entry", form="vision", nb=3, t=5, c=24),
                   _nulls(0, 3, 4) + _zeros(5, 6, 7) + [("neither ids nor cls", _set(2, None)), ("rows % t", _set(6, 4)), ("c % 8", _set(7, 20))]
                   + _misaligned(0, 2, 3, 4)),
    "clip_embed text": ("clip_embed", S.Case("clip_embed", "entry", form="text", nb=3, t=5, c=24),
                        _nulls(0, 3, 4) + [("neither ids nor cls", _set(1, None)), ("rows % t", _set(6, 4))] + _misaligned(0, 3, 4)),
    "permute_rows": ("permute_rows", S.Case("permute_rows", "orders", shape4=(2, 3, 4, 5), perm=(3, 1, 0, 2), c=24),
                     _nulls(0, 1, 2, 3) + _zeros(4) + [("c % 8", _set(4, 20)), ("a dimension 0", _dims_with(1, 0)), ("a dimension -1", _dims_with(3, -1)),
                                                       ("a dimension 2^30", _dims_with(0, 1 << 30))] + _misaligned(0, 1)),
}


def _other_refusal(text):
    """a refused call of ANOTHER entry, so that mvoc_last_error() is seen to change"""
    if text == "add":
        assert lib.mvoc_act_f16(None, None, 1, S.ACT_SILU, _stream()) == -1
    else:
        assert lib.mvoc_add_f16(None, None, None, 1, _stream()) == -1
    assert text + ":" not in _err()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    text, case, changes = REFUSALS[name]
    prob = S.problem(case)
    for i, (what, change) in enumerate(changes):
        pl = S.Placed(prob, i, DEV)
        before = pl.out_bytes()
        args = pl.c_args()
        change(args)
        _other_refusal(text)
        rc = _fn(case.entry)(*args, _stream())
        assert rc == -1, (name, what, rc, _err())
        assert text + ":" in _err(), (name, what, _err())
        torch.cuda.synchronize()
        after = pl.out_bytes()
        assert all(torch.equal(before[k], after[k]) for k in before), f"{name}: {what}: a refused call wrote to an output allocation"
        # the very buffers of the refused call, the arguments as the case describes them
        assert _fn(case.entry)(*pl.c_args(), _stream()) == 0, (name, what, _err())
        torch.cuda.synchronize()
        pl.verify(f"{name} after `{what}`")
