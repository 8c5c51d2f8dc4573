"""CPU checks of the folded transformer tail (mvoc_amd.unet.fold_proj_out) and of the code objects around the two-source plain
GEMM form (gemm.hip, PLAIN = 2) that carries it."""
import hashlib
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_util as I  # noqa: E402

CSRC = os.path.join(REPO, "mvoc_amd", "csrc")


@pytest.mark.parametrize("c", [64, 320])
def test_fold_proj_out_matches_the_chain_in_fp32(c):
    """[Wp W2 | Wp] [f | h] + (Wp b2 + bp) == proj_out(ff2(f) + h), both in fp32 on the same fp16 weights"""
    from mvoc_amd.unet import fold_proj_out
    g = torch.Generator().manual_seed(c)
    w2 = (torch.randn(c, 4 * c, generator=g) / 8).half()
    b2 = torch.randn(c, generator=g).half()
    wp = (torch.randn(c, c, generator=g) / 8).half()
    bp = torch.randn(c, generator=g).half()
    f = torch.randn(33, 4 * c, generator=g)
    h = torch.randn(33, c, generator=g)
    ref = F.linear(F.linear(f, w2.float(), b2.float()) + h, wp.float(), bp.float())
    w, b = fold_proj_out(w2, b2, wp, bp)
    assert w.dtype == torch.float16 and w.shape == (c, 5 * c) and b.shape == (c,)
    assert torch.equal(w[:, 4 * c:], wp)  # the h columns are proj_out's own weights
    out = F.linear(torch.cat([f, h], 1), w.float(), b.float())
    # the only difference is the single fp16 rounding of Wp W2 and Wp b2 + bp
    assert float((out - ref).norm() / ref.norm()) < 2e-3
    w32 = torch.cat([wp.float() @ w2.float(), wp.float()], 1)
    out32 = F.linear(torch.cat([f, h], 1), w32, wp.float() @ b2.float() + bp.float())
    assert torch.allclose(out32, ref, rtol=1e-4, atol=1e-4)


# Per kernel: digest of the instruction stream of every GEMM instantiation that existed before the two-source plain form was
# added (PC-relative address literals masked: they move with the code object's layout).  Adding PLAIN = 2 must leave them
# instruction for instruction as they were (code placement matters to these kernels: DESIGN section 7).
_PCREL = re.compile(r"0x[0-9a-f]+")
BEFORE = {
    "gemm": {
        "_ZN12_GLOBAL__N_111gemm_kernelILi1ELi4ELi2ELi1EEEv8GemmArgs": "2ba396477086787d",
        "_ZN12_GLOBAL__N_111gemm_kernelILi1ELi4ELi5ELi1EEEv8GemmArgs": "12540f126e59b10b",
        "_ZN12_GLOBAL__N_111gemm_kernelILi2ELi2ELi1ELi2EEEv8GemmArgs": "4242d6525415fd8b",
        "_ZN12_GLOBAL__N_111gemm_kernelILi2ELi2ELi2ELi2EEEv8GemmArgs": "4d8130b4774c3686",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi2ELi1ELi2ELi0ELi64ELi0ELi0EEEv8GemmArgs": "ba904f84dba95f62",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi2ELi1ELi2ELi0ELi64ELi0ELi1EEEv8GemmArgs": "2638cfda51928def",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi2ELi1ELi2ELi0ELi64ELi1ELi0EEEv8GemmArgs": "0b8bcc2e9c90fc95",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi2ELi1ELi2ELi0ELi64ELi1ELi1EEEv8GemmArgs": "5cab4430ba4488b3",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi1ELi2ELi0ELi32ELi0ELi0EEEv8GemmArgs": "c5642c1d97540f83",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi1ELi2ELi0ELi32ELi0ELi1EEEv8GemmArgs": "5d5722f573f2b845",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi1ELi2ELi0ELi32ELi1ELi0EEEv8GemmArgs": "7ce39ace7192e393",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi1ELi2ELi0ELi32ELi1ELi1EEEv8GemmArgs": "2e240a64031dd550",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi1ELi2ELi0ELi64ELi0ELi0EEEv8GemmArgs": "1b8e5921b786567c",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi1ELi2ELi0ELi64ELi0ELi1EEEv8GemmArgs": "41b75db60586ac07",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi1ELi2ELi0ELi64ELi1ELi0EEEv8GemmArgs": "2f13563a43ac1cf8",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi1ELi2ELi0ELi64ELi1ELi1EEEv8GemmArgs": "98c4a23992af6405",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi1ELi4ELi5ELi2ELi2ELi0ELi32ELi0ELi0EEEv8GemmArgs": "ca4ee6fd1567f2bf",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi2ELi2ELi2ELi2ELi2ELi0ELi32ELi0ELi0EEEv8GemmArgs": "072f7b3600b4ab4f",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi2ELi2ELi2ELi2ELi2ELi0ELi32ELi0ELi1EEEv8GemmArgs": "ae4de71bb30f7c7e",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi2ELi2ELi2ELi2ELi2ELi0ELi32ELi1ELi0EEEv8GemmArgs": "603b156738812bc2",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi2ELi2ELi2ELi2ELi2ELi0ELi32ELi1ELi1EEEv8GemmArgs": "e5cc5838f8e35ff5",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi2ELi2ELi2ELi2ELi2ELi0ELi64ELi0ELi0EEEv8GemmArgs": "ae6014c64ee9fb16",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi2ELi2ELi2ELi2ELi2ELi0ELi64ELi0ELi1EEEv8GemmArgs": "5ec67f5319593be9",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi2ELi2ELi2ELi2ELi2ELi0ELi64ELi1ELi0EEEv8GemmArgs": "ec3d0615cb1f5986",
        "_ZN12_GLOBAL__N_116gemm_glds_kernelILi2ELi2ELi2ELi2ELi2ELi0ELi64ELi1ELi1EEEv8GemmArgs": "1e304b11b5ab4ccc",
        "_ZN12_GLOBAL__N_120splitk_reduce_kernelE8GemmArgs": "551249ba77dcab8f",
        "_ZN12_GLOBAL__N_125splitk_reduce_sums_kernelE8GemmArgs": "90d49147e43e2b9f",
    },
    "gemm8": {
        "_ZN12_GLOBAL__N_112gemm8_kernelILi4ELb1ELb1ELb0ELb0ELi0ELb0EEEv8GemmArgs": "c526e127e400ec4d",
        "_ZN12_GLOBAL__N_112gemm8_kernelILi4ELb1ELb1ELb0ELb0ELi1ELb0EEEv8GemmArgs": "bf0b99d4a008824a",
        "_ZN12_GLOBAL__N_112gemm8_kernelILi4ELb1ELb1ELb0ELb0ELi2ELb0EEEv8GemmArgs": "ffd696b0f05cbcc0",
        "_ZN12_GLOBAL__N_112gemm8_kernelILi4ELb1ELb1ELb0ELb0ELi3ELb0EEEv8GemmArgs": "8683b033b7887909",
        "_ZN12_GLOBAL__N_112gemm8_kernelILi4ELb1ELb1ELb1ELb0ELi1ELb0EEEv8GemmArgs": "e51b81f9d4ad89b2",
        "_ZN12_GLOBAL__N_112gemm8_kernelILi5ELb0ELb0ELb0ELb1ELi1ELb0EEEv8GemmArgs": "708b9bcb64f4bc4c",
        "_ZN12_GLOBAL__N_112gemm8_kernelILi5ELb0ELb0ELb0ELb1ELi1ELb1EEEv8GemmArgs": "cdfd2309bdc321df",
        "_ZN12_GLOBAL__N_112gemm8_kernelILi5ELb0ELb0ELb0ELb1ELi2ELb0EEEv8GemmArgs": "5a020127d8330268",
        "_ZN12_GLOBAL__N_112gemm8_kernelILi5ELb0ELb0ELb0ELb1ELi3ELb0EEEv8GemmArgs": "2a7f477b7c62b6fd",
    },
}


def _digests(obj):
    out = {}
    for k, ins in I.disassemble(obj).items():
        h = hashlib.sha256()
        for i in ins:
            args = _PCREL.sub("#", i.args) if i.op in ("s_add_u32", "s_addc_u32", "s_getpc_b64") else i.args
            h.update(f"{i.op} {args}\n".encode())
        out[k] = h.hexdigest()[:16]
    return out


@pytest.mark.parametrize("src", ["gemm", "gemm8"])
def test_existing_gemm_instantiations_unchanged(src):
    obj = os.path.join(CSRC, src + ".o")
    if not os.path.exists(obj):
        from mvoc_amd import build
        build.build(verbose=False)
    now = _digests(obj)
    changed = [k for k, v in BEFORE[src].items() if now.get(k) != v]
    assert not changed, f"{len(changed)} kernels of {src}.o changed: {changed[:4]}"
