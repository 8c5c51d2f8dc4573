"""The kernel forms an in-process test cannot reach, run in a process of their own (helper, not collected by pytest):

    python tests/xs_forced_worker.py <dir>      with MVOC_XS_RG=2 MVOC_TFUSED_WAVES=8 in the environment

Both variables are read once per process by the library.  Under them every section of the xs_linear contract set (tests/xs_contract.py:
A, B, C, D, S at every K, with the same checks) runs on the two-row-group instantiations of xslin.hip -- a single 256-row block holds
every row up to m = 256, m = 257 makes two -- and the tfused cases of the attention contract set run on the 8-wave kernels of tfused.hip
at the same bound, with sections A, B and L of the fused kernel's own set (tests/tfused_contract.py) under their own checks.  The bits
of every output go to <dir>/<case key>.pt (int16; of the two thousand cases of tests/tfused_contract.py, 400 MB of them, the SHA-256
of the bits); tests/test_xs_contract_gpu.py, which starts this process, runs the same cases on the default forms and compares bit for bit.  The functions below are shared with that test."""
import ctypes as C
import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import attn_contract as AC  # noqa: E402
import launch_census as LC  # noqa: E402
import tfused_contract as TC  # noqa: E402
import xs_contract as XC  # noqa: E402
from mvoc_amd._ffi import lib  # noqa: E402

DEV = "cuda"
FORCED_ENV = {"MVOC_XS_RG": "2", "MVOC_TFUSED_WAVES": "8"}
ZERO_QK = (16, 9, 3)  # frames, hw, nsample of the zero-Q/K frame-mean case


def stream():
    return torch.cuda.current_stream().cuda_stream


KERNEL = XC.library_kernel(lib, stream)


def xs_bits(k, sections=XC.SECTIONS, figures=None):
    return XC.run_sections(k, DEV, KERNEL, sections, figures)


def rows_per_block():
    """128 (one row group per wave) or 256 (two), seen from outside: a weight set per 128 rows is refused by the two-row-group form"""
    p = XC._case(0, 64, 256, 32, XC.ACT_NONE, 0, 0, 0, set_rows=128)
    L = XC.XsLayout(DEV, p)
    L.fill(XC.draw("S", p))
    rc = lib.mvoc_xs_linear_f16(C.byref(L.desc()), stream())
    torch.cuda.synchronize()
    assert rc in (0, -2), lib.mvoc_last_error().decode()
    return 128 if rc == 0 else 256


def tfused_bits(check):
    """the tfused cases of tests/test_attention_contract_gpu.py (same builders, same seeds): case key -> output bits.  check: hold
    them to the fp64 reference at AC.TFUSED_BOUND as that file does (the caller of the default forms has that file for it)"""
    import test_attention_contract_gpu as TA
    bits = {}
    for c in AC.TF_C:
        for frames in AC.TF_FRAMES:
            for hw in AC.TF_HW:
                for nsample in AC.TF_NS:
                    d, bufs, Lg = TA.build_tfused(c, frames, hw, nsample, 1000 * c + 10 * frames + hw + nsample)
                    out = TA.run_tfused(d, bufs)
                    if check:
                        ref = LC.tfused_ref(d, bufs, Lg).reshape(nsample, -1)
                        AC.assert_close_slices(out, ref, (0,), AC.TFUSED_BOUND, f"tfused c {c} frames {frames} hw {hw} nsample {nsample}")
                    bits[f"tfused_c{c}_f{frames}_hw{hw}_ns{nsample}"] = out.cpu().view(torch.int16).clone()
        frames, hw, nsample = ZERO_QK
        d, bufs, Lg = TA.build_tfused(c, frames, hw, nsample, c, zero_qk=True)
        out = TA.run_tfused(d, bufs)
        if check:
            x = bufs["x"].reshape(-1, c)
            v = LC.r16(LC.r16(LC.layernorm64(x, Lg["gamma"], Lg["beta"], d.ln_eps)) @ Lg["w"][2 * c:].to(torch.float64).t())
            ref = v.reshape(nsample, frames, hw, c).mean(1, keepdim=True).expand(nsample, frames, hw, c).reshape(nsample, -1)
            AC.assert_close_slices(out, ref, (0,), AC.TFUSED_BOUND, f"tfused zero q/k c {c}")
        bits[f"tfused_zero_qk_c{c}"] = out.cpu().view(torch.int16).clone()
    # sections A, B and L of the fused kernel's own contract set (tests/tfused_contract.py): the same builders and keys; section D in
    # every case, the case's own check when asked (the exact sections are bit-equal between the forms by construction)
    import test_tfused_contract_gpu as TG
    for section in TC.EXACT_SECTIONS:
        for case in TC.section_cases(section):
            assert case["key"] not in bits, case["key"]
            bits[case["key"]] = bits_digest(TG.run_case(case, check))
    return bits


def bits_digest(out):
    """SHA-256 of an output's bits as 16 int16: equal digests, equal bits"""
    raw = out.contiguous().cpu().view(torch.int16).numpy().tobytes()
    return torch.frombuffer(bytearray(hashlib.sha256(raw).digest()), dtype=torch.int16).clone()


def main(out_dir):
    for name, value in FORCED_ENV.items():
        assert os.environ.get(name) == value, f"{name} must be {value} in this process's environment"
    assert rows_per_block() == 256, "MVOC_XS_RG=2 did not select the two-row-group form"
    bits = {}
    for k in XC.K:
        bits.update(xs_bits(k))
    bits.update(tfused_bits(check=True))
    torch.cuda.synchronize()
    for key, val in bits.items():
        torch.save(val, os.path.join(out_dir, key + ".pt"))
    print(f"{len(bits)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
