"""CPU-only: the compiler's resource-usage remarks for every kernel of pnp_warp.hip (mvoc_amd/build.py keeps them in
pnp_warp.o.res.txt; DESIGN.md 6q has the table).  The MAP2 kernels are the blend-scatter pieces with one more object load: none
of them may use scratch or spill, and none may fall below the occupancy of its ``_resampled`` twin in pnp.o (the floors of
tests/test_blend_resources_cpu.py)."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# waves / SIMD for 1 / 2 / 3 / 4 objects of nchw<8, NOBJ>; every tokens kernel, every nchw<1, .> kernel and the plane kernel run at 8
FLOOR_NCHW8 = (8, 6, 5, 4)
KEYS = ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]")


def _remarks():
    from mvoc_amd import build
    build.build(verbose=False)
    seen, name = {}, None
    for line in open(os.path.join(REPO, "mvoc_amd", "csrc", "pnp_warp.o.res.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key in KEYS:
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m and name:
                seen[name][key] = int(m.group(1))
    return seen


def test_every_warp_kernel_meets_the_bar_of_its_resampled_twin():
    seen = _remarks()
    kinds = {"tokens": 0, "nchw1": 0, "nchw8": 0, "planes": 0}
    for name, r in sorted(seen.items()):
        assert set(r) == set(KEYS), (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        m = re.search(r"\d+pnp_nchw_warped_kernelILi(8|1)ELi([1-4])E", name)
        if m and m.group(1) == "8":
            floor, kind = FLOOR_NCHW8[int(m.group(2)) - 1], "nchw8"
        elif m:
            floor, kind = 8, "nchw1"
        elif re.search(r"\d+pnp_tokens_warped_kernelILi[1-4]E", name):
            floor, kind = 8, "tokens"
        else:
            assert "gather_planes_warped_kernel" in name, name
            floor, kind = 8, "planes"
        kinds[kind] += 1
        assert r["Occupancy [waves/SIMD]"] >= floor, (name, r, floor)
    assert kinds == {"tokens": 4, "nchw1": 4, "nchw8": 4, "planes": 1}, kinds  # 13 kernels, each instantiation met once
