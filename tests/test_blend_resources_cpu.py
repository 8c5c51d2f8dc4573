"""CPU-only: the compiler's resource-usage remarks for every kernel of pnp.hip (mvoc_amd/build.py keeps them in pnp.o.res.txt).
The blend-scatter family is composed from shared pieces, so one edit moves the registers of forty instantiations at once: none of
them may use scratch or spill, and none may fall below the occupancy it had when the family was ten hand-written kernels."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# waves / SIMD for 1 / 2 / 3 / 4 objects of the nchw<8, NOBJ> instantiations that do not reach 8; every other kernel of the file
# (every tokens kernel, every nchw<1, .> kernel, the two run-time-loop kernels, shift / gather_planes, ddim_step*, fusion*) runs at 8
FLOOR_NCHW8 = {
    "pnp_nchw_variants_kernel": (8, 8, 8, 6),
    "pnp_nchw_variants_sel_kernel": (8, 8, 8, 6),
    "pnp_nchw_placed_kernel": (8, 6, 5, 4),
    "pnp_nchw_resampled_kernel": (8, 6, 5, 4),
    "pnp_nchw_placed_variants_kernel": (8, 4, 3, 3),
}
KEYS = ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]")


def _remarks():
    from mvoc_amd import build
    build.build(verbose=False)
    seen, name = {}, None
    for line in open(os.path.join(REPO, "mvoc_amd", "csrc", "pnp.o.res.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key in KEYS:
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m and name:
                seen[name][key] = int(m.group(1))
    return seen


def _floor(mangled):
    m = re.search(r"\d+(pnp_nchw_\w+_kernel)ILi8ELi([1-4])E", mangled)
    return (FLOOR_NCHW8[m.group(1)][int(m.group(2)) - 1], True) if m else (8, False)


def test_every_pnp_kernel_keeps_its_occupancy_without_scratch():
    seen = _remarks()
    assert len(seen) == 72, sorted(seen)
    tabled = 0
    for name, r in sorted(seen.items()):
        assert set(r) == set(KEYS), (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        floor, in_table = _floor(name)
        tabled += in_table
        assert r["Occupancy [waves/SIMD]"] >= floor, (name, r, floor)
    assert tabled == 4 * len(FLOOR_NCHW8)  # every row of the table met its four instantiations
