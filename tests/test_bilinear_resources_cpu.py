"""CPU-only: the compiler's resource-usage remarks for every kernel of pnp_bilinear.hip (mvoc_amd/build.py keeps them in
pnp_bilinear.o.res.txt; DESIGN.md 6r has the table beside the ``_warped`` twins).  The TAPS kernels are the blend-scatter pieces
with four loads per object: none of them may use scratch or spill (VGPRs or SGPRs), each instantiation exists exactly once, and
none may fall below the occupancy the build reported when the table was written."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# waves / SIMD for 1 / 2 / 3 / 4 objects of nchw<8, NOBJ> (the _warped twins: 8, 6, 5, 4); every tokens kernel (the Q/K sites), every
# nchw<1, .> kernel and the plane kernel run at 8
FLOOR_NCHW8 = (8, 4, 4, 3)
KEYS = ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]")


def _remarks():
    from mvoc_amd import build
    build.build(verbose=False)
    seen, name = {}, None
    for line in open(os.path.join(REPO, "mvoc_amd", "csrc", "pnp_bilinear.o.res.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            assert name not in seen, name
            seen[name] = {}
        for key in KEYS:
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m and name:
                seen[name][key] = int(m.group(1))
    return seen


def test_every_bilinear_kernel_is_free_of_scratch_and_spills_and_holds_its_occupancy():
    seen = _remarks()
    met = []
    for name, r in sorted(seen.items()):
        assert set(r) == set(KEYS), (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        m = re.search(r"\d+pnp_nchw_bilinear_kernelILi(8|1)ELi([1-4])E", name)
        t = re.search(r"\d+pnp_tokens_bilinear_kernelILi([1-4])E", name)
        if m and m.group(1) == "8":
            floor, inst = FLOOR_NCHW8[int(m.group(2)) - 1], ("nchw8", int(m.group(2)))
        elif m:
            floor, inst = 8, ("nchw1", int(m.group(2)))
        elif t:
            floor, inst = 8, ("tokens", int(t.group(1)))
        else:
            assert "gather_planes_bilinear_kernel" in name, name
            floor, inst = 8, ("planes", 0)
        met.append(inst)
        assert r["Occupancy [waves/SIMD]"] >= floor, (name, r, floor)
    want = [(k, n) for k in ("nchw1", "nchw8", "tokens") for n in (1, 2, 3, 4)] + [("planes", 0)]
    assert sorted(met) == sorted(want), met  # 13 kernels, each instantiation met exactly once


def test_the_older_units_do_not_see_the_taps_case():
    """the TAPS pieces of pnp_blend.h are reached through ``if constexpr (S == TAPS)`` alone: no kernel of the three older units
    holds a bilinear kernel, and pnp_warp.o keeps its 13"""
    from mvoc_amd import build
    build.build(verbose=False)
    counts = {}
    for unit in ("pnp", "pnp_variants2", "pnp_warp"):
        text = open(os.path.join(REPO, "mvoc_amd", "csrc", unit + ".o.res.txt")).read()
        names = re.findall(r"Function Name: (\S+)", text)
        assert len(names) == len(set(names)) and not any("bilinear" in n for n in names), unit
        counts[unit] = len(names)
    assert counts["pnp_warp"] == 13, counts
