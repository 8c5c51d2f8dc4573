"""CPU-only: the compiler's resource-usage remarks for the kernel of collage.hip (mvoc_amd/build.py keeps them in
collage.o.res.txt; DESIGN.md 6t has the table).  The kernel is HBM- and latency-bound and runs once per call: the bar is no scratch
and no spills (VGPRs or SGPRs), and one kernel in the unit."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]")


def _remarks(unit):
    from mvoc_amd import build
    build.build(verbose=False)
    seen, name = {}, None
    for line in open(os.path.join(REPO, "mvoc_amd", "csrc", unit + ".o.res.txt")):
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


def test_the_collage_kernel_is_free_of_scratch_and_spills():
    seen = _remarks("collage")
    assert len(seen) == 1, sorted(seen)
    (name, r), = seen.items()
    assert "collage_rgb_u8_kernel" in name and set(r) == set(KEYS), (name, r)
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    assert r["Occupancy [waves/SIMD]"] >= 1, (name, r)
