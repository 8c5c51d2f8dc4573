"""CPU-only: the compiler's resource-usage remarks for the kernels of mask_edit.hip (mvoc_amd/build.py keeps them in
mask_edit.o.res.txt; DESIGN.md 6u has the table).  The kernels are HBM- and latency-bound and run a handful of times per call: the
bar is no scratch and no spills (VGPRs or SGPRs) in any of the six instantiations (fp16 / uint8 x max / min / mean), the occupancy
of the cross-compiled build as a floor, and the table of 6u in step with the build."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]")
# (element type, op) of the mangled template arguments -> the row of the table in DESIGN.md 6u
ROWS = {("DF16_", 0): "fp16 max", ("DF16_", 1): "fp16 min", ("DF16_", 2): "fp16 mean",
        ("h", 0): "uint8 max", ("h", 1): "uint8 min", ("h", 2): "uint8 mean"}
OCCUPANCY_FLOOR = 8  # waves per SIMD of every instantiation in the gfx950 build (the most the hardware holds)


def _remarks():
    from mvoc_amd import build
    build.build(verbose=False)
    seen, name = {}, None
    for line in open(os.path.join(REPO, "mvoc_amd", "csrc", "mask_edit.o.res.txt")):
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


def _by_row(seen):
    out = {}
    for name, r in seen.items():
        m = re.search(r"mask_filter_kernelI(DF16_|h)Li(\d)EE", name)
        assert m, name
        out[ROWS[(m.group(1), int(m.group(2)))]] = r
    return out


def test_every_kernel_of_the_unit_is_free_of_scratch_and_spills_at_full_occupancy():
    seen = _remarks()
    assert len(seen) == 6, sorted(seen)
    rows = _by_row(seen)
    assert sorted(rows) == sorted(ROWS.values())
    for row, r in rows.items():
        assert set(r) == set(KEYS), (row, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (row, r)
        assert r["Occupancy [waves/SIMD]"] >= OCCUPANCY_FLOOR, (row, r)


def test_the_table_of_6u_holds_the_numbers_of_the_build():
    rows = _by_row(_remarks())
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    section = design[design.index("## 6u."):design.index("## 7. ")]
    for row, r in rows.items():
        want = (f"| `mask_filter_kernel` {row} | {r['VGPRs']} | {r['TotalSGPRs']} | {r['ScratchSize [bytes/lane]']} | "
                f"{r['VGPRs Spill']} / {r['SGPRs Spill']} | {r['Occupancy [waves/SIMD]']} |")
        assert want in section, want
