"""The register budget of the chemistry kernels, read from the compiler (no GPU needed).

The fused row kernel k_chem_step carries a super-droplet's 7 amounts, pH, volume, its cell's 17
constants and the state of the TOMS748 solve in registers; include/sdm_chemistry.h promises that
nothing of it lives in scratch memory.  One device-only compile of chemistry.hip with the flags of
csrc/build.sh and -Rpass-analysis=kernel-resource-usage, parsed the way
tests/test_kernel_resources.py does.
"""
import os
import re
import subprocess

from tests.test_kernel_resources import CSRC, _build_flags


def test_chemistry_kernels_are_without_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run(
        [hipcc, *_build_flags(), "--offload-device-only", "-c", "-o", os.devnull,
         "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "chemistry.hip")],
        capture_output=True, text=True, check=False)
    assert run.returncode == 0, run.stderr[-2000:]
    rows, cur = {}, None
    for line in run.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, value = m.group(1).partition(":")
        key, value = key.strip(), value.strip()
        if key == "Function Name":
            cur = rows.setdefault(value, {})
        elif cur is not None and re.fullmatch(r"\d+", value):
            cur[key] = int(value)
    kernels = {name: row for name, row in rows.items() if "k_chem_" in name}
    names = " ".join(kernels)
    for wanted in ("k_chem_step", "k_chem_equilibrate", "k_chem_dissolve", "k_chem_oxidize",
                   "k_chem_drops", "k_chem_cells", "k_chem_sum"):
        assert wanted in names, wanted
    for name, row in sorted(kernels.items()):
        print(name, {k: row[k] for k in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]",
                                         "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
                     if k in row})
        assert row["ScratchSize [bytes/lane]"] == 0, name
