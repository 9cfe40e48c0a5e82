"""The register budget of the parcel's chemistry kernel, read from the compiler (no GPU needed).

k_parcel_chem carries a super-droplet's 7 amounts, pH, volume, its six staged differences and the
state of the TOMS748 solve in registers through all sub-steps of a step; like k_chem_step, whose
row code it shares, nothing of it may live in scratch memory.  One device-only compile of
parcel_chem.hip with the flags of csrc/build.sh and -Rpass-analysis=kernel-resource-usage, parsed
the way tests/test_chemistry_resources.py does; the numbers are recorded in
profiles/parcel_chem_kernel_resources.tsv.
"""
import os
import re
import subprocess

from tests.test_kernel_resources import CSRC, _build_flags


def test_the_parcel_chemistry_kernel_is_without_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run(
        [hipcc, *_build_flags(), "--offload-device-only", "-c", "-o", os.devnull,
         "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "parcel_chem.hip")],
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
    kernels = {name: row for name, row in rows.items() if "k_parcel_chem" in name}
    assert len(kernels) == 1, sorted(rows)
    for name, row in kernels.items():
        print(name, {k: row[k] for k in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]",
                                         "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
                     if k in row})
        assert row["ScratchSize [bytes/lane]"] == 0, name
        assert row["VGPRs Spill"] == 0, name
        assert row["LDS Size [bytes/block]"] <= 64 * 1024, name
