"""The resources of the seeding kernels, read from the compiler (no GPU needed).

include/sdm_seeding.h's kernels (pysdm_amd/csrc/seeding.hip) are a ballot-and-scan selection: a
few registers, at most 64 bytes of LDS and nothing in scratch memory - the loop over the attribute rows
has a run-time length and must not turn into a private array.  One device-only compile of
seeding.hip with the flags of csrc/build.sh and -Rpass-analysis=kernel-resource-usage, parsed the
way tests/test_kernel_resources.py does.
"""
import os
import re
import subprocess

from tests.test_kernel_resources import CSRC, _build_flags


def test_seeding_kernels_are_present_and_without_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run(
        [hipcc, *_build_flags(), "--offload-device-only", "-c", "-o", os.devnull,
         "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "seeding.hip")],
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
    kernels = {name: row for name, row in rows.items() if "k_seed" in name}
    names = " ".join(kernels)
    for wanted in ("k_seed_count", "k_seed_scan", "k_seed_scatter", "k_seed_identity"):
        assert wanted in names, wanted
    assert len(kernels) == 4, names
    for name, row in sorted(kernels.items()):
        print(name, {k: row[k] for k in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]",
                                         "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
                     if k in row})
        assert row["ScratchSize [bytes/lane]"] == 0, name
        # (the largest is the scatter's sixteen run counts: 16 x 4 bytes)
        assert row["LDS Size [bytes/block]"] <= 64, name
