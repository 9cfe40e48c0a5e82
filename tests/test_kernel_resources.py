"""The register budget of k_pair_all_sort, read from the compiler (no GPU needed).

The kernel is launched in workgroups of 1024 threads = 4 waves per SIMD.  Its sort workgroups only
hide behind pair work when TWO workgroups fit on a CU, which takes a budget of 8 waves per SIMD
(fused.hip: PAIR_SORT_BUDGET; profiles/README.md, "two workgroups per CU").  One device-only
compile of fused.hip with the flags of csrc/build.sh and -Rpass-analysis=kernel-resource-usage,
parsed the way scripts/kernel_resources.py does.
"""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pysdm_amd", "csrc")

# sdm_hip.h: SDM_KERNEL_*
KERNELS = {0: "golovin", 1: "geometric", 2: "constant", 3: "parameterized", 4: "simple_geometric",
           5: "linear"}
# instantiations that stay at one workgroup per CU: 8 waves per SIMD would cost them scratch
# (parameterized: 34 VGPRs spilled, 48 B of scratch per lane under that budget)
ONE_PER_CU = {"parameterized"}


def _sdm_kernel_values():
    text = open(os.path.join(ROOT, "include", "sdm_hip.h"), encoding="utf-8").read()
    return {m.group(1).lower(): int(m.group(2))
            for m in re.finditer(r"#define SDM_KERNEL_([A-Z_]+) (\d+)", text)}


def _build_flags():
    text = open(os.path.join(CSRC, "build.sh"), encoding="utf-8").read()
    return shlex.split(re.search(r'^FLAGS="([^"]*)"', text, re.M).group(1))


@pytest.fixture(scope="module")
def fused_resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run(
        [hipcc, *_build_flags(), "--offload-device-only", "-c", "-o", os.devnull,
         "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "fused.hip")],
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
    return rows


def _pair_all_sort(rows):
    found = {}
    for name, row in rows.items():
        m = re.match(r"_Z15k_pair_all_sortILi(\d+)EE", name)
        if m:
            found[KERNELS[int(m.group(1))]] = row
    return found


def test_kernel_numbers_are_the_headers():
    assert {name: value for value, name in KERNELS.items()} == _sdm_kernel_values()


def test_pair_all_sort_golovin_fits_twice_on_a_cu(fused_resources):
    row = _pair_all_sort(fused_resources)["golovin"]
    print("k_pair_all_sort<SDM_KERNEL_GOLOVIN>:", row)
    assert row["Occupancy [waves/SIMD]"] == 8
    assert row["ScratchSize [bytes/lane]"] == 0
    assert row["VGPRs"] <= 64


def test_every_pair_all_sort_is_without_scratch(fused_resources):
    found = _pair_all_sort(fused_resources)
    assert set(found) == set(KERNELS.values())  # every collision kernel the launch code switches on
    for name, row in sorted(found.items()):
        print(f"k_pair_all_sort<{name}>:", row)
        assert row["ScratchSize [bytes/lane]"] == 0, name
        if name not in ONE_PER_CU:
            assert row["Occupancy [waves/SIMD]"] == 8, name
