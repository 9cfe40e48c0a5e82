"""The reference's OWN unit tests of the injection logic
(tests/unit_tests/backends/test_seeding_methods.py, untouched) against this package's backend
class bound to the checker of include/sdm_seeding.h: scripts/run_reference_unit_tests.py
--seeding.  Build container only: skipped where the reference tree is absent."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(
    not os.path.isdir("/root/reference/tests/unit_tests"), reason="reference tree not present")


def test_reference_seeding_unit_tests_pass_on_the_checker_class(tmp_path):
    report = tmp_path / "report.txt"
    done = subprocess.run(
        [sys.executable, "-B", os.path.join(ROOT, "scripts", "run_reference_unit_tests.py"),
         "--seeding", "--report", str(report)],
        capture_output=True, text=True, timeout=600, cwd=ROOT, check=False)
    text = report.read_text(encoding="utf-8") if report.exists() else ""
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    lines = text.splitlines()
    assert "files: backends/test_seeding_methods.py" in lines
    assert "SeedingCheckerBackend" in text
    outcomes = [line for line in lines if "test_seeding_methods.py::" in line]
    # 5 cases of the counts (two of them the ValueErrors of Particulator.seeding), 4 of the seed
    # index (repeated, identity, reversed, and the third ValueError)
    assert len(outcomes) == 9 and all(line.startswith("passed ") for line in outcomes), text
