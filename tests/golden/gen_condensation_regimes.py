#!/usr/bin/env python3
"""Writes tests/golden/condensation_regimes.npz: the planted inputs of
tests/condensation_regime_cases.py, the labels of every row, the results of the restatement there
at 50 digits (mpmath) rounded once to float64 next to those of its float64 run, and the per-row
relative bounds (four times the formulation's own first-order rounding error, plus the solvers'
contracts).

    python3 tests/golden/gen_condensation_regimes.py            # write the fixture
    python3 tests/golden/gen_condensation_regimes.py --check    # the committed one is the generated one

Rows on which the two precisions take different branches, or whose `minfun` is not strictly
monotone on the solver's bracket at 50 digits, are not planted; the coverage is demanded
afterwards.  Prints the worst error over bound of the float64 run of the restatement per label
group: the check of the error model (it has to stay below one).  With --measure ENGINE it also
writes tests/golden/condensation_regimes_measured.json from the CPU checkers."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import condensation_regime_cases as cases  # noqa: E402  pylint: disable=wrong-import-position


def measure():
    """worst checker-versus-50-digit error over bound per label group, through the CPU checkers"""
    fix = cases.Fixture()
    worst = {}
    for group in fix.groups:
        cases.check_group(cases.checker_engine(group), group, fix, report=worst)
    worst = {key: float(f"{value:.3g}") for key, value in sorted(worst.items())}
    with open(cases.MEASURED, "w", encoding="utf-8") as file:
        json.dump({"_about": "worst |checker - 50-digit value| / bound per label group "
                             "(gen_condensation_regimes.py --measure)", **worst}, file, indent=1)
        file.write("\n")
    print(f"wrote {cases.MEASURED}: the worst ratio is {max(worst.values()):.3g}")


def main():
    if "--measure" in sys.argv:
        measure()
        return
    out, ratios = cases.generate()
    worst = max(ratios.values())
    print(f"float64 run of the restatement: worst error over bound {worst:.3g} "
          f"({max(ratios, key=ratios.get)})")
    assert worst <= 1, {key: value for key, value in ratios.items() if value > 1}
    if "--check" in sys.argv:
        committed = np.load(cases.FIXTURE)
        assert sorted(committed.files) == sorted(out), "the set of arrays differs"
        for key, values in out.items():
            if "/float64/" in key or "/bound/" in key:  # libm of the day: to a few ulp
                np.testing.assert_allclose(committed[key], values, rtol=1e-9, atol=0, err_msg=key)
            elif key.endswith("/float_only") or "/expected/" not in key:
                np.testing.assert_array_equal(committed[key], values, err_msg=key)
            else:  # float-only rows carry the float64 run's value
                second = out[key.split("/")[0] + "/float_only"]
                np.testing.assert_array_equal(committed[key][~second], values[~second],
                                              err_msg=key)
                np.testing.assert_allclose(committed[key][second], values[second], rtol=1e-9,
                                           atol=0, err_msg=key)
        print("the committed fixture is the generated one")
        return
    np.savez_compressed(cases.FIXTURE, **out)
    print(f"wrote {cases.FIXTURE}: {os.path.getsize(cases.FIXTURE) / 1024:.1f} KiB")
    cases.check_coverage(cases.Fixture())


if __name__ == "__main__":
    main()
