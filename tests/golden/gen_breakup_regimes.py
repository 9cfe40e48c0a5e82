#!/usr/bin/env python3
"""Writes tests/golden/breakup_regimes.npz: the planted inputs of tests/breakup_regime_cases.py,
the label of every row, and the results of the restatement there at 50 digits (mpmath), rounded
once to float64, next to those of its float64 run.

    python3 tests/golden/gen_breakup_regimes.py            # write the fixture
    python3 tests/golden/gen_breakup_regimes.py --check    # the committed one is the generated one

Rows on which the two runs take different branches (or only one of them overflows) are not
planted: the search keeps what both agree on and then demands the coverage.  Prints, per group,
the measured rounding error E of the formulation (breakup_regime_cases.E holds them)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import breakup_regime_cases as cases  # noqa: E402  pylint: disable=wrong-import-position


def generate():
    from pysdm_amd.terminal_velocity import gunn_kinzer_table  # pylint: disable=import-outside-toplevel

    table = tuple(np.array(column) for column in gunn_kinzer_table())
    out = {"gk/a": table[0], "gk/b": table[1]}
    measured = {}
    mp50 = cases.Mp50()
    for group, columns in cases.plant(table).items():
        plain, labels, exact = cases.evaluate(cases.Float64, group, columns, table)
        precise, labels_mp, _ = cases.evaluate(mp50, group, columns, table)
        second = columns.pop("on_selector") != 0
        second |= np.asarray([any(tag in cases.FLOAT_ONLY_LABELS for tag in str(lab).split(";"))
                              for lab in labels])
        same = labels == labels_mp
        for key in plain:
            same &= np.isfinite(plain[key]) == np.isfinite(precise[key])
            same &= np.isnan(plain[key]) == np.isnan(precise[key])
        keep = same | second
        print(f"{group}: {int(keep.sum())} rows ({int((~keep).sum())} candidates on which the "
              f"two precisions part, {int(second.sum())} on the second list)")
        err = cases.errors(group, plain, precise)
        measured[group] = float(err[keep & ~second].max())
        for key, values in columns.items():
            out[f"{group}/in/{key}"] = values[keep]
        out[f"{group}/labels"] = labels[keep]
        out[f"{group}/exact"] = exact[keep]
        out[f"{group}/float_only"] = second[keep]
        for key in plain:
            out[f"{group}/expected/{key}"] = np.where(second, plain[key], precise[key])[keep]
            out[f"{group}/float64/{key}"] = plain[key][keep]
    return out, measured


def rounded_up(value):
    """four significant digits, never below the value"""
    text = f"{value:.3e}"
    if float(text) < value:
        mantissa, exponent = text.split("e")
        text = f"{float(mantissa) + 1e-3:.3f}e{exponent}"
    return text


def main():
    out, measured = generate()
    print("E = {")
    for group, value in measured.items():
        print(f'    "{group}": {rounded_up(value)},')
    print("}")
    if "--check" in sys.argv:
        committed = np.load(cases.FIXTURE)
        assert sorted(committed.files) == sorted(out), "the set of arrays differs"
        for key, values in out.items():
            if "/float64/" in key:  # libm of the day: to a few ulp
                np.testing.assert_allclose(committed[key], values, rtol=1e-9, atol=0, err_msg=key)
            else:
                np.testing.assert_array_equal(committed[key], values, err_msg=key)
        for group, value in measured.items():
            assert value <= cases.E[group] * (1 + 1e-6), (group, value, cases.E[group])
        print("the committed fixture is the generated one")
        return
    np.savez_compressed(cases.FIXTURE, **out)
    print(f"wrote {cases.FIXTURE}: {os.path.getsize(cases.FIXTURE) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
