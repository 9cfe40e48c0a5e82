#!/usr/bin/env python3
"""Share of the pairs that the tags of pysdm_amd/csrc/pair_tag.h decide without a gather, on the
CPU: the oracle's Shima box stepped through 3600 steps as one call would see it (references from
the initial state), one random pairing of the live population per checkpoint, the decisions those
of pair_tag.h compiled for the host (tests/pair_tag_model).

    python scripts/pair_tag_share.py [--n-sd 65536]

Prints the table of profiles/README.md, round 10.  No GPU."""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHECKPOINTS = (21, 120, 220, 600, 1200, 1800, 2400, 3000, 3600)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--n-sd", type=int, default=2**16)
    args = parser.parse_args()

    from oracle.engine import OracleEngine  # pylint: disable=import-outside-toplevel
    from pysdm_amd.cases import make_box  # pylint: disable=import-outside-toplevel
    from tests.pair_tag_model import model, skip_share  # pylint: disable=import-outside-toplevel

    mdl, rng = model(), np.random.default_rng(11)
    runner = make_box(OracleEngine.get(), "shima", n_sd=args.n_sd, adaptive=False)
    cfg = runner.step_cfg()
    numbers = dict(b=float(cfg.kernel_param[0]), rho_w=float(cfg.rho_w), dt=float(cfg.dt),
                   dv=float(cfg.dv), substeps=int(cfg.substeps))
    snap = runner.snapshot()
    live = snap["idx"][: int(snap["length"])]
    n_ref = int(snap["multiplicity"][live].max())
    m_base = mdl.m_base(float(snap["attributes"][0][live].max()))
    print(f"n_sd = {args.n_sd}, n_ref = {n_ref}, m_base = {m_base!r}")
    print("| step | pairs that skip the gather | pairs that collide |")
    print("|---|---|---|")
    done = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for upto in CHECKPOINTS:
            runner.run(upto - done)
            done = upto
            snap = runner.snapshot()
            live = snap["idx"][: int(snap["length"])]
            pairs, skipped, colliding, sound = skip_share(
                mdl, snap["multiplicity"], snap["attributes"][0], live, rng, n_ref=n_ref,
                m_base=m_base, **numbers)
            assert sound
            print(f"| {upto} | {skipped / pairs:.3f} | {colliding / pairs:.4f} |")


if __name__ == "__main__":
    main()
