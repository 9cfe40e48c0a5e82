#!/usr/bin/env python3
"""Runs the reference's own functions (its backend methods and its efficiency / fragmentation
classes, called the way tests/golden/gen_golden.py:gen_frag calls them, in its pure-Python mode)
on the planted inputs of tests/golden/breakup_regimes.npz and compares them with the float64 run of
the restatement recorded there at rtol 1e-12: a guard on how tests/breakup_regime_cases.py reads
the reference, not an accuracy test.  Only where the reference tree is present."""
# pylint: disable=wrong-import-position,import-error,too-many-locals,invalid-name
import os
import sys

os.environ.setdefault("CI", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "standins"), "/root/reference"]

import numpy as np

from PySDM import Formulae
from PySDM.backends import CPU
from PySDM.dynamics.collisions import breakup_fragmentations as frags
from PySDM.dynamics.collisions import coalescence_efficiencies as effs
from PySDM.physics import si

from tests import breakup_regime_cases as cases

RTOL = 1e-12


def storages(backend):
    from PySDM.backends.impl_common.index import make_Index
    from PySDM.backends.impl_common.indexed_storage import make_IndexedStorage
    from PySDM.backends.impl_common.pair_indicator import make_PairIndicator
    from PySDM.backends.impl_common.pairwise_storage import make_PairwiseStorage

    return (make_Index(backend), make_IndexedStorage(backend), make_PairIndicator(backend),
            make_PairwiseStorage(backend))


def by_scalars(columns, names):
    return cases._by_scalars(columns, names)  # pylint: disable=protected-access


def none_if_negative(value):
    return None if value < 0 else float(value)


def stage(group, columns, backends):
    backend = backends["LowList1982Nf" if group == "ll82" else
                       "Feingold1988" if group == "feingold" else "Straub2010Nf"]
    sto = backend.Storage.from_ndarray
    n_all = len(next(iter(columns.values())))
    out = {k: np.full(n_all, np.nan) for k in cases.STAGES[group][2]}
    scalars = {"ll82": ("vmin", "nfmax"), "straub": ("vmin", "nfmax"), "slams": ("vmin", "nfmax"),
               "exp": ("scale", "vmin", "nfmax"), "feingold": ("scale", "fragtol", "vmin", "nfmax"),
               "gauss": ("mu", "sigma", "vmin", "nfmax"), "lce": ("electric",), "ll82check": ()}
    for sel in by_scalars(columns, scalars[group]):
        c = {k: sto(np.ascontiguousarray(v[sel])) for k, v in columns.items()}
        one = {k: float(v[sel][0]) for k, v in columns.items()}
        n = len(sel)
        nf, fv = sto(np.zeros(n)), sto(np.zeros(n))
        limits = {}
        if "vmin" in one:
            limits = {"vmin": one["vmin"], "nfmax": none_if_negative(one["nfmax"])}
        got = {"nf": nf, "fv": fv}
        if group == "ll82":
            tmp = {k: sto(np.zeros(n)) for k in ("Rf", "Rs", "Rd")}
            backend.ll82_fragmentation(
                n_fragment=nf, CKE=c["CKE"], W=c["W"], W2=c["W2"], St=c["St"], ds=c["ds"],
                dl=c["dl"], dcoal=c["dcoal"], frag_volume=fv, x_plus_y=c["x_plus_y"],
                rand=c["rand"], **limits, **tmp)
            got.update(tmp, rand=c["rand"])
        elif group == "straub":
            tmp = {k: sto(np.zeros(n)) for k in ("Nr1", "Nr2", "Nr3", "Nr4", "Nrt", "d34")}
            backend.straub_fragmentation(
                n_fragment=nf, CW=c["CW"], gam=c["gam"], ds=c["ds"], frag_volume=fv,
                v_max=c["v_max"], x_plus_y=c["x_plus_y"], rand=c["rand"], **limits, **tmp)
        elif group == "slams":
            backend.slams_fragmentation(nf, fv, c["x_plus_y"], sto(np.zeros(n)), c["rand"],
                                        limits["vmin"], limits["nfmax"])
        elif group == "exp":
            backend.exp_fragmentation(n_fragment=nf, scale=one["scale"], frag_volume=fv,
                                      x_plus_y=c["x_plus_y"], rand=c["rand"], **limits)
        elif group == "feingold":
            backend.feingold1988_fragmentation(
                n_fragment=nf, scale=one["scale"], frag_volume=fv, x_plus_y=c["x_plus_y"],
                rand=c["rand"], fragtol=one["fragtol"], **limits)
        elif group == "gauss":
            backend.gauss_fragmentation(n_fragment=nf, mu=one["mu"], sigma=one["sigma"],
                                        frag_volume=fv, x_plus_y=c["x_plus_y"], rand=c["rand"],
                                        **limits)
        elif group == "lce":
            Index, _, PairIndicator, _ = storages(backend)
            radii = np.stack([columns["ra"][sel], columns["rb"][sel]], axis=1).reshape(-1)
            flag = PairIndicator(2 * n)
            flag.indicator[:] = np.tile([True, False], n)
            idx = Index.identity_index(2 * n)
            from PySDM.backends.impl_common.indexed_storage import make_IndexedStorage
            indexed = make_IndexedStorage(backend).from_ndarray(idx, radii)
            params = cases.C.BERRY_ELECTRIC if one["electric"] else cases.C.BERRY_HYDRODYNAMIC
            backend.linear_collection_efficiency(params=tuple(params), output=nf, radii=indexed,
                                                 is_first_in_pair=flag, unit=si.um)
            got = {"out": nf}
        elif group == "ll82check":
            backend.ll82_coalescence_check(Ec=c["Ec"], dl=c["dl"])
            got = {"out": c["Ec"]}
        for k, v in got.items():
            out[k][sel] = v.to_ndarray()
    return out


def pairs(group, columns, backends, table):
    name = group[5:]
    formulae_key = ("LowList1982Nf" if name == "lowlist_nf" else
                    "Feingold1988" if name == "feingold" else "Straub2010Nf")
    backend = backends[formulae_key]
    Index, IndexedStorage, PairIndicator, PairwiseStorage = storages(backend)
    const = backend.formulae.constants
    outputs = cases.PAIRS[name][2]
    n_all = len(columns["rand"])
    out = {k: np.full(n_all, np.nan) for k in outputs}
    for sel in by_scalars(columns, ("vmin", "nfmax")):
        n = len(sel)
        mass = np.stack([columns["mass_j"][sel], columns["mass_k"][sel]], axis=1).reshape(-1)
        idx = Index.identity_index(2 * n)
        mass_s = IndexedStorage.from_ndarray(idx, mass)
        vol_s = IndexedStorage.empty(idx, (2 * n,), float)
        backend.volume_of_water_mass(vol_s, mass_s)
        rad_s = IndexedStorage.empty(idx, (2 * n,), float)
        rad_s.product(vol_s, 1 / const.PI_4_3)
        rad_s **= 1 / 3
        vel_s = IndexedStorage.empty(idx, (2 * n,), float)
        backend.interpolation(output=vel_s.data, radius=rad_s.data, factor=cases.GK_FACTOR,
                              b=table[0], c=table[1])
        flag = PairIndicator(2 * n)
        flag.indicator[:] = np.tile([True, False], n)

        class Part:  # pylint: disable=too-few-public-methods
            pass

        part = Part()
        part.backend, part.formulae, part.n_sd = backend, backend.formulae, 2 * n
        part.PairwiseStorage = PairwiseStorage
        part.attributes = {"volume": vol_s, "radius": rad_s, "relative fall velocity": vel_s,
                           "water mass": mass_s}

        class Builder:  # pylint: disable=too-few-public-methods
            particulator = part

            @staticmethod
            def request_attribute(_):
                pass

        vmin = float(columns["vmin"][sel][0])
        nfmax = none_if_negative(float(columns["nfmax"][sel][0]))
        thing = {
            "lowlist_nf": lambda: frags.LowList1982Nf(vmin=vmin, nfmax=nfmax),
            "straub_nf": lambda: frags.Straub2010Nf(vmin=vmin, nfmax=nfmax),
            "slams": lambda: frags.SLAMS(vmin=vmin, nfmax=nfmax),
            "exp": lambda: frags.Exponential(scale=cases.EXP_SCALE, vmin=vmin, nfmax=nfmax),
            "feingold": lambda: frags.Feingold1988(scale=cases.FEINGOLD_SCALE, vmin=vmin,
                                                   nfmax=nfmax),
            "gauss": lambda: frags.Gaussian(mu=cases.GAUSS_MU, sigma=cases.GAUSS_SIGMA, vmin=vmin,
                                            nfmax=nfmax),
            "always_n": lambda: frags.AlwaysN(n=7.0),
            "constant_mass": lambda: frags.ConstantMass(
                c=cases.RHO_W * cases.K.PI_4_3 * (200 * cases.UM) ** 3),
            "lowlist_ec": effs.LowList1982Ec, "straub_ec": effs.Straub2010Ec,
            "berry_ec": effs.Berry1967,
        }[name]()
        thing.register(Builder)
        if outputs == ("out",):
            pw = PairwiseStorage.empty(n, dtype=float)
            thing(pw, flag)
            out["out"][sel] = pw.to_ndarray()
        else:
            nf, fm = PairwiseStorage.empty(n, dtype=float), PairwiseStorage.empty(n, dtype=float)
            u01 = backend.Storage.from_ndarray(np.ascontiguousarray(columns["rand"][sel]))
            thing(nf, fm, u01, flag)
            out["nf"][sel], out["fm"][sel] = nf.to_ndarray(), fm.to_ndarray()
    return out


def main():
    fix = cases.Fixture()
    backends = {name: CPU(Formulae(terminal_velocity="GunnKinzer1949",
                                   fragmentation_function=name))
                for name in ("Straub2010Nf", "LowList1982Nf", "Feingold1988")}
    failures = 0
    with np.errstate(all="ignore"):
        for group in fix.groups:
            columns = fix.inputs(group)
            got = (pairs(group, columns, backends, fix.table) if group.startswith("pair_")
                   else stage(group, columns, backends))
            want = fix.outputs(group, "float64")
            for key, values in want.items():
                a, b = got[key], values
                close = np.isclose(a, b, rtol=RTOL, atol=0, equal_nan=True)
                if not close.all():
                    failures += 1
                    rows = np.flatnonzero(~close)[:5]
                    print(f"{group}/{key}: {int((~close).sum())} rows differ, e.g.",
                          [(int(i), str(fix.groups[group]['labels'][i]), float(a[i]), float(b[i]))
                           for i in rows])
            print(f"{group}: compared {len(next(iter(want.values())))} rows")
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
