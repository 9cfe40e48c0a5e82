"""`pysdm_plugin.run_parcel` with `Coalescence` as the third dynamic (include/sdm_parcel_coal.h)
against `particulator.run` of the reference on the checker backend, bit for bit, and the refusals
of its argument check by name."""
import os
import sys

import numpy as np
import pytest

from tests import condensation_cases as cond
from tests import parcel_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("PYSDM_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def pysdm():
    """the reference's classes (the module is skipped where the reference is not importable)"""
    if not os.path.isdir(os.path.join(REFERENCE, "PySDM")):
        pytest.skip("reference tree not present")
    os.environ.setdefault("CI", "1")
    added = [os.path.join(HERE, "golden", "standins"), REFERENCE]
    sys.path[:0] = added
    try:
        pytest.importorskip("PySDM")
        from PySDM import Builder, Formulae  # pylint: disable=import-outside-toplevel,import-error
        from PySDM import dynamics  # pylint: disable=import-outside-toplevel,import-error
        from PySDM.dynamics.collisions import (  # pylint: disable=import-outside-toplevel,import-error
            breakup_fragmentations, coalescence_efficiencies, collision_kernels)
        from PySDM.environments import Parcel  # pylint: disable=import-outside-toplevel,import-error
    finally:
        for path in added:
            sys.path.remove(path)
    return {"Builder": Builder, "Formulae": Formulae, "dynamics": dynamics, "Parcel": Parcel,
            "kernels": collision_kernels, "fragmentations": breakup_fragmentations,
            "efficiencies": coalescence_efficiencies}


def twin(pysdm, order=("ambient", "condensation", "coalescence"), third=None, **options):
    """a particulator of the recorded parcel run a1 with multiplicities of 1, 2 and the recorded
    ones, and a constant kernel strong enough for collisions and deaths within a few steps"""
    from pysdm_amd.pysdm_plugin import as_pysdm_backend  # pylint: disable=import-outside-toplevel
    from tests.parcel_coal_checker import ParcelCoalCheckerBackend  # pylint: disable=import-outside-toplevel

    gold = cond.gold("cond_parcel_a1")
    cfg = {k[len("parcel/"):]: gold[k] for k in gold.files if k.startswith("parcel/")}
    backend = as_pysdm_backend(ParcelCoalCheckerBackend)(pysdm["Formulae"]())
    env = pysdm["Parcel"](dt=float(cfg["dt"]), mass_of_dry_air=float(cfg["mass_of_dry_air"]),
                          p0=float(cfg["p0"]),
                          initial_water_vapour_mixing_ratio=float(cfg["qv0"]),
                          T0=float(cfg["T0"]), w=float(cfg["w"]))
    builder = pysdm["Builder"](n_sd=int(cfg["n_sd"]), backend=backend, environment=env)
    dyn = pysdm["dynamics"]
    kernel = pysdm["kernels"].ConstantK(a=float(cfg["mass_of_dry_air"]) * 2e-2)
    parts = {"ambient": dyn.AmbientThermodynamics, "condensation": lambda: dyn.Condensation(
        adaptive=True), "coalescence": lambda: third or dyn.Coalescence(
            collision_kernel=kernel, dt_coal_range=(0.05, 100.0), **options)}
    for name in order:
        builder.add_dynamic(parts[name]())
    attributes = {k[len("init/"):]: np.array(gold[k]) for k in gold.files
                  if k.startswith("init/")}
    planted = np.arange(attributes["multiplicity"].size) % 3
    attributes["multiplicity"] = np.where(planted == 0, 1, np.where(
        planted == 1, 2, attributes["multiplicity"]))
    return builder.build(attributes=attributes, products=())


def state_of(particulator):
    env, coal = particulator.environment, particulator.dynamics["Collision"]
    attrs = particulator.attributes
    attrs.sanitize()
    idx = getattr(attrs, "_ParticleAttributes__idx")
    out = {"n_steps": np.asarray(particulator.n_steps), "dv": np.asarray(env.mesh.dv),
           "n_live": np.asarray(len(idx)), "idx": idx.to_ndarray()[:len(idx)].copy(),
           "stream": np.asarray(coal.rnd_opt_coll.rnd.offset)}
    for name in ("signed water mass", "multiplicity", "dry volume", "kappa times dry volume"):
        out[name] = attrs[name].to_ndarray(raw=True)
    out["kappa"] = attrs["kappa"].to_ndarray(raw=True)[out["idx"]]
    for var in env.variables:
        out["current/" + var] = env[var].to_ndarray()
    for name in ("collision_rate", "collision_rate_deficit", "coalescence_rate",
                 "stats_n_substep", "stats_dt_min"):
        out[name] = getattr(coal, name).to_ndarray()
    return out


def same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(pc.bits(np.asarray(a[key])), pc.bits(np.asarray(b[key]))), (
            what, key, a[key], b[key])


def test_run_parcel_with_coalescence_leaves_the_particulator_as_run_would(pysdm):
    from pysdm_amd.pysdm_plugin import run_parcel  # pylint: disable=import-outside-toplevel

    stepped, fused = twin(pysdm), twin(pysdm)
    n_sd = stepped.n_sd
    stepped.run(6)
    run_parcel(fused, 6)
    a = state_of(stepped)
    same(a, state_of(fused), "after 6 steps")
    assert a["coalescence_rate"][0] > 0 and a["n_live"] < n_sd  # collisions and deaths occurred
    assert not np.array_equal(a["idx"], np.sort(a["idx"]))      # ... in a shuffled order
    stepped.run(1)
    fused.run(1)  # the particulator goes on by itself: permutation, stream position, counters
    same(state_of(stepped), state_of(fused), "after one further particulator.run(1)")
    run_parcel(fused, 2)  # ... and from a permutation that is not the identity
    stepped.run(2)
    same(state_of(stepped), state_of(fused), "after a further run_parcel(2)")


def test_run_parcel_with_fixed_substeps(pysdm):
    from pysdm_amd.pysdm_plugin import run_parcel  # pylint: disable=import-outside-toplevel

    options = dict(adaptive=False, substeps=3)
    stepped, fused = twin(pysdm, **options), twin(pysdm, **options)
    stepped.run(4)
    run_parcel(fused, 4)
    a = state_of(stepped)
    same(a, state_of(fused), "after 4 steps")
    assert a["coalescence_rate"][0] > 0 and a["stats_n_substep"][0] == 3


def test_refusals_of_the_argument_check_by_name(pysdm):
    from pysdm_amd.pysdm_plugin import run_parcel  # pylint: disable=import-outside-toplevel

    dyn, kernels = pysdm["dynamics"], pysdm["kernels"]
    with pytest.raises(ValueError, match="order AmbientThermodynamics, Condensation, Coalesc"):
        run_parcel(twin(pysdm, order=("ambient", "coalescence", "condensation")), 1)
    with pytest.raises(ValueError, match="order AmbientThermodynamics, Condensation, Coalesc"):
        run_parcel(twin(pysdm, order=("coalescence", "ambient", "condensation")), 1)
    kernel = kernels.ConstantK(a=1e-3)
    breakup = dyn.Breakup(collision_kernel=kernel,
                          fragmentation_function=pysdm["fragmentations"].AlwaysN(n=2))
    with pytest.raises(ValueError, match="not Breakup"):
        run_parcel(twin(pysdm, third=breakup), 1)
    collision = dyn.Collision(
        collision_kernel=kernel, coalescence_efficiency=pysdm["efficiencies"].ConstEc(Ec=0.5),
        breakup_efficiency=pysdm["dynamics"].collisions.breakup_efficiencies.ConstEb(Eb=0.5),
        fragmentation_function=pysdm["fragmentations"].AlwaysN(n=2))
    with pytest.raises(ValueError, match="not Collision"):
        run_parcel(twin(pysdm, third=collision), 1)
    with pytest.raises(NotImplementedError, match="optimized_random"):
        run_parcel(twin(pysdm, optimized_random=True), 1)
    with pytest.raises(NotImplementedError, match="global croupier"):
        run_parcel(twin(pysdm, croupier="global"), 1)
    extra = twin(pysdm)
    extra.dynamics["Extra"] = object()
    with pytest.raises(ValueError, match="exactly the dynamics"):
        run_parcel(extra, 1)
    with pytest.raises(NotImplementedError, match="products"):
        run_parcel(twin(pysdm), 1, products=(object(),))
