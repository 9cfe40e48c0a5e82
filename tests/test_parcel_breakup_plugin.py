"""`pysdm_plugin.run_parcel(..., breakup=True)` with `Collision` or `Breakup` as the third dynamic
(include/sdm_parcel_breakup.h) against `particulator.run` of the reference on the checker backend,
and the refusals that stay without the keyword.

Every comparison is bit for bit: on the checker backend the reference's own route goes through this
project's stage symbols (the backend methods `Collision.__call__` calls are the CPU oracle's, whose
transcendentals are csrc/sdm_math.h's), so no comparison here crosses into the reference's libm and
the README's breakup bound (1e-12 relative) is not needed."""
import numpy as np
import pytest

from tests import test_parcel_coal_plugin as coal_plugin
from tests.test_parcel_coal_plugin import pysdm  # noqa: F401  pylint: disable=unused-import


def third_dynamic(pysdm, kind, **options):  # noqa: F811  pylint: disable=redefined-outer-name
    dyn = pysdm["dynamics"]
    kernel = pysdm["kernels"].ConstantK(a=2e-3)
    fragmentation = pysdm["fragmentations"].AlwaysN(n=3)
    options = dict(collision_kernel=kernel, fragmentation_function=fragmentation,
                   dt_coal_range=(0.25, 100.0), **options)
    if kind == "Breakup":
        return dyn.Breakup(**options)
    return dyn.Collision(
        coalescence_efficiency=pysdm["efficiencies"].ConstEc(Ec=0.4),
        breakup_efficiency=dyn.collisions.breakup_efficiencies.ConstEb(Eb=0.5), **options)


def twin(pysdm, kind, **options):  # noqa: F811  pylint: disable=redefined-outer-name
    """tests/test_parcel_coal_plugin.py's particulator on the backend that has the library of
    include/sdm_parcel_breakup.h, with `kind` as the third dynamic"""
    from tests import parcel_coal_checker  # pylint: disable=import-outside-toplevel
    from tests.parcel_breakup_checker import ParcelBreakupCheckerBackend  # pylint: disable=import-outside-toplevel

    kept = parcel_coal_checker.ParcelCoalCheckerBackend
    parcel_coal_checker.ParcelCoalCheckerBackend = ParcelBreakupCheckerBackend
    try:
        third = None if kind == "Coalescence" else third_dynamic(pysdm, kind, **options)
        return coal_plugin.twin(pysdm, third=third)
    finally:
        parcel_coal_checker.ParcelCoalCheckerBackend = kept


def state_of(particulator):
    """what tests/test_parcel_coal_plugin.py compares, the breakup counters and the positions of
    the proc / frag streams"""
    out = coal_plugin.state_of(particulator)
    collision = particulator.dynamics["Collision"]
    for name in ("breakup_rate", "breakup_rate_deficit"):
        out[name] = getattr(collision, name).to_ndarray()
    out["stream_proc"] = np.asarray(collision.rnd_opt_proc.rnd.offset)
    out["stream_frag"] = np.asarray(collision.rnd_opt_frag.rnd.offset)
    return out


@pytest.mark.parametrize("kind", ("Collision", "Breakup"))
def test_run_parcel_with_breakup_leaves_the_particulator_as_run_would(pysdm, kind):  # noqa: F811  pylint: disable=redefined-outer-name
    from pysdm_amd.pysdm_plugin import run_parcel  # pylint: disable=import-outside-toplevel

    stepped, fused = twin(pysdm, kind), twin(pysdm, kind)
    stepped.run(3)
    run_parcel(fused, 3, breakup=True)
    a = state_of(stepped)
    coal_plugin.same(a, state_of(fused), "after 3 steps")
    assert a["breakup_rate"][0] > 0 and a["stream_proc"] > 0  # breakups occurred, the stream moved
    assert a["stream_proc"] == a["stream_frag"]
    if kind == "Collision":
        assert a["coalescence_rate"][0] > 0
    assert not np.array_equal(a["idx"], np.sort(a["idx"]))  # ... in a shuffled order
    stepped.run(1)
    fused.run(1)  # the particulator goes on by itself: permutation, stream positions, counters
    coal_plugin.same(state_of(stepped), state_of(fused), "after one further particulator.run(1)")
    run_parcel(fused, 1, breakup=True)  # ... and takes its turn again
    stepped.run(1)
    coal_plugin.same(state_of(stepped), state_of(fused), "after a further run_parcel(1)")


def test_run_parcel_with_breakup_and_fixed_substeps(pysdm):  # noqa: F811  pylint: disable=redefined-outer-name
    from pysdm_amd.pysdm_plugin import run_parcel  # pylint: disable=import-outside-toplevel

    options = dict(adaptive=False, substeps=3)
    stepped, fused = twin(pysdm, "Collision", **options), twin(pysdm, "Collision", **options)
    stepped.run(2)
    run_parcel(fused, 2, breakup=True)
    a = state_of(stepped)
    coal_plugin.same(a, state_of(fused), "after 2 steps")
    assert a["breakup_rate"][0] > 0 and a["stats_n_substep"][0] == 3


def test_a_coalescence_runs_with_the_keyword_as_without(pysdm):  # noqa: F811  pylint: disable=redefined-outer-name
    from pysdm_amd.pysdm_plugin import run_parcel  # pylint: disable=import-outside-toplevel

    with_keyword, without = twin(pysdm, "Coalescence"), coal_plugin.twin(pysdm)
    run_parcel(with_keyword, 3, breakup=True)
    run_parcel(without, 3)
    a = coal_plugin.state_of(without)
    coal_plugin.same(a, coal_plugin.state_of(with_keyword), "Coalescence with breakup=True")
    assert a["coalescence_rate"][0] > 0


def test_the_refusals_stay_without_the_keyword(pysdm):  # noqa: F811  pylint: disable=redefined-outer-name
    from pysdm_amd.pysdm_plugin import run_parcel  # pylint: disable=import-outside-toplevel

    for kind in ("Breakup", "Collision"):
        with pytest.raises(ValueError, match=f"not {kind}"):
            run_parcel(twin(pysdm, kind), 1)
    with pytest.raises(NotImplementedError, match="optimized_random"):
        run_parcel(twin(pysdm, "Collision", optimized_random=True), 1, breakup=True)
    with pytest.raises(NotImplementedError, match="global croupier"):
        run_parcel(twin(pysdm, "Collision", croupier="global"), 1, breakup=True)
    with pytest.raises(NotImplementedError, match="products"):
        run_parcel(twin(pysdm, "Collision"), 1, products=(object(),), breakup=True)
