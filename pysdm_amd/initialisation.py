"""Initialisation on the library (include/sdm_initialisation.h): from a dry-aerosol spectrum to
wet droplets in Koehler equilibrium with the ambient air - the input of `Population(...)` and of
`CondensationRunner(dry_volume=..., kappa=...)`.

`equilibrate_wet_radii` is PySDM/initialisation/equilibrate_wet_radii.py with the root search per
super-droplet done by `sdm_equilibrate_wet_radii` (T and RH stay where the engine keeps them);
`wet_radii_call` is the raw call (r_wet, iters and the status words, nothing raised);
`discretise_multiplicities` is PySDM/initialisation/discretise_multiplicities.py; `wet_aerosol` is
the part of `Kinematic2D.init_attributes` after the positions (environments/kinematic_2d.py:63-86).
The surface tension and the hygroscopicity are those of the formulae (any choice of
pysdm_amd/physics/condensation_formulae.py `CHOICES`), routed as the condensation path routes them.
"""
import numpy as np

from . import spectra as _spectra
from .condensation import CONSTANT_NAMES, OPTION_ORDER, check_formulae
from .engine import FLOAT, INT

DEFAULT_RTOL = 1e-5      # equilibrate_wet_radii.py:12-13
DEFAULT_MAX_ITERS = 64
# SDM_INIT_STATUS_* of include/sdm_initialisation.h
STATUS_FAILED, STATUS_MAX_ITERS, STATUS_FIRST, STATUS_SIGMA_FAILED, STATUS_WORDS = 0, 1, 2, 3, 4
SAMPLERS = {"constant_multiplicity": _spectra.sample_constant_multiplicity,
            "logarithmic": _spectra.sample_logarithmic}


class WetRadiusError(AssertionError):
    """the search of some rows failed or used up its iterations (where the reference asserts,
    equilibrate_wet_radii.py:128); `status` holds the four status words"""

    def __init__(self, message, status):
        super().__init__(message)
        self.status = status


def _on_engine(engine, array, dtype):
    """host arrays (and sequences) are uploaded, engine arrays pass (their element type is checked
    at the call)"""
    if array is None:
        return None
    if isinstance(array, (np.ndarray, list, tuple)):
        return engine.upload(np.ascontiguousarray(array, dtype=dtype))
    return array


def wet_radii_call(engine, formulae, *, r_dry, kappa_times_dry_volume, T, RH, f_org=None,
                   cell_id=None, rtol=DEFAULT_RTOL, max_iters=DEFAULT_MAX_ITERS,
                   descriptor=None):
    """one `sdm_equilibrate_wet_radii` call: (r_wet, iters, status) as engine arrays, nothing
    downloaded and nothing raised (`descriptor`: one of condensation.descriptor_of instead of the
    formulae's own, the constants of the default path still from `formulae`)"""
    if descriptor is None:
        descriptor = check_formulae(formulae)
    r_dry = _on_engine(engine, r_dry, FLOAT)
    n = engine.size(r_dry)
    T, RH = _on_engine(engine, T, FLOAT), _on_engine(engine, RH, FLOAT)
    r_wet, iters = engine.empty(n, FLOAT), engine.empty(n, INT)
    status = engine.empty(STATUS_WORDS, INT)  # (the call writes its start values on the device)
    if n == 0:  # ... unless it returns before any launch
        engine.fill(status, 0)
    engine.call_initialisation(
        "sdm_equilibrate_wet_radii", int(n), r_dry,
        _on_engine(engine, kappa_times_dry_volume, FLOAT), _on_engine(engine, f_org, FLOAT),
        _on_engine(engine, cell_id, INT), T, RH, int(engine.size(T)), float(rtol), int(max_iters),
        [float(getattr(formulae.constants, name)) for name in CONSTANT_NAMES], descriptor,
        r_wet, iters, status)
    return r_wet, iters, status


def _row_context(engine, first, r_dry, ktdv, T, RH, f_org, cell_id, formulae):
    """the context of the reference's warning (equilibrate_wet_radii.py:104-121) for one row"""
    def at(array, index):
        return engine.download(array[index:index + 1])[0]

    r_d = float(at(r_dry, first))
    cell = 0 if cell_id is None else int(at(cell_id, first))
    inside = 0 <= cell < engine.size(T)
    kappa = float(at(ktdv, first)) / float(formulae.trivia.volume(radius=r_d))
    return (f"i={first}, r_d={r_d!r}, cell={cell}, "
            f"T={float(at(T, cell)) if inside else 'outside the cells'!r}, "
            f"RH={float(at(RH, cell)) if inside else 'outside the cells'!r}, "
            f"f_org={0.0 if f_org is None else float(at(f_org, first))!r}, kappa={kappa!r}")


def equilibrate_wet_radii(engine, formulae, *, r_dry, kappa_times_dry_volume, T, RH, f_org=None,
                          cell_id=None, rtol=DEFAULT_RTOL, max_iters=DEFAULT_MAX_ITERS,
                          descriptor=None):
    """the wet radii (an engine array) at which dry particles of radius `r_dry` and
    `kappa_times_dry_volume` are in equilibrium with T[cell_id], min(RH[cell_id], 1); r_dry itself
    where there is no such radius above it.  Inputs are host or engine arrays.  The status words
    are read once; WetRadiusError (an AssertionError, as the reference asserts) if the search of
    any row failed or used up `max_iters`"""
    if descriptor is None:
        descriptor = check_formulae(formulae)
    r_dry = _on_engine(engine, r_dry, FLOAT)
    ktdv = _on_engine(engine, kappa_times_dry_volume, FLOAT)
    T, RH = _on_engine(engine, T, FLOAT), _on_engine(engine, RH, FLOAT)
    if f_org is None and descriptor.option[OPTION_ORDER.index("surface_tension")] != 0:
        f_org = engine.zeros(engine.size(r_dry), FLOAT)  # equilibrate_wet_radii.py:29-30
    f_org, cell_id = _on_engine(engine, f_org, FLOAT), _on_engine(engine, cell_id, INT)
    r_wet, _, status = wet_radii_call(
        engine, formulae, r_dry=r_dry, kappa_times_dry_volume=ktdv, T=T, RH=RH, f_org=f_org,
        cell_id=cell_id, rtol=rtol, max_iters=max_iters, descriptor=descriptor)
    words = [int(w) for w in engine.download(status)]
    n = engine.size(r_dry)
    if words[STATUS_FAILED] or words[STATUS_MAX_ITERS] or words[STATUS_SIGMA_FAILED]:
        message = (f"failed to find wet radius for {words[STATUS_FAILED]} particle(s), "
                   f"{words[STATUS_MAX_ITERS]} more used up max_iters={max_iters}")
        if words[STATUS_SIGMA_FAILED]:
            message += (f"; the surface tension's inner search used up its iterations on "
                        f"{words[STATUS_SIGMA_FAILED]} particle(s)")
        if words[STATUS_FIRST] < n:
            message += "; first: " + _row_context(engine, words[STATUS_FIRST], r_dry, ktdv, T,
                                                  RH, f_org, cell_id, formulae)
        raise WetRadiusError(message, words)
    return r_wet


def discretise_multiplicities(values):
    """integer multiplicities by rounding, NaN -> 0, with the reference's checks (no multiplicity
    of zero, at most 1% change of the total)"""
    values = np.asarray(values)
    values_int = np.where(np.isnan(values), 0, values).round().astype(np.int64)
    if np.issubdtype(values.dtype, np.floating):
        if np.isnan(values).all():
            return values_int
        if not np.logical_or(values_int > 0, np.isnan(values)).all():
            raise ValueError("int-casting resulted in multiplicity of zero "
                             f"(min(y_float)={min(values)})")
        percent_diff = 100 * abs(1 - np.nansum(values) / np.sum(values_int.astype(float)))
        if percent_diff > 1:
            raise ValueError(f"{percent_diff}% error in total real-droplet number"
                             " due to casting multiplicities to ints")
    return values_int


def wet_aerosol(engine, formulae, ambient, *, spectrum, kappa, n_sd, cell_id=None, f_org=None,
                sampling="constant_multiplicity", rtol=DEFAULT_RTOL, domain_volume=None):
    """`n_sd` super-droplets sampled from the dry-radius `spectrum` (per kg of dry air, as the
    kinematic environments take it) and brought to equilibrium with `ambient` (an AmbientColumns,
    whose T and RH stay on the device): a dict of host arrays `dry_volume`,
    `kappa_times_dry_volume`, `kappa`, `r_dry`, `r_wet`, `water_mass` and `n_per_kg`; with
    `domain_volume` also `multiplicity` = discretise(n_per_kg * rhod[cell_id] * domain_volume)"""
    sampler = SAMPLERS[sampling] if isinstance(sampling, str) else sampling
    r_dry, n_per_kg = sampler(spectrum, n_sd)
    cells = np.zeros(n_sd, dtype=np.int64) if cell_id is None else np.asarray(cell_id,
                                                                               dtype=np.int64)
    dry_volume = formulae.trivia.volume(radius=r_dry)
    ktdv = kappa * dry_volume
    if np.all(np.asarray(kappa) == 0):  # kinematic_2d.py:69-70
        r_wet = np.array(r_dry)
    else:
        r_wet = engine.download(equilibrate_wet_radii(
            engine, formulae, r_dry=r_dry, kappa_times_dry_volume=ktdv, T=ambient.T,
            RH=ambient.RH, f_org=f_org, cell_id=cells, rtol=rtol))
    out = {"r_dry": r_dry, "dry_volume": dry_volume, "kappa_times_dry_volume": ktdv,
           "kappa": np.broadcast_to(np.asarray(kappa, dtype=float), (n_sd,)).copy(),
           "r_wet": r_wet, "cell_id": cells, "n_per_kg": n_per_kg,
           "water_mass": formulae.constants.rho_w * formulae.trivia.volume(radius=r_wet)}
    if domain_volume is not None:
        rhod = engine.download(ambient.rhod)
        out["multiplicity"] = discretise_multiplicities(n_per_kg * rhod[cells] * domain_volume)
    return out
