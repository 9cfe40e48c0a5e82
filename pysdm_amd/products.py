"""Products of a parcel's droplet population, by PySDM's names, constructor arguments and units
(PySDM/products/size_spectral/, products/impl/{moment,concentration,spectrum_moment,
activation_filtered}_product.py, the unit scaling of products/impl/product.py), served by the
request table of include/sdm_parcel_diag.h.

A product states which moments (and at most one size spectrum) it reads and how its value follows
on the host from `moment_0 / moments / spectrum / dv / rhod`.  `RequestTable` compiles a sequence
of products into one table - identical requests are shared - and hands the evaluated rows back
to the products.  The moments follow the backend method `moments` for one cell with
weighting_rank = 0: a rank-0 request yields moment_0, any other rank the moment divided by
moment_0 (PySDM's MomentProduct._download_moment_to_buffer).

Units: a product's `unit` may be its default (base SI) or the same dimension with the prefixes
and symbols of `_SYMBOLS` ("cm^-3", "mg^-1 um^-1", "g/kg", "um"); values are returned in that unit.
"""
import re
from collections import namedtuple

import numpy as np

from . import abi

# (attr, rank, filter_attr, min_x, max_x, skip_division_by_m0) by the names of abi.PARCEL_ATTRS /
# abi.PARCEL_FILTERS
MomentRequest = namedtuple("MomentRequest", "attr rank filter_attr min_x max_x skip")
SpectrumRequest = namedtuple("SpectrumRequest", "bin_attr edges")

_SYMBOLS = {  # symbol: (magnitude in base SI units, dimension)
    "m": (1.0, "m"), "cm": (1e-2, "m"), "mm": (1e-3, "m"), "um": (1e-6, "m"), "nm": (1e-9, "m"),
    "kg": (1.0, "kg"), "g": (1e-3, "kg"), "mg": (1e-6, "kg"), "ug": (1e-9, "kg"),
}


def _parse_unit(unit):
    """(magnitude in base SI units, {dimension: power}) of e.g. "cm^-3", "kg^-1 m^-1", "g/kg" """
    text = unit.strip()
    if text in ("dimensionless", "1"):
        return 1.0, {}
    if text in ("%", "percent"):
        return 0.01, {}
    magnitude, dims, sign = 1.0, {}, 1
    for token in re.findall(r"/|[^\s/*]+", text):
        if token == "/":
            sign = -1
            continue
        match = re.fullmatch(r"([A-Za-z]+)(?:\^|\*\*)?(-?\d+)?", token)
        if not match or match.group(1) not in _SYMBOLS:
            raise ValueError(f"products: cannot read the unit {unit!r} (symbols: "
                             f"{sorted(_SYMBOLS)}, 'dimensionless', '%')")
        scale, dim = _SYMBOLS[match.group(1)]
        power = sign * int(match.group(2) or 1)
        magnitude *= scale ** power
        dims[dim] = dims.get(dim, 0) + power
        sign = 1 if sign == -1 else sign
    return magnitude, {dim: power for dim, power in dims.items() if power}


def _words(camel):
    """PySDM/impl/camel_case.py: "ParticleConcentration" -> "particle concentration" """
    return re.sub(r"(?<!^)(?=[A-Z])", " ", camel).lower()


class Product:
    """a named quantity with a unit; subclasses state `requests`, optionally `spectrum`, and
    `_impl(formulae, rows)` in base SI units"""
    default_unit = "dimensionless"

    def __init__(self, *, unit, name=None):
        self.name = name or _words(type(self).__name__)
        self.unit = unit
        self.unit_magnitude_in_base_units, dims = _parse_unit(unit)
        if dims != _parse_unit(self.default_unit)[1]:
            raise AssertionError(f"provided unit ({unit}) has a different dimensionality than the "
                                 f"default one ({self.default_unit}) for product "
                                 f"{type(self).__name__}")

    def requests(self, formulae):  # pylint: disable=unused-argument
        return ()

    def spectrum(self, formulae):  # pylint: disable=unused-argument
        return None

    def _impl(self, formulae, rows):
        raise NotImplementedError

    def get(self, formulae, rows):
        """the product's values for evaluated rows (`Rows`), in the product's unit"""
        return self._impl(formulae, rows) / self.unit_magnitude_in_base_units


def _volume(const, radius):  # trivia.volume
    return const.PI_4_3 * np.power(np.asarray(radius, dtype=float), const.THREE)


def _radius(const, volume):  # trivia.radius
    return np.power(np.asarray(volume, dtype=float) / const.PI_4_3, const.ONE_THIRD)


def _radius_to_mass(const, radius):  # LiquidSpheres.radius_to_mass
    return const.rho_w * const.PI_4_3 * np.power(np.asarray(radius, dtype=float), const.THREE)


def _rho_stp(const):
    return getattr(const, "rho_STP", None) or const.p_STP / const.Rd / const.T_STP


def _buffer(rows, request):
    """what MomentProduct._download_moment_to_buffer leaves in the buffer"""
    return rows.moment_0(request) if request.rank == 0 else rows.moments(request)


def _check_ctor_arguments(specific, stp):
    if stp and specific:
        raise ValueError("std-temperature-and-pressure precludes specific conc. option")


class _Concentration(Product):
    """ConcentrationProduct: a count divided by dv, then by rhod (specific) or rhod / rho_STP"""

    def __init__(self, *, unit, name, specific, stp):
        _check_ctor_arguments(specific, stp)
        super().__init__(unit=unit, name=name)
        self.specific, self.stp = specific, stp

    def _count(self, formulae):
        raise NotImplementedError

    def requests(self, formulae):
        return (self._count(formulae),)

    def _impl(self, formulae, rows):
        result = _buffer(rows, self._count(formulae)) / rows.dv
        if self.specific or self.stp:
            result = result / rows.rhod
            if self.stp:
                result = result * _rho_stp(formulae.constants)
        return result


class ParticleConcentration(_Concentration):
    default_unit = "m^-3"

    def __init__(self, radius_range=(0, np.inf), specific=False, stp=False, name=None,
                 unit="m^-3"):
        self.radius_range = radius_range
        super().__init__(name=name, unit=unit, specific=specific, stp=stp)

    def _count(self, formulae):
        const = formulae.constants
        lo, hi = (const.rho_w * _volume(const, r) for r in self.radius_range)
        return MomentRequest("water mass", 0, "signed water mass", float(lo), float(hi), False)


class ParticleSpecificConcentration(ParticleConcentration):
    default_unit = "kg^-1"

    def __init__(self, radius_range=(0, np.inf), name=None, unit="kg^-1"):
        super().__init__(radius_range=radius_range, specific=True, name=name, unit=unit)


class WaterMixingRatio(Product):
    def __init__(self, radius_range=None, name=None, unit="dimensionless"):
        self.radius_range = radius_range or (0, np.inf)
        super().__init__(unit=unit, name=name)

    def requests(self, formulae):
        lo, hi = _radius_to_mass(formulae.constants, self.radius_range)
        return tuple(MomentRequest("water mass", rank, "signed water mass", float(lo), float(hi),
                                   False) for rank in (0, 1))

    def _impl(self, formulae, rows):
        count, mean_mass = self.requests(formulae)
        return rows.moments(mean_mass) * rows.moment_0(count) / rows.dv / rows.rhod


class MeanRadius(Product):
    default_unit = "m"

    def __init__(self, name=None, unit="m", radius_range=(0, np.inf)):
        self.radius_range = radius_range
        super().__init__(name=name, unit=unit)

    def requests(self, formulae):
        lo, hi = (_radius_to_mass(formulae.constants, r) for r in self.radius_range)
        return (MomentRequest("volume", 1 / 3, "signed water mass", float(lo), float(hi), False),)

    def _impl(self, formulae, rows):
        return rows.moments(self.requests(formulae)[0]) / formulae.constants.PI_4_3 ** (1 / 3)


def _effective_radius(const, volume, volume_2_3):
    """EffectiveRadius.nan_aware_reff_impl: <r^3> / <r^2> from <v> and <v^(2/3)>"""
    geom_factor = const.PI_4_3 ** (-1 / 3)
    return np.where(volume_2_3 > 0, volume * geom_factor / (volume_2_3 + (volume_2_3 == 0)),
                    np.nan)


class EffectiveRadius(Product):
    default_unit = "m"

    def __init__(self, *, radius_range=None, unit="m", name=None):
        super().__init__(name=name, unit=unit)
        self.radius_range = radius_range or (0, np.inf)

    def requests(self, formulae):
        lo, hi = _volume(formulae.constants, self.radius_range)
        return tuple(MomentRequest("volume", rank, "volume", float(lo), float(hi), False)
                     for rank in (2 / 3, 1))

    def _impl(self, formulae, rows):
        volume_2_3, volume = (rows.moments(r) for r in self.requests(formulae))
        return _effective_radius(formulae.constants, volume, volume_2_3)


def _activation_range(count_unactivated, count_activated):
    """ActivationFilteredProduct: the range of the wet to critical volume ratio"""
    return (0.0 if count_unactivated else 1.0, np.inf if count_activated else 1.0)


def _activation_request(self, rank):
    return MomentRequest("volume", rank, "wet to critical volume ratio",
                         *_activation_range(self.count_unactivated, self.count_activated), False)


class ActivatedParticleConcentration(_Concentration):
    default_unit = "m^-3"

    def __init__(self, *, count_unactivated, count_activated, specific=False, stp=False,
                 name=None, unit="m^-3"):
        super().__init__(name=name, unit=unit, specific=specific, stp=stp)
        self.count_unactivated, self.count_activated = count_unactivated, count_activated

    def _count(self, formulae):
        return _activation_request(self, 0)


class ActivatedParticleSpecificConcentration(ActivatedParticleConcentration):
    default_unit = "kg^-1"

    def __init__(self, count_unactivated, count_activated, name=None, unit="kg^-1"):
        super().__init__(count_unactivated=count_unactivated, count_activated=count_activated,
                         specific=True, name=name, unit=unit)


class ActivatedMeanRadius(Product):
    default_unit = "m"

    def __init__(self, count_unactivated, count_activated, name=None, unit="m"):
        super().__init__(name=name, unit=unit)
        self.count_unactivated, self.count_activated = count_unactivated, count_activated

    def requests(self, formulae):
        return (_activation_request(self, 1 / 3),)

    def _impl(self, formulae, rows):
        return rows.moments(self.requests(formulae)[0]) / formulae.constants.PI_4_3 ** (1 / 3)


class ActivatedEffectiveRadius(Product):
    default_unit = "m"

    def __init__(self, *, count_unactivated, count_activated, name=None, unit="m"):
        super().__init__(name=name, unit=unit)
        self.count_unactivated, self.count_activated = count_unactivated, count_activated

    def requests(self, formulae):
        return (_activation_request(self, 2 / 3), _activation_request(self, 1))

    def _impl(self, formulae, rows):
        volume_2_3, volume = (rows.moments(r) for r in self.requests(formulae))
        return _effective_radius(formulae.constants, volume, volume_2_3)


class _ParticleSizeSpectrum(Product):
    """ParticleSizeSpectrum: counts per bin of the (dry) volume, per dv and per width in radius"""

    def __init__(self, *, stp, radius_bins_edges, name, unit, dry=False, specific=False):
        _check_ctor_arguments(specific, stp)
        self.volume_attr = "dry volume" if dry else "volume"
        self.radius_bins_edges = np.asarray(radius_bins_edges, dtype=float)
        self.specific, self.stp = specific, stp
        super().__init__(name=name, unit=unit)

    def spectrum(self, formulae):
        edges = _volume(formulae.constants, self.radius_bins_edges)
        return SpectrumRequest(self.volume_attr, tuple(float(e) for e in edges))

    def _impl(self, formulae, rows):
        const = formulae.constants
        edges = np.asarray(self.spectrum(formulae).edges)
        vals = rows.spectrum / rows.dv[..., None]
        vals = vals / (_radius(const, edges[1:]) - _radius(const, edges[:-1]))
        if self.specific or self.stp:
            vals = vals / rows.rhod[..., None]
            if self.stp:
                vals = vals * _rho_stp(const)
        return vals


class ParticleSizeSpectrumPerMassOfDryAir(_ParticleSizeSpectrum):
    default_unit = "kg^-1 m^-1"

    def __init__(self, *, radius_bins_edges, dry=False, name=None, unit="kg^-1 m^-1"):
        super().__init__(radius_bins_edges=radius_bins_edges, dry=dry, specific=True, name=name,
                         unit=unit, stp=False)


class ParticleSizeSpectrumPerVolume(_ParticleSizeSpectrum):
    default_unit = "m^-3 m^-1"

    def __init__(self, *, radius_bins_edges, dry=False, name=None, unit="m^-3 m^-1", stp=False):
        super().__init__(radius_bins_edges=radius_bins_edges, dry=dry, specific=False, name=name,
                         unit=unit, stp=stp)


class Rows:
    """evaluated rows of a request table: arrays of a common leading shape (steps x parcels, or
    parcels), `moment_0 / moments` with one more axis over the table's moment requests,
    `spectrum` over its bins; `dv` and `rhod` of the leading shape"""

    def __init__(self, table, *, moment_0, moments, spectrum, dv, rhod):
        self.table = table
        self._moment_0, self._moments, self.spectrum = moment_0, moments, spectrum
        self.dv, self.rhod = np.asarray(dv, dtype=float), np.asarray(rhod, dtype=float)

    @property
    def moment_0_all(self):
        return self._moment_0

    @property
    def moments_all(self):
        return self._moments

    def moment_0(self, request):
        return self._moment_0[..., self.table.index[request]]

    def moments(self, request):
        return self._moments[..., self.table.index[request]]


class RequestTable:
    """the products of a run compiled into one abi.ParcelRequests: identical moment requests
    share an entry, all spectrum products must ask for the same bins"""

    def __init__(self, products, formulae):
        self.products, self.formulae = tuple(products), formulae
        names = [product.name for product in self.products]
        if len(set(names)) != len(names):
            raise ValueError(f"products: names must be unique, got {names}")
        self.index, self.spectrum = {}, None
        for product in self.products:
            for request in product.requests(formulae):
                self.index.setdefault(request, len(self.index))
            wanted = product.spectrum(formulae)
            if wanted is not None:
                if self.spectrum not in (None, wanted):
                    raise NotImplementedError(
                        "products: one size spectrum per run (the same attribute and bin edges "
                        "in every spectrum product)")
                self.spectrum = wanted
        if len(self.index) > abi.PARCEL_MAX_MOMENTS:
            raise NotImplementedError(f"products: {len(self.index)} distinct moment requests, the "
                                      f"table holds {abi.PARCEL_MAX_MOMENTS}")
        self.n_moments = len(self.index)
        self.n_bins = 0 if self.spectrum is None else len(self.spectrum.edges) - 1
        if self.n_bins > abi.PARCEL_MAX_BINS:
            raise NotImplementedError(f"products: {self.n_bins} bins, the table holds "
                                      f"{abi.PARCEL_MAX_BINS}")

    @classmethod
    def from_requests(cls, moments, spectrum, formulae):
        """a table of raw requests without products (its `values` are empty: read the evaluated
        `Rows`)"""
        table = cls((), formulae)
        table.index = {request: at for at, request in enumerate(moments)}
        if len(table.index) != len(moments):
            raise ValueError("products: raw moment requests must differ")
        table.spectrum = spectrum
        table.n_moments = len(moments)
        table.n_bins = 0 if spectrum is None else len(spectrum.edges) - 1
        return table

    def c_struct(self):
        return requests_struct(list(self.index), self.spectrum)

    def values(self, rows):
        """{product name: array} for evaluated rows"""
        return {product.name: product.get(self.formulae, rows) for product in self.products}


def requests_struct(moments, spectrum=None):
    """abi.ParcelRequests of MomentRequest tuples and an optional SpectrumRequest; the counts are
    passed on as given (the library refuses what the table cannot hold)"""
    out = abi.ParcelRequests()
    out.n_moments = len(moments)
    for slot, request in zip(out.moment, moments):
        slot.attr = abi.PARCEL_ATTRS.get(request.attr, -1) if isinstance(request.attr, str) \
            else int(request.attr)
        slot.filter_attr = abi.PARCEL_FILTERS.get(request.filter_attr, -1) \
            if isinstance(request.filter_attr, str) else int(request.filter_attr)
        slot.rank, slot.min_x, slot.max_x = (float(request.rank), float(request.min_x),
                                             float(request.max_x))
        slot.skip_division_by_m0 = int(bool(request.skip))
    if spectrum is not None:
        out.n_bins = len(spectrum.edges) - 1
        out.bin_attr = abi.PARCEL_FILTERS.get(spectrum.bin_attr, -1) \
            if isinstance(spectrum.bin_attr, str) else int(spectrum.bin_attr)
        for at, edge in enumerate(spectrum.edges[:abi.PARCEL_MAX_BINS + 1]):
            out.edges[at] = float(edge)
    return out
