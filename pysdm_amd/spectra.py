"""Initial size spectra of the box set-ups and their deterministic sampling into super-droplets.

`Exponential(norm_factor, scale)`: n(x) = norm_factor / scale * exp(-x / scale), in closed form
(what the reference evaluates through scipy.stats.expon, PySDM/initialisation/spectra/
exponential.py:11-13).  Samplers return (x at the odd nodes of a 2 n_sd + 1 node grid, number of
real droplets between the even nodes), the construction of PySDM/initialisation/sampling/
spectral_sampling.py:45-108:
  * `sample_constant_multiplicity`: nodes equidistant in the cumulative distribution, so every
    super-droplet stands for (nearly) the same number of droplets - Shima et al. 2009;
  * `sample_logarithmic`: nodes equidistant in log10(x) - used for the rain spectrum.
`Lognormal(norm_factor, m_mode, s_geom)` (m_mode the median, s_geom the geometric standard
deviation: what the reference evaluates through scipy.stats.lognorm, PySDM/initialisation/spectra/
lognormal.py:13-18) and `Sum(spectra)` (spectra/sum.py: percentiles by linear interpolation of its
own cumulative on the percentile grids of its terms) are the dry-aerosol spectra of
pysdm_amd.initialisation; the samplers take them as they take `Exponential`.
The default range cuts the spectrum at the 1e-5 and 1 - 1e-5 quantiles.  The samples are inputs
that full-size parity digests depend on bit for bit (tests/golden/digest_*.npz pin them).
"""
import math

import numpy as np
from scipy import special

CDF_RANGE = (0.00001, 0.99999)


class Exponential:
    def __init__(self, norm_factor, scale):
        self.norm_factor = norm_factor
        self.scale = scale

    def cumulative(self, x):
        # scipy.special (not numpy): scipy.stats.expon evaluates its cdf / ppf with these very
        # functions, and numpy's expm1 / log1p round differently in the last bit
        return self.norm_factor * -special.expm1(-(np.asarray(x) / self.scale))

    def percentiles(self, quantiles):
        return -special.log1p(-np.asarray(quantiles)) * self.scale


class Lognormal:
    def __init__(self, norm_factor, m_mode, s_geom):
        self.norm_factor = norm_factor
        self.m_mode = m_mode
        self.s_geom = s_geom
        self._s = math.log(s_geom)

    def cumulative(self, x):
        # scipy.stats.lognorm: ndtr(log((x - 0) / scale) / s) inside the support, 0 at x <= 0
        y = (np.asarray(x, dtype=float) - 0) / self.m_mode
        with np.errstate(divide="ignore", invalid="ignore"):
            cdf = np.where(y > 0, special.ndtr(np.log(y) / self._s), 0.0)
        return self.norm_factor * cdf

    def percentiles(self, quantiles):
        return np.exp(self._s * special.ndtri(np.asarray(quantiles, dtype=float))) * self.m_mode + 0


class Sum:
    """a sum of spectra; `interpolation_grid`: the quantiles of each term at which the inverse of
    the cumulative is tabulated (999 between the ends of CDF_RANGE unless given)"""

    def __init__(self, spectra, interpolation_grid=None):
        grid = (np.linspace(*CDF_RANGE, 999) if interpolation_grid is None
                else np.asarray(interpolation_grid, dtype=float))
        self.spectra = tuple(spectra)
        self.norm_factor = sum(s.norm_factor for s in self.spectra)
        arg = np.zeros(len(grid) * len(self.spectra) + 1)
        arg[1:] = np.concatenate([s.percentiles(grid) for s in self.spectra])
        cdf = self.cumulative(arg) / self.norm_factor
        order = np.argsort(cdf, kind="mergesort")  # (scipy.interpolate.interp1d sorts its x so)
        self._cdf, self._arg = cdf[order], arg[order]

    def cumulative(self, x):
        result = 0.0
        for spectrum in self.spectra:
            result = result + spectrum.cumulative(x)
        return result

    def percentiles(self, quantiles):
        # interp1d(kind="linear"): slope * (x_new - x_lo) + y_lo; outside the table it raises
        q = np.asarray(quantiles, dtype=float)
        if np.any(q < self._cdf[0]) or np.any(q > self._cdf[-1]):
            raise ValueError("a quantile outside the interpolation range of the Sum")
        hi = np.searchsorted(self._cdf, q).clip(1, len(self._cdf) - 1).astype(int)
        lo = hi - 1
        slope = (self._arg[hi] - self._arg[lo]) / (self._cdf[hi] - self._cdf[lo])
        return slope * (q - self._cdf[lo]) + self._arg[lo]


def _between_even_nodes(spectrum, grid, tolerance):
    x = grid[1:-1:2]
    cdf = spectrum.cumulative(grid[0::2])
    counts = cdf[1:] - cdf[:-1]
    lost = abs(1 - np.sum(counts) / spectrum.norm_factor)
    if lost > tolerance:
        raise ValueError(f"{lost * 100:.3g}% error in total real-droplet number due to sampling "
                         f"({len(x)} samples)")
    return x, counts


def sample_constant_multiplicity(spectrum, n_sd, size_range=None, tolerance=0.01):
    lo, hi = size_range or spectrum.percentiles(CDF_RANGE)
    cdf_lo, cdf_hi = spectrum.cumulative(lo), spectrum.cumulative(hi)
    if not 0 < cdf_lo < cdf_hi:
        raise ValueError("empty size range")
    quantiles = np.linspace(cdf_lo, cdf_hi, num=2 * n_sd + 1)
    quantiles /= spectrum.norm_factor
    grid = spectrum.percentiles(quantiles)
    if not np.isfinite(grid).all():
        raise ValueError("non-finite percentile")
    return _between_even_nodes(spectrum, grid, tolerance)


def sample_logarithmic(spectrum, n_sd, size_range=None, tolerance=0.01):
    lo, hi = size_range or spectrum.percentiles(CDF_RANGE)
    grid = np.logspace(np.log10(lo), np.log10(hi), num=2 * n_sd + 1)
    return _between_even_nodes(spectrum, grid, tolerance)
