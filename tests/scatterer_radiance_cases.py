"""What tests/test_scatterer_radiance_host.py (CPU), tests/test_gpu_scatterer_radiance_shapes.py and
tests/test_gpu_scatterer_radiance.py (GPU) share: the definition of
Spectroscopy.compute_thermal_radiance_spectral and compute_solar_radiance_spectral in numpy
(include/lbl_amd_scatterer_radiance.h) -- the per-element level tables of tests/scatterer_cases.py
(longwave_table, shortwave_table: where a grid point lies among the knots, the interpolation and its
limit, in float64 as the kernels form them) handed to the level functions of
tests/thermal_radiance_cases.py and tests/solar_radiance_cases.py, for float64 "as written" and
numpy.longdouble as the reference --, a stand-in engine with the two new calls, and the case
tables.  Nothing of the layers or of the view's levels is written again here.

What the view adds to the flux calls' definition:
    longwave:  a level that scatters at no knot is clear with tau_c(nu) and reads no flux row; in
               any other level every element takes the cloudy lines with its own tau_c, w_c, f, gp
               and a = (3*(gp*mu))/2; tau == 0 takes the clear line
    shortwave: tau_c, w_c, h_c and PH per element, gc = h_c/w_c (0 where w_c == 0) limited to
               1 - 2^-53; without a Rayleigh row a level that scatters at no knot only attenuates

scale is thermal_radiance_cases' and solar_radiance_cases'.  E_CPU_THERMAL and E_CPU_SOLAR are the
worst |float64 mirror - long-double mirror|/scale over every case table of this file, as
tests/test_scatterer_radiance_host.py measures them; the GPU tests hold every radiance to
(4*E_CPU + FLOOR)*scale of the long-double mirror."""
import contextlib

import numpy as np

from tests import scatterer_cases as sc
from tests import solar_radiance_cases as src
from tests import surface_cases as surface
from tests import sweep_cases as cases
from tests import thermal_cases as tc
from tests import thermal_radiance_cases as trc
from tests import two_stream_cases as ts

F64, LD = np.float64, np.longdouble
PATHS = cases.PATHS
MAX_KNOTS = sc.MAX_KNOTS
MAX_ASYMMETRY = 1. - 2.**-53        # kSolarViewMaxAsymmetry
SPECTRAL_METHOD = {"compute_thermal_radiance": "compute_thermal_radiance_spectral",
                   "compute_solar_radiance": "compute_solar_radiance_spectral"}
MU = np.array(trc.MU)               # (1, 0.6, 0.05)
PHI = np.array(src.PHI)
GUARDED_MU = np.array([0.9, 0.5, 0.05])     # none of two_stream_cases.RESONANCE_MU0
# The worst errors of the float64 mirrors over the case tables (see above):
# tests/test_scatterer_radiance_host.py measures 1.09e-11 (longwave: the 1031 x 1 table with two
# knots, in the general branch just above the conservative threshold, as in
# thermal_radiance_cases) and 8.3e-12 (shortwave: the 1031 x 2 table with 1024 knots).
E_CPU_THERMAL = 1.1e-11
E_CPU_SOLAR = 8.4e-12
E_CPU_CAP = 1e-10           # thermal_radiance_cases.E_CPU_CAP and solar_radiance_cases.E_CPU_CAP
FLOOR = 1e-13
# How far, relative to its threshold, every branch decision of the case tables stays from it (the
# conservative criterion, the guard's edge and its centre, the series of linear_weight and y = 0
# unless y is 0 exactly): the float64 mirror's roundings are nine orders of magnitude smaller, so
# the long-double mirror would decide every element alike.
DECISION_MARGIN = 1e-6


# ---------------------------------------------------------------------------------------------
# The longwave mirror: thermal_radiance_cases' on the per-element table.
def thermal_flux_rows(inputs, from_last):
    """The float64 flux rows lbl_path_thermal_two_stream_spectral writes for a
    scatterer_cases.Longwave (the source of the level temperatures): {"up", "down"}."""
    return trc.flux_rows(inputs.isothermal(), from_last)


def thermal_mirror(kind, inputs, mu, from_last, fluxes=None):
    """thermal_radiance_cases.mirror's dict of lbl_path_thermal_radiance_spectral on a
    scatterer_cases.Longwave."""
    if fluxes is None:
        fluxes = thermal_flux_rows(inputs, from_last)
    return trc.mirror(kind, inputs.isothermal(), mu, from_last, fluxes)


def thermal_worst_error(inputs, mu, from_last):
    return trc.worst_error(inputs.isothermal(), mu, from_last)


# ---------------------------------------------------------------------------------------------
# The shortwave mirror: solar_radiance_cases' levels on the per-element table.
def solar_view_inputs(inputs, from_last):
    """solar_radiance_cases.view_inputs of every element of a scatterer_cases.Shortwave: arrays
    [L, PATHS, columns] in the Sun's order, gc limited as the kernel limits it."""
    order = inputs.sun_order(from_last).T
    table = sc.shortwave_table(inputs.table, inputs.knots, inputs.optics, inputs.nu)
    li = src.view_inputs(table[order], inputs.mu0[None, :, None], inputs.beta[order],
                         inputs.sigma[None, None, :])
    li["gc"] = np.minimum(li["gc"], MAX_ASYMMETRY)
    return li


def solar_flux_rows(inputs, from_last):
    """The float64 flux rows lbl_path_two_stream_spectral writes for a scatterer_cases.Shortwave:
    {"up", "direct", "diffuse"}."""
    return src.flux_rows(inputs, from_last)


def solar_mirror(kind, inputs, mu, cos_theta, from_last, fluxes=None):
    """solar_radiance_cases.mirror's dict of lbl_path_solar_radiance_spectral on a
    scatterer_cases.Shortwave: its loop over its level(), with the elements' own scatterer."""
    if fluxes is None:
        fluxes = solar_flux_rows(inputs, from_last)
    mu = np.asarray(mu, dtype=F64)[:, None]
    cos_theta = np.asarray(cos_theta, dtype=F64)[:, None]
    order = inputs.sun_order(from_last)
    li = solar_view_inputs(inputs, from_last)
    albedo = inputs.albedo[:, None] if inputs.albedo.ndim == 1 else inputs.albedo
    albedo = np.asarray(albedo, dtype=F64).astype(kind)
    pi = kind(cases.FLUX_PI)
    f0 = inputs.f0()
    last = order[:, -1]
    rad = albedo*((fluxes["direct"][last].astype(kind) + fluxes["diffuse"][last].astype(kind))/pi)
    peak = np.abs(rad)
    for i in range(inputs.levels_per_path - 1, -1, -1):
        here = {name: value[i] for name, value in li.items()}
        direct0 = fluxes["direct"][order[:, i - 1]] if i > 0 else f0
        diffuse0 = fluxes["diffuse"][order[:, i - 1]] if i > 0 else np.zeros_like(f0)
        rad = src.level(kind, here, mu, cos_theta, fluxes["up"][order[:, i]], direct0, diffuse0,
                        rad)
        peak = np.maximum(peak, np.abs(rad))
    return {"radiance": rad, "peak": peak}


def solar_worst_error(inputs, mu, cos_theta, from_last):
    """solar_radiance_cases.worst_error with the mirror above."""
    fluxes = solar_flux_rows(inputs, from_last)
    low = solar_mirror(F64, inputs, mu, cos_theta, from_last, fluxes)
    high = solar_mirror(LD, inputs, mu, cos_theta, from_last, fluxes)
    size = src.scale(inputs, high)
    finite = bool(np.all(np.isfinite(low["radiance"])) and np.all(np.isfinite(high["radiance"])))
    error = np.abs(low["radiance"].astype(LD) - high["radiance"])
    dark = size == 0.
    assert np.all(error[dark] == 0.)
    worst = float(np.max(error[~dark]/size[~dark])) if np.any(~dark) else 0.
    return worst, finite


# ---------------------------------------------------------------------------------------------
# How far the decisions of a problem stay from their thresholds.
def _distance(value, threshold):
    """The smallest |value - threshold|/threshold over the finite values."""
    value = np.asarray(value, dtype=F64)
    value = value[np.isfinite(value)]
    return float(np.min(np.abs(value - threshold)/threshold)) if value.size else np.inf


def thermal_margin(inputs, mu, from_last):
    """The smallest relative distance of a decision of the longwave view from its threshold."""
    li = inputs.layer_inputs(from_last)
    cloudy = li["branch"] != tc.CLEAR
    if not np.any(cloudy):
        return np.inf
    mu = np.asarray(mu, dtype=F64)[None, :, None]
    _, _, y = trc.decisions(li, mu)
    with np.errstate(all="ignore"):
        criterion = li["k2"]*(1. + li["t"]*li["t"])
        z = np.broadcast_to(li["t"]/mu, cloudy.shape)
        # y = ((1 - k*mu)*t)/mu changes sign where k*mu = 1.
        _, _, k, _ = trc.scalars(F64, li)
        pole = np.where(y == 0., 2., k*mu)
    return min(_distance(criterion[cloudy], tc.CONSERVATIVE),
               _distance(np.abs(z[cloudy]), trc.LINEAR_SERIES_BELOW), _distance(pole[cloudy], 1.))


def solar_margin(inputs, mu, from_last):
    """The same of the shortwave view: also the guard's two edges."""
    li = solar_view_inputs(inputs, from_last)
    scattering = ~np.isin(li["branch"], (ts.IDENTITY, src.NO_SCATTERING))
    if not np.any(scattering):
        return np.inf
    mu = np.asarray(mu, dtype=F64)[None, :, None]
    k = src.scalars(F64, li)["k"]
    general = scattering & (li["branch"] != ts.CONSERVATIVE_BRANCH)
    with np.errstate(all="ignore"):
        criterion = li["k2"]*(1. + li["t"]*li["t"])
        z = np.broadcast_to(li["t"]/mu, scattering.shape)
        y = ((1. - k*mu)*li["t"])/mu
        pole = np.where(y == 0., 2., k*mu)
        edge = np.abs(1. - li["x"])
    out = min(_distance(criterion[scattering], ts.CONSERVATIVE),
              _distance(np.abs(z[scattering]), trc.LINEAR_SERIES_BELOW))
    if np.any(general):
        out = min(out, _distance(pole[general], 1.), _distance(edge[general], ts.RESONANCE))
    return out


# ---------------------------------------------------------------------------------------------
# The case tables.
COLUMNS = (1, 3, 512, 513, 1031)    # a lane holds 2 columns and a block 512
DEPTHS = (1, 2, 9)
KNOT_COUNTS = (2, 3, MAX_KNOTS)
# (columns, levels per path, M, seed, descending grid, from_last)
SHAPES = ((1, 2, 2, 1, False, True), (3, 9, 3, 2, False, False),
          (512, 1, MAX_KNOTS, 3, False, True), (513, 9, 2, 4, False, True),
          (513, 2, MAX_KNOTS, 5, True, False), (1031, 9, 3, 6, False, False),
          (1031, 1, 2, 7, True, True), (1031, 2, MAX_KNOTS, 8, False, False))


def one_cloud(inputs):
    """`inputs` with a scatterer in one level of each path only, the second where there is one:
    clear and cloudy levels alternate along the sweep."""
    n = inputs.levels_per_path
    keep = np.arange(inputs.levels) % n == min(1, n - 1)
    inputs.optics[~keep] = 0.
    inputs.optics[keep, :, 0] = np.maximum(inputs.optics[keep, :, 0], 0.05)
    inputs.optics[keep, :, 1] = np.maximum(inputs.optics[keep, :, 1], 0.3)
    inputs.name += ", one cloud"
    return inputs


def without_rayleigh(inputs):
    """A shortwave problem without a Rayleigh row: sigma is 0 in the mirror and the entry gets
    none."""
    inputs.sigma = np.zeros_like(inputs.sigma)
    inputs.rayleigh = False
    inputs.name += ", no Rayleigh row"
    return inputs


def guarded():
    """two_stream_cases.resonance's columns inside the guard k*mu0 = 1 (and beside it), with its
    scatterer (tau_c = 1, omega_c = 1, g_c = 0) as a table of three knots that is flat over the
    first 30 columns and changes over the last 15."""
    base = ts.resonance()
    nu = np.linspace(100., 1000., base.columns)
    knots = np.array([50., nu[29], nu[-1] + 10.])
    optics = np.empty((base.levels, 3, 3))
    optics[:, :2] = (1., 1., 0.)
    optics[:, 2] = (3., 0.6, 0.5)
    table = base.table.copy()
    table[:, 2:] = 0.
    inputs = sc.Shortwave("guarded", nu, base.beta, table, base.mu0, base.solar, base.sigma,
                          base.albedo, knots, optics)
    return without_rayleigh(inputs)


def conservative():
    """omega_c = 1 at both knots without gas in the even columns and without a Rayleigh row: 2
    levels per path on 12 columns, tau_c from 0.3 to 5 and g_c from 0.5 to 0.8 across the grid."""
    rng = np.random.default_rng(31)
    n, columns = 2, 12
    levels = PATHS*n
    nu = np.linspace(4000., 4100., columns)
    beta = 10.**rng.uniform(-3., 0., size=(levels, columns))
    beta[:, ::2] = 0.
    table = np.stack([np.ones(levels)] + [np.zeros(levels)]*4, axis=1)
    optics = np.empty((levels, 2, 3))
    optics[:, 0], optics[:, 1] = (0.3, 1., 0.5), (5., 1., 0.8)
    inputs = sc.Shortwave("conservative", nu, beta, table, src.MU0,
                          np.linspace(0.2, 1., columns), np.zeros(columns), (0., 0.3, 1.),
                          np.array([3990., 4110.]), optics)
    return without_rayleigh(inputs)


def thermal_cases():
    """Every problem of the longwave entry: [(inputs, mu, from_last)]."""
    out = [(sc.longwave_inputs(columns, depth, m, 300 + seed, descending,
                               emissivity_rows=seed % 2 == 0), MU, from_last)
           for columns, depth, m, seed, descending, from_last in SHAPES]
    out += [(sc.longwave_to_zero(), MU, from_last) for from_last in (False, True)]
    out += [(one_cloud(sc.longwave_inputs(131, 9, 3, 340)), MU, from_last)
            for from_last in (False, True)]
    return out


def solar_cases():
    """Every problem of the shortwave entry: [(inputs, mu, phi, from_last)]; inputs.rayleigh says
    whether the entry gets a Rayleigh row."""
    out = []
    for index, (columns, depth, m, seed, descending, from_last) in enumerate(SHAPES):
        inputs = sc.shortwave_inputs(columns, depth, m, 400 + seed, descending,
                                     albedo_rows=seed % 2 == 0)
        inputs.mu0 = np.array(src.MU0)
        inputs.rayleigh = True
        if index % 3 == 2:
            without_rayleigh(inputs)
        out.append((inputs, MU, PHI, from_last))
    for from_last in (False, True):
        inputs = sc.shortwave_to_zero()
        inputs.mu0, inputs.rayleigh = np.array(src.MU0), True
        out.append((inputs, MU, PHI, from_last))
        inputs = one_cloud(sc.shortwave_inputs(131, 9, 3, 440))
        inputs.mu0, inputs.rayleigh = np.array(src.MU0), from_last
        if not from_last:
            without_rayleigh(inputs)
        out.append((inputs, np.roll(MU, 1), np.roll(PHI, -1), from_last))
        # (k*mu0 = 1 in the guard: another mu than mu0 keeps k*mu away from the pole of h.)
        out.append((guarded(), GUARDED_MU, PHI, from_last))
        out.append((conservative(), MU, PHI, from_last))
    return out


# ---------------------------------------------------------------------------------------------
# The queue of a call on a stand-in engine.
class ScattererRadianceRecorder(sc.ScattererRecorder, trc.RadianceRecorder,
                                src.SolarRadianceRecorder):
    """The engines of tests/scatterer_cases.py, tests/thermal_radiance_cases.py and
    tests/solar_radiance_cases.py in one, with the two spectral radiance calls."""
    def path_thermal_radiance_spectral(self, beta, columns, grid, n_paths, levels_per_path,
                                       level_begin, level_table, knot_wavenumber, knot_optics,
                                       view_cosine, surface_temperature, **keywords):
        self.view_tables = getattr(self, "view_tables", [])
        self.view_tables.append((int(level_begin), np.array(knot_wavenumber),
                                 np.array(knot_optics)))
        self.record("path_thermal_radiance_spectral", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    knot_wavenumber=np.asarray(knot_wavenumber),
                    knot_optics=np.asarray(knot_optics), view_cosine=np.asarray(view_cosine),
                    surface_temperature=np.asarray(surface_temperature),
                    **self._described(keywords))

    def path_solar_radiance_spectral(self, beta, columns, grid, n_paths, levels_per_path,
                                     level_begin, level_table, knot_wavenumber, knot_optics,
                                     solar_zenith_cosine, view_cosine, scattering_cosine,
                                     solar_row, **keywords):
        self.view_tables = getattr(self, "view_tables", [])
        self.view_tables.append((int(level_begin), np.array(knot_wavenumber),
                                 np.array(knot_optics)))
        self.record("path_solar_radiance_spectral", beta=beta, columns=columns, grid=grid,
                    n_paths=n_paths, levels_per_path=levels_per_path, level_begin=level_begin,
                    level_table=np.asarray(level_table),
                    knot_wavenumber=np.asarray(knot_wavenumber),
                    knot_optics=np.asarray(knot_optics),
                    solar_zenith_cosine=np.asarray(solar_zenith_cosine),
                    view_cosine=np.asarray(view_cosine),
                    scattering_cosine=np.asarray(scattering_cosine), solar_row=solar_row,
                    **self._described(keywords))


@contextlib.contextmanager
def recorded(directory, recorder=ScattererRadianceRecorder):
    """surface_cases.recorded with `recorder`."""
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = recorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before

