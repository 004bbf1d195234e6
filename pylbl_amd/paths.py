"""The path products of Spectroscopy -- compute_path, compute_radiance, compute_flux,
compute_jacobian, compute_solar and the per-level compute_kdistribution -- on the host: their
quantities and units, the checks of their arguments (one request per call, made before anything
touches the GPU), the run loop that sweeps the "total" absorption block of a run of levels at a
time (_sweep_runs), the HBM accounting behind its run cuts (_level_bytes), what the sweepers of
several products share (_FilledOnce, _Rows, _first_rows) and the assembly of the results.  The
two-stream products build on these in two_stream.py; their public constants are here.  The
sweeps themselves are the kernels of csrc/path.h behind Engine.path_*; the "total" block is
queued by Spectroscopy.total_into (absorption.py, whose pipeline guard the run loop shares).
"""
from collections import namedtuple

import numpy as np

from .absorption import _Levels, pipeline, present_gases
from .synthetic import grid_arguments

# Levels of one run at most: what one call of the continuum group kernels takes
# (lbl_continuum_compute_many), so that atmospheres of any size can be integrated.
_MAX_RUN_LEVELS = 65535

PATH_QUANTITIES = ("optical_depth", "transmittance")
PATH_CUMULATIVE = (None, "from_first", "from_last")
RADIANCE_QUANTITIES = ("radiance", "brightness_temperature")
RADIANCE_DIRECTIONS = ("toward_last", "toward_first")
# compute_radiance with reflection_path_length: D, the radiance that arrives at the boundary.
DOWNWELLING = "boundary_downwelling_radiance"
SURFACE_RADIANCE_QUANTITIES = RADIANCE_QUANTITIES + (DOWNWELLING,)
MAX_EMISSIVITY_KNOTS = 1024             # kSurfaceMaxKnots of csrc/surface.h
MAX_SCATTERER_KNOTS = 1024              # kScattererMaxKnots of csrc/scatterer.h

# Planck's function per wavenumber, B(nu, T) = C1 nu^3 / expm1(C2 nu / T) [W m-2 sr-1 (cm-1)-1]
# for nu in cm-1: from the exact CODATA 2018 h, c and k (the same literals as LBL_PLANCK_C1 and
# LBL_PLANCK_C2 in include/lbl_amd.h).
PLANCK_C1 = 1.1910429723971885e-08     # 2 h c^2 1e8 [W m-2 sr-1 (cm-1)-4]
PLANCK_C2 = 1.4387768775039338         # h c / k 1e2 [cm K]
# Dry air for heating rates: R_d = R/M_d from the CODATA 2018 molar gas constant and the molar
# mass of dry air, and c_p = (7/2) R_d of an ideal diatomic gas.
R_DRY = 8.314462618/0.0289644          # [J kg-1 K-1]
CP_DRY = 3.5*R_DRY                     # [J kg-1 K-1]

# compute_jacobian: the radiance and its derivatives, per level and per path.
JACOBIAN_LEVEL_QUANTITIES = ("optical_depth_jacobian", "log_optical_depth_jacobian",
                             "temperature_jacobian")
JACOBIAN_PATH_QUANTITIES = ("radiance", "boundary_temperature_jacobian",
                            "boundary_emissivity_jacobian")
JACOBIAN_QUANTITIES = ("radiance",) + JACOBIAN_LEVEL_QUANTITIES + JACOBIAN_PATH_QUANTITIES[1:]

# The source inside a level of compute_radiance and compute_flux: B(T_level) throughout, or
# linear in optical depth between the Planck values at the level's two interfaces.
SOURCES = ("isothermal", "linear_in_tau")

FLUX_QUANTITIES = ("upward_flux", "downward_flux", "heating_rate")
FLUX_SURFACES = ("first", "last")
MAX_FLUX_ANGLES = 8

# compute_solar: the Sun as a blackbody of SOLAR_TEMPERATURE that fills SOLAR_SOLID_ANGLE =
# pi*(6.957e8/1.495978707e11)**2 sr at 1 au (the IAU 2015 nominal solar radius and the au),
# evaluated once in fp64: the same literals as LBL_SOLAR_TEMPERATURE and LBL_SOLAR_SOLID_ANGLE in
# include/lbl_amd.h.
SOLAR_TEMPERATURE = 5772.               # [K]
SOLAR_SOLID_ANGLE = 6.794273971369406e-05   # [sr]
MAX_SOLAR_KNOTS = 1 << 22               # kSolarMaxKnots of csrc/solar.h
SOLAR_QUANTITIES = ("direct_irradiance", "surface_irradiance", "reflected_radiance",
                    "heating_rate")
SOLAR_PATH_QUANTITIES = ("surface_irradiance", "reflected_radiance")
# What the sweep writes for the paths it starts beside the interface rows: F0 at the space end.
_SPACE = "space_irradiance"

# compute_solar_flux: the two-stream shortwave fluxes.  K_B: the exact SI Boltzmann constant, for
# the air column c_l = (p_l/(K_B*T_l))*s_l of the Rayleigh optical depth.  The Bucholtz (1995) fit
# of the Rayleigh cross-section, rows (A [cm2], B, C, D) for lambda <= and > RAYLEIGH_SPLIT um: the
# same literals as kRayleighShort and kRayleighLong in csrc/twostream.h.
SOLAR_FLUX_QUANTITIES = ("upward_flux", "downward_flux", "direct_irradiance",
                         "diffuse_downward_flux", "heating_rate")
SOLAR_FLUX_INTERFACE_QUANTITIES = SOLAR_FLUX_QUANTITIES[:4]
K_B = 1.380649e-23                      # [J K-1]
RAYLEIGH_SPLIT = 0.5                    # [um]
RAYLEIGH_SHORT = (3.01577e-28, 3.55212, 1.35579, 0.11563)
RAYLEIGH_LONG = (4.01061e-28, 3.99668, 1.10298e-3, 2.71393e-2)

# compute_thermal_flux: the two-stream longwave fluxes.  The diffusivity factor D lies in
# DIFFUSIVITY_RANGE; 1.66 is Elsasser's, 2 the hemispheric mean of Toon et al. (1989).
THERMAL_FLUX_QUANTITIES = FLUX_QUANTITIES
DIFFUSIVITY = 1.66
DIFFUSIVITY_RANGE = (1., 2.)

# compute_kdistribution: per band and g interval, per band and g point, and on the grid.
KDISTRIBUTION_QUANTITIES = ("absorption_g_mean", "absorption_g_quantile", "sorted_absorption")
# ... and those that need compute_kdistribution's `weighting`; the interval sums of W and W*k
# they are formed from on the host (_create_kdistribution_dataset).
KDISTRIBUTION_WEIGHTED_QUANTITIES = ("weight_g_fraction", "absorption_g_weighted_mean",
                                     "sorted_column")
KDISTRIBUTION_WEIGHTINGS = ("planck",)
_WEIGHT_SUMS, _WEIGHTED_SUMS = "weight_sums", "weighted_sums"
MAX_G_INTERVALS = 64
# _sweep_runs: the product source that stands for the run's block of beta itself.
_BETA = "beta"

_PATH_UNITS = {"optical_depth": "1", "transmittance": "1",
               "radiance": "W m-2 sr-1 (cm-1)-1", "brightness_temperature": "K",
               DOWNWELLING: "W m-2 sr-1 (cm-1)-1",
               "optical_depth_jacobian": "W m-2 sr-1 (cm-1)-1",
               "log_optical_depth_jacobian": "W m-2 sr-1 (cm-1)-1",
               "temperature_jacobian": "W m-2 sr-1 (cm-1)-1 K-1",
               "boundary_temperature_jacobian": "W m-2 sr-1 (cm-1)-1 K-1",
               "boundary_emissivity_jacobian": "W m-2 sr-1 (cm-1)-1"}
# compute_flux, compute_solar and the two-stream flux products: on the grid (and per channel), per
# band.
_FLUX_UNITS = {"upward_flux": ("W m-2 (cm-1)-1", "W m-2"),
               "downward_flux": ("W m-2 (cm-1)-1", "W m-2"),
               "direct_irradiance": ("W m-2 (cm-1)-1", "W m-2"),
               "diffuse_downward_flux": ("W m-2 (cm-1)-1", "W m-2"),
               "surface_irradiance": ("W m-2 (cm-1)-1", "W m-2"),
               "reflected_radiance": ("W m-2 sr-1 (cm-1)-1", "W m-2 sr-1 (cm-1)-1"),
               "heating_rate": ("K day-1 (cm-1)-1", "K day-1")}

# What every product checked and derived from its arguments: flat lengths, the atmosphere's shape,
# the quantities asked for, band edges and their column starts (or None), the Instrument (or
# None), and whether the result is per level (compute_path: None, "from_first" or "from_last").
_COMMON = ("lengths", "shape", "quantities", "edges", "starts", "instrument", "cumulative")
_PathRequest = namedtuple("_PathRequest", _COMMON)
# compute_radiance's and compute_jacobian's: the sweep order and one boundary value per path;
# edge_temperature: None (isothermal levels) or the interface temperatures per flat level,
# [levels, 2] (_edge_temperatures), of the linear-in-tau source.  The surface of compute_radiance:
# emissivity_knots [M] with boundary_emissivity [paths, M] (a spectral emissivity) and
# reflection_lengths, the flat lengths of the down pass (a reflecting surface), each None where
# the call does not ask for it.
_RadianceRequest = namedtuple("_RadianceRequest", _COMMON + (
    "from_last", "boundary_temperature", "boundary_emissivity", "edge_temperature",
    "emissivity_knots", "reflection_lengths"),
    defaults=(None, None, None))
# compute_flux's: the angles and the surface of every path; edge_temperature as above.
_FluxRequest = namedtuple("_FluxRequest", _COMMON + (
    "surface", "mu", "weight", "surface_temperature", "surface_emissivity", "edge_temperature"),
    defaults=(None,))

# compute_solar's: mu0 per path, the flat solar and view lengths (view_lengths None: no viewer),
# the albedo per path -- [paths], or [paths, M] at albedo_knots [M] -- and the Sun: solar_values
# None (a blackbody of SOLAR_TEMPERATURE), [V] on the grid, or [M] at solar_knots [M]; scale: what
# multiplies it (the distance factor, for the blackbody times SOLAR_SOLID_ANGLE).
_SolarRequest = namedtuple("_SolarRequest", _COMMON + (
    "surface", "mu0", "solar_lengths", "view_lengths", "albedo", "albedo_knots", "solar_knots",
    "solar_values", "scale"))

# compute_kdistribution's (lengths: None, it is a per-level product): the g edges [Q + 1] and
# points [P], the column starts of every band's intervals [B, Q + 1] (interval_columns) and the
# quantile tables [B, P] (quantile_table).  weighting: None, "planck" or "array"; weights: the
# caller's [V] with "array"; weight_temperature: the flat [levels] T of B(nu, T) with "planck".
_KDistributionRequest = namedtuple("_KDistributionRequest", _COMMON + (
    "g_edges", "g_points", "interval_starts", "point_index", "point_fraction", "weighting",
    "weights", "weight_temperature"), defaults=(None, None, None))

# One pass of _sweep_runs over the levels: its order, and what it writes per level and per path.
_Pass = namedtuple("_Pass", ["from_last", "level_quantities", "path_quantities"])
# One returned array of _sweep_runs: host array `name` is filled from the sweeps' block `source`,
# per level or per path -- copied as it is without an instrument, reduced to channels (of
# exp(-source) with `transmittance`) by Engine.instrument_apply with one.
_Product = namedtuple("_Product", ["name", "source", "per_level", "transmittance"],
                      defaults=(False,))
# What _sweep_runs hands a sweeper: the engine, take(rows, columns=n) for blocks of its own for
# the call (carries, scratch), the layout of the paths, the columns of the grid, the flat level
# temperatures and grid(), the handle of the grid in HBM.
_Call = namedtuple("_Call", ["engine", "take", "paths", "per_path", "columns", "temperature",
                             "grid"])


def _path_layout(shape):
    """(levels per path, paths) of an atmosphere of this shape: paths run along its last axis."""
    per_path = shape[-1] if shape else 1
    return per_path, int(np.prod(shape, dtype=np.int64))//per_path


def band_columns(grid, band_edges):
    """Column starts of the bands [e_b, e_b+1) of strictly increasing, finite edges on an
    ascending grid: int64 [B + 1]; band b is the columns starts[b] <= j < starts[b + 1], i.e. the
    points with e_b <= grid[j] < e_b+1 (a band without points has starts[b] == starts[b + 1])."""
    edges = np.asarray(band_edges, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError("band_edges must be a 1-d array of at least two edges.")
    if not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0.):
        raise ValueError("band_edges must be finite and strictly increasing.")
    return np.searchsorted(np.asarray(grid, dtype=np.float64), edges, side="left").astype(np.int64)


def g_intervals(g_edges=16):
    """The g edges [Q + 1] of compute_kdistribution's `g_edges`, checked: an int Q in 1..64 gives
    [0, cumsum(w/2)] of x, w = leggauss(Q) with the last edge set to exactly 1 (intervals of the
    Gauss weights, narrow near g = 1); an array is taken as it is: Q + 1 strictly increasing
    values from exactly 0 to exactly 1, Q <= 64."""
    if isinstance(g_edges, (bool, np.bool_)):
        raise ValueError("g_edges must be an int in 1..64 or an array of edges.")
    if isinstance(g_edges, (int, np.integer)):
        count = int(g_edges)
        if not 1 <= count <= MAX_G_INTERVALS:
            raise ValueError(f"g_edges must be an int in 1..{MAX_G_INTERVALS}, not {count}.")
        _, w = np.polynomial.legendre.leggauss(count)
        edges = np.concatenate([[0.], np.cumsum(w/2.)])
        edges[-1] = 1.
    else:
        edges = np.array(g_edges, dtype=np.float64)
        if edges.ndim != 1 or not 2 <= edges.size <= MAX_G_INTERVALS + 1:
            raise ValueError(f"g_edges must be a 1-d array of 2..{MAX_G_INTERVALS + 1} edges.")
    if not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0.):
        raise ValueError("g_edges must be finite and strictly increasing.")
    if edges[0] != 0. or edges[-1] != 1.:
        raise ValueError("g_edges must run from exactly 0 to exactly 1.")
    return np.ascontiguousarray(edges)


def g_quadrature_points(g_points, intervals):
    """The g points [P] of compute_kdistribution's `g_points`, checked: None gives (x + 1)/2 of
    x, w = leggauss(intervals); an array of values in [0, 1] is taken as it is."""
    if g_points is None:
        x, _ = np.polynomial.legendre.leggauss(int(intervals))
        return np.ascontiguousarray((x + 1.)/2.)
    points = np.array(g_points, dtype=np.float64)
    if points.ndim != 1 or points.size < 1:
        raise ValueError("g_points must be a non-empty 1-d array.")
    if not np.all((points >= 0.) & (points <= 1.)):
        raise ValueError("g_points must lie in [0, 1].")
    return np.ascontiguousarray(points)


def interval_columns(starts, g_edges):
    """int64 [B, Q + 1]: the column starts of every band's g intervals.  Interval q of band b
    (N = starts[b + 1] - starts[b] points) holds the sorted samples ceil(G_q N) <= i <
    ceil(G_q+1 N), the products formed in fp64; its columns are starts[b] + i."""
    starts = np.asarray(starts, dtype=np.int64)
    counts = np.diff(starts).astype(np.float64)
    first = np.ceil(np.asarray(g_edges, dtype=np.float64)[None, :]*counts[:, None])
    return np.ascontiguousarray(starts[:-1, None] + first.astype(np.int64))


def quantile_table(counts, g_points):
    """(i int64 [B, P], f float64 [B, P]) of the quantile at every g point of bands of `counts`
    points: x = min(max(g N - 0.5, 0), N - 1), i = floor(x), f = x - i, in fp64; i = -1 and
    f = 0 for a band without points."""
    n = np.asarray(counts, dtype=np.int64).astype(np.float64)[:, None]
    g = np.asarray(g_points, dtype=np.float64)[None, :]
    x = np.minimum(np.maximum(g*n - 0.5, 0.), np.maximum(n - 1., 0.))
    index = np.floor(x)
    fraction = x - index
    empty = np.broadcast_to(n == 0., x.shape)
    return (np.ascontiguousarray(np.where(empty, -1, index.astype(np.int64))),
            np.ascontiguousarray(np.where(empty, 0., fraction)))


def flux_angles(angles):
    """(mu, weight) of compute_flux's `angles`, checked: an int K in 1..8 gives Gauss-Legendre
    on mu in (0, 1] -- x, w = leggauss(K), mu = (x + 1)/2, weight = mu*w -- so that
    sum_k weight_k*mu_k^n = integral over (0, 1] of 2 mu mu^n for n <= 2K - 2; a pair
    (mu, weight) of equal 1-d arrays of 1..8 values is taken as it is, with 0 < mu <= 1, weights
    finite and >= 0 that sum to 1 within 1e-12 (an isotropic I then gives F = pi I)."""
    if isinstance(angles, (int, np.integer)) and not isinstance(angles, (bool, np.bool_)):
        count = int(angles)
        if not 1 <= count <= MAX_FLUX_ANGLES:
            raise ValueError(f"angles must be an int in 1..{MAX_FLUX_ANGLES}, not {count}.")
        x, w = np.polynomial.legendre.leggauss(count)
        mu = (x + 1.)/2.
        return mu, mu*w
    try:
        mu, weight = angles
    except (TypeError, ValueError):
        raise ValueError("angles must be an int in 1..8 or a pair (mu, weight).") from None
    mu = np.asarray(mu, dtype=np.float64)
    weight = np.asarray(weight, dtype=np.float64)
    if mu.ndim != 1 or weight.shape != mu.shape or not 1 <= mu.size <= MAX_FLUX_ANGLES:
        raise ValueError(f"angles: mu and weight must be 1-d arrays of the same length in "
                         f"1..{MAX_FLUX_ANGLES}.")
    if not np.all((mu > 0.) & (mu <= 1.)):
        raise ValueError("angles: mu must lie in (0, 1].")
    if not np.all(np.isfinite(weight)) or np.any(weight < 0.):
        raise ValueError("angles: weights must be finite and >= 0.")
    if not abs(float(np.sum(weight)) - 1.) <= 1.e-12:
        raise ValueError("angles: the weights must sum to 1 (they include the factor mu).")
    return np.ascontiguousarray(mu), np.ascontiguousarray(weight)


def heating_rate(upward_flux, downward_flux, pressure, temperature, thickness, surface="first"):
    """H_l = 86400*(Fnet[i_lower] - Fnet[i_upper]) / ((rho_l*c_p)*s_l) [K day-1, per cm-1 on the
    grid], in fp64: fluxes [..., L + 1, W] at the interfaces, pressure [Pa], temperature [K] and
    thickness [m] [..., L]; Fnet = up - down; i_lower is the interface of level l nearer the
    surface (l for surface "first", l + 1 for "last"); rho_l = p_l/(R_DRY*T_l); c_p = CP_DRY.
    NaN where s_l = 0."""
    net = np.asarray(upward_flux, dtype=np.float64) - np.asarray(downward_flux, dtype=np.float64)
    lower, upper = (net[..., :-1, :], net[..., 1:, :]) if surface == "first" else \
        (net[..., 1:, :], net[..., :-1, :])
    thickness = np.asarray(thickness, dtype=np.float64)
    density = np.asarray(pressure, dtype=np.float64)/(R_DRY*np.asarray(temperature, np.float64))
    capacity = (density*CP_DRY)*thickness
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = (86400.*(lower - upper))/capacity[..., None]
    return np.where((thickness == 0.)[..., None], np.nan, rate)


def _selection(quantities, names):
    """A non-empty selection of `names` (one name or several) as a tuple in the order of `names`."""
    if isinstance(quantities, str):
        quantities = (quantities,)
    quantities = tuple(quantities)
    unknown = [q for q in quantities if q not in names]
    if unknown or not quantities:
        raise ValueError(f"quantities must be a non-empty selection of {names}, not {quantities}.")
    return tuple(q for q in names if q in quantities)


# ---------------------------------------------------------------------------------------------
# The requests: every argument of a product checked before anything touches the GPU.
def _check_range_policy(range_policy):
    if range_policy not in ("reference", "skip"):
        raise ValueError(f"unknown range_policy {range_policy!r}.")


def _path_geometry(spec, path_length, name, argument="path_length", what="path lengths"):
    """(flat lengths, atmosphere shape): the checks of the path lengths that every product
    shares."""
    if spec.group is not None:
        raise NotImplementedError(f"{name} does not split paths over processes yet "
                                  "(group is set): the levels of a path would need a sum "
                                  "over ranks before exp(-tau).")
    shape = tuple(spec.atmosphere.temperature.shape)
    lengths = np.asarray(path_length, dtype=np.float64)
    if lengths.shape != shape:
        raise ValueError(f"{argument} has shape {lengths.shape}, the atmosphere {shape}.")
    if not np.all(np.isfinite(lengths)) or np.any(lengths < 0.):
        raise ValueError(f"{what} must be finite and >= 0.")
    if lengths.size == 0:
        raise ValueError("the atmosphere has no levels.")
    return np.ascontiguousarray(lengths.ravel()), shape


def _check_level_temperatures(spec):
    temperature = spec.atmosphere.temperature
    if not np.all(np.isfinite(temperature)) or np.any(temperature <= 0.):
        raise ValueError("the atmosphere's temperatures must be finite and > 0.")


def _check_pressures(spec, what="heating rates need"):
    pressure = spec.atmosphere.pressure
    if not np.all(np.isfinite(pressure)) or np.any(pressure <= 0.):
        raise ValueError(f"{what} pressures that are finite and > 0.")


def _per_path(value, name, shape):
    """A scalar or one value per path (shaped like the atmosphere without its last dimension), as
    a flat float64 array of one value per path."""
    per_path_shape = shape[:-1]
    values = np.asarray(value, dtype=np.float64)
    if values.shape not in ((), per_path_shape):
        raise ValueError(f"{name} has shape {values.shape}: give a scalar or one value "
                         f"per path, shaped {per_path_shape}.")
    return np.ascontiguousarray(np.broadcast_to(values, per_path_shape).ravel())


def _emitter(temperature, emissivity, what, shape, optional=False):
    """(temperatures, emissivities), one per path, of what lies behind the paths (`what`:
    "boundary" or "surface"): a temperature per path, finite and > 0 (None without one, where
    that is `optional`), and an emissivity per path in [0, 1]."""
    if temperature is None and optional:
        temperatures = None
    else:
        temperatures = _per_path(temperature, f"{what}_temperature", shape)
        if not np.all(np.isfinite(temperatures)) or np.any(temperatures <= 0.):
            raise ValueError(f"{what} temperatures must be finite and > 0.")
    emissivities = _per_path(emissivity, f"{what}_emissivity", shape)
    if not np.all((emissivities >= 0.) & (emissivities <= 1.)):
        raise ValueError(f"{what} emissivities must lie in [0, 1].")
    return temperatures, emissivities


def _spectral_emissivity(emissivity_wavenumber, boundary_emissivity, shape,
                         names=("emissivity_wavenumber", "boundary_emissivity",
                                "boundary emissivities")):
    """(knots [M], emissivities [paths, M]) of compute_radiance's emissivity_wavenumber: M knots
    [cm-1], finite and strictly ascending, 2 <= M <= 1024; boundary_emissivity [..., M] (the
    atmosphere's shape without its last axis, then M) or [M] for every path, in [0, 1].
    names: what the messages call the two arguments and the values (compute_solar's albedo)."""
    knot_name, value_name, what = names
    knots = np.asarray(emissivity_wavenumber, dtype=np.float64)
    if knots.ndim != 1 or not 2 <= knots.size <= MAX_EMISSIVITY_KNOTS:
        raise ValueError(f"{knot_name} must be a 1-d array of 2..{MAX_EMISSIVITY_KNOTS} "
                         f"knots, not of shape {knots.shape}.")
    if not np.all(np.isfinite(knots)) or not np.all(np.diff(knots) > 0.):
        raise ValueError(f"{knot_name} must be finite and strictly ascending.")
    _, paths = _path_layout(shape)
    per_path_shape = tuple(shape[:-1]) + (knots.size,)
    values = np.asarray(boundary_emissivity, dtype=np.float64)
    if values.shape not in ((knots.size,), per_path_shape):
        raise ValueError(f"{value_name} has shape {values.shape}: with "
                         f"{knot_name} give [{knots.size}] or one table per path, "
                         f"shaped {per_path_shape}.")
    if not np.all((values >= 0.) & (values <= 1.)):
        raise ValueError(f"{what} must lie in [0, 1].")
    values = np.broadcast_to(values, per_path_shape).reshape(paths, knots.size)
    return np.ascontiguousarray(knots), np.ascontiguousarray(values)


def interpolate_emissivity(knots, values, grid):
    """E on the grid as lbl_surface_emissivity forms it, in the float type of the arguments:
    for k_j <= nu < k_{j+1}, E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)); E = e_0 for
    nu <= k_0 and E = e_{M-1} for nu >= k_{M-1}.  values [..., M] -> [..., grid.size]."""
    knots, values, grid = np.asarray(knots), np.asarray(values), np.asarray(grid)
    last = knots.size - 1
    j = np.clip(np.searchsorted(knots, grid, side="right") - 1, 0, last - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        slope = (values[..., j + 1] - values[..., j])/(knots[j + 1] - knots[j])
        inside = values[..., j] + (grid - knots[j])*slope
    return np.where(grid >= knots[last], values[..., last:],
                    np.where(grid > knots[0], inside, values[..., :1]))


def _edge_temperatures(source, interface_temperature, shape):
    """None for source "isothermal"; for "linear_in_tau" the interface temperatures as the path
    entries take them, float64 [levels, 2]: row i = p*L + l holds interface l (between levels
    l - 1 and l, the first-level side) and interface l + 1 (the last-level side) of path p.
    interface_temperature: the atmosphere's shape with L + 1 in place of L, finite and > 0."""
    if not (isinstance(source, str) and source in SOURCES):
        raise ValueError(f"source must be one of {SOURCES}, not {source!r}.")
    if source == "isothermal":
        if interface_temperature is not None:
            raise ValueError('interface_temperature is only used with source="linear_in_tau".')
        return None
    if interface_temperature is None:
        raise ValueError('source="linear_in_tau" needs interface_temperature.')
    per_path, paths = _path_layout(shape)
    expected = tuple(shape[:-1]) + (per_path + 1,)
    interfaces = np.asarray(interface_temperature, dtype=np.float64)
    if interfaces.shape != expected:
        raise ValueError(f"interface_temperature has shape {interfaces.shape}, need {expected}: "
                         "the atmosphere's with one more value along the last axis.")
    if not np.all(np.isfinite(interfaces)) or np.any(interfaces <= 0.):
        raise ValueError("interface temperatures must be finite and > 0.")
    interfaces = interfaces.reshape(paths, per_path + 1)
    edges = np.stack([interfaces[:, :-1], interfaces[:, 1:]], axis=-1)
    return np.ascontiguousarray(edges.reshape(paths*per_path, 2))


def _run_edges(request, a, b):
    """What a sweep of the flat levels [a, b) passes on to Engine.path_radiance / path_flux
    beside its other tables: nothing for isothermal levels, edge_temperature [b - a, 2] for the
    linear-in-tau source."""
    if request.edge_temperature is None:
        return {}
    return {"edge_temperature": request.edge_temperature[a:b]}


def _path_bands(spec, band_edges, instrument=None):
    """(edges, column starts) of band_edges, or (None, None); checks `instrument` too."""
    if instrument is not None:
        from .instrument import Instrument
        if band_edges is not None:
            raise ValueError("give band_edges or instrument, not both.")
        if not isinstance(instrument, Instrument):
            raise ValueError(f"instrument must be an Instrument, not {type(instrument)}.")
        if spec.grid.size > 1 and not np.all(np.diff(spec.grid) > 0.):
            raise ValueError("instrument channels need an increasing grid.")
    if band_edges is None:
        return None, None
    if spec.grid.size > 1 and not np.all(np.diff(spec.grid) > 0.):
        raise ValueError("band means need an increasing grid.")
    starts = band_columns(spec.grid, band_edges)
    return np.asarray(band_edges, dtype=np.float64), starts


def _path_request(spec, path_length, quantities, band_edges, cumulative, range_policy,
                  instrument=None):
    """Checks every argument of compute_path."""
    lengths, shape = _path_geometry(spec, path_length, "compute_path")
    quantities = _selection(quantities, PATH_QUANTITIES)
    if not (cumulative is None or (isinstance(cumulative, str) and
                                   cumulative in PATH_CUMULATIVE)):
        raise ValueError(f"cumulative must be one of {PATH_CUMULATIVE}, not {cumulative!r}.")
    _check_range_policy(range_policy)
    edges, starts = _path_bands(spec, band_edges, instrument)
    return _PathRequest(lengths=lengths, shape=shape, quantities=quantities, edges=edges,
                        starts=starts, instrument=instrument, cumulative=cumulative)


def _radiance_request(spec, path_length, boundary_temperature, boundary_emissivity, direction,
                      quantities, band_edges, cumulative, range_policy, instrument=None,
                      names=RADIANCE_QUANTITIES, caller="compute_radiance", source="isothermal",
                      interface_temperature=None, emissivity_wavenumber=None,
                      reflection_path_length=None):
    """Checks every argument of compute_radiance; compute_jacobian's too, with its `names`."""
    lengths, shape = _path_geometry(spec, path_length, caller)
    _check_level_temperatures(spec)
    edge_temperature = _edge_temperatures(source, interface_temperature, shape)
    knots = reflection_lengths = None
    if emissivity_wavenumber is None:
        boundary, emissivity = _emitter(boundary_temperature, boundary_emissivity, "boundary",
                                        shape, optional=True)
    else:
        boundary, _ = _emitter(boundary_temperature, 1., "boundary", shape, optional=True)
        knots, emissivity = _spectral_emissivity(emissivity_wavenumber, boundary_emissivity,
                                                 shape)
    if reflection_path_length is not None:
        reflection_lengths, _ = _path_geometry(spec, reflection_path_length, caller,
                                               "reflection_path_length",
                                               "reflection path lengths")
        if boundary is None:
            raise ValueError("reflection_path_length needs a boundary_temperature: the surface "
                             "that reflects.")
    if not (isinstance(direction, str) and direction in RADIANCE_DIRECTIONS):
        raise ValueError(f"direction must be one of {RADIANCE_DIRECTIONS}, not {direction!r}.")
    quantities = _selection(quantities, names)
    if not isinstance(cumulative, (bool, np.bool_)):
        raise ValueError(f"cumulative must be True or False, not {cumulative!r}.")
    _check_range_policy(range_policy)
    if band_edges is not None and "brightness_temperature" in quantities:
        raise ValueError("brightness_temperature is only available on the grid: band means "
                         "are formed of the radiance alone.")
    if DOWNWELLING in quantities:
        if reflection_lengths is None:
            raise ValueError(f'"{DOWNWELLING}" is only formed with reflection_path_length.')
        if cumulative:
            raise ValueError(f'"{DOWNWELLING}" is one result per path: not with cumulative=True.')
    edges, starts = _path_bands(spec, band_edges, instrument)
    return _RadianceRequest(lengths=lengths, shape=shape, quantities=quantities, edges=edges,
                            starts=starts, instrument=instrument, cumulative=bool(cumulative),
                            from_last=direction == "toward_first",
                            boundary_temperature=boundary, boundary_emissivity=emissivity,
                            edge_temperature=edge_temperature, emissivity_knots=knots,
                            reflection_lengths=reflection_lengths)


def _flux_request(spec, layer_thickness, surface_temperature, surface_emissivity, surface,
                  angles, quantities, band_edges, range_policy, source="isothermal",
                  interface_temperature=None):
    """Checks every argument of compute_flux."""
    lengths, shape = _path_geometry(spec, layer_thickness, "compute_flux", "layer_thickness",
                                    "layer thicknesses")
    _check_level_temperatures(spec)
    edge_temperature = _edge_temperatures(source, interface_temperature, shape)
    if "heating_rate" in (quantities if not isinstance(quantities, str) else (quantities,)):
        _check_pressures(spec)
    ts, es = _emitter(surface_temperature, surface_emissivity, "surface", shape)
    if not (isinstance(surface, str) and surface in FLUX_SURFACES):
        raise ValueError(f"surface must be one of {FLUX_SURFACES}, not {surface!r}.")
    mu, weight = flux_angles(angles)
    quantities = _selection(quantities, FLUX_QUANTITIES)
    _check_range_policy(range_policy)
    edges, starts = _path_bands(spec, band_edges)
    return _FluxRequest(lengths=lengths, shape=shape, quantities=quantities, edges=edges,
                        starts=starts, instrument=None, cumulative=False, surface=surface, mu=mu,
                        weight=weight, surface_temperature=ts, surface_emissivity=es,
                        edge_temperature=edge_temperature)


def _solar_spectrum(spec, solar_irradiance, solar_wavenumber, distance_factor):
    """(knots or None, values or None, scale) of compute_solar's Sun, checked."""
    factor = np.asarray(distance_factor, dtype=np.float64)
    if factor.shape != () or not np.isfinite(factor) or not factor > 0.:
        raise ValueError("distance_factor must be one finite number > 0.")
    factor = float(factor)
    if solar_irradiance is None:
        if solar_wavenumber is not None:
            raise ValueError("solar_wavenumber needs solar_irradiance at its knots.")
        return None, None, SOLAR_SOLID_ANGLE*factor
    values = np.asarray(solar_irradiance, dtype=np.float64)
    if solar_wavenumber is None:
        if values.shape != (spec.grid.size,):
            raise ValueError(f"solar_irradiance has shape {values.shape}: without "
                             f"solar_wavenumber give one value per grid point, "
                             f"[{spec.grid.size}].")
        knots = None
    else:
        knots = np.asarray(solar_wavenumber, dtype=np.float64)
        if knots.ndim != 1 or not 2 <= knots.size <= MAX_SOLAR_KNOTS:
            raise ValueError(f"solar_wavenumber must be a 1-d array of 2..{MAX_SOLAR_KNOTS} "
                             f"knots, not of shape {knots.shape}.")
        if not np.all(np.isfinite(knots)) or not np.all(np.diff(knots) > 0.):
            raise ValueError("solar_wavenumber must be finite and strictly ascending.")
        if values.shape != knots.shape:
            raise ValueError(f"solar_irradiance has shape {values.shape}: with solar_wavenumber "
                             f"give one value per knot, [{knots.size}].")
        knots = np.ascontiguousarray(knots)
    if not np.all(np.isfinite(values)) or np.any(values < 0.):
        raise ValueError("solar irradiances must be finite and >= 0.")
    return knots, np.ascontiguousarray(values), factor


def _solar_request(spec, layer_thickness, solar_zenith_cosine, solar_irradiance,
                   solar_wavenumber, distance_factor, solar_path_length, surface, surface_albedo,
                   albedo_wavenumber, view_path_length, quantities, band_edges, instrument,
                   range_policy):
    """Checks every argument of compute_solar."""
    lengths, shape = _path_geometry(spec, layer_thickness, "compute_solar", "layer_thickness",
                                    "layer thicknesses")
    per_path, _ = _path_layout(shape)
    if not (isinstance(surface, str) and surface in FLUX_SURFACES):
        raise ValueError(f"surface must be one of {FLUX_SURFACES}, not {surface!r}.")
    mu0 = _per_path(solar_zenith_cosine, "solar_zenith_cosine", shape)
    if not np.all((mu0 > 0.) & (mu0 <= 1.)):
        raise ValueError("solar_zenith_cosine must lie in (0, 1].")
    if solar_path_length is None:
        solar_lengths = np.ascontiguousarray(lengths/np.repeat(mu0, per_path))
    else:
        solar_lengths, _ = _path_geometry(spec, solar_path_length, "compute_solar",
                                          "solar_path_length", "solar path lengths")
    solar_knots, solar_values, scale = _solar_spectrum(spec, solar_irradiance, solar_wavenumber,
                                                       distance_factor)
    quantities = _selection(quantities, SOLAR_QUANTITIES)
    reflected = "reflected_radiance" in quantities
    if reflected and (view_path_length is None or surface_albedo is None):
        raise ValueError('"reflected_radiance" needs view_path_length and surface_albedo.')
    if not reflected and not (view_path_length is None and surface_albedo is None and
                              albedo_wavenumber is None):
        raise ValueError('view_path_length, surface_albedo and albedo_wavenumber are only used '
                         'by "reflected_radiance", which is not among the quantities.')
    view_lengths = albedo = albedo_knots = None
    if reflected:
        view_lengths, _ = _path_geometry(spec, view_path_length, "compute_solar",
                                         "view_path_length", "view path lengths")
        if albedo_wavenumber is None:
            albedo = _per_path(surface_albedo, "surface_albedo", shape)
            if not np.all((albedo >= 0.) & (albedo <= 1.)):
                raise ValueError("surface albedos must lie in [0, 1].")
        else:
            albedo_knots, albedo = _spectral_emissivity(
                albedo_wavenumber, surface_albedo, shape,
                ("albedo_wavenumber", "surface_albedo", "surface albedos"))
    if "heating_rate" in quantities:
        _check_level_temperatures(spec)
        _check_pressures(spec)
    _check_range_policy(range_policy)
    edges, starts = _path_bands(spec, band_edges, instrument)
    if instrument is not None and any(q not in SOLAR_PATH_QUANTITIES for q in quantities):
        raise ValueError(f"instrument reduces the quantities per path, {SOLAR_PATH_QUANTITIES}, "
                         f"not {quantities}.")
    return _SolarRequest(lengths=lengths, shape=shape, quantities=quantities, edges=edges,
                         starts=starts, instrument=instrument, cumulative=False, surface=surface,
                         mu0=mu0, solar_lengths=solar_lengths, view_lengths=view_lengths,
                         albedo=albedo, albedo_knots=albedo_knots, solar_knots=solar_knots,
                         solar_values=solar_values, scale=scale)


def rayleigh_cross_section(wavenumber):
    """sigma(nu) [m2] of compute_solar_flux in fp64, as lbl_rayleigh_row forms it: Bucholtz (1995)
    with lambda = 1e4/nu in um, sigma = (1e-4*A)*exp(-(e*log(lambda))), e = (B + C*lambda) +
    D/lambda, the row RAYLEIGH_SHORT for lambda <= 0.5 and RAYLEIGH_LONG above; 0 for nu <= 0."""
    nu = np.asarray(wavenumber, dtype=np.float64)
    positive = nu > 0.
    lam = 1e4/np.where(positive, nu, 1.)
    a, b, c, d = (np.where(lam <= RAYLEIGH_SPLIT, short, long)
                  for short, long in zip(RAYLEIGH_SHORT, RAYLEIGH_LONG))
    e = (b + c*lam) + d/lam
    return np.where(positive, (1e-4*a)*np.exp(-(e*np.log(lam))), 0.)


def _kdistribution_weighting(spec, weighting, weighting_temperature):
    """(weighting, weights, weight_temperature) of a _KDistributionRequest from
    compute_kdistribution's `weighting` and `weighting_temperature`, checked."""
    if weighting is None:
        if weighting_temperature is not None:
            raise ValueError('weighting_temperature needs weighting="planck".')
        return None, None, None
    if isinstance(weighting, str):
        if weighting not in KDISTRIBUTION_WEIGHTINGS:
            raise ValueError(f"weighting must be one of {KDISTRIBUTION_WEIGHTINGS} or an array "
                             f"of one weight per grid point, not {weighting!r}.")
        shape = spec.atmosphere.temperature.shape
        if weighting_temperature is None:
            temperature = np.asarray(spec.atmosphere.temperature, dtype=np.float64)
        else:
            temperature = np.asarray(weighting_temperature, dtype=np.float64)
            if temperature.shape not in ((), shape):
                raise ValueError(f"weighting_temperature has shape {temperature.shape}: give one "
                                 f"number or the atmosphere's shape {shape}.")
            temperature = np.broadcast_to(temperature, shape)
        if not np.all(np.isfinite(temperature)) or not np.all(temperature > 0.):
            raise ValueError("the temperatures of the Planck weighting must be finite and > 0.")
        return weighting, None, np.ascontiguousarray(temperature.ravel())
    if weighting_temperature is not None:
        raise ValueError('weighting_temperature needs weighting="planck".')
    weights = np.asarray(weighting, dtype=np.float64)
    if weights.shape != (spec.grid.size,):
        raise ValueError(f"weighting has shape {weights.shape}: give one weight per grid point, "
                         f"[{spec.grid.size}].")
    if not np.all(np.isfinite(weights)) or np.any(weights < 0.):
        raise ValueError("weights must be finite and >= 0.")
    return "array", np.ascontiguousarray(weights), None


def _kdistribution_request(spec, band_edges, g_edges, g_points, quantities, range_policy,
                           weighting=None, weighting_temperature=None):
    """Checks every argument of compute_kdistribution."""
    if spec.group is not None:
        raise NotImplementedError("compute_kdistribution does not split levels over processes "
                                  "yet (group is set).")
    shape = tuple(spec.atmosphere.temperature.shape)
    if spec.atmosphere.temperature.size == 0:
        raise ValueError("the atmosphere has no levels.")
    if band_edges is None:
        raise ValueError("compute_kdistribution needs band_edges.")
    kind, weights, weight_temperature = _kdistribution_weighting(spec, weighting,
                                                                 weighting_temperature)
    asked = (quantities,) if isinstance(quantities, str) else tuple(quantities)
    if kind is None and any(q in KDISTRIBUTION_WEIGHTED_QUANTITIES for q in asked):
        raise ValueError(f"the quantities {KDISTRIBUTION_WEIGHTED_QUANTITIES} need a weighting.")
    quantities = _selection(asked, KDISTRIBUTION_QUANTITIES + (
        KDISTRIBUTION_WEIGHTED_QUANTITIES if kind is not None else ()))
    _check_range_policy(range_policy)
    edges, starts = _path_bands(spec, band_edges)
    g = g_intervals(g_edges)
    points = g_quadrature_points(g_points, g.size - 1)
    index, fraction = quantile_table(np.diff(starts), points)
    return _KDistributionRequest(
        lengths=None, shape=shape, quantities=quantities, edges=edges, starts=starts,
        instrument=None, cumulative=False, g_edges=g, g_points=points,
        interval_starts=interval_columns(starts, g), point_index=index, point_fraction=fraction,
        weighting=kind, weights=weights, weight_temperature=weight_temperature)


# ---------------------------------------------------------------------------------------------
# The run loop.
def _sweep_pass(quantities, cumulative, from_last):
    """The one pass of compute_path and compute_radiance."""
    return _Pass(from_last, tuple(quantities) if cumulative else (),
                 () if cumulative else tuple(quantities))


def _cut_runs(levels, per_path, level_bytes, limit, whole_paths=False):
    """(run, [(a, b)]): the runs of consecutive flat levels of _sweep_runs, `run` levels each but
    the last, for blocks of level_bytes per level within `limit` bytes and _MAX_RUN_LEVELS
    levels.  whole_paths: every run is a whole number of paths of per_path levels -- the most
    that fit; ValueError where one path does not."""
    if whole_paths:
        path_bytes = per_path*level_bytes
        paths = min(limit//path_bytes, _MAX_RUN_LEVELS//per_path)
        if paths < 1:
            raise ValueError(f"device_output_limit = {limit} bytes does not hold one path: its "
                             f"blocks need {path_bytes} bytes ({per_path} levels, and at most "
                             f"{_MAX_RUN_LEVELS} levels in a run).")
        run = min(paths*per_path, levels)
    else:
        run = levels if levels*level_bytes <= limit else max(1, limit//level_bytes)
        run = min(run, _MAX_RUN_LEVELS)
    return run, [(a, min(a + run, levels)) for a in range(0, levels, run)]


def _level_bytes(n, request, level_quantities, level_blocks, grid_outputs):
    """Bytes per level of a run that count against device_output_limit (_cut_runs' level_bytes),
    in blocks of n float64: the caller's `level_blocks` -- beta and what its sweeper takes per
    level (compute_path and compute_radiance 1, compute_flux 2: the fluxes of a level,
    compute_jacobian 1 and its work blocks) -- and one block per per-level quantity of the passes
    where an instrument reduces it from the grid, or where the caller says its `grid_outputs`
    count (compute_jacobian) and there are no bands; and the knot table of a spectral scatterer,
    24 bytes per level and knot.
    Known undercount, kept because it decides where runs are cut: without an instrument the
    per-level grid outputs of compute_path and compute_radiance (cumulative=) are not counted,
    and compute_flux counts one output block where it holds two on the grid; neither are the
    per-path blocks and carries.  Counting them is a follow-up that changes the run cuts."""
    blocks = level_blocks
    if request.instrument is not None or (grid_outputs and request.starts is None):
        blocks += len(level_quantities)
    # The knot table of a spectral scatterer travels with its run: 3 float64 per level and knot.
    knots = getattr(request, "scatterer_knots", None)
    return blocks*n*8 + (0 if knots is None else knots.size*24)


def _first_rows(block, count):
    return block if count == block.shape[0] else block.rows(count)


class _FilledOnce(object):
    """The blocks of a call that do not depend on the run -- S, sigma, the rows of a spectral
    surface, a row of weights -- and are filled once, before its first sweep.  A sweeper makes
    one first of all (that fetches the grid's handle), takes these blocks through it in the
    order of its other blocks (the order is the call's HBM layout), and every sweep begins with
    queue(): the first one queues the fills in the order they were taken, the others nothing."""
    def __init__(self, call):
        self.call, self.grid, self.pending = call, call.grid(), []

    def take(self, rows, fill):
        """A block of `rows` rows of the call that fill(block) queues the filling of."""
        block = self.call.take(rows)
        self.pending.append(lambda: fill(block))
        return block

    def queue(self):
        while self.pending:
            self.pending.pop(0)()

    def solar_row(self, request):
        """S on the grid, of a request with _SolarRequest's Sun."""
        return self.take(1, lambda row: self.call.engine.solar_spectrum(
            self.grid, row, self.call.columns, irradiance=request.solar_values,
            wavenumber=request.solar_knots, temperature=SOLAR_TEMPERATURE, scale=request.scale,
            asynchronous=True))

    def rayleigh_row(self, cross_section):
        """sigma on the grid: the caller's values, or the fit for None."""
        return self.take(1, lambda row: self.call.engine.rayleigh_row(
            self.grid, row, self.call.columns, cross_section=cross_section, asynchronous=True))

    def surface_rows(self, knots, values):
        """One row per path of a surface's emissivity or albedo table on the grid; None, and no
        block, without knots."""
        if knots is None:
            return None
        return self.take(self.call.paths, lambda rows: self.call.engine.surface_emissivity(
            self.grid, rows, knots, values, asynchronous=True))


class _Rows(object):
    """Where the entry of a pass writes its rows on the grid.  Without bands they are the outputs
    themselves; with bands they are blocks of this call, taken here in the order of
    step.level_quantities + step.path_quantities, and the outputs receive their means."""
    def __init__(self, call, step, run, bands):
        self.per_level = step.level_quantities
        self.fine = {q: call.take(run if q in self.per_level else call.paths)
                     for q in step.level_quantities + step.path_quantities} if bands else {}

    def keywords(self, names, outputs, rows):
        """The <name>_rows (and, with bands, <name>_mean) keywords of a run of `rows` levels for
        the quantities among `outputs`; names: {quantity: what the entry calls it}."""
        blocks = {}
        for q, name in names.items():
            if q not in outputs:
                continue
            blocks[name + "_rows"] = outputs[q]
            if q in self.fine:
                fine = self.fine[q]
                blocks[name + "_rows"] = _first_rows(fine, rows) if q in self.per_level else fine
                blocks[name + "_mean"] = outputs[q]
        return blocks


def _swept_radiance(request, quantities):
    """What the sweeps of a radiance call form of `quantities` (those of its up pass): with an
    instrument the radiance alone, as channel radiances on the GPU -- their brightness
    temperatures are formed at the channel centres on the host (_channel_brightness)."""
    return ("radiance",) if request.instrument is not None and quantities else quantities


def _channel_brightness(values, request):
    """`values` of a radiance call, with an instrument's brightness temperatures where asked
    for."""
    if request.instrument is not None and "brightness_temperature" in request.quantities:
        from .instrument import brightness_temperature
        values["brightness_temperature"] = brightness_temperature(
            values["radiance"], request.instrument.centers)
    return values


def _sweep_runs(spec, request, passes, remove_pedestal, range_policy, sweeper, level_blocks=1,
                products=None, grid_outputs=False, whole_paths=False, widths=None):
    """{product: array [levels or paths, columns, bands or channels]}: the "total" block of a run
    of levels at a time (Spectroscopy.total_into), then the path kernels on it -- for each of
    `passes` (_Pass) in turn, every pass over all levels.
    sweeper(call, run) (call: _Call) returns sweep(index, beta, a, b, outputs), which queues the
    path kernels of pass `index` on the levels [a, b) and their block `beta`, with `outputs`
    {quantity of any pass: DeviceSpectra}.  A pass that starts on the run the previous pass ended
    on finds that run's block still in HBM and does not compute it again: sweeps of a call with
    several passes must leave beta as they found it.
    products: what goes to the host (_Product); None: every quantity of the passes as it is.
    With request.instrument the sweeps write their quantities on the grid and only the products,
    reduced to [rows, channels] by lbl_instrument_apply, travel.
    level_blocks, grid_outputs: see _level_bytes.  whole_paths: every run is a whole number of
    paths (_cut_runs), for sweeps that carry nothing from run to run.
    widths: {quantity: columns} of the outputs whose rows are neither the grid nor the bands
    (compute_kdistribution).  A product of source _BETA is the run's block itself as the sweep
    leaves it, sent home after every run of the one pass."""
    widths = widths or {}
    if remove_pedestal is None:
        remove_pedestal = spec.continua_backend == "mt_ckd"
    whole = _Levels(spec, 0, spec.atmosphere.temperature.size, remove_pedestal, range_policy)
    temperature, levels = whole.temperature, whole.count
    per_path, paths = _path_layout(request.shape)
    v0, vn, n_per_v = grid_arguments(spec.grid)
    n = (vn - v0)*n_per_v
    instrument, starts = request.instrument, request.starts
    level_quantities = [q for step in passes for q in step.level_quantities]
    path_quantities = [q for step in passes for q in step.path_quantities]
    if products is None:
        products = [_Product(q, q, True) for q in level_quantities] + \
            [_Product(q, q, False) for q in path_quantities]
    products = sorted(products, key=lambda product: not product.per_level)
    # Runs of consecutive levels when the blocks would not fit: the sweep carries over in HBM.
    run, runs = _cut_runs(levels, per_path,
                          _level_bytes(n, request, level_quantities, level_blocks, grid_outputs),
                          spec.device_output_limit, whole_paths)
    # What the sweeps write per row, and what goes home per row.
    band_width = n if starts is None else starts.size - 1
    width = spec.grid.size if starts is None else starts.size - 1

    gases = present_gases(spec, whole, total=True)
    engine = gases.engine
    if engine is None:
        from .engine import default_engine
        engine = default_engine(spec.device)
    if instrument is not None:
        from .instrument import resident_instrument
        handle = resident_instrument(engine, instrument, spec.grid)
        width = len(instrument)
    results = {product.name: engine.host_array((levels if product.per_level else paths,
                                                widths.get(product.source, width)))
               for product in products}
    # One block of `run` levels for beta (and for each per-level output) serves every run; the
    # shorter last run uses its leading rows.  Together with the sweeper's blocks and the
    # per-path outputs that is all this call holds in HBM.
    taken = []

    def take(rows, columns=n):
        block = engine.blocks.take(rows, columns)
        taken.append(block)
        return block

    def grid_handle():
        from .mt_ckd import resident_grid
        return resident_grid(engine, spec.grid)

    def send_home(product, rows, target):
        """Queues the copy of the first `rows` rows of the product's source to `target`: reduced
        to channels first with an instrument."""
        block = _first_rows(beta if product.source == _BETA else outputs[product.source], rows)
        if instrument is not None:
            engine.instrument_apply(block, rows, handle, channels[product.name],
                                    transmittance=product.transmittance, asynchronous=True)
            block = _first_rows(channels[product.name], rows)
        block.to_host_into(target, widths.get(product.source, width), asynchronous=True)
    # The pooled blocks go back whether the call failed or not: behind the guard's cancel-and-wait.
    with pipeline(engine, give_back=taken):
        sweep = sweeper(_Call(engine, take, paths, per_path, spec.grid.size, temperature,
                              grid_handle), run)
        beta = take(run, n)
        outputs = {q: take(run, widths.get(q, band_width)) for q in level_quantities}
        outputs.update({q: take(paths, band_width) for q in path_quantities})
        channels = {} if instrument is None else {
            product.name: take(run if product.per_level else paths, width)
            for product in products}
        resident = None
        for index, step in enumerate(passes):
            for a, b in (runs[::-1] if step.from_last else runs):
                kept = (a, b) == resident
                if resident is not None and not kept:
                    # The previous run's block and outputs are written again below: what
                    # still reads them -- its sweep, its copies to the host -- is done first.
                    engine.synchronize()
                rows = _first_rows(beta, b - a)
                if not kept:
                    spec.total_into(rows, a, b, remove_pedestal, range_policy, gases=gases)
                resident = (a, b)
                sweep(index, rows, a, b,
                      {q: _first_rows(block, b - a) if q in level_quantities else block
                       for q, block in outputs.items()})
                for product in products:
                    if product.per_level and (product.source in step.level_quantities or
                                              product.source == _BETA):
                        send_home(product, b - a, results[product.name][a:b])
        for product in products:
            if not product.per_level:
                send_home(product, paths, results[product.name])
        engine.synchronize()
    return results


# ---------------------------------------------------------------------------------------------
# The results.
def _spectral_axis(request):
    """The last dim of a path result: "channel", "band" or "wavenumber"."""
    if request.instrument is not None:
        return "channel"
    return "wavenumber" if request.edges is None else "band"


def _band_widths(spec, request):
    """What turns a band mean into the band's integral: the band's width in grid steps over
    n_per_v [bands]; 1. on the grid."""
    if request.starts is None:
        return 1.
    _, _, n_per_v = grid_arguments(spec.grid)
    return np.diff(request.starts).astype(np.float64)/float(n_per_v)


def _interface_rows(below, space, request):
    """[paths, L + 1, W] at the interfaces from a sweep's rows in the Sun's order: `below`
    [levels, W] at the interface below each level and `space` [paths, W] at the space end."""
    per_path, paths = _path_layout(request.shape)
    width = below.shape[-1]
    below = np.asarray(below).reshape(paths, per_path, width)
    space = np.asarray(space).reshape(paths, 1, width)
    # Sweeping toward level 0 the interface below level l is interface l, toward level L-1
    # interface l + 1.
    return np.concatenate([below, space] if request.surface == "first" else [space, below],
                          axis=1)


def _level_heating(spec, upward, downward, request):
    """heating_rate of the fluxes [paths, L + 1, W] in the atmosphere's shape, [..., L, W]."""
    per_path, paths = _path_layout(request.shape)
    return heating_rate(
        upward, downward, spec.atmosphere.pressure.reshape(paths, per_path),
        spec.atmosphere.temperature.reshape(paths, per_path),
        request.lengths.reshape(paths, per_path), request.surface).reshape(
            list(request.shape) + [-1])


def _flux_interfaces(spec, values, request):
    """{quantity: [..., L + 1 or L, W]} of compute_flux from the sweeps' per-level rows (the
    flux just after each level in sweep order) and the surface rows."""
    shape = list(request.shape)
    per_path, paths = _path_layout(request.shape)
    width = values["downward_flux"].shape[-1]
    down = np.asarray(values["downward_flux"]).reshape(paths, per_path, width)
    up = np.asarray(values["upward_flux"]).reshape(paths, per_path, width)
    surface = np.asarray(values["surface_flux"]).reshape(paths, 1, width)
    space = np.zeros((paths, 1, width))
    if request.starts is not None:
        points = np.diff(request.starts)
        space[..., points == 0] = np.nan
    # Sweeping toward level 0 the flux after level l is at interface l, toward level L-1 at
    # interface l + 1.
    if request.surface == "first":
        fluxes = {"downward_flux": np.concatenate([down, space], axis=1),
                  "upward_flux": np.concatenate([surface, up], axis=1)}
    else:
        fluxes = {"downward_flux": np.concatenate([space, down], axis=1),
                  "upward_flux": np.concatenate([up, surface], axis=1)}
    if request.starts is not None:
        widths = _band_widths(spec, request)
        fluxes = {q: f*widths for q, f in fluxes.items()}
    out = {}
    lead = shape[:-1] + [per_path + 1, width]
    for q in ("upward_flux", "downward_flux"):
        if q in request.quantities:
            out[q] = fluxes[q].reshape(lead)
    if "heating_rate" in request.quantities:
        out["heating_rate"] = _level_heating(spec, fluxes["upward_flux"],
                                             fluxes["downward_flux"], request)
    return out


def _solar_interfaces(spec, values, request):
    """{quantity: array} of compute_solar from the sweep's rows: the direct irradiance below each
    level and at the space end of each path, the surface rows and the reflected rows."""
    shape = list(request.shape)
    per_path, _ = _path_layout(request.shape)
    widths = _band_widths(spec, request)
    out = {}
    if "direct_irradiance" in values:
        direct = _interface_rows(values["direct_irradiance"], values[_SPACE], request)*widths
        if "direct_irradiance" in request.quantities:
            out["direct_irradiance"] = direct.reshape(shape[:-1] + [per_path + 1, -1])
        if "heating_rate" in request.quantities:
            out["heating_rate"] = _level_heating(spec, np.zeros_like(direct), direct, request)
    if "surface_irradiance" in request.quantities:
        scale = 1. if request.instrument is not None else widths
        out["surface_irradiance"] = (np.asarray(values["surface_irradiance"])*scale).reshape(
            shape[:-1] + [-1])
    if "reflected_radiance" in request.quantities:
        out["reflected_radiance"] = np.asarray(values["reflected_radiance"]).reshape(
            shape[:-1] + [-1])
    return out


def _create_path_dataset(spec, values, request):
    """compute_path's, compute_radiance's and compute_jacobian's result from {quantity:
    [paths or levels, columns, bands or channels]}: per level when cumulative and for the
    per-level Jacobians."""
    axis = _spectral_axis(request)
    variables = {}
    for q in request.quantities:
        dims, shape = list(spec.atmosphere.dims), list(request.shape)
        if not (request.cumulative or q in JACOBIAN_LEVEL_QUANTITIES) or q == DOWNWELLING:
            dims, shape = dims[:-1], shape[:-1]
        variables[q] = (dims + [axis], np.asarray(values[q]).reshape(shape + [-1]),
                        _PATH_UNITS[q])
    return _path_variables(spec, variables, request)


def _create_flux_dataset(spec, values, request):
    """The result of compute_flux, of compute_solar and of the two-stream flux products from
    {quantity: [..., interfaces or levels, columns or bands]}: fluxes and irradiances on the
    "interface" dim in place of the atmosphere's last, heating rates on it, compute_solar's
    SOLAR_PATH_QUANTITIES per path."""
    dims = list(spec.atmosphere.dims)
    axis = _spectral_axis(request)
    variables = {}
    for q in request.quantities:
        here = dims + [axis] if q == "heating_rate" else dims[:-1] + ["interface", axis]
        if q in SOLAR_PATH_QUANTITIES:
            here = dims[:-1] + [axis]
        variables[q] = (here, values[q], _FLUX_UNITS[q][request.edges is not None])
    return _path_variables(spec, variables, request)


_create_solar_dataset = _create_flux_dataset


def _create_kdistribution_dataset(spec, values, request):
    """compute_kdistribution's result from the sweeps' rows: the means of the device's flat
    interval list [levels, B (Q + 1) - 1] (the last of every band's Q + 1 is the gap to the next
    band), the quantiles [levels, B P] and the sorted block [levels, grid]; with a weighting the
    interval sums of W and W*k, flat like the means, and pi as int32 pairs in float64 rows."""
    from .spectroscopy import _optional_xarray
    dims, shape = list(spec.atmosphere.dims), list(request.shape)
    bands, q, p = request.starts.size - 1, request.g_edges.size - 1, request.g_points.size
    levels = int(np.prod(shape, dtype=np.int64))
    units = {"units": "m-1"}
    variables = {}

    def per_interval(name):
        flat = np.full((levels, bands*(q + 1)), np.nan)
        flat[:, :-1] = values[name]
        return np.ascontiguousarray(flat.reshape(levels, bands, q + 1)[:, :, :q]).reshape(
            shape + [bands, q])
    if "absorption_g_mean" in request.quantities:
        variables["absorption_g_mean"] = (dims + ["band", "g_interval"],
                                          per_interval("absorption_g_mean"), units)
    with np.errstate(divide="ignore", invalid="ignore"):
        if "weight_g_fraction" in request.quantities:
            sums = per_interval(_WEIGHT_SUMS)
            variables["weight_g_fraction"] = (dims + ["band", "g_interval"],
                                              sums/np.sum(sums, axis=-1, keepdims=True), {})
        if "absorption_g_weighted_mean" in request.quantities:
            sums = per_interval(_WEIGHT_SUMS)
            variables["absorption_g_weighted_mean"] = (
                dims + ["band", "g_interval"],
                np.where(sums == 0., np.nan, per_interval(_WEIGHTED_SUMS)/sums), units)
    if "absorption_g_quantile" in request.quantities:
        variables["absorption_g_quantile"] = (
            dims + ["band", "g_point"],
            np.array(values["absorption_g_quantile"]).reshape(shape + [bands, p]), units)
    in_band = np.zeros(spec.grid.size, dtype=bool)
    g = np.full(spec.grid.size, np.nan)
    for b in range(bands):
        a, e = int(request.starts[b]), int(request.starts[b + 1])
        in_band[a:e] = True
        g[a:e] = (np.arange(e - a) + 0.5)/max(e - a, 1)
    if "sorted_absorption" in request.quantities:
        block = np.array(values["sorted_absorption"])
        block[:, ~in_band] = np.nan
        variables["sorted_absorption"] = (dims + ["wavenumber"],
                                          block.reshape(shape + [spec.grid.size]), units)
    if "sorted_column" in request.quantities:
        pairs = np.ascontiguousarray(values["sorted_column"]).view(np.int32)
        block = np.array(pairs[:, :spec.grid.size])
        block[:, ~in_band] = -1
        variables["sorted_column"] = (dims + ["wavenumber"],
                                      block.reshape(shape + [spec.grid.size]), {})
    coords = {"band_lower": (("band",), request.edges[:-1], {"units": "cm-1"}),
              "band_upper": (("band",), request.edges[1:], {"units": "cm-1"}),
              "band_points": (("band",), np.diff(request.starts), {}),
              "g_lower": (("g_interval",), request.g_edges[:-1], {}),
              "g_upper": (("g_interval",), request.g_edges[1:], {}),
              "g_weight": (("g_interval",), np.diff(request.g_edges), {}),
              "g_interval_points": (("band", "g_interval"),
                                    np.diff(request.interval_starts, axis=1), {}),
              "g_point": (("g_point",), request.g_points, {})}
    if "sorted_absorption" in request.quantities or "sorted_column" in request.quantities:
        coords["wavenumber"] = (("wavenumber",), spec.grid, {"units": "cm-1"})
        coords["g"] = (("wavenumber",), g, {})
    given = {} if request.weighting is None else {"weighting": request.weighting}
    xarray = _optional_xarray()
    if xarray is None:
        out = {name: value for name, (_, value, _) in coords.items()}
        out.update({name: value for name, (_, value, _) in variables.items()})
        out.update(given)
        return out
    DataArray, Dataset = xarray.DataArray, xarray.Dataset
    return Dataset(
        data_vars={name: DataArray(value, dims=d, attrs=attrs)
                   for name, (d, value, attrs) in variables.items()},
        coords={name: DataArray(value, dims=d, attrs=attrs)
                for name, (d, value, attrs) in coords.items()}, attrs=given)


def _path_variables(spec, variables, request):
    """{name: (dims, values, units)} with the grid's, the bands' or the channels' coordinates, in
    the conventions of Spectroscopy._create_output_dataset."""
    from .spectroscopy import _optional_xarray
    axis = _spectral_axis(request)
    if axis == "channel":
        instrument = request.instrument
        lower, upper = instrument.window()
        start, end = instrument.columns(spec.grid)
        coords = {"channel_center": (instrument.centers, {"units": "cm-1"}),
                  "channel_lower": (lower, {"units": "cm-1"}),
                  "channel_upper": (upper, {"units": "cm-1"}),
                  "channel_points": (end - start, {})}
    elif axis == "wavenumber":
        coords = {"wavenumber": (spec.grid, {"units": "cm-1"})}
    else:
        coords = {"band_lower": (request.edges[:-1], {"units": "cm-1"}),
                  "band_upper": (request.edges[1:], {"units": "cm-1"}),
                  "band_points": (np.diff(request.starts), {})}
    # Only a result formed with the linear-in-tau source says so: the others are as they were.
    linear = getattr(request, "edge_temperature", None) is not None
    marks = {"source": "linear_in_tau"} if linear else {}
    # Likewise the surface of compute_radiance.
    if getattr(request, "reflection_lengths", None) is not None:
        marks["surface"] = "reflecting"
    if getattr(request, "emissivity_knots", None) is not None:
        marks["emissivity"] = "spectral"
    if getattr(request, "scatterer_knots", None) is not None:
        marks["scatterer"] = "spectral"
    xarray = _optional_xarray()
    if xarray is None:
        out = {name: value for name, (value, _) in coords.items()}
        out.update({q: v for q, (_, v, _) in variables.items()})
        out.update(marks)
        return out
    DataArray, Dataset = xarray.DataArray, xarray.Dataset
    return Dataset(
        data_vars={q: DataArray(v, dims=dims, attrs={"units": units})
                   for q, (dims, v, units) in variables.items()},
        coords={name: DataArray(value, dims=(axis,), attrs=attrs)
                for name, (value, attrs) in coords.items()},
        **({"attrs": marks} if marks else {}))
