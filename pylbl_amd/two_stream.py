"""The two-stream products of Spectroscopy -- compute_solar_flux, compute_solar_flux_spectral,
compute_thermal_flux, compute_thermal_flux_linear, compute_thermal_flux_spectral,
compute_thermal_radiance, compute_thermal_radiance_linear, compute_thermal_radiance_at,
compute_solar_radiance, compute_thermal_radiance_spectral and compute_solar_radiance_spectral -- on
the host: their requests (every
argument checked before anything touches the GPU), their sweeps and their results.  The functions
take the Spectroscopy first; the public methods with the definitions are in spectroscopy.py, the
run loop, the helpers every path product shares and the public constants in paths.py, which does
not import this module.

One frame serves the sweeps.  A call holds whole paths per run (paths._sweep_runs with
whole_paths), in the Sun's order from space to the surface; its rows that do not depend on the
run -- S, sigma, a spectral surface -- are blocks filled once before the first sweep
(paths._FilledOnce); with bands the entries write their rows into blocks of the call and the
outputs receive the means (paths._Rows).  _flux_sweep is that frame for the two flux products:
what a product supplies is the blocks it takes, its fills, and which entry it calls with which
tables (solar_flux, thermal_flux).  thermal_radiance is the same frame with one more entry
behind the flux entry and compute_radiance's result, and solar_radiance is that again on the
shortwave flux entry.
"""
from collections import namedtuple

import numpy as np

from .paths import (_COMMON, DIFFUSIVITY_RANGE, FLUX_SURFACES, K_B, MAX_SCATTERER_KNOTS,
                    RADIANCE_QUANTITIES, SOLAR_FLUX_INTERFACE_QUANTITIES, SOLAR_FLUX_QUANTITIES,
                    THERMAL_FLUX_QUANTITIES, _FilledOnce, _Pass, _Product, _Rows,
                    _band_widths, _channel_brightness, _check_level_temperatures,
                    _check_pressures, _check_range_policy, _create_flux_dataset,
                    _create_path_dataset, _edge_temperatures, _emitter, _first_rows,
                    _interface_rows, _level_heating, _path_bands, _path_geometry, _path_layout,
                    _per_path, _selection, _solar_spectrum, _spectral_emissivity,
                    _swept_radiance)

# compute_solar_flux's: mu0 per path, the level table [levels, 5] of lbl_path_two_stream (s_l, c_l,
# tau_c, w_c, h_c), the albedo per path -- [paths], or [paths, M] at albedo_knots [M] -- the Sun
# as in paths._SolarRequest, and rayleigh_values: None (the fit, or no Rayleigh scattering:
# `rayleigh`) or the caller's cross-sections [V] on the grid.  scatterer_knots [M] and
# scatterer_optics [levels, M, 3] (tau_c, omega_c, g_c at every knot): None, or the spectral
# scatterer of lbl_path_two_stream_spectral, beside which tau_c, w_c and h_c of the level table
# are 0.
_SolarFluxRequest = namedtuple("_SolarFluxRequest", _COMMON + (
    "surface", "mu0", "level_table", "albedo", "albedo_knots", "solar_knots", "solar_values",
    "scale", "rayleigh", "rayleigh_values", "scatterer_knots", "scatterer_optics"),
    defaults=(None, None))

# compute_thermal_flux's: the level table [levels, 5] of lbl_path_thermal_two_stream (s_l, tau_c,
# w_c, g_c, T_l), D, the surface temperature per path and its emissivity -- [paths], or [paths, M]
# at emissivity_knots [M].  edge_temperature: None (compute_thermal_flux: isothermal levels) or
# compute_thermal_flux_linear's interface temperatures per flat level (paths._edge_temperatures).
# scatterer_knots and scatterer_optics as in _SolarFluxRequest
# (lbl_path_thermal_two_stream_spectral: tau_c, w_c and g_c of the level table are 0 beside them).
_ThermalFluxRequest = namedtuple("_ThermalFluxRequest", _COMMON + (
    "surface", "level_table", "diffusivity", "surface_temperature", "surface_emissivity",
    "emissivity_knots", "edge_temperature", "scatterer_knots", "scatterer_optics"),
    defaults=(None, None, None))

# compute_thermal_radiance's: _ThermalFluxRequest's (edge_temperature stays None unless the call
# is compute_thermal_radiance_linear; the scatterer knots too, unless it is
# compute_thermal_radiance_spectral) with mu, the viewing zenith cosine of every path; its
# quantities are RADIANCE_QUANTITIES.
_ThermalRadianceRequest = namedtuple("_ThermalRadianceRequest",
                                     _ThermalFluxRequest._fields + ("mu",))

# compute_thermal_radiance_at's: _ThermalRadianceRequest's (edge_temperature: its
# interface_temperature, or None) with the observer: observer_interface [paths], the interface of
# compute_thermal_flux's "interface" dim at which every path's observer stands, `looking` ("down" or
# "up") and observer_levels [paths], int32: n_p, the levels the ray passes on its way there.
_ThermalObserverRequest = namedtuple(
    "_ThermalObserverRequest",
    _ThermalRadianceRequest._fields + ("observer_interface", "looking", "observer_levels"))
LOOKING = ("down", "up")

# compute_solar_radiance's: _SolarFluxRequest's (the scatterer knots stay None unless the call is
# compute_solar_radiance_spectral) with mu, the viewing
# zenith cosine, and cos_theta, the cosine of the scattering angle, of every path; its quantity is
# "radiance".
_SolarRadianceRequest = namedtuple("_SolarRadianceRequest",
                                   _SolarFluxRequest._fields + ("mu", "cos_theta"))
SOLAR_RADIANCE_QUANTITIES = RADIANCE_QUANTITIES[:1]

# What the entries call the rows of a quantity, and of what the sweep writes at interface 0
# beside it ("top_" + quantity: a per-path output of the pass).
_TOP = "top_"
_TWO_STREAM_ROWS = {"upward_flux": "up", "downward_flux": "down", "direct_irradiance": "direct",
                    "diffuse_downward_flux": "diffuse"}
_TWO_STREAM_ROWS.update({_TOP + q: _TOP + name for q, name in tuple(_TWO_STREAM_ROWS.items())})
_RADIANCE_ROWS = {"radiance": "radiance", "brightness_temperature": "brightness"}


# ---------------------------------------------------------------------------------------------
# The requests.
def _scatterer_arrays(shape, optical_depth, single_scattering_albedo, asymmetry, knots=None):
    """None without a scatterer, or its (tau_c, omega_c, g_c), checked: each shaped like the
    atmosphere -- with `knots` [M] like the atmosphere with one more axis of M at the end --,
    finite and in its range."""
    given = [x is not None for x in (optical_depth, single_scattering_albedo, asymmetry)]
    if not any(given):
        return None
    if not all(given):
        raise ValueError("scatterer_optical_depth, scatterer_single_scattering_albedo and "
                         "scatterer_asymmetry are given together or not at all.")
    expected = tuple(shape) + (() if knots is None else (knots.size,))
    arrays = []
    for name, value in (("scatterer_optical_depth", optical_depth),
                        ("scatterer_single_scattering_albedo", single_scattering_albedo),
                        ("scatterer_asymmetry", asymmetry)):
        value = np.asarray(value, dtype=np.float64)
        if value.shape != expected:
            if knots is not None:
                raise ValueError(f"{name} has shape {value.shape}: with scatterer_wavenumber "
                                 f"give the atmosphere's shape and one value per knot, "
                                 f"{expected}.")
            raise ValueError(f"{name} has shape {value.shape}, the atmosphere {shape}.")
        if not np.all(np.isfinite(value)):
            raise ValueError(f"{name} must be finite.")
        arrays.append(value)
    tau_c, omega_c, g_c = arrays
    if np.any(tau_c < 0.):
        raise ValueError("scatterer_optical_depth must be >= 0.")
    if not np.all((omega_c >= 0.) & (omega_c <= 1.)):
        raise ValueError("scatterer_single_scattering_albedo must lie in [0, 1].")
    if not np.all((g_c >= 0.) & (g_c < 1.)):
        raise ValueError("scatterer_asymmetry must lie in [0, 1).")
    return tau_c, omega_c, g_c


def _given_knots(wavenumber):
    """scatterer_wavenumber of the *_spectral calls, which need it."""
    if wavenumber is None:
        raise ValueError("scatterer_wavenumber must be given: [M] knots in cm-1.")
    return wavenumber


def _spectral_scatterers(shape, wavenumber, optical_depth, single_scattering_albedo, asymmetry):
    """(None, None) without scatterer_wavenumber, or (knots [M], optics [levels, M, 3]) of the
    spectral scatterer, checked: M knots [cm-1], finite and strictly ascending, 2 <= M <= 1024,
    and tau_c, omega_c and g_c of every level at every knot, which the kernels interpolate
    linearly in wavenumber and hold constant outside the knots (include/lbl_amd_scatterer.h)."""
    if wavenumber is None:
        return None, None
    knots = np.asarray(wavenumber, dtype=np.float64)
    if knots.ndim != 1 or not 2 <= knots.size <= MAX_SCATTERER_KNOTS:
        raise ValueError(f"scatterer_wavenumber must be a 1-d array of 2..{MAX_SCATTERER_KNOTS} "
                         f"knots, not of shape {knots.shape}.")
    if not np.all(np.isfinite(knots)) or not np.all(np.diff(knots) > 0.):
        raise ValueError("scatterer_wavenumber must be finite and strictly ascending.")
    arrays = _scatterer_arrays(shape, optical_depth, single_scattering_albedo, asymmetry, knots)
    if arrays is None:
        raise ValueError("scatterer_wavenumber needs scatterer_optical_depth, "
                         "scatterer_single_scattering_albedo and scatterer_asymmetry at its "
                         "knots.")
    optics = np.stack([x.reshape(-1, knots.size) for x in arrays], axis=2)
    return np.ascontiguousarray(knots), np.ascontiguousarray(optics)


def _scatterers(spec, shape, optical_depth, single_scattering_albedo, asymmetry):
    """(tau_c, w_c, h_c, g_c) per flat level of the grey scatterer, checked: zeros without one;
    w_c = omega_c*tau_c and h_c = (omega_c*tau_c)*g_c in fp64."""
    levels = int(np.prod(shape, dtype=np.int64))
    arrays = _scatterer_arrays(shape, optical_depth, single_scattering_albedo, asymmetry)
    if arrays is None:
        return np.zeros(levels), np.zeros(levels), np.zeros(levels), np.zeros(levels)
    tau_c, omega_c, g_c = (x.ravel() for x in arrays)
    w_c = omega_c*tau_c
    return tau_c, w_c, w_c*g_c, g_c


# The front the solar and the thermal request share: _layers first and _level_scatterers behind
# the product's own checks, which lie between them where they always lay, so that the same error
# wins as before; then range_policy and the bands.
def _layers(spec, layer_thickness, surface, caller, emitting):
    """(flat thicknesses, atmosphere shape) of a two-stream call: no group, the geometry, the
    level temperatures of an atmosphere that emits, and `surface`."""
    if spec.group is not None:
        raise NotImplementedError(f"{caller} does not split paths over processes yet "
                                  "(group is set).")
    lengths, shape = _path_geometry(spec, layer_thickness, caller,
                                    "layer_thickness", "layer thicknesses")
    if emitting:
        _check_level_temperatures(spec)
    if not (isinstance(surface, str) and surface in FLUX_SURFACES):
        raise ValueError(f"surface must be one of {FLUX_SURFACES}, not {surface!r}.")
    return lengths, shape


def _level_scatterers(spec, shape, wavenumber, optical_depth, single_scattering_albedo,
                      asymmetry):
    """(knots, optics, (tau_c, w_c, h_c, g_c)): the spectral scatterer (_spectral_scatterers),
    beside which the grey one of the level table is zeros, or the grey one (_scatterers)."""
    knots, optics = _spectral_scatterers(shape, wavenumber, optical_depth,
                                         single_scattering_albedo, asymmetry)
    grey = (None, None, None) if knots is not None else (
        optical_depth, single_scattering_albedo, asymmetry)
    return knots, optics, _scatterers(spec, shape, *grey)


def _solar_flux_request(spec, layer_thickness, solar_zenith_cosine, solar_irradiance,
                        solar_wavenumber, distance_factor, surface, surface_albedo,
                        albedo_wavenumber, rayleigh, rayleigh_cross_section,
                        scatterer_optical_depth, scatterer_single_scattering_albedo,
                        scatterer_asymmetry, quantities, band_edges, range_policy,
                        scatterer_wavenumber=None, caller="compute_solar_flux"):
    """Checks every argument of compute_solar_flux (of `caller`, which shares them)."""
    lengths, shape = _layers(spec, layer_thickness, surface, caller, emitting=False)
    mu0 = _per_path(solar_zenith_cosine, "solar_zenith_cosine", shape)
    if not np.all((mu0 > 0.) & (mu0 <= 1.)):
        raise ValueError("solar_zenith_cosine must lie in (0, 1].")
    solar_knots, solar_values, scale = _solar_spectrum(spec, solar_irradiance, solar_wavenumber,
                                                       distance_factor)
    albedo_knots = None
    if albedo_wavenumber is None:
        albedo = _per_path(surface_albedo, "surface_albedo", shape)
        if not np.all((albedo >= 0.) & (albedo <= 1.)):
            raise ValueError("surface albedos must lie in [0, 1].")
    else:
        albedo_knots, albedo = _spectral_emissivity(
            albedo_wavenumber, surface_albedo, shape,
            ("albedo_wavenumber", "surface_albedo", "surface albedos"))
    if not isinstance(rayleigh, (bool, np.bool_)):
        raise ValueError(f"rayleigh must be True or False, not {rayleigh!r}.")
    quantities = _selection(quantities, SOLAR_FLUX_QUANTITIES)
    rayleigh_values = None
    if rayleigh_cross_section is not None:
        if not rayleigh:
            raise ValueError("rayleigh_cross_section is only used with rayleigh=True.")
        rayleigh_values = np.asarray(rayleigh_cross_section, dtype=np.float64)
        if rayleigh_values.shape != (spec.grid.size,):
            raise ValueError(f"rayleigh_cross_section has shape {rayleigh_values.shape}: give "
                             f"one value per grid point, [{spec.grid.size}].")
        if not np.all(np.isfinite(rayleigh_values)) or np.any(rayleigh_values < 0.):
            raise ValueError("Rayleigh cross-sections must be finite and >= 0.")
        rayleigh_values = np.ascontiguousarray(rayleigh_values)
    if rayleigh or "heating_rate" in quantities:
        _check_pressures(spec, "Rayleigh scattering needs" if rayleigh else "heating rates need")
        _check_level_temperatures(spec)
    knots, optics, (tau_c, w_c, h_c, _) = _level_scatterers(
        spec, shape, scatterer_wavenumber, scatterer_optical_depth,
        scatterer_single_scattering_albedo, scatterer_asymmetry)
    column = np.zeros(lengths.size)
    if rayleigh:
        column = (np.asarray(spec.atmosphere.pressure, dtype=np.float64).ravel() /
                  (K_B*np.asarray(spec.atmosphere.temperature, dtype=np.float64).ravel()))*lengths
        if not np.all(np.isfinite(column)):
            raise ValueError("the air columns (p/(K_B*T))*layer_thickness must be finite.")
    _check_range_policy(range_policy)
    edges, starts = _path_bands(spec, band_edges)
    table = np.ascontiguousarray(np.stack([lengths, column, tau_c, w_c, h_c], axis=1))
    return _SolarFluxRequest(lengths=lengths, shape=shape, quantities=quantities, edges=edges,
                             starts=starts, instrument=None, cumulative=False, surface=surface,
                             mu0=mu0, level_table=table, albedo=albedo, albedo_knots=albedo_knots,
                             solar_knots=solar_knots, solar_values=solar_values, scale=scale,
                             rayleigh=bool(rayleigh), rayleigh_values=rayleigh_values,
                             scatterer_knots=knots, scatterer_optics=optics)


def _thermal_flux_request(spec, layer_thickness, surface_temperature, surface_emissivity,
                          emissivity_wavenumber, surface, diffusivity, scatterer_optical_depth,
                          scatterer_single_scattering_albedo, scatterer_asymmetry, quantities,
                          band_edges, range_policy, scatterer_wavenumber=None,
                          caller="compute_thermal_flux"):
    """Checks every argument of compute_thermal_flux (of `caller`, which shares them)."""
    lengths, shape = _layers(spec, layer_thickness, surface, caller, emitting=True)
    factor = np.asarray(diffusivity, dtype=np.float64)
    low, high = DIFFUSIVITY_RANGE
    if factor.shape != () or not low <= factor <= high:
        raise ValueError(f"diffusivity must be one number in [{low:g}, {high:g}].")
    emissivity_knots = None
    if emissivity_wavenumber is None:
        ts, es = _emitter(surface_temperature, surface_emissivity, "surface", shape)
    else:
        ts, _ = _emitter(surface_temperature, 1., "surface", shape)
        emissivity_knots, es = _spectral_emissivity(
            emissivity_wavenumber, surface_emissivity, shape,
            ("emissivity_wavenumber", "surface_emissivity", "surface emissivities"))
    quantities = _selection(quantities, THERMAL_FLUX_QUANTITIES)
    if "heating_rate" in quantities:
        _check_pressures(spec, "heating rates need")
    knots, optics, (tau_c, w_c, _, g_c) = _level_scatterers(
        spec, shape, scatterer_wavenumber, scatterer_optical_depth,
        scatterer_single_scattering_albedo, scatterer_asymmetry)
    _check_range_policy(range_policy)
    edges, starts = _path_bands(spec, band_edges)
    temperature = np.asarray(spec.atmosphere.temperature, dtype=np.float64).ravel()
    table = np.ascontiguousarray(np.stack([lengths, tau_c, w_c, g_c, temperature], axis=1))
    return _ThermalFluxRequest(lengths=lengths, shape=shape, quantities=quantities, edges=edges,
                               starts=starts, instrument=None, cumulative=False, surface=surface,
                               level_table=table, diffusivity=float(factor),
                               surface_temperature=ts, surface_emissivity=es,
                               emissivity_knots=emissivity_knots, scatterer_knots=knots,
                               scatterer_optics=optics)


def _thermal_flux_linear_request(spec, layer_thickness, surface_temperature,
                                 interface_temperature, *arguments, scatterer_wavenumber=None,
                                 caller="compute_thermal_flux_linear"):
    """Checks every argument of compute_thermal_flux_linear: compute_thermal_flux's request with
    the interface temperatures of the linear-in-tau source."""
    request = _thermal_flux_request(spec, layer_thickness, surface_temperature, *arguments,
                                    scatterer_wavenumber=scatterer_wavenumber, caller=caller)
    return request._replace(edge_temperature=_edge_temperatures(
        "linear_in_tau", interface_temperature, request.shape))


def _thermal_radiance_request(spec, layer_thickness, surface_temperature, view_zenith_cosine,
                              surface_emissivity, emissivity_wavenumber, surface, diffusivity,
                              scatterer_optical_depth, scatterer_single_scattering_albedo,
                              scatterer_asymmetry, quantities, band_edges, instrument,
                              range_policy, scatterer_wavenumber=None,
                              caller="compute_thermal_radiance"):
    """Checks every argument of compute_thermal_radiance (of `caller`, which shares them):
    compute_thermal_flux's checks of the atmosphere, the surface, D and the scatterer, the view,
    and compute_radiance's rules for the quantities, the bands and the instrument."""
    flux = _thermal_flux_request(
        spec, layer_thickness, surface_temperature, surface_emissivity, emissivity_wavenumber,
        surface, diffusivity, scatterer_optical_depth, scatterer_single_scattering_albedo,
        scatterer_asymmetry, THERMAL_FLUX_QUANTITIES[:2], None, range_policy,
        scatterer_wavenumber=scatterer_wavenumber, caller=caller)
    mu = _per_path(view_zenith_cosine, "view_zenith_cosine", flux.shape)
    if not np.all((mu > 0.) & (mu <= 1.)):
        raise ValueError("view_zenith_cosine must lie in (0, 1].")
    quantities = _selection(quantities, RADIANCE_QUANTITIES)
    if band_edges is not None and "brightness_temperature" in quantities:
        raise ValueError("brightness_temperature is only available on the grid: band means "
                         "are formed of the radiance alone.")
    edges, starts = _path_bands(spec, band_edges, instrument)
    return _ThermalRadianceRequest(*flux._replace(quantities=quantities, edges=edges,
                                                  starts=starts, instrument=instrument), mu=mu)


def _thermal_radiance_linear_request(spec, layer_thickness, surface_temperature,
                                     interface_temperature, view_zenith_cosine, *arguments):
    """Checks every argument of compute_thermal_radiance_linear: compute_thermal_radiance's
    request with the interface temperatures of the linear-in-tau source."""
    request = _thermal_radiance_request(spec, layer_thickness, surface_temperature,
                                        view_zenith_cosine, *arguments,
                                        caller="compute_thermal_radiance_linear")
    return request._replace(edge_temperature=_edge_temperatures(
        "linear_in_tau", interface_temperature, request.shape))


def _observer_levels(observer_interface, looking, surface, shape):
    """(observer_interface, n_p), one of each per path: the interface (0 ... L, on the level-0
    side of level i, L beyond the last level; None: the far end of the view) and the levels the
    ray passes -- looking down those between the surface and the observer, looking up those
    between space and the observer."""
    if looking not in LOOKING:
        raise ValueError(f'looking must be "down" or "up", not {looking!r}.')
    levels, per_path_shape = int(shape[-1]), tuple(shape[:-1])
    # The surface is at interface 0 ("first") or L; the far end of a view down is space.
    surface_at_zero = surface == "first"
    if observer_interface is None:
        observer_interface = levels if surface_at_zero == (looking == "down") else 0
    given = np.asarray(observer_interface)
    if given.dtype.kind not in "iu":
        raise ValueError("observer_interface must be an integer, or integers, one per path.")
    if given.shape not in ((), per_path_shape):
        raise ValueError(f"observer_interface has shape {given.shape}: give one integer or one "
                         f"per path, shaped {per_path_shape}.")
    if np.any(given < 0) or np.any(given > levels):
        raise ValueError(f"observer_interface must lie in 0 ... {levels}, the interfaces of the "
                         "atmosphere.")
    interface = np.ascontiguousarray(np.broadcast_to(given, per_path_shape).ravel(),
                                     dtype=np.int64)
    from_zero = surface_at_zero == (looking == "down")
    passed = interface if from_zero else levels - interface
    return interface, np.ascontiguousarray(passed, dtype=np.int32)


def _thermal_radiance_at_request(spec, layer_thickness, surface_temperature, observer_interface,
                                 looking, interface_temperature, view_zenith_cosine,
                                 surface_emissivity, emissivity_wavenumber, surface, *arguments):
    """Checks every argument of compute_thermal_radiance_at: compute_thermal_radiance's request,
    with interface temperatures compute_thermal_radiance_linear's, and the observer."""
    request = _thermal_radiance_request(spec, layer_thickness, surface_temperature,
                                        view_zenith_cosine, surface_emissivity,
                                        emissivity_wavenumber, surface, *arguments,
                                        caller="compute_thermal_radiance_at")
    if interface_temperature is not None:
        request = request._replace(edge_temperature=_edge_temperatures(
            "linear_in_tau", interface_temperature, request.shape))
    interface, passed = _observer_levels(observer_interface, looking, surface, request.shape)
    return _ThermalObserverRequest(*request, observer_interface=interface, looking=looking,
                                   observer_levels=passed)


def _solar_radiance_request(spec, layer_thickness, solar_zenith_cosine, view_zenith_cosine,
                            relative_azimuth, solar_irradiance, solar_wavenumber, distance_factor,
                            surface, surface_albedo, albedo_wavenumber, rayleigh,
                            rayleigh_cross_section, scatterer_optical_depth,
                            scatterer_single_scattering_albedo, scatterer_asymmetry, quantities,
                            band_edges, instrument, range_policy, scatterer_wavenumber=None,
                            caller="compute_solar_radiance"):
    """Checks every argument of compute_solar_radiance (of `caller`, which shares them):
    compute_solar_flux's checks of the
    atmosphere, the Sun, the surface, the Rayleigh row and the scatterer, the view, and
    compute_thermal_radiance's rules for the bands and the instrument.  cos_theta is formed
    here, in float64 and as written:
        cosT = -mu*mu0 + (sqrt((1 - mu)*(1 + mu))*sqrt((1 - mu0)*(1 + mu0)))*cos(phi*pi/180)
    limited to [-1, 1]."""
    flux = _solar_flux_request(
        spec, layer_thickness, solar_zenith_cosine, solar_irradiance, solar_wavenumber,
        distance_factor, surface, surface_albedo, albedo_wavenumber, rayleigh,
        rayleigh_cross_section, scatterer_optical_depth, scatterer_single_scattering_albedo,
        scatterer_asymmetry, SOLAR_FLUX_INTERFACE_QUANTITIES[:1], None, range_policy,
        scatterer_wavenumber=scatterer_wavenumber, caller=caller)
    mu = _per_path(view_zenith_cosine, "view_zenith_cosine", flux.shape)
    if not np.all((mu > 0.) & (mu <= 1.)):
        raise ValueError("view_zenith_cosine must lie in (0, 1].")
    phi = _per_path(relative_azimuth, "relative_azimuth", flux.shape)
    if not np.all(np.isfinite(phi)):
        raise ValueError("relative_azimuth must be finite [degrees].")
    mu0 = flux.mu0
    cos_theta = -mu*mu0 + (np.sqrt((1. - mu)*(1. + mu))*np.sqrt((1. - mu0)*(1. + mu0))) * \
        np.cos(phi*np.pi/180.)
    cos_theta = np.ascontiguousarray(np.minimum(np.maximum(cos_theta, -1.), 1.))
    quantities = _selection(quantities, SOLAR_RADIANCE_QUANTITIES)
    edges, starts = _path_bands(spec, band_edges, instrument)
    return _SolarRadianceRequest(*flux._replace(quantities=quantities, edges=edges,
                                                starts=starts, instrument=instrument),
                                 mu=mu, cos_theta=cos_theta)


# ---------------------------------------------------------------------------------------------
# The sweeps.
def _flux_sweep(spec, request, remove_pedestal, range_policy, interface_quantities, product):
    """The result of a two-stream flux call: one pass in the Sun's order over runs of whole
    paths, every run one call of the product's entry.  product(call, fills) takes the product's
    blocks (fills: paths._FilledOnce, for those filled once) and returns entry(beta, a, b, work,
    **keywords), which queues the run of the flat levels [a, b): `keywords` are the run's bands,
    order and row blocks, the same for every product."""
    heating = "heating_rate" in request.quantities
    wanted = tuple(q for q in interface_quantities
                   if q in request.quantities or
                   (heating and q in ("upward_flux", "downward_flux")))
    # From space to the surface: "first" has its surface at level 0.
    step = _Pass(request.surface == "first", wanted, tuple(_TOP + q for q in wanted))

    def sweeper(call, run):
        fills = _FilledOnce(call)
        work = call.take(2*run)
        entry = product(call, fills)
        rows = _Rows(call, step, run, request.starts is not None)

        def sweep(index, beta, a, b, outputs):
            fills.queue()
            entry(beta, a, b, _first_rows(work, 2*(b - a)), band_start=request.starts,
                  from_last=step.from_last, asynchronous=True,
                  **rows.keywords(_TWO_STREAM_ROWS, outputs, b - a))
        return sweep
    # Three blocks per level: beta and the two work rows; the interface rows on the grid
    # count as compute_jacobian's do.
    values = spec._sweep_runs(request, [step], remove_pedestal, range_policy, sweeper,
                              level_blocks=3, grid_outputs=True, whole_paths=True)
    return _create_flux_dataset(spec, _solar_flux_interfaces(spec, values, request), request)


def solar_flux(spec, request, remove_pedestal, range_policy):
    """The sweeps of compute_solar_flux and, where the request holds a knot table, of
    compute_solar_flux_spectral."""
    def product(call, fills):
        solar = fills.solar_row(request)
        sigma = fills.rayleigh_row(request.rayleigh_values) if request.rayleigh else None
        albedo_rows = fills.surface_rows(request.albedo_knots, request.albedo)
        surface = dict(rayleigh_row=sigma, albedo_rows=albedo_rows,
                       albedo=None if albedo_rows is not None else request.albedo)

        def entry(beta, a, b, work, **keywords):
            if request.scatterer_knots is None:
                call.engine.path_two_stream(
                    beta, call.columns, call.paths, call.per_path, a, request.level_table[a:b],
                    request.mu0, solar, work, **surface, **keywords)
            else:
                call.engine.path_two_stream_spectral(
                    beta, call.columns, fills.grid, call.paths, call.per_path, a,
                    request.level_table[a:b], request.scatterer_knots,
                    request.scatterer_optics[a:b], request.mu0, solar, work, **surface,
                    **keywords)
        return entry
    return _flux_sweep(spec, request, remove_pedestal, range_policy,
                       SOLAR_FLUX_INTERFACE_QUANTITIES, product)


def _thermal_surface(request, fills):
    """The keywords of the thermal entries that say what lies below the paths."""
    emissivity_rows = fills.surface_rows(request.emissivity_knots, request.surface_emissivity)
    return dict(diffusivity=request.diffusivity, emissivity_rows=emissivity_rows,
                emissivity=None if emissivity_rows is not None else request.surface_emissivity)


def thermal_flux(spec, request, remove_pedestal, range_policy):
    """The sweeps of compute_thermal_flux and, where the request holds interface temperatures or
    a knot table, of compute_thermal_flux_linear and compute_thermal_flux_spectral."""
    def product(call, fills):
        surface = _thermal_surface(request, fills)

        def entry(beta, a, b, work, **keywords):
            run = (beta, call.columns, fills.grid, call.paths, call.per_path, a,
                   request.level_table[a:b])
            edges = None if request.edge_temperature is None else request.edge_temperature[a:b]
            if request.scatterer_knots is not None:
                source = {} if edges is None else {"edge_temperature": edges}
                call.engine.path_thermal_two_stream_spectral(
                    *run, request.scatterer_knots, request.scatterer_optics[a:b],
                    request.surface_temperature, work, **source, **surface, **keywords)
            elif edges is not None:
                call.engine.path_thermal_two_stream_source(
                    *run, edges, request.surface_temperature, work, **surface, **keywords)
            else:
                call.engine.path_thermal_two_stream(
                    *run, request.surface_temperature, work, **surface, **keywords)
        return entry
    return _flux_sweep(spec, request, remove_pedestal, range_policy, THERMAL_FLUX_QUANTITIES[:2],
                       product)


def thermal_radiance(spec, request, remove_pedestal, range_policy):
    """The sweeps of compute_thermal_radiance and, where the request holds a knot table or
    interface temperatures, of compute_thermal_radiance_spectral and
    compute_thermal_radiance_linear: the flux entry into two blocks of the call, and the view
    entry behind it on the same run.  A request with an observer (compute_thermal_radiance_at)
    queues the same flux entry and the observer's view entry behind it."""
    bands = request.starts is not None
    swept = _swept_radiance(request, request.quantities)
    # From space to the surface: "first" has its surface at level 0.
    step = _Pass(request.surface == "first", (), swept)

    def sweeper(call, run):
        fills = _FilledOnce(call)
        work, up, down = call.take(2*run), call.take(run), call.take(run)
        surface = dict(_thermal_surface(request, fills), from_last=step.from_last,
                       asynchronous=True)
        # With bands the radiance on the grid is a block of this call, the output its means.
        rows = _Rows(call, step, run, bands)

        def spectral_sweep(beta, a, b, outputs, fluxes):
            # The same two entries with the knot table, whose rows are the run's.
            run = (beta, call.columns, fills.grid, call.paths, call.per_path, a,
                   request.level_table[a:b], request.scatterer_knots,
                   request.scatterer_optics[a:b])
            call.engine.path_thermal_two_stream_spectral(
                *run, request.surface_temperature, _first_rows(work, 2*(b - a)), **surface,
                **fluxes)
            blocks = dict.fromkeys(() if bands else ("radiance_rows", "brightness_rows"))
            blocks.update(rows.keywords(_RADIANCE_ROWS, outputs, b - a))
            call.engine.path_thermal_radiance_spectral(
                *run, request.mu, request.surface_temperature, band_start=request.starts,
                **surface, **fluxes, **blocks)

        def linear_sweep(beta, a, b, outputs, fluxes):
            # The same two entries with the linear-in-tau source, whose edge rows are the run's.
            run = (beta, call.columns, fills.grid, call.paths, call.per_path, a,
                   request.level_table[a:b], request.edge_temperature[a:b])
            call.engine.path_thermal_two_stream_source(
                *run, request.surface_temperature, _first_rows(work, 2*(b - a)), **surface,
                **fluxes)
            blocks = dict.fromkeys(() if bands else ("radiance_rows", "brightness_rows"))
            blocks.update(rows.keywords(_RADIANCE_ROWS, outputs, b - a))
            call.engine.path_thermal_radiance_source(
                *run, request.mu, request.surface_temperature, band_start=request.starts,
                **surface, **fluxes, **blocks)

        def observer_sweep(beta, a, b, outputs, fluxes):
            # The flux entry of the source, then the one view entry for both sources; the run's
            # paths are a//per_path ... b//per_path.
            run = (beta, call.columns, fills.grid, call.paths, call.per_path, a,
                   request.level_table[a:b])
            edges = None if request.edge_temperature is None else request.edge_temperature[a:b]
            work_rows = _first_rows(work, 2*(b - a))
            if edges is None:
                call.engine.path_thermal_two_stream(
                    *run, request.surface_temperature, work_rows, **surface, **fluxes)
            else:
                call.engine.path_thermal_two_stream_source(
                    *run, edges, request.surface_temperature, work_rows, **surface, **fluxes)
            blocks = dict.fromkeys(() if bands else ("radiance_rows", "brightness_rows"))
            blocks.update(rows.keywords(_RADIANCE_ROWS, outputs, b - a))
            call.engine.path_thermal_radiance_observer(
                *run, request.mu, request.observer_levels, request.surface_temperature,
                edge_temperature=edges, view_up=request.looking == "up",
                band_start=request.starts, **surface, **fluxes, **blocks)

        def sweep(index, beta, a, b, outputs):
            fills.queue()
            fluxes = dict(up_rows=_first_rows(up, b - a), down_rows=_first_rows(down, b - a))
            if isinstance(request, _ThermalObserverRequest):
                return observer_sweep(beta, a, b, outputs, fluxes)
            if request.scatterer_knots is not None:
                return spectral_sweep(beta, a, b, outputs, fluxes)
            if request.edge_temperature is not None:
                return linear_sweep(beta, a, b, outputs, fluxes)
            call.engine.path_thermal_two_stream(
                beta, call.columns, fills.grid, call.paths, call.per_path, a,
                request.level_table[a:b], request.surface_temperature,
                _first_rows(work, 2*(b - a)), **surface, **fluxes)
            # On the grid the entry is told of both quantities, None for the one not wanted.
            blocks = dict.fromkeys(() if bands else ("radiance_rows", "brightness_rows"))
            blocks.update(rows.keywords(_RADIANCE_ROWS, outputs, b - a))
            call.engine.path_thermal_radiance(
                beta, call.columns, fills.grid, call.paths, call.per_path, a,
                request.level_table[a:b], request.mu, request.surface_temperature,
                band_start=request.starts, **surface, **fluxes, **blocks)
        return sweep
    products = None if request.instrument is None else \
        [_Product(q, q, False) for q in swept]
    # Five blocks per level: beta, the two work rows and the two flux rows.
    values = spec._sweep_runs(request, [step], remove_pedestal, range_policy, sweeper,
                              level_blocks=5, products=products, whole_paths=True)
    return _create_path_dataset(spec, _channel_brightness(values, request), request)


def thermal_radiance_at(spec, request, remove_pedestal, range_policy):
    """compute_thermal_radiance_at: thermal_radiance's sweeps with the observer's view entry, and
    its result with the per-path coordinate observer_interface and the attribute looking."""
    result = thermal_radiance(spec, request, remove_pedestal, range_policy)
    per_path = request.observer_interface.reshape(request.shape[:-1])
    if isinstance(result, dict):
        result.update(observer_interface=per_path, looking=request.looking)
        return result
    result = result.assign_coords(
        observer_interface=(list(spec.atmosphere.dims)[:-1], per_path))
    result.attrs["looking"] = request.looking
    return result


def solar_radiance(spec, request, remove_pedestal, range_policy):
    """The sweeps of compute_solar_radiance and, where the request holds a knot table, of
    compute_solar_radiance_spectral: the flux entry into three blocks of the call, and the view
    entry behind it on the same run."""
    bands = request.starts is not None
    # From space to the surface: "first" has its surface at level 0.
    step = _Pass(request.surface == "first", (), request.quantities)

    def sweeper(call, run):
        fills = _FilledOnce(call)
        solar = fills.solar_row(request)
        sigma = fills.rayleigh_row(request.rayleigh_values) if request.rayleigh else None
        albedo_rows = fills.surface_rows(request.albedo_knots, request.albedo)
        work = call.take(2*run)
        up, direct, diffuse = call.take(run), call.take(run), call.take(run)
        surface = dict(rayleigh_row=sigma, albedo_rows=albedo_rows,
                       albedo=None if albedo_rows is not None else request.albedo,
                       from_last=step.from_last, asynchronous=True)
        # With bands the radiance on the grid is a block of this call, the output its means.
        rows = _Rows(call, step, run, bands)

        def spectral_sweep(beta, a, b, outputs, fluxes):
            # The same two entries with the knot table, whose rows are the run's.
            run = (beta, call.columns, fills.grid, call.paths, call.per_path, a,
                   request.level_table[a:b], request.scatterer_knots,
                   request.scatterer_optics[a:b], request.mu0)
            call.engine.path_two_stream_spectral(
                *run, solar, _first_rows(work, 2*(b - a)), **surface, **fluxes)
            call.engine.path_solar_radiance_spectral(
                *run, request.mu, request.cos_theta, solar, band_start=request.starts,
                **surface, **fluxes, **rows.keywords(_RADIANCE_ROWS, outputs, b - a))

        def sweep(index, beta, a, b, outputs):
            fills.queue()
            fluxes = dict(up_rows=_first_rows(up, b - a), direct_rows=_first_rows(direct, b - a),
                          diffuse_rows=_first_rows(diffuse, b - a))
            if request.scatterer_knots is not None:
                return spectral_sweep(beta, a, b, outputs, fluxes)
            call.engine.path_two_stream(
                beta, call.columns, call.paths, call.per_path, a, request.level_table[a:b],
                request.mu0, solar, _first_rows(work, 2*(b - a)), **surface, **fluxes)
            call.engine.path_solar_radiance(
                beta, call.columns, call.paths, call.per_path, a, request.level_table[a:b],
                request.mu0, request.mu, request.cos_theta, solar, band_start=request.starts,
                **surface, **fluxes, **rows.keywords(_RADIANCE_ROWS, outputs, b - a))
        return sweep
    products = None if request.instrument is None else \
        [_Product(q, q, False) for q in request.quantities]
    # Six blocks per level: beta, the two work rows and the three flux rows.
    values = spec._sweep_runs(request, [step], remove_pedestal, range_policy, sweeper,
                              level_blocks=6, products=products, whole_paths=True)
    return _create_path_dataset(spec, values, request)


# ---------------------------------------------------------------------------------------------
# The results.
def _solar_flux_interfaces(spec, values, request):
    """{quantity: [..., L + 1 or L, W]} of the flux calls from the sweep's rows: the fluxes at the
    interface below each level and at interface 0 (the space end) of each path."""
    widths = _band_widths(spec, request)
    fluxes = {q: _interface_rows(values[q], values[_TOP + q], request)*widths
              for q in SOLAR_FLUX_INTERFACE_QUANTITIES if q in values}
    per_path, _ = _path_layout(request.shape)
    out = {q: fluxes[q].reshape(list(request.shape[:-1]) + [per_path + 1, -1])
           for q in SOLAR_FLUX_INTERFACE_QUANTITIES if q in request.quantities}
    if "heating_rate" in request.quantities:
        out["heating_rate"] = _level_heating(spec, fluxes["upward_flux"],
                                             fluxes["downward_flux"], request)
    return out
