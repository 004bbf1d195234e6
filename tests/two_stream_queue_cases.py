"""What tests/test_two_stream_queues_host.py and tests/golden/make_two_stream_queues.py share: a
stand-in engine with every call of the two-stream family, and the calls of compute_solar_flux,
compute_solar_flux_spectral, compute_thermal_flux, compute_thermal_flux_linear,
compute_thermal_flux_spectral, compute_thermal_radiance and compute_solar that reach every branch
of their sweepers -- one run and two, the grid, bands and an instrument, grey and spectral
surfaces and scatterers, both ends of the paths, and one refusal per family.  run_cases() is what
tests/golden/two_stream_queues.json records: the engine calls of every case, line by line, and
the shapes of its result."""
import numpy as np

from tests import scatterer_cases
from tests import surface_cases as surface
from tests import thermal_radiance_cases


class Recorder(scatterer_cases.ScattererRecorder, thermal_radiance_cases.RadianceRecorder):
    """Every path entry of the family on one engine, and the instrument's three calls."""
    def instrument_create(self, grid, shape, centers, parameter=None, half_width=None,
                          offsets=None, response=None):
        return self._upload("instrument_create", grid=grid, shape=shape,
                            centers=np.asarray(centers), half_width=np.asarray(half_width))

    def instrument_free(self, instrument):
        self.record("instrument_free", instrument=instrument)

    def instrument_apply(self, values, rows, instrument, out, transmittance=False,
                         asynchronous=False):
        self.record("instrument_apply", values=values, rows=rows, instrument=instrument, out=out,
                    transmittance=transmittance, asynchronous=asynchronous)


THICKNESS = np.linspace(50., 300., 6).reshape(surface.SHAPE)
ONES = np.ones(surface.SHAPE)
BANDS = [20., 30., 60.]
ALBEDO_TABLE = dict(surface_albedo=[[0.2, 0.4], [0.1, 0.3]], albedo_wavenumber=[10., 70.])
EMISSIVITY_TABLE = dict(surface_emissivity=[[0.9, 0.7], [1., 0.6]],
                        emissivity_wavenumber=[10., 70.])
CLOUD = dict(scatterer_optical_depth=np.linspace(0., 2., 6).reshape(surface.SHAPE),
             scatterer_single_scattering_albedo=0.9*ONES, scatterer_asymmetry=0.8*ONES)
KNOTS = np.array([15., 40., 65.])
SPECTRAL_CLOUD = dict(
    scatterer_wavenumber=KNOTS,
    scatterer_optical_depth=np.linspace(0., 2., 18).reshape(surface.SHAPE + (3,)),
    scatterer_single_scattering_albedo=np.linspace(0.5, 1., 18).reshape(surface.SHAPE + (3,)),
    scatterer_asymmetry=np.linspace(0., 0.85, 18).reshape(surface.SHAPE + (3,)))
SOLAR = dict(layer_thickness=THICKNESS, solar_zenith_cosine=[0.5, 0.8])
THERMAL = dict(layer_thickness=THICKNESS, surface_temperature=[288., 270.])


def instrument():
    from pylbl_amd.instrument import Instrument
    return Instrument.gaussian(np.array([30., 45.]), 2.)


def cases():
    """[(name, method, device_output_limit in rows of surface.ROW_BYTES or None, the number of
    path_* calls it queues, keywords)].  A path of three levels holds 3 rows per block of a
    level: the flux sweeps take 3 blocks per level and on the grid one more per interface
    quantity, compute_thermal_radiance 5, compute_solar 2 (and cuts inside paths); a spectral
    scatterer's 3 knots add 72 bytes a level."""
    channels = instrument()
    return [
        ("solar flux: all on the grid, albedo table, first", "compute_solar_flux", None, 1, dict(
            SOLAR, surface="first", quantities=(
                "upward_flux", "downward_flux", "direct_irradiance", "diffuse_downward_flux",
                "heating_rate"), **ALBEDO_TABLE)),
        ("solar flux: all on the grid, albedo table, last, two runs", "compute_solar_flux", 41, 2,
         dict(SOLAR, surface="last", quantities=(
             "upward_flux", "downward_flux", "direct_irradiance", "diffuse_downward_flux",
             "heating_rate"), **ALBEDO_TABLE)),
        ("solar flux: grey scatterer, two runs", "compute_solar_flux", 29, 2, dict(
            SOLAR, surface_albedo=[0.1, 0.3], **CLOUD)),
        ("solar flux: rayleigh_cross_section given", "compute_solar_flux", None, 1, dict(
            SOLAR, rayleigh_cross_section=np.linspace(1e-31, 3e-31, 160))),
        ("solar flux: no Rayleigh, bands, scalar albedo", "compute_solar_flux", None, 1, dict(
            layer_thickness=THICKNESS, solar_zenith_cosine=0.5, rayleigh=False,
            surface_albedo=0.3, band_edges=BANDS, quantities=("upward_flux", "heating_rate"))),
        ("solar flux: one path does not fit", "compute_solar_flux", 14, 0, dict(SOLAR)),
        ("solar flux spectral: grid, two runs", "compute_solar_flux_spectral", 29, 2, dict(
            SOLAR, **SPECTRAL_CLOUD)),
        ("solar flux spectral: bands", "compute_solar_flux_spectral", None, 1, dict(
            SOLAR, band_edges=BANDS, surface="last", **SPECTRAL_CLOUD)),
        ("thermal flux: clear, scalar emissivity, first", "compute_thermal_flux", None, 1, dict(
            THERMAL, surface_emissivity=0.9)),
        ("thermal flux: cloudy, emissivity table, last, two runs", "compute_thermal_flux", 29, 2,
         dict(THERMAL, surface="last", diffusivity=2., **EMISSIVITY_TABLE, **CLOUD)),
        ("thermal flux: cloudy, bands, heating rate, two runs", "compute_thermal_flux", 17, 2,
         dict(THERMAL, band_edges=BANDS, quantities=("downward_flux", "heating_rate"), **CLOUD)),
        ("thermal flux: one path does not fit", "compute_thermal_flux", 14, 0, dict(THERMAL)),
        ("thermal flux linear: grid, two runs", "compute_thermal_flux_linear", 29, 2, dict(
            THERMAL, interface_temperature=surface.interfaces(), **CLOUD)),
        ("thermal flux linear: bands, two runs", "compute_thermal_flux_linear", 17, 2, dict(
            THERMAL, interface_temperature=surface.interfaces(), band_edges=BANDS,
            surface="last", **EMISSIVITY_TABLE)),
        ("thermal flux spectral: isothermal, two runs", "compute_thermal_flux_spectral", 29, 2,
         dict(THERMAL, **SPECTRAL_CLOUD)),
        ("thermal flux spectral: linear, two runs", "compute_thermal_flux_spectral", 29, 2, dict(
            THERMAL, interface_temperature=surface.interfaces(), quantities="heating_rate",
            **SPECTRAL_CLOUD)),
        ("thermal radiance: both on the grid, emissivity table, two runs",
         "compute_thermal_radiance", 29, 4, dict(
             THERMAL, view_zenith_cosine=[1., 0.4], surface="last",
             quantities=("radiance", "brightness_temperature"), **EMISSIVITY_TABLE, **CLOUD)),
        ("thermal radiance: bands", "compute_thermal_radiance", None, 2, dict(
            THERMAL, surface_emissivity=0.3, band_edges=BANDS)),
        ("thermal radiance: instrument, brightness temperature", "compute_thermal_radiance", None,
         2, dict(THERMAL, instrument=channels, quantities=("radiance", "brightness_temperature"),
                 **CLOUD)),
        ("thermal radiance: one path does not fit", "compute_thermal_radiance", 14, 0,
         dict(THERMAL)),
        ("solar: grid, irradiance and heating rate, two runs", "compute_solar", 8, 2, dict(
            SOLAR, quantities=("direct_irradiance", "heating_rate"))),
        ("solar: bands, irradiance and heating rate, two runs", "compute_solar", 8, 2, dict(
            SOLAR, surface="last", band_edges=BANDS,
            quantities=("direct_irradiance", "heating_rate"))),
        ("solar: albedo table, viewer, every quantity", "compute_solar", None, 1, dict(
            SOLAR, view_path_length=2.*THICKNESS, quantities=(
                "direct_irradiance", "surface_irradiance", "reflected_radiance", "heating_rate"),
            **ALBEDO_TABLE)),
        ("solar: instrument on the per-path quantities", "compute_solar", None, 1, dict(
            SOLAR, surface_albedo=0.3, view_path_length=THICKNESS, instrument=channels,
            quantities=("surface_irradiance", "reflected_radiance"))),
    ]


def run_cases(directory):
    """{case: {"log": [...], "result": {key: shape, or the mark itself}}} of cases(), all in one
    recorder session in their order; a refusal is recorded as its message."""
    from pylbl_amd import spectroscopy
    before_recorder, before_xarray = surface.SurfaceRecorder, spectroscopy._XARRAY
    surface.SurfaceRecorder, spectroscopy._XARRAY = Recorder, [None]
    records = {}
    try:
        with surface.recorded(directory) as (spec, engine):
            for name, method, limit_rows, sweeps, keywords in cases():
                spec.device_output_limit = (8 << 30) if limit_rows is None else \
                    limit_rows*surface.ROW_BYTES
                engine.begin()
                try:
                    values = getattr(spec, method)(**keywords)
                    result = {key: list(value.shape) if isinstance(value, np.ndarray) else value
                              for key, value in values.items()}
                except ValueError as error:
                    result = str(error)
                    assert "does not hold one path" in result, (name, result)
                log = list(engine.log)
                # Every case cuts the runs it says it does.
                assert sum(line.startswith("path_") for line in log) == sweeps, name
                records[name] = {"log": log, "result": result}
    finally:
        surface.SurfaceRecorder, spectroscopy._XARRAY = before_recorder, before_xarray
    return records
