"""Spectroscopy.compute_radiance / compute_path with `instrument` on the GPU against the numpy
weighted mean of Instrument.response over the same Spectroscopy's fine-grid rows; NaN rules,
band means, determinism, runs of levels, tiles and segments, and the C ABI's checks."""
from ctypes import byref, c_int32

import numpy as np
import pytest

from pylbl_amd import EngineError, Instrument, MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd.instrument import brightness_temperature
from pylbl_amd.spectroscopy import band_columns

pytestmark = pytest.mark.gpu

GASES = ("H2O", "CO2", "O3")
SHAPE = (2, 5)
GRID = np.arange(600., 700., 0.01)
_TABLES = {}


def spectroscopy(shape=SHAPE, grid=GRID, **keywords):
    if "small" not in _TABLES:
        _TABLES["small"] = [synthetic.line_table(name, 576., 724., num_lines=3000, seed=40 + i)
                            for i, name in enumerate(GASES)]
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    atmos = synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                            vmr={k: full.vmr[k].reshape(shape) for k in GASES})
    return Spectroscopy(atmos, grid, MemoryDatabase(_TABLES["small"]), **keywords)


def lengths(shape=SHAPE, seed=0):
    return np.random.default_rng(seed).uniform(0.5, 1.5, size=shape)*200.


def reference(instrument, grid, rows):
    """numpy: the weighted mean and its error bound 1e-12 * sum|w v| / |sum w| per channel."""
    w = instrument.response(grid)
    total = w.sum(axis=1)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, grid.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (rows @ w.T)/total
        bound = 1e-12*(np.abs(rows) @ np.abs(w).T)/np.abs(total)
    bad = ~instrument.covered(grid) | ~(total > 0.)
    return np.where(bad, np.nan, mean), bound


def check(got, instrument, grid, rows):
    expected, bound = reference(instrument, grid, rows)
    got = np.asarray(got).reshape(expected.shape)
    assert np.array_equal(np.isnan(got), np.isnan(expected))
    ok = ~np.isnan(expected)
    assert np.all(np.abs(got[ok] - expected[ok]) <= bound[ok] + 1e-300)


SHAPES = {
    "boxcar": lambda c: Instrument.boxcar(c, 0.7),
    "triangle": lambda c: Instrument.triangle(c, 0.5),
    "gaussian": lambda c: Instrument.gaussian(c, 0.5, half_width=1.5),
    "fts": lambda c: Instrument.fts(c, 1.5, half_width=2.),
    "fts-hamming": lambda c: Instrument.fts(c, 1.5, apodization="hamming", half_width=2.),
    "tabulated": lambda c: Instrument.tabulated(c, [-1., -0.2, 0., 0.3, 1.2],
                                                [0., 0.8, 1., 0.6, 0.]),
}
CENTERS = np.arange(603., 697., 0.25)


@pytest.fixture(scope="module")
def spec():
    return spectroscopy()


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
@pytest.mark.parametrize("cumulative", [False, True])
def test_radiance_channels_match_numpy(spec, name, direction, cumulative):
    x = SHAPES[name](CENTERS)
    s = lengths()
    boundary = 290. if direction == "toward_last" else None
    fine = spec.compute_radiance(s, boundary_temperature=boundary, direction=direction,
                                 cumulative=cumulative)
    got = spec.compute_radiance(s, boundary_temperature=boundary, direction=direction,
                                cumulative=cumulative, instrument=x,
                                quantities=("radiance", "brightness_temperature"))
    assert got["radiance"].shape[-1] == len(CENTERS)
    check(got["radiance"], x, GRID, fine["radiance"])
    bt = brightness_temperature(np.asarray(got["radiance"]), CENTERS)
    np.testing.assert_array_equal(np.asarray(got["brightness_temperature"]), bt)
    np.testing.assert_array_equal(np.asarray(got["channel_center"]), CENTERS)


def test_radiance_with_and_without_boundary(spec):
    x = SHAPES["gaussian"](CENTERS)
    s = lengths()
    for boundary in (None, 300.):
        fine = spec.compute_radiance(s, boundary_temperature=boundary, boundary_emissivity=0.9)
        got = spec.compute_radiance(s, boundary_temperature=boundary, boundary_emissivity=0.9,
                                    instrument=x)
        check(got["radiance"], x, GRID, fine["radiance"])


@pytest.mark.parametrize("cumulative", [None, "from_first", "from_last"])
def test_path_channels_match_numpy(spec, cumulative):
    x = SHAPES["triangle"](CENTERS)
    s = lengths()
    fine = spec.compute_path(s, cumulative=cumulative)
    got = spec.compute_path(s, cumulative=cumulative, instrument=x)
    check(got["optical_depth"], x, GRID, fine["optical_depth"])
    check(got["transmittance"], x, GRID, fine["transmittance"])
    # the mean of exp(-tau), not exp of the mean tau
    mean_exp = np.asarray(got["transmittance"])
    exp_mean = np.exp(-np.asarray(got["optical_depth"]))
    assert np.max(np.abs(mean_exp - exp_mean)) > 1e-6


def test_per_channel_parameters_and_tables_and_order(spec):
    rng = np.random.default_rng(3)
    centers = rng.permutation(CENTERS)
    s = lengths()
    fine = spec.compute_radiance(s, boundary_temperature=290.)["radiance"]
    fwhm = rng.uniform(0.2, 0.8, centers.size)
    x = Instrument.gaussian(centers, fwhm, half_width=3.*fwhm)
    got = spec.compute_radiance(s, boundary_temperature=290., instrument=x)
    check(got["radiance"], x, GRID, fine)
    np.testing.assert_array_equal(np.asarray(got["channel_center"]), centers)
    offsets = np.array([-0.6, -0.1, 0.2, 0.7])
    table = rng.uniform(0.1, 1., (centers.size, offsets.size))
    y = Instrument.tabulated(centers, offsets, table)
    check(spec.compute_radiance(s, boundary_temperature=290., instrument=y)["radiance"], y,
          GRID, fine)


def test_empty_and_partial_channels_are_nan(spec):
    centers = np.array([650., 600.2, 699.9, 650.004, 640.])
    x = Instrument.boxcar(centers, [1., 1., 1., 0.002, 0.5])
    got = spec.compute_path(lengths(), instrument=x, quantities="optical_depth")
    tau = np.asarray(got["optical_depth"])
    assert np.all(np.isfinite(tau[:, [0, 4]]))
    assert np.all(np.isnan(tau[:, [1, 2, 3]]))
    lo, hi = x.window()
    points = np.searchsorted(GRID, hi, "right") - np.searchsorted(GRID, lo, "left")
    np.testing.assert_array_equal(np.asarray(got["channel_points"]), points)


def test_boxcar_matches_band_means(spec):
    edges = np.arange(600.005, 699.1, 1.)
    assert not np.any(np.isin(GRID, edges))
    x = Instrument.boxcar((edges[:-1] + edges[1:])/2., np.diff(edges))
    np.testing.assert_array_equal(x.columns(GRID)[0], band_columns(GRID, edges)[:-1])
    s = lengths()
    bands = spec.compute_radiance(s, boundary_temperature=290., band_edges=edges)["radiance"]
    got = spec.compute_radiance(s, boundary_temperature=290., instrument=x)["radiance"]
    np.testing.assert_allclose(np.asarray(got), np.asarray(bands), rtol=1e-13, atol=0.)


def test_same_bits_twice_and_over_runs_of_levels():
    x = SHAPES["gaussian"](CENTERS)
    s = lengths()
    one = spectroscopy()
    first = one.compute_radiance(s, boundary_temperature=290., cumulative=True, instrument=x)
    again = one.compute_radiance(s, boundary_temperature=290., cumulative=True, instrument=x)
    np.testing.assert_array_equal(np.asarray(first["radiance"]), np.asarray(again["radiance"]))
    # 3 blocks (beta and the fine-grid radiance of the run) of ~3 levels: several runs
    split = spectroscopy()
    split.device_output_limit = 3*2*GRID.size*8
    runs = split.compute_radiance(s, boundary_temperature=290., cumulative=True, instrument=x)
    np.testing.assert_array_equal(np.asarray(first["radiance"]), np.asarray(runs["radiance"]))
    paths = split.compute_path(s, instrument=x)
    whole = one.compute_path(s, instrument=x)
    for q in ("optical_depth", "transmittance"):
        np.testing.assert_array_equal(np.asarray(paths[q]), np.asarray(whole[q]))


def test_one_instrument_on_two_grids():
    x = SHAPES["fts-hamming"](np.arange(610., 690., 0.5))
    s = lengths()
    coarse_grid = np.arange(600., 700., 0.02)
    for grid in (GRID, coarse_grid, GRID):
        spec = spectroscopy(grid=grid)
        fine = spec.compute_radiance(s, boundary_temperature=290.)["radiance"]
        got = spec.compute_radiance(s, boundary_temperature=290., instrument=x)
        check(got["radiance"], x, grid, fine)
        again = spec.compute_radiance(s, boundary_temperature=290., instrument=x)
        np.testing.assert_array_equal(np.asarray(got["radiance"]), np.asarray(again["radiance"]))


def test_many_overlapping_channels_and_long_windows(spec):
    """2400 channels 0.04 apart with 1 cm-1 windows (~25x overlap, 100 points, tiles of
    neighbours), and 30 cm-1 windows (3000 points: several segments per channel)."""
    s = lengths()
    fine = spec.compute_radiance(s, boundary_temperature=290., cumulative=True)["radiance"]
    dense = Instrument.gaussian(np.linspace(601., 699., 2400), 0.3, half_width=0.5)
    check(spec.compute_radiance(s, boundary_temperature=290., cumulative=True,
                                instrument=dense)["radiance"], dense, GRID, fine)
    wide = Instrument.triangle(np.arange(631., 670., 0.7), 15.)
    check(spec.compute_radiance(s, boundary_temperature=290., cumulative=True,
                                instrument=wide)["radiance"], wide, GRID, fine)


def test_c_abi_checks():
    from pylbl_amd.engine import LBL_OK, default_engine
    from pylbl_amd.mt_ckd import resident_grid
    engine = default_engine(0)
    lib = engine.lib
    grid = resident_grid(engine, GRID)
    centers = np.array([650., 651.])
    width = np.array([0.5, 0.5])
    handle = c_int32(-1)

    def create(**changes):
        a = dict(grid=grid, shape=0, n=2, centers=centers.ctypes.data,
                 parameter=width.ctypes.data, half_width=None, n_table=0, offsets=None,
                 response=None, rows=0)
        a.update(changes)
        return lib.lbl_instrument_create(engine.handle, a["grid"], a["shape"], a["n"],
                                         a["centers"], a["parameter"], a["half_width"],
                                         a["n_table"], a["offsets"], a["response"], a["rows"],
                                         byref(handle))
    bad = np.array([0.5, -1.])
    offsets = np.array([1., 0.])
    for status in (create(grid=12345), create(shape=9), create(n=0), create(centers=None),
                   create(parameter=bad.ctypes.data), create(shape=2),
                   create(shape=5, n_table=2, offsets=offsets.ctypes.data,
                          response=width.ctypes.data, rows=1)):
        assert status == 2                  # LBL_BAD_ARGUMENT
        assert lib.lbl_last_error(engine.handle)
    assert create() == LBL_OK
    from pylbl_amd.engine import DeviceSpectra
    values = DeviceSpectra(engine, 1, GRID.size)
    out = DeviceSpectra(engine, 1, 2)
    assert lib.lbl_instrument_apply(engine.handle, values.pointer, GRID.size, 1, 999, 0,
                                    out.pointer) == 2
    assert b"unknown instrument" in lib.lbl_last_error(engine.handle)
    assert lib.lbl_instrument_apply(engine.handle, values.pointer, GRID.size - 1, 1,
                                    handle.value, 0, out.pointer) == 2
    assert lib.lbl_instrument_apply(engine.handle, None, GRID.size, 1, handle.value, 0,
                                    out.pointer) == 2
    with pytest.raises(EngineError):
        engine.instrument_free(999)
    engine.fill_zero(values)
    engine.instrument_apply(values, 1, handle.value, out)
    np.testing.assert_array_equal(out.to_host(), [[0., 0.]])
    engine.instrument_apply(values, 1, handle.value, out, transmittance=True)
    np.testing.assert_array_equal(out.to_host(), [[1., 1.]])
    engine.instrument_free(handle.value)
    assert lib.lbl_instrument_apply(engine.handle, values.pointer, GRID.size, 1, handle.value,
                                    0, out.pointer) == 2
