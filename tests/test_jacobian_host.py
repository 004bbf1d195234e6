"""CPU-only checks of Spectroscopy.compute_jacobian: the formulas (the numpy mirror of
tests/jacobian_cases.py against central differences of the forward recurrence in long double), the
entry's declaration, flags and binding, the argument checks (all raised before anything touches the
GPU), the whole-path cutting of runs, and the naming and shapes of the result."""
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import engine as engine_module
from pylbl_amd import spectroscopy
from tests import abi_header, jacobian_cases as jac
from tests import sweep_cases as cases
from tests.test_radiance_host import make_spectroscopy

ROOT = Path(__file__).resolve().parents[1]
LD = np.longdouble
HEADER = (ROOT / "include" / "lbl_amd.h").read_text()


# ---------------------------------------------------------------------------------------------
# The formulas.
@pytest.mark.parametrize("from_last", [False, True])
def test_formulas_against_central_differences(from_last):
    """Every Jacobian of the mirror (float64) within 1e-8 of (|K| + I/300 K) of the central
    difference of sweep_cases.sweep_radiance in long double: steps 1e-6 relative in a level's
    length (d ln x) and 1e-3 K.  The differences' own truncation is ~2e-10 of that scale; a wrong
    formula misses by orders of magnitude -- this is not a rounding bound."""
    problem = jac.SmoothProblem()
    n, levels = problem.levels_per_path, problem.levels
    values, _ = jac.jacobian(np.float64, problem.nu, problem.beta, problem.lengths,
                             problem.temperature, n, from_last, problem.boundary_t,
                             problem.boundary_e)
    radiance = problem.radiance(from_last=from_last)
    worst = {}

    def compare(name, got, difference):
        scale = np.abs(got.astype(LD)) + radiance/LD(300.)
        ratio = float(np.max(np.abs(got.astype(LD) - difference)/scale))
        worst[name] = max(worst.get(name, 0.), ratio)

    assert np.max(np.abs(values["radiance"].astype(LD) - radiance)/radiance) < 1e-12
    d, h = LD(1e-6), LD(1e-3)
    for level in range(n):
        rows = cases._flat(n, level)
        factor = np.ones(levels, dtype=LD)
        factor[rows] = 1 + d
        up = problem.radiance(lengths=problem.lengths.astype(LD)*factor, from_last=from_last)
        factor[rows] = 1 - d
        down = problem.radiance(lengths=problem.lengths.astype(LD)*factor, from_last=from_last)
        difference = (up - down)/(2*d)
        compare("log_optical_depth_jacobian", values["log_optical_depth_jacobian"][rows],
                difference)
        x = problem.lengths[rows, None]*problem.beta[rows]
        compare("x * optical_depth_jacobian", x*values["optical_depth_jacobian"][rows],
                difference)
        shift = np.zeros(levels, dtype=LD)
        shift[rows] = h
        up = problem.radiance(temperature=problem.temperature.astype(LD) + shift,
                              from_last=from_last)
        down = problem.radiance(temperature=problem.temperature.astype(LD) - shift,
                                from_last=from_last)
        compare("temperature_jacobian", values["temperature_jacobian"][rows], (up - down)/(2*h))
    up = problem.radiance(boundary_t=problem.boundary_t.astype(LD) + h, from_last=from_last)
    down = problem.radiance(boundary_t=problem.boundary_t.astype(LD) - h, from_last=from_last)
    compare("boundary_temperature_jacobian", values["boundary_temperature_jacobian"],
            (up - down)/(2*h))
    up = problem.radiance(boundary_e=np.ones(cases.PATHS), from_last=from_last)
    down = problem.radiance(boundary_e=np.zeros(cases.PATHS), from_last=from_last)
    compare("boundary_emissivity_jacobian", values["boundary_emissivity_jacobian"], up - down)
    print("worst |mirror - difference| / (|K| + I/300 K):", worst)
    assert len(worst) == 5
    for name, ratio in worst.items():
        assert ratio <= 1e-8, (name, ratio)


def test_mirror_in_float64_meets_long_double():
    """The float64 mirror within the project's 1e-12 of the long-double one, on the magnitudes the
    GPU tests use."""
    problem = jac.SmoothProblem(levels_per_path=12, columns=300)
    arguments = (problem.nu, problem.beta, problem.lengths, problem.temperature, 12, False,
                 problem.boundary_t, problem.boundary_e)
    got, _ = jac.jacobian(np.float64, *arguments)
    reference, magnitude = jac.jacobian(LD, *arguments)
    for q in jac.QUANTITIES:
        assert got[q].shape == reference[q].shape
        assert np.all(np.abs(got[q].astype(LD) - reference[q]) <= LD(1e-12)*magnitude[q]), q


def test_isothermal_closure_in_the_mirror():
    """sum_k a_k*trail_k + trail_b telescopes to 1: the temperature Jacobians of an isothermal
    path behind a black boundary at the same temperature add up to dB(nu, T)."""
    problem = jac.SmoothProblem(levels_per_path=12, columns=300)
    t = 260.
    values, _ = jac.jacobian(LD, problem.nu, problem.beta, problem.lengths,
                             np.full(problem.levels, t), 12, True, np.full(cases.PATHS, t),
                             np.ones(cases.PATHS))
    total = values["temperature_jacobian"].reshape(cases.PATHS, 12, -1).sum(axis=1) + \
        values["boundary_temperature_jacobian"]
    expected = jac.planck_dt(LD, problem.nu, t)
    assert np.max(np.abs(total - expected)/expected) < 1e-15
    source = cases.planck(LD, problem.nu, t)
    assert np.max(np.abs(values["optical_depth_jacobian"])/source) < 1e-15


# ---------------------------------------------------------------------------------------------
# The entry: header, flags, binding.
def defines(pattern):
    return {name: int(value, 0) for name, value in
            re.findall(r"#define\s+(" + pattern + r")\s+(0x[0-9a-fA-F]+|\d+)", HEADER)}


def test_header_declares_the_entry_and_its_flags():
    match = re.search(r"int lbl_path_jacobian\(([^;]*)\);", HEADER)
    assert match is not None
    parameters = [p.strip() for p in match.group(1).replace("\n", " ").split(",")]
    names = [re.sub(r".*[ *]", "", p) for p in parameters]
    assert names == ["engine", "beta", "row_stride", "columns", "grid", "n_paths",
                     "levels_per_path", "level_begin", "level_count", "path_length",
                     "temperature", "boundary_temperature", "boundary_emissivity", "n_bands",
                     "band_start", "work", "radiance", "optical_depth_jacobian",
                     "log_optical_depth_jacobian", "temperature_jacobian",
                     "boundary_temperature_jacobian", "boundary_emissivity_jacobian", "flags"]
    assert "carry" not in names
    flags = defines(r"LBL_PATH_JACOBIAN_\w+")
    assert set(flags) == {"LBL_PATH_JACOBIAN_DEPTH", "LBL_PATH_JACOBIAN_LOG_DEPTH",
                          "LBL_PATH_JACOBIAN_TEMPERATURE", "LBL_PATH_JACOBIAN_BOUNDARY_T",
                          "LBL_PATH_JACOBIAN_BOUNDARY_E"}
    every = defines(r"LBL_PATH_\w+")
    assert len(every) == len(flags) + 8
    bits = list(every.values()) + [1, 2, 4, 8, 16, 32]      # and the call flags (LBL_ASYNC ...)
    assert all(v > 0 and v & (v - 1) == 0 for v in bits)    # single bits
    assert len(set(bits)) == len(bits)                      # no collision
    assert min(flags.values()) > every["LBL_PATH_FLUX_UP"]
    assert max(flags.values()) < 2**31


def test_python_mirrors_the_flags_and_binds_every_argument():
    flags = defines(r"LBL_PATH_JACOBIAN_\w+")
    for name, value in flags.items():
        assert getattr(engine_module, name[len("LBL_"):]) == value
    assert dict(engine_module.PATH_JACOBIAN_OUTPUTS) == {
        "radiance": defines("LBL_PATH_RADIANCE")["LBL_PATH_RADIANCE"],
        "optical_depth_jacobian": flags["LBL_PATH_JACOBIAN_DEPTH"],
        "log_optical_depth_jacobian": flags["LBL_PATH_JACOBIAN_LOG_DEPTH"],
        "temperature_jacobian": flags["LBL_PATH_JACOBIAN_TEMPERATURE"],
        "boundary_temperature_jacobian": flags["LBL_PATH_JACOBIAN_BOUNDARY_T"],
        "boundary_emissivity_jacobian": flags["LBL_PATH_JACOBIAN_BOUNDARY_E"]}
    assert tuple(q for q, _ in engine_module.PATH_JACOBIAN_OUTPUTS) == jac.OUTPUTS
    assert "lbl_path_jacobian" in engine_module.EXPORTED_SYMBOLS
    lib = engine_module.library()
    match = re.search(r"int lbl_path_jacobian\(([^;]*)\);", HEADER)
    declared = match.group(1).count(",") + 1
    assert len(lib.lbl_path_jacobian.argtypes) == declared == 23
    abi_header.check_argtypes("lbl_path_jacobian", addresses=True)
    bound = inspect.signature(engine_module.Engine.path_jacobian).parameters
    for name in ("beta", "columns", "grid", "n_paths", "levels_per_path", "level_begin", "lengths",
                 "temperature", "work", "boundary_temperature", "boundary_emissivity",
                 "band_start", "from_last", "asynchronous") + jac.OUTPUTS:
        assert name in bound, name
    assert "carry" not in bound


def test_the_kernel_is_built_on_the_sweep_skeleton():
    source = (ROOT / "pylbl_amd" / "csrc" / "jacobian.h").read_text()
    assert "path_jacobian_kernel" in source and "struct PathJacobian : PathLevels" in source
    ahead = int(re.search(r"kJacobianAhead = (\d+);", source).group(1))
    assert ahead == jac.JACOBIAN_AHEAD
    entry = (ROOT / "pylbl_amd" / "csrc" / "jacobian_entry.inc").read_text()
    for shared in ("path_entry(", "PathCall", "PathTables", "PathBands", "note_rows"):
        assert shared in entry, shared
    engine_source = (ROOT / "pylbl_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "jacobian_entry.inc"' in engine_source


def test_depths_reach_every_loop():
    """jacobian_cases.DEPTHS holds a depth below, at, above and beyond twice the rows in flight of
    loop 1 (kPathAhead) and of loop 2 (kJacobianAhead)."""
    for ahead in (cases.PATH_AHEAD, jac.JACOBIAN_AHEAD):
        classes = {cases.depth_class(n, ahead) for n in jac.DEPTHS}
        assert classes == {"below", "one batch", "batch and remainder", "batches",
                           "batches and remainder"}
        assert any(n > 2*ahead for n in jac.DEPTHS)


# ---------------------------------------------------------------------------------------------
# Argument checks.
@pytest.mark.parametrize("keywords, match", [
    (dict(path_length=np.ones(4)), "shape"),
    (dict(path_length=-np.ones((3, 5))), ">= 0"),
    (dict(path_length=np.full((3, 5), np.nan)), "finite"),
    (dict(boundary_temperature=np.ones(5)), "boundary_temperature"),
    (dict(boundary_temperature=0.), "boundary temperatures"),
    (dict(boundary_temperature=np.array([280., np.nan, 290.])), "boundary temperatures"),
    (dict(boundary_emissivity=1.5), "emissivities"),
    (dict(boundary_emissivity=np.ones(4)), "boundary_emissivity"),
    (dict(direction="up"), "direction"),
    (dict(quantities=("radiance", "optical_depth")), "quantities"),
    (dict(quantities="brightness_temperature"), "quantities"),
    (dict(quantities="jacobian"), "quantities"),
    (dict(quantities=()), "quantities"),
    (dict(boundary_temperature=None, quantities="boundary_temperature_jacobian"),
     "need a boundary_temperature"),
    (dict(boundary_temperature=None,
          quantities=("radiance", "boundary_emissivity_jacobian")), "need a boundary_temperature"),
    (dict(band_edges=[600.5]), "band_edges"),
    (dict(band_edges=[601., 600.]), "increasing"),
    (dict(band_edges=[600., 601.], instrument="not checked before band_edges"), "not both"),
    (dict(instrument="an instrument"), "Instrument"),
    (dict(range_policy="everything"), "range_policy"),
])
def test_bad_arguments_raise_before_the_gpu(keywords, match):
    spec = make_spectroscopy((3, 5))
    arguments = dict(path_length=np.ones((3, 5)), boundary_temperature=290.)
    arguments.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_jacobian(**arguments)
    assert spec.cache == {}             # no backend object was built: nothing touched the GPU


def test_bad_level_temperatures_raise_before_the_gpu():
    spec = make_spectroscopy((5,))
    spec.atmosphere.temperature[2] = 0.
    with pytest.raises(ValueError, match="temperatures"):
        spec.compute_jacobian(np.ones(5))
    assert spec.cache == {}


def test_group_is_not_implemented():
    spec = make_spectroscopy(group=True)
    with pytest.raises(NotImplementedError, match="compute_jacobian"):
        spec.compute_jacobian(np.ones(5))
    assert spec.cache == {}


def test_default_quantities():
    default = inspect.signature(spectroscopy.Spectroscopy.compute_jacobian).parameters
    assert default["quantities"].default == ("radiance", "optical_depth_jacobian",
                                             "temperature_jacobian")
    assert default["direction"].default == "toward_last"
    assert default["boundary_emissivity"].default == 1.
    assert set(spectroscopy.JACOBIAN_QUANTITIES) == set(jac.QUANTITIES)


# ---------------------------------------------------------------------------------------------
# Run cutting.
def parent_runs(levels, level_bytes, limit):
    """What _sweep_runs cut before it knew whole paths."""
    run = levels if levels*level_bytes <= limit else max(1, limit//level_bytes)
    run = min(run, spectroscopy._MAX_RUN_LEVELS)
    return run, [(a, min(a + run, levels)) for a in range(0, levels, run)]


N_BYTES = 8*1000        # one row

CUTS = [  # paths, levels per path, limit [rows], blocks
    (1, 1, 2, 2), (1, 64, 64*4, 4), (1, 64, 64*4 + 63, 4), (3, 19, 19*3*3, 3),
    (3, 19, 19*3*3 - 1, 3), (3, 19, 19*3, 3), (7, 5, 5*2*4 + 7, 4), (7, 5, 10**9, 2),
    (100, 64, 64*5*10, 5), (2000, 40, 10**9, 1), (70000, 1, 10**9, 2), (3, 30000, 10**9, 2),
    (5, 13, 13*2*2, 2), (64, 64, 64*64*3 - 1, 3),
]


@pytest.mark.parametrize("paths, per_path, limit_rows, blocks", CUTS)
def test_whole_path_runs(paths, per_path, limit_rows, blocks):
    levels = paths*per_path
    limit = limit_rows*N_BYTES
    run, runs = spectroscopy._cut_runs(levels, per_path, blocks*N_BYTES, limit, whole_paths=True)
    covered = np.zeros(levels, dtype=int)
    for a, b in runs:
        assert 0 <= a < b <= levels
        assert a % per_path == 0 and b % per_path == 0
        assert b - a <= run <= spectroscopy._MAX_RUN_LEVELS
        assert (b - a)*blocks*N_BYTES <= limit
        covered[a:b] += 1
    assert np.all(covered == 1)
    assert [a for a, _ in runs] == sorted(a for a, _ in runs)
    # The largest number of whole paths that fits: one more path would not.
    if run < levels:
        more = run + per_path
        assert more*blocks*N_BYTES > limit or more > spectroscopy._MAX_RUN_LEVELS
    # With the keyword off: the parent's runs.
    assert spectroscopy._cut_runs(levels, per_path, blocks*N_BYTES, limit) == \
        parent_runs(levels, blocks*N_BYTES, limit)


@pytest.mark.parametrize("paths, per_path, limit_rows, blocks", [
    (3, 19, 19*3 - 1, 3), (1, 64, 1, 2), (2, 5, 0, 1)])
def test_a_limit_below_one_path_raises(paths, per_path, limit_rows, blocks):
    with pytest.raises(ValueError, match="device_output_limit") as error:
        spectroscopy._cut_runs(paths*per_path, per_path, blocks*N_BYTES, limit_rows*N_BYTES,
                               whole_paths=True)
    assert str(per_path*blocks*N_BYTES) in str(error.value)      # the bytes one path needs


def test_a_path_longer_than_a_run_raises():
    with pytest.raises(ValueError, match="device_output_limit"):
        spectroscopy._cut_runs(70000, 70000, 8, 10**12, whole_paths=True)


# ---------------------------------------------------------------------------------------------
# The result.
@pytest.mark.parametrize("shape", [(5,), (3, 5), (2, 3, 5)])
@pytest.mark.parametrize("bands", [False, True])
def test_output_names_dims_and_shapes(monkeypatch, shape, bands):
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    spec = make_spectroscopy(shape)
    edges = [599., 600.2, 600.2001, 600.5] if bands else None
    request = spec._radiance_request(
        np.ones(shape), 290., 1., "toward_first", jac.QUANTITIES, edges, False, "reference",
        names=spectroscopy.JACOBIAN_QUANTITIES, caller="compute_jacobian")
    assert request.quantities == spectroscopy.JACOBIAN_QUANTITIES and request.from_last
    levels, paths = int(np.prod(shape)), int(np.prod(shape[:-1]))
    width = 3 if bands else spec.grid.size
    values = {q: np.arange((levels if q in jac.PER_LEVEL else paths)*width,
                           dtype=np.float64).reshape(-1, width) + i
              for i, q in enumerate(request.quantities)}
    out = spec._create_path_dataset(values, request)
    assert set(out) == set(jac.QUANTITIES) | ({"band_lower", "band_upper", "band_points"}
                                              if bands else {"wavenumber"})
    for q in jac.QUANTITIES:
        lead = shape if q in jac.PER_LEVEL else shape[:-1]
        assert out[q].shape == tuple(lead) + (width,), q
        assert np.array_equal(out[q].reshape(-1, width), values[q])


def test_units():
    units = spectroscopy._PATH_UNITS
    radiance = units["radiance"]
    assert units["optical_depth_jacobian"] == radiance
    assert units["log_optical_depth_jacobian"] == radiance
    assert units["boundary_emissivity_jacobian"] == radiance
    assert units["temperature_jacobian"] == radiance + " K-1"
    assert units["boundary_temperature_jacobian"] == radiance + " K-1"
