"""CPU-only checks of the surface of compute_radiance (spectral emissivity, reflected downwelling
radiance): the interpolation as written against a long-double mirror, the two-pass mirror itself,
the argument checks (all raised before anything touches the GPU), the C header and the ctypes
signatures of the two new entries, that a call without the new keywords queues what it queued on
the commit before them (tests/golden/radiance_default_queue.json, recorded there on the stand-in
engine of tests/surface_cases.py), and what a reflecting call queues."""
import inspect
import json
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths
from pylbl_amd import engine as engine_module
from pylbl_amd.paths import DOWNWELLING, SURFACE_RADIANCE_QUANTITIES
from tests import abi_header, surface_cases as surface
from tests.abi_header import parameters_of
from tests import sweep_cases as cases
from tests.test_linear_source_host import make_spectroscopy

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd.h").read_text()
F64, LD = np.float64, np.longdouble
assert DOWNWELLING == surface.DOWNWELLING


# ---------------------------------------------------------------------------------------------
# The interpolation.
def tables(seed, m, count=4):
    rng = np.random.default_rng(seed)
    knots = np.sort(rng.uniform(600., 3000., size=m))
    assert np.all(np.diff(knots) > 0.)
    values = rng.uniform(0., 1., size=(count, m))
    values[0] = 0.75                    # a flat table
    values[1, ::2], values[1, 1::2] = 0., 1.
    return knots, values


@pytest.mark.parametrize("m", [2, 3, 17, 1024])
def test_written_formula_meets_the_long_double_mirror(m):
    """Knots hit exactly, 1 ulp on either side, between knots, below and above all of them:
    float64 as written is within INTERPOLATION_BOUND (derived in surface_cases) of long double,
    paths.interpolate_emissivity (what the docstring states) gives the same bits as the mirror in
    float64, both are numpy.interp up to its own rounding, and a flat table is exact."""
    knots, values = tables(10 + m, m)
    nu = surface.knot_samples(knots)
    got = surface.emissivity(F64, knots, values, nu)
    reference = surface.emissivity(LD, knots, values, nu)
    error = np.abs(got.astype(LD) - reference)
    print("worst interpolation error, M = %d: %.3g" % (m, float(error.max())))
    assert float(error.max()) <= surface.INTERPOLATION_BOUND
    assert got.dtype == F64 and np.all((got >= 0.) & (got <= 1. + 1e-15))
    package = paths.interpolate_emissivity(knots, values, nu)
    assert np.array_equal(package.view(np.uint64), got.view(np.uint64))
    for row, table in zip(got, values):
        assert np.allclose(row, np.interp(nu, knots, table), rtol=0., atol=4e-16)
    assert np.all(got[0] == 0.75)
    # On a knot the value is the knot's own, outside the end values.
    on = surface.emissivity(F64, knots, values, knots)
    assert np.array_equal(on, values)
    assert np.all(surface.emissivity(F64, knots, values, [knots[0] - 5., -1., 0.]) ==
                  values[:, :1])
    assert np.all(surface.emissivity(F64, knots, values, [knots[-1] + 5., 1e9]) ==
                  values[:, -1:])


def test_interval_is_the_count_of_knots_below():
    knots = np.array([1., 2., 4.])
    nu = np.array([0., 1., np.nextafter(1., 2.), 2., 3., 4., 5., np.nan])
    assert list(surface.interval(knots, nu)) == [-1, -1, 0, 1, 1, 2, 2, -1]


# ---------------------------------------------------------------------------------------------
# The two-pass mirror.
def test_two_pass_mirror():
    problem = cases.Problem(67, 9, seed=5)
    problem.boundary_t = np.array([0., 288., 215.])
    e = np.array([1., 0.9, 0.25])
    lengths = 1.66*problem.thickness
    for from_last in (False, True):
        plain = surface.two_pass(LD, problem, from_last, e)
        start = cases.boundary_start(LD, problem.nu, problem.boundary_t, e)
        expect, mag = cases.sweep_radiance(LD, problem.nu, problem.beta, problem.thickness,
                                           problem.temperature, 9, from_last, start)
        assert np.array_equal(plain["up"][0], expect) and np.array_equal(plain["up"][1], mag)
        both = surface.two_pass(LD, problem, from_last, e, lengths)
        down, down_mag = both["down"]
        sweep, _ = cases.sweep_radiance(LD, problem.nu, problem.beta, lengths,
                                        problem.temperature, 9, not from_last)
        assert np.array_equal(down, sweep[surface.final_rows(9, not from_last)])
        assert np.all(down >= 0.) and np.array_equal(down, down_mag)
        # Path 0 has no boundary, path 1 reflects a tenth, path 2 three quarters.
        assert np.array_equal(both["start"][0][0], np.zeros(67))
        b = cases.planck(LD, problem.nu, LD(288.))
        assert np.array_equal(both["start"][0][1], LD(0.9)*b + (LD(1.) - LD(0.9))*down[1])
        assert np.all(both["up"][0][9:] >= plain["up"][0][9:])
        assert np.any(both["up"][0][9:] > plain["up"][0][9:])
        assert np.array_equal(both["up"][0][:9], plain["up"][0][:9])
        assert np.all(both["up"][1] >= np.abs(both["up"][0]))
        # Emissivity 1 everywhere: the reflection changes nothing.
        black = surface.two_pass(LD, problem, from_last, np.ones(3), lengths)
        assert np.array_equal(black["up"][0],
                              surface.two_pass(LD, problem, from_last, np.ones(3))["up"][0])


# ---------------------------------------------------------------------------------------------
# The requests.
def request_of(spec, **keywords):
    arguments = dict(path_length=np.ones(spec.atmosphere.temperature.shape),
                     boundary_temperature=288., boundary_emissivity=1., direction="toward_last",
                     quantities=("radiance",), band_edges=None, cumulative=False,
                     range_policy="reference", names=SURFACE_RADIANCE_QUANTITIES)
    arguments.update(keywords)
    return spec._radiance_request(**arguments)


KNOTS = np.array([590., 600., 610.])
ONES = np.ones((3, 5))
BAD = [
    (dict(emissivity_wavenumber=[600., 600., 610.], boundary_emissivity=[1., 1., 1.]),
     "strictly ascending"),
    (dict(emissivity_wavenumber=[610., 600.], boundary_emissivity=[1., 1.]),
     "strictly ascending"),
    (dict(emissivity_wavenumber=[600., np.nan], boundary_emissivity=[1., 1.]),
     "strictly ascending"),
    (dict(emissivity_wavenumber=[600., np.inf], boundary_emissivity=[1., 1.]),
     "strictly ascending"),
    (dict(emissivity_wavenumber=[600.], boundary_emissivity=[1.]), "2..1024"),
    (dict(emissivity_wavenumber=np.arange(1025.), boundary_emissivity=np.ones(1025)),
     "2..1024"),
    (dict(emissivity_wavenumber=np.ones((2, 2)), boundary_emissivity=[1., 1.]), "2..1024"),
    (dict(emissivity_wavenumber=KNOTS, boundary_emissivity=[1., 1.1, 1.]), r"\[0, 1\]"),
    (dict(emissivity_wavenumber=KNOTS, boundary_emissivity=[1., -0.1, 1.]), r"\[0, 1\]"),
    (dict(emissivity_wavenumber=KNOTS, boundary_emissivity=[1., np.nan, 1.]), r"\[0, 1\]"),
    (dict(emissivity_wavenumber=KNOTS, boundary_emissivity=1.), "shape"),
    (dict(emissivity_wavenumber=KNOTS, boundary_emissivity=np.ones(4)), "shape"),
    (dict(emissivity_wavenumber=KNOTS, boundary_emissivity=np.ones((5, 3))), "shape"),
    (dict(emissivity_wavenumber=KNOTS, boundary_emissivity=np.ones((3, 5, 3))), "shape"),
    (dict(boundary_emissivity=np.ones((3, 3)) * 0.5), "shape"),
    (dict(reflection_path_length=np.ones((3, 4))), "shape"),
    (dict(reflection_path_length=np.ones(5)), "shape"),
    (dict(reflection_path_length=-ONES), "finite and >= 0"),
    (dict(reflection_path_length=ONES*np.nan), "finite and >= 0"),
    (dict(reflection_path_length=ONES, boundary_temperature=None), "needs a boundary_temperature"),
    (dict(quantities=("radiance", DOWNWELLING)), "only formed with reflection_path_length"),
    (dict(quantities=DOWNWELLING, reflection_path_length=ONES, cumulative=True),
     "not with cumulative"),
    (dict(quantities="downwelling", reflection_path_length=ONES), "quantities must be"),
]


@pytest.mark.parametrize("keywords, match", BAD)
def test_bad_surfaces_are_refused_before_the_gpu(monkeypatch, keywords, match):
    def touched(*arguments, **more):
        raise AssertionError("the GPU side was reached")
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", touched)
    monkeypatch.setattr(engine_module, "default_engine", lambda device=0: surface.Untouchable())
    spec = make_spectroscopy((3, 5))
    with pytest.raises(ValueError, match=match):
        request_of(spec, **keywords)
    call = dict(boundary_temperature=288.)
    call.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_radiance(ONES, **call)


def test_group_stays_not_implemented(monkeypatch):
    spec = make_spectroscopy((3, 5))
    spec.group = object()
    with pytest.raises(NotImplementedError):
        spec.compute_radiance(ONES, boundary_temperature=288., reflection_path_length=ONES)


def test_requests_hold_the_tables():
    spec = make_spectroscopy((3, 5))
    plain = request_of(spec)
    assert plain.emissivity_knots is None and plain.reflection_lengths is None
    one = request_of(spec, emissivity_wavenumber=KNOTS, boundary_emissivity=[0.9, 0.8, 0.7])
    assert one.boundary_emissivity.shape == (3, 3) and one.boundary_emissivity.flags.c_contiguous
    assert np.array_equal(one.boundary_emissivity, np.tile([0.9, 0.8, 0.7], (3, 1)))
    assert np.array_equal(one.emissivity_knots, KNOTS)
    table = np.random.default_rng(1).uniform(size=(3, 3))
    assert np.array_equal(request_of(spec, emissivity_wavenumber=KNOTS,
                                     boundary_emissivity=table).boundary_emissivity, table)
    lengths = np.arange(15.).reshape(3, 5)
    both = request_of(spec, reflection_path_length=lengths, quantities=("radiance", DOWNWELLING))
    assert np.array_equal(both.reflection_lengths, lengths.ravel())
    assert both.quantities == ("radiance", DOWNWELLING)
    bound = inspect.signature(Spectroscopy.compute_radiance).parameters
    assert bound["emissivity_wavenumber"].default is None
    assert bound["reflection_path_length"].default is None
    assert "reflection_path_length" not in inspect.signature(
        Spectroscopy.compute_jacobian).parameters
    assert paths.RADIANCE_QUANTITIES == ("radiance", "brightness_temperature")
    assert paths._PATH_UNITS[DOWNWELLING] == paths._PATH_UNITS["radiance"]
    assert paths.MAX_EMISSIVITY_KNOTS == surface.MAX_KNOTS


# ---------------------------------------------------------------------------------------------
# The C ABI.
def check_argtypes(name, parameters):
    """The shared comparison (tests/abi_header.py); these entries take plain addresses."""
    abi_header.check_argtypes(name, parameters, addresses=True)
    assert name in engine_module.EXPORTED_SYMBOLS


def test_header_declares_both_entries_and_ctypes_match():
    source = parameters_of("lbl_path_radiance_source")
    surface_entry = parameters_of("lbl_path_radiance_surface")
    assert surface_entry == source + ["const double *emissivity_rows", "const double *reflection"]
    check_argtypes("lbl_path_radiance_surface", surface_entry)
    fill = parameters_of("lbl_surface_emissivity")
    assert fill == ["lbl_engine *engine", "int32_t grid", "int32_t n_paths", "int32_t path_begin",
                    "int32_t path_count", "int32_t n_knots", "const double *knot_wavenumber",
                    "const double *knot_emissivity", "double *rows", "int64_t row_stride",
                    "int32_t flags"]
    check_argtypes("lbl_surface_emissivity", fill)
    assert len(parameters_of("lbl_path_radiance")) == 19
    assert len(source) == 20
    for keyword in ("emissivity_rows", "reflection"):
        assert inspect.signature(
            engine_module.Engine.path_radiance).parameters[keyword].default is None


def test_header_docstring_and_kernel_state_the_same_formulas():
    kernel = (ROOT / "pylbl_amd" / "csrc" / "surface.h").read_text()
    radiance = (ROOT / "pylbl_amd" / "csrc" / "radiance.h").read_text()
    docstring = Spectroscopy.compute_radiance.__doc__
    def squeeze(text):
        """Without the comment marks at the starts of lines, runs of blanks as one."""
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    interpolation = "E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j))"
    for text in (HEADER, kernel, docstring):
        assert interpolation in squeeze(text)
        assert "E = e_0 for nu <= k_0" in squeeze(text)
        assert "E = e_{M-1} for nu >= k_{M-1}" in squeeze(text)
    for text in (HEADER, kernel, radiance, docstring):
        assert re.search(r"I = E\*B\(nu, T_b(oundary)?\) \+ \(1\. - E\)\*D", squeeze(text))
    assert "kSurfaceMaxKnots = %d" % surface.MAX_KNOTS in kernel
    assert "template <bool kVector, bool kLinear, bool kSurface, typename Args>" in radiance


# ---------------------------------------------------------------------------------------------
# The queue.
def test_default_calls_queue_what_they_queued(tmp_path):
    golden = json.loads((ROOT / "tests" / "golden" / "radiance_default_queue.json").read_text())
    assert set(golden) == set(surface.default_calls())
    got = surface.default_queues(tmp_path)
    for name, log in golden.items():
        assert any(line.startswith("path_radiance(") for line in log), name
        assert got[name] == log, name


def kernel_lines(log):
    names = ("path_radiance", "surface_emissivity", "compute(", "synchronize", "to_host_into")
    return [line for line in log if line.startswith(names)]


def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
def test_reflecting_call_queues_down_fill_up(tmp_path, direction):
    lengths = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    knots = np.array([10., 30., 70.])
    table = np.array([[0.9, 0.7, 0.95], [1., 0.5, 0.6]])
    with surface.recorded(tmp_path) as (spec, engine):
        log = surface.queue_of(spec, engine, None, dict(
            path_length=lengths, boundary_temperature=288., boundary_emissivity=table,
            emissivity_wavenumber=knots, reflection_path_length=1.66*lengths,
            direction=direction, quantities=("radiance", DOWNWELLING)))
        # Everything fits: the absorption is computed once (two lines gases: two compute calls).
        assert sum(line.startswith("compute(") for line in log) == 2
        calls = [line for line in kernel_lines(log) if not line.startswith(("compute(", "sync"))]
        assert [line.split("(")[0] for line in calls] == [
            "path_radiance", "surface_emissivity", "path_radiance", "to_host_into",
            "to_host_into"]
        down, fill, up = calls[:3]
        from_last = direction == "toward_first"
        assert argument(down, "from_last") == str(not from_last)
        assert argument(up, "from_last") == str(from_last)
        assert "boundary_temperature" not in down        # the down pass starts from 0
        assert "emissivity_rows" not in down and "reflection=" not in down
        # D on the grid is returned: the down pass writes the rows the up pass reflects.
        assert argument(down, "radiance") == argument(up, "reflection")
        assert argument(fill, "rows") == argument(up, "emissivity_rows")
        assert argument(up, "boundary_emissivity") == "None"
        assert argument(down, "carry") == argument(up, "carry")
        assert argument(down, "beta") == argument(up, "beta")
        assert argument(down, "lengths") != argument(up, "lengths")

        # Runs of two levels: the down pass ends on the run the up pass starts on, which is
        # computed once; the other two runs twice.  D is not returned: a block of its own.
        log = surface.queue_of(spec, engine, 2, dict(
            path_length=lengths, boundary_temperature=288., boundary_emissivity=0.8,
            reflection_path_length=lengths, direction=direction))
        calls = [line for line in kernel_lines(log) if line.startswith(("path_", "surface_"))]
        assert len(calls) == 6 and all(line.startswith("path_radiance") for line in calls)
        begins = [int(argument(line, "level_begin")) for line in calls]
        order = [0, 2, 4] if from_last else [4, 2, 0]
        assert begins == order + order[::-1]
        assert sum(line.startswith("compute(") for line in log) == 2*5
        assert all("reflection=" not in line for line in calls[:3])
        assert len({argument(line, "reflection") for line in calls[3:]}) == 1
        assert argument(calls[3], "reflection") == argument(calls[0], "radiance")
        assert argument(calls[3], "emissivity_rows") == "None"

        # Bands with D returned: the down pass keeps D in the reflection rows as its carry.
        log = surface.queue_of(spec, engine, None, dict(
            path_length=lengths, boundary_temperature=288., boundary_emissivity=0.8,
            reflection_path_length=lengths, direction=direction,
            band_edges=[20., 30., 60.], quantities=("radiance", DOWNWELLING)))
        down, up = [line for line in log if line.startswith("path_radiance")]
        assert argument(down, "carry") == argument(up, "reflection")
        assert argument(down, "carry") != argument(up, "carry")
        assert argument(down, "band_start") == argument(up, "band_start") != "None"


def test_results_are_marked_only_when_the_surface_is_used(tmp_path, monkeypatch):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    lengths = np.ones(surface.SHAPE)
    with surface.recorded(tmp_path) as (spec, engine):
        plain = spec.compute_radiance(lengths, boundary_temperature=288.)
        assert "surface" not in plain and "emissivity" not in plain
        both = spec.compute_radiance(lengths, boundary_temperature=288.,
                                     boundary_emissivity=[0.5, 0.6], emissivity_wavenumber=[1., 2.],
                                     reflection_path_length=lengths,
                                     quantities=("radiance", DOWNWELLING), cumulative=False)
        assert both["surface"] == "reflecting" and both["emissivity"] == "spectral"
        assert both[DOWNWELLING].shape == (2, 160) and both["radiance"].shape == (2, 160)
        spectral = spec.compute_radiance(lengths, boundary_temperature=288.,
                                         boundary_emissivity=[0.5, 0.6],
                                         emissivity_wavenumber=[1., 2.], cumulative=True)
        assert "surface" not in spectral and spectral["emissivity"] == "spectral"
        assert spectral["radiance"].shape == (2, 3, 160)
