"""CPU-only checks of the linear-in-tau source of compute_radiance and compute_flux: the weight
w = 1 - a/x in the form the kernels use against a long-double mirror that shares nothing with it,
the argument checks (all raised before anything touches the GPU), the [count][2] interface table
and its slices across run cuts in both directions, the C header and the ctypes signatures of the
two new entries, and that calls without the keyword queue what they queued."""
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import MemoryDatabase, Spectroscopy, synthetic
from pylbl_amd import engine as engine_module, paths, spectroscopy
from tests import abi_header, linear_source_cases as linear
from tests.abi_header import parameters_of

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd.h").read_text()
F64, LD = np.float64, np.longdouble


def make_spectroscopy(shape=(5,), **keywords):
    tables = [synthetic.line_table("H2O", 590., 610., num_lines=50, seed=1)]
    full = synthetic.standard_atmosphere(int(np.prod(shape)))
    atmos = synthetic.Atmos(p=full.p.reshape(shape), t=full.t.reshape(shape),
                            vmr={"H2O": full.vmr["H2O"].reshape(shape)})
    return Spectroscopy(atmos, np.arange(600., 601., 0.01), MemoryDatabase(tables), **keywords)


# ---------------------------------------------------------------------------------------------
# The weight.
# 1 - a/x with |x| >= 1/16 has |w| >= 0.0306 next to a quotient near 1: expm1 (1 ulp), the division
# and the difference (half an ulp each of a value <= 1.04) leave at most 2*2^-52*1.04/0.0306 =
# 1.5e-14 relative; the 8-term Horner series below 1/16 rounds 16 times on terms that shrink by 48
# per step (under 3 ulp) and stops at x^8/10!/(x/2) <= 1.4e-16.
WEIGHT_BOUND = 1.5e-14


def relative_error(got, x):
    reference = linear.weight(LD, x)
    return np.abs(got.astype(LD) - reference)/np.abs(reference)


def test_weight_form_meets_the_long_double_mirror():
    x = linear.weight_samples()
    assert x.size > 500000 and x.min() <= -3. and x.max() >= 1e3
    assert np.abs(x).min() <= 1e-12
    error = relative_error(linear.device_weight(x), x)
    print("worst relative error of the weight: %.3g at x = %.17g"
          % (float(error.max()), x[np.argmax(error)]))
    assert float(error.max()) <= WEIGHT_BOUND
    # The series alone and the quotient alone, on their own sides of the threshold.
    below = np.abs(x) < linear.SERIES_BELOW
    assert np.count_nonzero(below) > 1000 and np.count_nonzero(~below) > 1000
    assert np.array_equal(linear.device_weight(x[~below]), linear.naive_weight(x[~below]))


def test_mirror_series_and_quotient_agree_where_both_are_good():
    """The mirror's two branches, both in long double, against each other around |x| = 0.5: the
    quotient loses little there and the 24-term series has long converged."""
    x = np.concatenate([np.linspace(0.3, 0.7, 2001), -np.linspace(0.3, 0.7, 2001)]).astype(LD)
    series = np.zeros(x.shape, dtype=LD)
    from math import factorial
    for n in range(24, 0, -1):
        series = LD(1.)/LD(factorial(n + 1)) - x*series
    series = x*series
    direct = LD(1.) - (-np.expm1(-x))/x
    assert float(np.max(np.abs(series - direct)/np.abs(direct))) < 1e-17


def test_naive_quotient_is_what_the_bound_catches():
    x = np.array([1e-12, 1e-10, 1e-8, 1e-6])
    error = relative_error(linear.naive_weight(x), x)
    assert float(error[0]) > 1e-6 and np.all(error > 1e3*WEIGHT_BOUND)
    with np.errstate(invalid="ignore"):
        assert np.isnan(linear.naive_weight(np.array([0.]))[0])


def test_weight_at_zero_and_its_limits():
    assert linear.device_weight(np.array([0.]))[0] == 0.
    assert linear.weight(LD, np.array([0.]))[0] == 0.
    x = np.array([1e-9, -1e-9])
    assert np.allclose(linear.device_weight(x), x/2., rtol=1e-8, atol=0.)
    assert abs(linear.device_weight(np.array([700.]))[0] - (1. - 1./700.)) < 1e-15


def test_update_in_float64_at_zero_negative_and_saturated_x():
    rad = np.array([0., 1.25e-3, 7.5])
    b_in, b_out = np.full(3, 0.11), np.full(3, 0.17)
    same, _ = linear.update(F64, rad, np.abs(rad), np.zeros(3), b_in, b_out)
    assert np.array_equal(same.view(np.uint64), rad.view(np.uint64))
    negative, _ = linear.update(F64, rad, np.abs(rad), np.full(3, -3.), b_in, b_out)
    assert np.all(np.isfinite(negative))
    thick, _ = linear.update(F64, rad, np.abs(rad), np.full(3, 700.), b_in, b_out)
    assert np.allclose(thick, 0.17 - (0.17 - 0.11)/700., rtol=1e-14)
    thin, _ = linear.update(F64, np.zeros(3), np.zeros(3), np.full(3, 1e-9), b_in, b_out)
    assert np.allclose(thin, 1e-9*(0.11 + 0.17)/2., rtol=1e-8)


# ---------------------------------------------------------------------------------------------
# The requests.
def radiance_request_of(spec, **keywords):
    arguments = dict(path_length=np.ones(spec.atmosphere.temperature.shape),
                     boundary_temperature=None, boundary_emissivity=1., direction="toward_last",
                     quantities=("radiance",), band_edges=None, cumulative=False,
                     range_policy="reference")
    arguments.update(keywords)
    return spec._radiance_request(**arguments)


def flux_request_of(spec, **keywords):
    arguments = dict(layer_thickness=np.ones(spec.atmosphere.temperature.shape),
                     surface_temperature=290., surface_emissivity=1., surface="first", angles=3,
                     quantities=spectroscopy.FLUX_QUANTITIES, band_edges=None,
                     range_policy="reference")
    arguments.update(keywords)
    return spec._flux_request(**arguments)


BAD_SOURCES = [
    (dict(source="linear"), "source must be one of"),
    (dict(source=None), "source must be one of"),
    (dict(source=1), "source must be one of"),
    (dict(source="linear_in_tau"), "needs interface_temperature"),
    (dict(interface_temperature=np.full((3, 6), 250.)), "only used with"),
    (dict(source="isothermal", interface_temperature=np.full((3, 6), 250.)), "only used with"),
    (dict(source="linear_in_tau", interface_temperature=np.full((3, 5), 250.)), "shape"),
    (dict(source="linear_in_tau", interface_temperature=np.full((6,), 250.)), "shape"),
    (dict(source="linear_in_tau", interface_temperature=np.full((3, 6, 1), 250.)), "shape"),
    (dict(source="linear_in_tau", interface_temperature=250.), "shape"),
    (dict(source="linear_in_tau", interface_temperature=np.zeros((3, 6))), "finite and > 0"),
    (dict(source="linear_in_tau", interface_temperature=-np.ones((3, 6))), "finite and > 0"),
    (dict(source="linear_in_tau", interface_temperature=np.full((3, 6), np.nan)),
     "finite and > 0"),
    (dict(source="linear_in_tau", interface_temperature=np.full((3, 6), np.inf)),
     "finite and > 0"),
]


@pytest.mark.parametrize("request_of", [radiance_request_of, flux_request_of],
                         ids=["radiance", "flux"])
@pytest.mark.parametrize("keywords, match", BAD_SOURCES)
def test_bad_sources_are_refused_before_the_gpu(monkeypatch, request_of, keywords, match):
    def touched(*arguments, **more):
        raise AssertionError("the GPU side was reached")
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", touched)
    spec = make_spectroscopy((3, 5))
    with pytest.raises(ValueError, match=match):
        request_of(spec, **keywords)
    shape = spec.atmosphere.temperature.shape
    with pytest.raises(ValueError, match=match):
        if request_of is radiance_request_of:
            spec.compute_radiance(np.ones(shape), **keywords)
        else:
            spec.compute_flux(np.ones(shape), 290., **keywords)


def test_one_bad_interface_value_is_found():
    spec = make_spectroscopy((3, 5))
    interfaces = np.full((3, 6), 250.)
    interfaces[2, 5] = np.nan
    with pytest.raises(ValueError, match="finite and > 0"):
        radiance_request_of(spec, source="linear_in_tau", interface_temperature=interfaces)


def test_default_requests_carry_no_table():
    spec = make_spectroscopy((3, 5))
    assert radiance_request_of(spec).edge_temperature is None
    assert flux_request_of(spec).edge_temperature is None
    assert paths._run_edges(radiance_request_of(spec), 0, 15) == {}
    assert paths.SOURCES == ("isothermal", "linear_in_tau")
    for method in (Spectroscopy.compute_radiance, Spectroscopy.compute_flux):
        bound = inspect.signature(method).parameters
        assert bound["source"].default == "isothermal"
        assert bound["interface_temperature"].default is None
    assert "source" not in inspect.signature(Spectroscopy.compute_jacobian).parameters


@pytest.mark.parametrize("shape", [(5,), (3, 5), (2, 3, 4)])
def test_interface_table_layout(shape):
    spec = make_spectroscopy(shape)
    per_path = shape[-1]
    paths_ = int(np.prod(shape[:-1], dtype=int))
    interfaces = 200. + np.arange(paths_*(per_path + 1), dtype=F64).reshape(
        shape[:-1] + (per_path + 1,))
    for request in (radiance_request_of(spec, source="linear_in_tau",
                                        interface_temperature=interfaces),
                    flux_request_of(spec, source="linear_in_tau",
                                    interface_temperature=interfaces)):
        table = request.edge_temperature
        assert table.shape == (paths_*per_path, 2) and table.dtype == F64
        assert table.flags["C_CONTIGUOUS"]
        flat = interfaces.reshape(paths_, per_path + 1)
        for p in range(paths_):
            for level in range(per_path):
                assert table[p*per_path + level, 0] == flat[p, level]
                assert table[p*per_path + level, 1] == flat[p, level + 1]
        assert np.array_equal(table, linear.edge_table(flat))


class Recorder(object):
    """An Engine that writes down its path calls."""
    def __init__(self):
        self.calls = []

    def path_radiance(self, *arguments, **keywords):
        self.calls.append(("path_radiance", arguments, keywords))

    def path_flux(self, *arguments, **keywords):
        self.calls.append(("path_flux", arguments, keywords))


class Block(object):
    def __init__(self, rows):
        self.shape = (rows, 100)

    def rows(self, count):
        return Block(count)


def recording_sweep_runs(recorder, limit_levels):
    """A _sweep_runs that cuts the levels into runs of `limit_levels` and calls the sweeps of
    every pass in the order of the real one, on a Recorder."""
    def fake(self, request, passes, remove_pedestal, range_policy, sweeper, **keywords):
        per_path, count = paths._path_layout(request.shape)
        levels = per_path*count
        run, runs = paths._cut_runs(levels, per_path, 8, 8*limit_levels)
        call = paths._Call(recorder, lambda rows, columns=None: Block(rows), count, per_path,
                           self.grid.size, self.atmosphere.temperature.ravel(), lambda: 7)
        sweep = sweeper(call, run)
        names = [q for step in passes for q in step.level_quantities + step.path_quantities]
        for index, step in enumerate(passes):
            for a, b in (runs[::-1] if step.from_last else runs):
                sweep(index, Block(b - a), a, b, {q: Block(b - a) for q in names})
        width = self.grid.size
        return {q: np.zeros((levels if any(q in s.level_quantities for s in passes) else count,
                             width)) for q in names}
    return fake


@pytest.mark.parametrize("direction", ["toward_last", "toward_first"])
def test_radiance_runs_get_their_slices(monkeypatch, direction):
    """15 levels in runs of 4: runs cut paths in the middle; every call gets rows [a, b) of the
    table, in both directions, and the default call gets no table."""
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    recorder = Recorder()
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", recording_sweep_runs(recorder, 4))
    spec = make_spectroscopy((3, 5))
    shape = (3, 5)
    interfaces = np.random.default_rng(3).uniform(200., 300., size=(3, 6))
    table = linear.edge_table(interfaces)
    out = spec.compute_radiance(np.ones(shape), direction=direction, source="linear_in_tau",
                                interface_temperature=interfaces)
    assert out["source"] == "linear_in_tau"
    begins = [0, 4, 8, 12]
    assert len(recorder.calls) == 4
    for (name, arguments, keywords), a in zip(
            recorder.calls, begins[::-1] if direction == "toward_first" else begins):
        b = min(a + 4, 15)
        assert name == "path_radiance" and arguments[5] == a
        assert np.array_equal(keywords["edge_temperature"], table[a:b])
        assert keywords["from_last"] == (direction == "toward_first")
    linear_calls, recorder.calls = recorder.calls, []
    for keywords in (dict(), dict(source="isothermal")):
        out = spec.compute_radiance(np.ones(shape), direction=direction, **keywords)
        assert "source" not in out
        assert len(recorder.calls) == 4
        for (name, arguments, got), (_, expected, with_table) in zip(recorder.calls,
                                                                     linear_calls):
            assert "edge_temperature" not in got
            assert set(got) == set(with_table) - {"edge_temperature"}
            assert arguments[1:6] == expected[1:6]
        recorder.calls = []


@pytest.mark.parametrize("surface", ["first", "last"])
def test_flux_runs_get_their_slices(monkeypatch, surface):
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    recorder = Recorder()
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", recording_sweep_runs(recorder, 4))
    spec = make_spectroscopy((3, 5))
    shape = (3, 5)
    interfaces = np.random.default_rng(4).uniform(200., 300., size=(3, 6))
    table = linear.edge_table(interfaces)
    out = spec.compute_flux(np.ones(shape), 290., surface=surface, source="linear_in_tau",
                            interface_temperature=interfaces)
    assert out["source"] == "linear_in_tau"
    assert len(recorder.calls) == 8
    down_last = surface == "first"
    begins = [0, 4, 8, 12]
    expected = (begins[::-1] if down_last else begins) + (begins if down_last else begins[::-1])
    for index, ((name, arguments, keywords), a) in enumerate(zip(recorder.calls, expected)):
        assert name == "path_flux" and arguments[5] == a
        assert np.array_equal(keywords["edge_temperature"], table[a:min(a + 4, 15)])
        assert keywords["up"] == (index >= 4)
    recorder.calls = []
    out = spec.compute_flux(np.ones(shape), 290., surface=surface)
    assert "source" not in out and len(recorder.calls) == 8
    assert all("edge_temperature" not in keywords for _, _, keywords in recorder.calls)


# ---------------------------------------------------------------------------------------------
# The C ABI.
@pytest.mark.parametrize("old, new, after", [
    ("lbl_path_radiance", "lbl_path_radiance_source", "const double *temperature"),
    ("lbl_path_flux", "lbl_path_flux_source", "const double *temperature"),
])
def test_header_declares_the_entries_beside_the_old_ones(old, new, after):
    before, now = parameters_of(old), parameters_of(new)
    at = before.index(after) + 1
    assert now == before[:at] + ["const double *edge_temperature"] + before[at:]
    assert new in engine_module.EXPORTED_SYMBOLS and old in engine_module.EXPORTED_SYMBOLS
    lib = engine_module.library()
    argtypes = getattr(lib, new).argtypes
    assert len(argtypes) == len(now) == len(getattr(lib, old).argtypes) + 1
    abi_header.check_argtypes(new, now, addresses=True)


def test_old_signatures_are_what_they_were():
    assert len(parameters_of("lbl_path_radiance")) == 19
    assert len(parameters_of("lbl_path_flux")) == 23
    assert "edge_temperature" not in " ".join(parameters_of("lbl_path_radiance") +
                                              parameters_of("lbl_path_flux") +
                                              parameters_of("lbl_path_jacobian"))
    for method in (engine_module.Engine.path_radiance, engine_module.Engine.path_flux):
        assert inspect.signature(method).parameters["edge_temperature"].default is None
    assert "edge_temperature" not in inspect.signature(
        engine_module.Engine.path_jacobian).parameters


def test_engine_refuses_a_table_of_the_wrong_shape():
    assert engine_module._edge_rows(None, 4) is None
    assert engine_module._edge_rows(np.ones((4, 2)), 4).shape == (4, 2)
    for bad in (np.ones((3, 2)), np.ones((4, 3)), np.ones(8)):
        with pytest.raises(ValueError, match="edge_temperature"):
            engine_module._edge_rows(bad, 4)


def test_kernels_and_entries_state_the_form():
    radiance = (ROOT / "pylbl_amd" / "csrc" / "radiance.h").read_text()
    flux = (ROOT / "pylbl_amd" / "csrc" / "flux.h").read_text()
    assert "template <bool kVector, bool kLinear = false>" in radiance
    assert "template <bool kVector, int K, bool kLinear = false>" in flux
    below = re.search(r"kLinearSeriesBelow = 1\./(\d+)\.;", radiance)
    assert below and 1./int(below.group(1)) == linear.SERIES_BELOW
    terms = "1./2. 1./6. 1./24. 1./120. 1./720. 1./5040. 1./40320. 1./362880.".split()
    assert len(terms) == linear.SERIES_TERMS
    body = radiance[radiance.index("double linear_weight"):]
    body = body[:body.index("}")]
    assert [t for t in re.findall(r"1\./\d+\.", body) if t != "1./16."] == terms
    for text in (HEADER, radiance):
        assert all(t in text for t in terms)
    for name in ("radiance", "flux"):
        entry = (ROOT / "pylbl_amd" / "csrc" / ("%s_entry.inc" % name)).read_text()
        assert "check_edge_temperatures" in entry
        assert re.search(r"return lbl_path_%s_source\(" % name, entry)
