"""CPU-only checks of the spectral scatterer of compute_solar_flux_spectral and
compute_thermal_flux_spectral (scatterer_wavenumber): the numpy mirror of its definition
(tests/scatterer_cases.py) -- where grid points lie among the knots, what the limit guarantees, that
a flat table is the grey scatterer to the bit, that the case tables hold what they are named for --
the float64-vs-long-double scan of the mirrors over the case tables that measures E_cpu (printed;
scatterer_cases.E_CPU_SHORTWAVE and E_CPU_LONGWAVE record it and the GPU tests take their bound from
it), the argument checks (all raised before anything touches the GPU), the header of the two
entries (include/lbl_amd_scatterer.h) against abi.SCATTERER_PROTOTYPES, and what the spectral
calls and the grey ones queue on a stand-in engine."""
import ctypes
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths, two_stream
from pylbl_amd import engine as engine_module
from tests import abi_header, scatterer_cases as sc, sweep_cases as cases
from tests import surface_cases as surface
from tests import thermal_cases as tc, thermal_source_cases as tsc, two_stream_cases as ts
from tests.test_linear_source_host import make_spectroscopy

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_scatterer.h").read_text()
F64, LD = np.float64, np.longdouble
SHAPE = (3, 5)
ONES = np.ones(SHAPE)
INTERFACES = np.linspace(210., 290., 18).reshape(3, 6)
KNOTS = np.array([590., 600.5, 610.])
METHODS = ("compute_solar_flux", "compute_thermal_flux", "compute_thermal_flux_linear")


# ---------------------------------------------------------------------------------------------
# The definition.
def test_grid_points_on_below_between_and_above_the_knots():
    knots = np.array([-2., 1., 1.5, 7.])
    nu = np.array([-5., -2., np.nextafter(-2., 0.), 0., 1., 1.25, np.nextafter(1.5, 0.), 1.5, 6.,
                   7., np.nextafter(7., 8.), 1e300])
    j, u = sc.place(knots, nu)
    # j by counting, nothing of numpy's searches.
    count = np.array([np.sum(knots <= x) for x in nu]) - 1
    assert np.array_equal(j, np.clip(count, 0, 2))
    assert np.array_equal(j, [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2])
    assert np.all((u >= 0.) & (u <= 1.))
    assert u[0] == u[1] == 0. and u[4] == 0. and u[7] == 0. and u[5] == 0.5
    assert u[9] == u[10] == u[11] == 1. and 0. < u[2] < 1e-15 and 1. - 1e-15 < u[6] <= 1.
    # On a knot the value is the knot's, outside the knots the nearest knot's.
    optics = np.random.default_rng(1).uniform(0., 0.99, size=(4, 4, 3))
    e = sc.interpolate(knots, optics, nu)
    assert e.shape == (4, 12, 3)
    for column, knot in ((0, 0), (1, 0), (4, 1), (7, 2), (9, 3), (10, 3), (11, 3)):
        assert np.array_equal(e[:, column], optics[:, knot]), column
    assert np.array_equal(e[:, 5], optics[:, 1] + 0.5*(optics[:, 2] - optics[:, 1]))
    # A descending grid gives the same values in the other order.
    assert np.array_equal(sc.interpolate(knots, optics, nu[::-1]), e[:, ::-1])


def test_the_limit_keeps_every_precondition_of_the_grey_layer():
    """Random tables with values at the ends of their ranges, on grid points that include every
    knot and its two neighbours: tau_c >= 0, 0 <= omega_c <= 1, 0 <= g_c < 1, each inside its two
    knots' range -- also where the rounded interpolation leaves it, which happens."""
    rng = np.random.default_rng(2)
    knots = np.sort(rng.uniform(0., 3000., size=64))
    nu = np.concatenate([surface.knot_samples(knots), rng.uniform(-10., 3100., size=4000)])
    optics = np.stack([10.**rng.uniform(-300., 2., size=(50, 64)),
                       rng.choice([0., 1., np.nextafter(1., 0.), 0.3], size=(50, 64)),
                       rng.choice([0., np.nextafter(1., 0.), 0.9], size=(50, 64))], axis=2)
    optics[:, ::5, 0] = 0.
    j, u = sc.place(knots, nu)
    e0, e1 = optics[:, j, :], optics[:, j + 1, :]
    raw = e0 + u[:, None]*(e1 - e0)
    e = sc.interpolate(knots, optics, nu)
    low, high = np.minimum(e0, e1), np.maximum(e0, e1)
    assert np.all((e >= low) & (e <= high))
    assert np.all(e[..., 0] >= 0.) and np.all((e[..., 1] >= 0.) & (e[..., 1] <= 1.))
    assert np.all((e[..., 2] >= 0.) & (e[..., 2] < 1.))
    outside = (raw < low) | (raw > high)
    print("the rounded interpolation left its knots' range in %d of %d values" % (
        np.count_nonzero(outside), raw.size))
    assert np.any(outside)
    assert np.array_equal(e[~outside], raw[~outside])
    w_c = e[..., 1]*e[..., 0]
    assert np.all(w_c <= e[..., 0]) and np.all(w_c*e[..., 2] <= w_c)


@pytest.mark.parametrize("m", [2, 5, sc.MAX_KNOTS])
def test_a_flat_table_is_the_grey_scatterer_to_the_bit(m):
    """e_j = c at every knot: the per-element tables the layers receive are the grey level tables,
    so the mirrors agree bit for bit (and so must the entries)."""
    short = sc.shortwave_inputs(67, 3, m, 3)
    level = short.optics[:, 0, :].copy()
    short.optics[:] = sc.flat_optics(level, m)
    grey = short.grey(level)
    table = sc.shortwave_table(short.table, short.knots, short.optics, short.nu)
    assert np.array_equal(table, np.broadcast_to(grey.table[:, None, :], table.shape))
    a, b = ts.mirror(F64, short, True), ts.mirror(F64, grey, True)
    assert all(np.array_equal(a[name], b[name]) for name in b)
    long = sc.longwave_inputs(67, 3, m, 3)
    level = long.optics[:, 0, :].copy()
    level[::2, 1] = 0.                          # levels that only absorb
    long.optics[:] = sc.flat_optics(level, m)
    grey = long.grey(level)
    table = sc.longwave_table(long.table, long.knots, long.optics, long.nu)
    expect = np.broadcast_to(grey.table[:, None, :], table.shape)
    # (g_c of a level without w_c is not read.)
    assert np.array_equal(table[..., (0, 1, 2, 4)], expect[..., (0, 1, 2, 4)])
    assert np.array_equal(table[..., 3][table[..., 2] > 0.], expect[..., 3][table[..., 2] > 0.])
    for linear in (False, True):
        a = sc.longwave_mirror(F64, long, False, linear)
        b = tsc.mirror(F64, grey, False) if linear else tc.mirror(F64, grey.isothermal(), False)
        assert all(np.array_equal(a[name], b[name]) for name in b), linear


def lane_of(column):
    return column//cases.PATH_WIDTH


def test_case_tables_hold_what_they_are_named_for():
    short, long = sc.shortwave_cases(), sc.longwave_cases()
    assert len(short) == len(long)
    seen = {"kinds": set(), "m": set(), "depths": set(), "columns": set(), "descending": 0}
    for table in (short, long):
        for inputs, from_last in table:
            nu, knots, m = inputs.nu, inputs.knots, inputs.knots.size
            assert inputs.levels == cases.PATHS*inputs.levels_per_path
            assert np.all(np.diff(knots) > 0.) and 2 <= m <= sc.MAX_KNOTS
            seen["m"].add(m)
            seen["depths"].add(inputs.levels_per_path)
            seen["columns"].add(inputs.columns)
            seen["kinds"].update(sc.KINDS[k] for k in inputs.kind)
            descending = inputs.columns > 1 and nu[0] > nu[-1]
            seen["descending"] += descending
            # (The tables that move grid points onto a knot are looked at below.)
            if inputs.columns >= 8 and not hasattr(inputs, "at_zero"):
                # A knot interval ends between the two columns of a lane, and one between two
                # lanes of one wavefront: a knot lies between those columns.
                steps = np.flatnonzero(np.any(
                    (nu[None, :-1] - knots[:, None])*(nu[None, 1:] - knots[:, None]) < 0.,
                    axis=0))
                inside = [c for c in steps if lane_of(c) == lane_of(c + 1)]
                across = [c for c in steps if lane_of(c) != lane_of(c + 1) and
                          lane_of(c)//64 == lane_of(c + 1)//64]
                assert inside and across, inputs.name
                # (Two knots are both spent on that; with more, a grid point lies on a knot.)
                assert m == 2 or np.any(np.isin(nu, knots)), inputs.name
                assert np.any(nu < knots[0]) and np.any(nu > knots[-1]), inputs.name
    assert seen["m"] == set(sc.KNOT_COUNTS) and seen["depths"] == set(sc.DEPTHS) | {3}
    assert set(cases.LAYOUT_COLUMNS) <= seen["columns"]
    assert seen["kinds"] == set(sc.KINDS) and seen["descending"] == 4
    # What the kinds are: no scatterer, one that only absorbs (both clear levels of the longwave
    # entry), one that scatters at some knots only, omega_c in {0, 1} among random values, g_c up
    # to 0.9, tau_c exactly 0 at a knot.
    inputs = sc.shortwave_inputs(513, 17, sc.MAX_KNOTS, 57)
    tau, omega, g = (inputs.optics[..., i] for i in range(3))
    kind = np.array(sc.KINDS)[inputs.kind]
    assert np.all(tau[kind == "none"] == 0.) and np.all(omega[kind == "absorbing"] == 0.)
    assert np.all(tau[kind == "absorbing"] > 0.)
    clear = ~sc.scatters(inputs.optics)
    assert np.array_equal(clear, (kind == "none") | (kind == "absorbing"))
    some = omega[kind == "some knots"]
    assert np.all(some[:, ::2] == 0.) and np.all(some[:, 1::2] > 0.)
    assert np.any(omega[kind == "random"] == 0.) and np.any(omega[kind == "random"] == 1.)
    assert g.max() == 0.9 and np.any(g == 0.)
    zero = tau[kind == "to zero"]
    assert np.all(zero[:, 1::2] == 0.) and np.all(zero[:, ::2] > 0.)
    # The table with grid points one ulp either side of a knot where tau_c is exactly 0.
    for inputs in (sc.shortwave_to_zero(), sc.longwave_to_zero()):
        c, k = inputs.at_zero, inputs.knots[1]
        assert inputs.nu[c] == k and inputs.nu[c - 1] == np.nextafter(k, -np.inf)
        assert inputs.nu[c + 1] == np.nextafter(k, np.inf)
        e = sc.interpolate(inputs.knots, inputs.optics, inputs.nu)
        has = np.any(inputs.optics[:, :, 0] > 0., axis=1)
        assert np.any(has) and np.all(e[has, c, 0] == 0.) and np.all(e[..., 0] >= 0.)
        assert np.all(e[has, c - 1, 0] < 1e-12) and np.all(e[has, c + 1, 0] < 1e-12)
        assert np.all(e[has, c - 2, 0] > 1e-3)
    # In the longwave table some element of a level that scatters has tau == 0 exactly (a
    # thickness of 0 under tau_c == 0 at the knot): the clear branch of that element.
    inputs = sc.longwave_to_zero()
    li = inputs.layer_inputs(False)
    order = inputs.order(False).T
    scattering = sc.scatters(inputs.optics)[order]
    assert np.any((li["tau"] == 0.) & scattering[:, :, None])
    assert np.all(li["branch"][li["tau"] == 0.] == tc.CLEAR)


# ---------------------------------------------------------------------------------------------
# E_cpu.
def test_float64_mirrors_stay_close_to_long_double():
    worst = 0.
    for inputs, from_last in sc.shortwave_cases():
        error, finite = ts.worst_error(inputs, from_last)
        assert finite, inputs.name
        worst = max(worst, error)
    print("shortwave: worst |float64 - long double|/F0 = %.3g" % worst)
    assert worst <= sc.E_CPU_SHORTWAVE <= sc.E_CPU_CAP == ts.E_CPU_CAP
    for linear in (False, True):
        worst = 0.
        for inputs, from_last in sc.longwave_cases():
            error, finite = sc.longwave_worst_error(inputs, from_last, linear)
            assert finite, inputs.name
            worst = max(worst, error)
        print("longwave, linear = %s: worst |float64 - long double|/scale = %.3g" % (
            linear, worst))
        assert worst <= sc.E_CPU_LONGWAVE <= sc.E_CPU_CAP == tc.E_CPU_CAP == tsc.E_CPU_CAP


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_scatterer.h against abi.SCATTERER_PROTOTYPES, whole, as
# tests/test_thermal_source_host.py compares its header.
def declarations(header):
    """{function: [parameter, ...]} of a header, in its order, by abi_header's own pattern."""
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = {}
    for result, name, inside in re.findall(
            r"^(int|const char \*|void \*)\s*(lbl_\w+)\s*\(([^)]*)\)\s*;", code, re.M):
        assert result == "int" and name not in found, name
        found[name] = [re.sub(r"\s+", " ", p).strip() for p in inside.split(",")]
    assert set(re.findall(r"\b(lbl_\w+)\s*\(", code)) == set(found)
    return found


def test_header_declares_both_entries_and_ctypes_match():
    from pylbl_amd import abi
    declared = declarations(HEADER)
    short, long = "lbl_path_two_stream_spectral", "lbl_path_thermal_two_stream_spectral"
    assert list(declared) == list(abi.SCATTERER_PROTOTYPES) == [short, long]
    knots = ["int32_t n_knots", "const double *knot_wavenumber", "const double *knot_optics"]
    # lbl_path_two_stream's arguments with the grid and the knots behind level_table.
    old = declarations((ROOT / "include" / "lbl_amd_twostream.h").read_text())[
        "lbl_path_two_stream"]
    assert old[8] == "const double *level_table"
    assert declared[short] == old[:9] + ["int32_t grid"] + knots + old[9:]
    assert abi.SCATTERER_PROTOTYPES[short] == \
        abi.TWO_STREAM_PROTOTYPES["lbl_path_two_stream"][:9] + \
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p] + \
        abi.TWO_STREAM_PROTOTYPES["lbl_path_two_stream"][9:]
    # lbl_path_thermal_two_stream_source's with the knots behind edge_temperature.
    old = declarations((ROOT / "include" / "lbl_amd_thermal_source.h").read_text())[
        "lbl_path_thermal_two_stream_source"]
    assert old[10] == "const double *edge_temperature"
    assert declared[long] == old[:11] + knots + old[11:]
    source = abi.THERMAL_SOURCE_PROTOTYPES["lbl_path_thermal_two_stream_source"]
    assert abi.SCATTERER_PROTOTYPES[long] == \
        source[:11] + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p] + source[11:]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    for name, parameters in declared.items():
        argtypes = abi.SCATTERER_PROTOTYPES[name]
        assert len(argtypes) == len(parameters), name
        for argtype, parameter in zip(argtypes, parameters):
            abi_header.check_parameter(argtype, parameter, addresses=True)
        function = getattr(lib, name)
        assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
        for table in (abi.PROTOTYPES, abi.TWO_STREAM_PROTOTYPES, abi.THERMAL_PROTOTYPES,
                      abi.THERMAL_SOURCE_PROTOTYPES, abi.KDIST_PROTOTYPES, abi.RESULT_TYPES):
            assert name not in table
    # lbl_amd.h is as it was: the new header includes it and declares nothing of its own twice.
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    for method in ("path_two_stream_spectral", "path_thermal_two_stream_spectral"):
        assert callable(getattr(engine_module.Engine, method))
    bound = inspect.signature(engine_module.Engine.path_thermal_two_stream_spectral).parameters
    assert bound["edge_temperature"].default is None


def test_header_docstrings_and_kernels_state_the_same_definition():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    kernels = (ROOT / "pylbl_amd" / "csrc" / "scatterer.h").read_text()
    design = (ROOT / "DESIGN.md").read_text()
    section = design[design.index("## 26."):]
    for text in (HEADER, kernels, Spectroscopy.compute_solar_flux_spectral.__doc__, section,
                 sc.__doc__):
        text = squeeze(text)
        for line in ("j = the largest index with k_j <= nu, limited to 0 .. M-2",
                     "u = (nu - k_j)/(k_{j+1} - k_j), limited to [0, 1]",
                     "v = e_j + u*(e_{j+1} - e_j), then",
                     "limited to [min(e_j, e_{j+1}), max(e_j, e_{j+1})]"):
            assert line in text, line
    assert "kScattererMaxKnots = %d" % sc.MAX_KNOTS in kernels
    assert paths.MAX_SCATTERER_KNOTS == sc.MAX_KNOTS == paths.MAX_EMISSIVITY_KNOTS
    short = (ROOT / "pylbl_amd" / "csrc" / "twostream.h").read_text()
    long = (ROOT / "pylbl_amd" / "csrc" / "twostream_thermal.h").read_text()
    assert "kTwoStreamSpectralUpAhead = %d;" % sc.SHORTWAVE_UP_AHEAD in short
    assert "kThermalSpectralUpAhead = %d;" % sc.LONGWAVE_UP_AHEAD in long
    # The layers are not written again: the spectral element goes through the one of each file.
    assert short.count("TwoStreamLayer two_stream_layer(") == 1
    assert long.count("ThermalLayer thermal_layer(") == long.count("thermal_layer<") == 1
    for kernel in ("two_stream_up_kernel", "two_stream_down_kernel"):
        assert re.search(r"template <bool kVector, bool kSpectral = false>\s*__global__ "
                         r"__launch_bounds__\(kPathThreads\) void %s\(" % kernel, short), kernel
    for kernel in ("thermal_up_kernel", "thermal_down_kernel"):
        assert re.search(r"template <bool kVector, bool kLinear, bool kSpectral = false>\s*"
                         r"__global__ __launch_bounds__\(kPathThreads\) void %s\(" % kernel,
                         long), kernel


# ---------------------------------------------------------------------------------------------
# The requests.
def spectral(m=3, shape=SHAPE):
    tau = np.linspace(0., 2., int(np.prod(shape))*m).reshape(shape + (m,))
    return dict(scatterer_optical_depth=tau,
                scatterer_single_scattering_albedo=np.full(shape + (m,), 0.9),
                scatterer_asymmetry=np.full(shape + (m,), 0.8))


def changed(name, value, index=(1, 2, 1)):
    out = spectral()
    out[name] = out[name].copy()
    out[name][index] = value
    return out


TAU, OMEGA, G = ("scatterer_optical_depth", "scatterer_single_scattering_albedo",
                 "scatterer_asymmetry")
NONE = {TAU: None, OMEGA: None, G: None}
BAD = [
    (dict(NONE), "scatterer_wavenumber needs"),
    (dict(spectral(), scatterer_wavenumber=None), "scatterer_wavenumber must be given"),
    (dict(spectral(), scatterer_wavenumber=[600.]), "2..1024 knots"),
    (dict(spectral(), scatterer_wavenumber=np.arange(1025.)), "2..1024 knots"),
    (dict(spectral(), scatterer_wavenumber=np.ones((3, 1))), "2..1024 knots"),
    (dict(spectral(), scatterer_wavenumber=[590., 590., 610.]), "strictly ascending"),
    (dict(spectral(), scatterer_wavenumber=[610., 600., 590.]), "strictly ascending"),
    (dict(spectral(), scatterer_wavenumber=[590., np.nan, 610.]), "finite and strictly"),
    (dict(spectral(), scatterer_wavenumber=[590., 600., np.inf]), "finite and strictly"),
    (dict(spectral(2)), "one value per knot"),                       # a wrong trailing axis
    (dict(spectral(4)), "one value per knot"),
    (dict(scatterer_optical_depth=ONES, scatterer_single_scattering_albedo=ONES,
          scatterer_asymmetry=0.5*ONES), "one value per knot"),      # the grey shape
    (dict(spectral(), scatterer_asymmetry=np.full((3, 3, 5), 0.5)), "one value per knot"),
    (dict(spectral(), scatterer_asymmetry=None), "together or not at all"),
    (dict(NONE, scatterer_optical_depth=spectral()[TAU]), "together or not at all"),
    (changed(TAU, -1e-9), ">= 0"),
    (changed(TAU, np.nan), "must be finite"),
    (changed(TAU, np.inf), "must be finite"),
    (changed(OMEGA, 1.0000001), r"\[0, 1\]"),
    (changed(OMEGA, -0.1), r"\[0, 1\]"),
    (changed(OMEGA, np.nan), "must be finite"),
    (changed(G, 1.), r"\[0, 1\)"),
    (changed(G, -0.5), r"\[0, 1\)"),
    (changed(G, np.inf), "must be finite"),
]


def call_of(method, **keywords):
    call = dict(layer_thickness=ONES, scatterer_wavenumber=KNOTS)
    if method == "compute_solar_flux":
        call["solar_zenith_cosine"] = 0.5
    else:
        call["surface_temperature"] = 288.
    if method == "compute_thermal_flux_linear":
        call["interface_temperature"] = INTERFACES
    call.update(keywords)
    return call


def untouchable(monkeypatch):
    def touched(*arguments, **more):
        raise AssertionError("the GPU side was reached")
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", touched)
    monkeypatch.setattr(engine_module, "default_engine", lambda device=0: surface.Untouchable())


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("keywords, match", BAD)
def test_bad_arguments_are_refused_before_the_gpu(monkeypatch, method, keywords, match):
    untouchable(monkeypatch)
    spec = make_spectroscopy(SHAPE)
    with pytest.raises(ValueError, match=match):
        getattr(spec, sc.SPECTRAL_METHOD[method])(**call_of(method, **keywords))


@pytest.mark.parametrize("method", METHODS)
def test_group_is_still_not_offered(method):
    spec = make_spectroscopy(SHAPE)
    spec.group = object()
    with pytest.raises(NotImplementedError, match=sc.SPECTRAL_METHOD[method] + " does"):
        getattr(spec, sc.SPECTRAL_METHOD[method])(**call_of(method, **spectral()))


@pytest.mark.parametrize("method", METHODS)
def test_the_spectral_methods_take_the_grey_ones_arguments_and_the_knots(method):
    """The grey methods keep their signatures; the spectral ones take the same arguments with the
    knots and the three tables up front, none of them optional, and (the longwave one)
    interface_temperature as a keyword that selects the source."""
    grey = inspect.signature(getattr(Spectroscopy, method)).parameters
    assert "scatterer_wavenumber" not in grey
    new = inspect.signature(getattr(Spectroscopy, sc.SPECTRAL_METHOD[method])).parameters
    assert list(new)[3:7] == ["scatterer_wavenumber", TAU, OMEGA, G]
    empty = inspect.Parameter.empty
    assert all(new[name].default is empty for name in list(new)[1:7])
    assert set(new) == set(grey) | {"scatterer_wavenumber"} | (
        {"interface_temperature"} if method != "compute_solar_flux" else set())
    for name in set(grey) - {TAU, OMEGA, G, "interface_temperature"}:
        assert new[name].default == grey[name].default, name
    if method != "compute_solar_flux":
        assert new["interface_temperature"].default is None


def test_requests_hold_the_knot_table_and_a_level_table_without_scatterer():
    spec = make_spectroscopy(SHAPE)
    optics = spectral()
    thickness = np.arange(1., 16.).reshape(SHAPE)
    short = spec._solar_flux_request(
        thickness, 0.5, None, None, 1., "first", 0.2, None, True, None, optics[TAU],
        optics[OMEGA], optics[G], ("upward_flux",), None, "reference",
        scatterer_wavenumber=KNOTS)
    long = spec._thermal_flux_request(
        thickness, 288., 1., None, "first", 1.66, optics[TAU], optics[OMEGA], optics[G],
        ("upward_flux",), None, "reference", scatterer_wavenumber=KNOTS)
    linear = two_stream._thermal_flux_linear_request(
        spec, thickness, 288., INTERFACES, 1., None, "first", 1.66, optics[TAU], optics[OMEGA],
        optics[G], ("upward_flux",), None, "reference", scatterer_wavenumber=KNOTS)
    expect = np.stack([optics[name].reshape(15, 3) for name in (TAU, OMEGA, G)], axis=2)
    for request in (short, long, linear):
        assert np.array_equal(request.scatterer_knots, KNOTS)
        assert request.scatterer_knots.dtype == F64 and request.scatterer_knots.flags.c_contiguous
        assert request.scatterer_optics.shape == (15, 3, 3)
        assert request.scatterer_optics.flags.c_contiguous
        assert np.array_equal(request.scatterer_optics, expect)
        assert np.array_equal(request.level_table[:, 0], thickness.ravel())
    assert np.all(short.level_table[:, 2:] == 0.) and np.all(short.level_table[:, 1] > 0.)
    assert np.all(long.level_table[:, 1:4] == 0.) and np.all(linear.level_table[:, 1:4] == 0.)
    assert linear.edge_temperature.shape == (15, 2) and long.edge_temperature is None
    # Without the keyword the requests are what they were, and hold no table.
    grey = {name: value[..., 1] for name, value in optics.items()}
    plain = spec._thermal_flux_request(
        thickness, 288., 1., None, "first", 1.66, grey[TAU], grey[OMEGA], grey[G],
        ("upward_flux",), None, "reference")
    assert plain.scatterer_knots is None and plain.scatterer_optics is None
    assert np.array_equal(plain.level_table[:, 1], grey[TAU].ravel())
    assert np.array_equal(plain.level_table[:, 2], (grey[OMEGA]*grey[TAU]).ravel())
    # The table's bytes count against device_output_limit: 24 per level and knot.
    n = 1000
    assert paths._level_bytes(n, plain, ["a", "b"], 3, True) == 5*n*8
    assert paths._level_bytes(n, long, ["a", "b"], 3, True) == 5*n*8 + 3*24


# ---------------------------------------------------------------------------------------------
# The queue.
def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


def queue_of(spec, engine, limit_bytes, method, **keywords):
    spec.device_output_limit = (8 << 30) if limit_bytes is None else limit_bytes
    engine.begin()
    engine.knot_tables = []
    name = sc.SPECTRAL_METHOD[method] if "scatterer_wavenumber" in keywords else method
    result = getattr(spec, name)(**keywords)
    return list(engine.log), result


GREY_ENTRY = {"compute_solar_flux": "path_two_stream",
              "compute_thermal_flux": "path_thermal_two_stream",
              "compute_thermal_flux_linear": "path_thermal_two_stream_source"}
SPECTRAL_ENTRY = {"compute_solar_flux": "path_two_stream_spectral",
                  "compute_thermal_flux": "path_thermal_two_stream_spectral",
                  "compute_thermal_flux_linear": "path_thermal_two_stream_spectral"}


def queue_call(method, surface_end, **keywords):
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    call = dict(layer_thickness=thickness, surface=surface_end)
    if method == "compute_solar_flux":
        call.update(solar_zenith_cosine=[0.5, 0.8], surface_albedo=[0.2, 0.4],
                    quantities=("upward_flux", "downward_flux"))
    else:
        call.update(surface_temperature=[288., 270.], surface_emissivity=[0.9, 1.],
                    quantities=("upward_flux", "downward_flux"))
    if method == "compute_thermal_flux_linear":
        call["interface_temperature"] = surface.interfaces()
    call.update(keywords)
    return call


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_the_spectral_methods_queue_one_spectral_call_per_run_and_the_grey_ones_todays_calls(
        tmp_path, monkeypatch, method, surface_end):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    m = 4
    knots = np.array([10., 30., 50., 70.])
    shape = surface.SHAPE + (m,)
    rng = np.random.default_rng(5)
    optics = dict(scatterer_optical_depth=rng.uniform(0., 2., size=shape),
                  scatterer_single_scattering_albedo=rng.uniform(0., 1., size=shape),
                  scatterer_asymmetry=rng.uniform(0., 0.9, size=shape))
    table = np.stack([optics[name].reshape(6, m) for name in (TAU, OMEGA, G)], axis=2)
    grey = {name: value[..., 0] for name, value in optics.items()}
    new, old = SPECTRAL_ENTRY[method] + "(", GREY_ENTRY[method] + "("
    # Per level beta, two work rows and two flux rows of 164 values, and the table's 24 bytes
    # per knot: a path of three levels needs 3*(5*164*8 + 24*m) bytes.
    path_bytes = 3*(5*surface.ROW_BYTES + 24*m)
    with sc.recorded(tmp_path) as (spec, engine):
        for limit, runs in ((None, 1), (2*path_bytes, 1), (2*path_bytes - 1, 2),
                            (path_bytes, 2)):
            log, result = queue_of(spec, engine, limit, method, scatterer_wavenumber=knots,
                                   **queue_call(method, surface_end, **optics))
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            sweeps = [line for line in log if line.startswith(new)]
            assert len(sweeps) == runs and not any(line.startswith(old) for line in log)
            begins = [int(argument(line, "level_begin")) for line in sweeps]
            from_last = surface_end == "first"
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            assert {argument(line, "from_last") for line in sweeps} == {str(from_last)}
            # Every run passes the knots and its own rows of the table, and the level table it
            # passes holds no scatterer.
            assert [begin for begin, _, _ in engine.knot_tables] == begins
            rows = 6//runs
            for begin, k, rows_of_table in engine.knot_tables:
                assert np.array_equal(k, knots)
                assert np.array_equal(rows_of_table, table[begin:begin + rows])
            assert result["scatterer"] == "spectral"
            assert result["upward_flux"].shape == (2, 4, 160)
            linear = method == "compute_thermal_flux_linear"
            assert all(("edge_temperature" in line) == linear for line in sweeps)
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, path_bytes - 1, method, scatterer_wavenumber=knots,
                     **queue_call(method, surface_end, **optics))
        # Without the table's bytes the same limit holds a path: the grey call is cut as it was.
        log, plain = queue_of(spec, engine, path_bytes - 1, method,
                              **queue_call(method, surface_end, **grey))
        assert sum(line.startswith(old) for line in log) == 2
        assert not any(line.startswith(new) for line in log) and not engine.knot_tables
        assert "scatterer" not in plain
        grey_logs = {limit: queue_of(spec, engine, limit, method,
                                     **queue_call(method, surface_end, **grey))[0]
                     for limit in (None, 15*surface.ROW_BYTES)}
    # The recorders from before know nothing of the new entries, and a grey call queues on them
    # what it queues here, line by line.
    before = {"compute_solar_flux": ts, "compute_thermal_flux": tc,
              "compute_thermal_flux_linear": tsc}[method]
    with before.recorded(tmp_path) as (spec, engine):
        assert not hasattr(engine, SPECTRAL_ENTRY[method])
        for limit, expect in grey_logs.items():
            log, _ = queue_of(spec, engine, limit, method,
                              **queue_call(method, surface_end, **grey))
            # (The grid goes to an engine once: here with the first call.)
            log, expect = ([line for line in lines if not line.startswith("load_grid(")]
                           for lines in (log, expect))
            assert log == expect and sum(line.startswith(old) for line in log) >= 1
