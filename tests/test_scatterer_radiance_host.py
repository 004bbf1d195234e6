"""CPU-only checks of compute_thermal_radiance_spectral and compute_solar_radiance_spectral: the
numpy mirror of their definition (tests/scatterer_radiance_cases.py) against the properties
include/lbl_amd_scatterer_radiance.h states -- a flat table is the grey view to the bit, a longwave
level that scatters nowhere is a clear level with tau_c(nu) and without any scatterer the result is
the clear-sky radiance to the bit, a shortwave table that scatters nowhere only attenuates along
both slant paths --, that the case tables hold what they are named for and decide every branch far
from its threshold, the float64-vs-long-double scan that measures E_cpu (printed;
scatterer_radiance_cases.E_CPU_THERMAL and E_CPU_SOLAR record it and the GPU tests take their bound
from it), the argument checks (all raised before anything touches the GPU), the header of the two
entries against abi.SCATTERER_RADIANCE_PROTOTYPES, and what the spectral calls and the grey ones
queue on a stand-in engine."""
import ctypes
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy
from pylbl_amd import engine as engine_module
from tests import abi_header, scatterer_cases as sc, scatterer_radiance_cases as rc
from tests import solar_radiance_cases as src, surface_cases as surface, sweep_cases as cases
from tests import thermal_cases as tc, thermal_radiance_cases as trc, two_stream_cases as ts
from tests.test_linear_source_host import make_spectroscopy
from tests.test_scatterer_host import BAD, G, KNOTS, OMEGA, ONES, SHAPE, TAU, declarations, spectral

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_scatterer_radiance.h").read_text()
F64, LD = np.float64, np.longdouble
METHODS = ("compute_thermal_radiance", "compute_solar_radiance")
THERMAL_CASES, SOLAR_CASES = rc.thermal_cases(), rc.solar_cases()


def cosines(inputs, mu, phi):
    return src.scattering_cosine(mu, inputs.mu0, phi)


# ---------------------------------------------------------------------------------------------
# Property 1: a flat table is the grey view.
@pytest.mark.parametrize("m", [2, rc.MAX_KNOTS])
@pytest.mark.parametrize("from_last", [False, True])
def test_a_flat_table_is_the_grey_view_to_the_bit(m, from_last):
    long = sc.longwave_inputs(67, 3, m, 3)
    level = long.optics[:, 0, :].copy()
    level[::2, 1] = 0.                          # levels that only absorb
    long.optics[:] = sc.flat_optics(level, m)
    grey = long.grey(level).isothermal()
    a = rc.thermal_mirror(F64, long, rc.MU, from_last)
    b = trc.mirror(F64, grey, rc.MU, from_last)
    assert np.array_equal(a["radiance"], b["radiance"])
    assert np.array_equal(a["brightness_temperature"], b["brightness_temperature"],
                          equal_nan=True)
    short = sc.shortwave_inputs(67, 3, m, 3)
    level = short.optics[:, 0, :].copy()
    short.optics[:] = sc.flat_optics(level, m)
    grey = short.grey(level)
    cos_theta = cosines(short, rc.MU, rc.PHI)
    a = rc.solar_mirror(F64, short, rc.MU, cos_theta, from_last)
    b = src.mirror(F64, grey, rc.MU, cos_theta, from_last)
    assert np.array_equal(a["radiance"], b["radiance"]) and np.any(a["radiance"] > 0.)
    # Every branch of the grey level is among them.
    li = rc.solar_view_inputs(short, from_last)
    assert {ts.CONSERVATIVE_BRANCH, ts.GENERAL} <= set(np.unique(li["branch"]))


# ---------------------------------------------------------------------------------------------
# Property 2: the longwave view without scattering.
def test_a_longwave_level_that_scatters_nowhere_is_clear_with_its_own_optical_depth():
    inputs = sc.longwave_inputs(131, 3, 3, 9)
    inputs.optics[:, :, 1] = 0.                 # nothing scatters: tau_c(nu) only absorbs
    assert np.any(inputs.optics[:, :, 0] > 0.) and not np.any(sc.scatters(inputs.optics))
    li = inputs.layer_inputs(True)
    order = inputs.order(True).T
    tau_c = sc.interpolate(inputs.knots, inputs.optics, inputs.nu)[..., 0][order]
    assert np.all(li["branch"] == tc.CLEAR)
    assert np.array_equal(li["t"], inputs.table[order][:, :, None, 0]*inputs.beta[order] + tau_c)
    assert np.any(tau_c > 0.) and np.any(np.diff(tau_c, axis=-1) != 0.)


@pytest.mark.parametrize("from_last", [False, True])
def test_without_any_scatterer_the_longwave_view_is_the_clear_sky_radiance_to_the_bit(from_last):
    """eps = 1 and mu = 1: lbl_path_radiance's lines, I = I*exp(-x) + B*(-expm1(-x)) with x =
    s*beta from the surface's B(T_s) upwards, in float64 as written."""
    inputs = sc.longwave_inputs(131, 3, 3, 9)
    inputs.optics[:] = 0.
    inputs.emissivity = np.ones(rc.PATHS)
    got = rc.thermal_mirror(F64, inputs, np.ones(rc.PATHS), from_last)["radiance"]
    order = inputs.order(from_last)
    nu = inputs.nu[None, :]
    rad = cases.planck(F64, nu, inputs.surface_t[:, None])
    for i in range(inputs.levels_per_path - 1, -1, -1):
        level = order[:, i]
        x = inputs.table[level, 0][:, None]*inputs.beta[level]
        planck = cases.planck(F64, nu, inputs.table[level, 4][:, None])
        rad = rad*np.exp(-x) + planck*(-np.expm1(-x))
    assert np.array_equal(got, rad) and np.any(rad > 0.)


# ---------------------------------------------------------------------------------------------
# Property 3: the shortwave view without scattering.
@pytest.mark.parametrize("absorbing", [False, True])
def test_a_shortwave_table_that_scatters_nowhere_only_attenuates_along_both_slant_paths(absorbing):
    inputs = rc.without_rayleigh(sc.shortwave_inputs(131, 3, 3, 9))
    inputs.mu0 = np.array(src.MU0)
    inputs.optics[:, :, 1] = 0.
    if not absorbing:
        inputs.optics[:] = 0.
    cos_theta = cosines(inputs, rc.MU, rc.PHI)
    high = rc.solar_mirror(LD, inputs, rc.MU, cos_theta, False)
    low = rc.solar_mirror(F64, inputs, rc.MU, cos_theta, False)
    li = rc.solar_view_inputs(inputs, False)
    assert set(np.unique(li["branch"])) <= {ts.IDENTITY, src.NO_SCATTERING}
    tau_c = sc.interpolate(inputs.knots, inputs.optics, inputs.nu)[..., 0]
    assert np.any(tau_c > 0.) == absorbing
    n = inputs.levels_per_path
    tau = (inputs.table[:, None, 0]*inputs.beta + tau_c).astype(LD)
    depth = np.sum(tau.reshape(rc.PATHS, n, -1), axis=1)
    mu0, mu = inputs.mu0.astype(LD)[:, None], rc.MU.astype(LD)[:, None]
    expect = inputs.albedo.astype(LD)[:, None]*(inputs.f0().astype(LD)/LD(cases.FLUX_PI)) * \
        np.exp(-(depth/mu0))*np.exp(-(depth/mu))
    # The few roundings per level that solar_radiance_cases documents, the surface's three and the
    # flux rows' direct beam (one product and one exp per level).
    allowed = LD((2.*src.NO_SCATTERING_ROUNDINGS*n + 3.)*2.**-53)*src.scale(inputs, high)
    for got in (low, high):
        assert np.all(np.abs(got["radiance"].astype(LD) - expect) <= allowed)
    assert np.any(expect > 0.)


# ---------------------------------------------------------------------------------------------
# The case tables.
def test_case_tables_hold_what_they_are_named_for():
    seen = {"columns": set(), "depths": set(), "m": set(), "orders": set(), "descending": 0}
    for inputs, _, from_last in THERMAL_CASES:
        seen["columns"].add(inputs.columns)
        seen["depths"].add(inputs.levels_per_path)
        seen["m"].add(inputs.knots.size)
        seen["orders"].add(from_last)
        seen["descending"] += inputs.columns > 1 and inputs.nu[0] > inputs.nu[-1]
        assert inputs.levels == rc.PATHS*inputs.levels_per_path
    assert set(rc.COLUMNS) <= seen["columns"] and set(rc.DEPTHS) <= seen["depths"]
    assert seen["m"] == set(rc.KNOT_COUNTS) and seen["orders"] == {False, True}
    assert seen["descending"] == 2
    assert [(i.columns, i.levels_per_path, i.knots.size, f) for i, _, f in THERMAL_CASES][:8] == \
        [(i.columns, i.levels_per_path, i.knots.size, f) for i, _, _, f in SOLAR_CASES][:8]
    assert {i.rayleigh for i, _, _, _ in SOLAR_CASES} == {False, True}
    assert all(np.all(i.sigma == 0.) for i, _, _, _ in SOLAR_CASES if not i.rayleigh)
    assert any(np.any(i.sigma > 0.) for i, _, _, _ in SOLAR_CASES if i.rayleigh)
    # Grid points below k_0, on a knot, between knots and above k_{M-1}.
    inputs = THERMAL_CASES[5][0]
    assert inputs.columns == 1031 and inputs.knots.size == 3
    assert np.any(inputs.nu < inputs.knots[0]) and np.any(inputs.nu > inputs.knots[-1])
    assert np.any(np.isin(inputs.nu, inputs.knots))
    assert np.any((inputs.nu > inputs.knots[0]) & (inputs.nu < inputs.knots[1]))
    # A level whose omega_c is 0 at every knot beside tau_c > 0, and levels without a scatterer.
    kinds = np.array(sc.KINDS)[inputs.kind]
    absorbing = inputs.optics[kinds == "absorbing"]
    assert absorbing.size and np.all(absorbing[..., 1] == 0.) and np.all(absorbing[..., 0] > 0.)
    assert np.any(kinds == "none") and np.any(kinds == "random")
    # One cloud: clear and cloudy levels alternate, one scattering level per path.
    for table in (THERMAL_CASES, SOLAR_CASES):
        inputs = next(c[0] for c in table if c[0].name.endswith("one cloud") or
                      "one cloud," in c[0].name)
        scattering = sc.scatters(inputs.optics).reshape(rc.PATHS, -1)
        assert np.all(np.sum(scattering, axis=1) == 1) and np.all(scattering[:, 1])
    # tau == 0 inside a level that scatters: the clear line (longwave), the identity (shortwave).
    inputs = sc.longwave_to_zero()
    li = inputs.layer_inputs(False)
    scattering = sc.scatters(inputs.optics)[inputs.order(False).T]
    assert np.any((li["tau"] == 0.) & scattering[:, :, None])
    assert np.all(li["branch"][li["tau"] == 0.] == tc.CLEAR)
    inputs = sc.shortwave_to_zero()
    li = rc.solar_view_inputs(inputs, False)
    scattering = sc.scatters(inputs.optics)[inputs.sun_order(False).T]
    assert np.any((li["branch"] == ts.IDENTITY) & scattering[:, :, None])
    # The guard around k*mu0 = 1 and the conservative column.
    li = rc.solar_view_inputs(rc.guarded(), False)
    assert np.count_nonzero(li["branch"] == ts.GUARDED) >= 30
    assert np.any(li["above"][li["branch"] == ts.GUARDED])
    assert not np.all(li["above"][li["branch"] == ts.GUARDED])
    inputs = rc.conservative()
    li = rc.solar_view_inputs(inputs, False)
    assert np.all(inputs.optics[:, :, 1] == 1.) and np.all(inputs.beta[:, ::2] == 0.)
    assert np.all(li["branch"][:, :, ::2] == ts.CONSERVATIVE_BRANCH)
    assert np.all(li["branch"][:, :, 1::2] == ts.GENERAL)
    # Over all tables every branch of both views occurs.
    thermal = np.concatenate([i.layer_inputs(f)["branch"].ravel() for i, _, f in THERMAL_CASES])
    assert set(np.unique(thermal)) == {tc.CLEAR, tc.CONSERVATIVE_BRANCH, tc.GENERAL}
    solar = np.concatenate([rc.solar_view_inputs(i, f)["branch"].ravel()
                            for i, _, _, f in SOLAR_CASES])
    assert set(np.unique(solar)) == {ts.IDENTITY, ts.CONSERVATIVE_BRANCH, ts.GENERAL, ts.GUARDED,
                                     src.NO_SCATTERING}


def test_both_mirrors_take_the_same_branch_in_every_element():
    """The long-double mirror continues from the float64 decisions; the tables keep every decision
    at least DECISION_MARGIN (relative) from its threshold, a distance that float64 rounding (1e-16)
    and the difference between the two mirrors' scalars (below 1e-10) cannot bridge: decided in
    long double, every element would take the branch it takes."""
    worst = np.inf
    for inputs, mu, from_last in THERMAL_CASES:
        worst = min(worst, rc.thermal_margin(inputs, mu, from_last))
    print("longwave: the nearest decision lies %.3g of its threshold away" % worst)
    assert worst >= rc.DECISION_MARGIN
    worst = np.inf
    for inputs, mu, _, from_last in SOLAR_CASES:
        worst = min(worst, rc.solar_margin(inputs, mu, from_last))
    print("shortwave: the nearest decision lies %.3g of its threshold away" % worst)
    assert worst >= rc.DECISION_MARGIN


# ---------------------------------------------------------------------------------------------
# E_cpu.
def test_float64_mirrors_stay_close_to_long_double():
    worst = 0.
    for inputs, mu, from_last in THERMAL_CASES:
        error, finite = rc.thermal_worst_error(inputs, mu, from_last)
        assert finite, inputs.name
        worst = max(worst, error)
    print("E_CPU_THERMAL: worst |float64 - long double|/scale = %.3g" % worst)
    assert worst <= rc.E_CPU_THERMAL < rc.E_CPU_CAP == trc.E_CPU_CAP
    assert rc.E_CPU_THERMAL <= 1.05*worst + 1e-13, "the recorded constant is the measured value"
    worst = 0.
    for inputs, mu, phi, from_last in SOLAR_CASES:
        error, finite = rc.solar_worst_error(inputs, mu, cosines(inputs, mu, phi), from_last)
        assert finite, inputs.name
        worst = max(worst, error)
    print("E_CPU_SOLAR: worst |float64 - long double|/scale = %.3g" % worst)
    assert worst <= rc.E_CPU_SOLAR < rc.E_CPU_CAP == src.E_CPU_CAP
    assert rc.E_CPU_SOLAR <= 1.05*worst + 1e-13, "the recorded constant is the measured value"


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_scatterer_radiance.h against abi.SCATTERER_RADIANCE_PROTOTYPES.
def test_header_declares_both_entries_and_ctypes_match():
    from pylbl_amd import abi
    declared = declarations(HEADER)
    long, short = "lbl_path_thermal_radiance_spectral", "lbl_path_solar_radiance_spectral"
    assert list(declared) == list(abi.SCATTERER_RADIANCE_PROTOTYPES) == [long, short]
    knots = ["int32_t n_knots", "const double *knot_wavenumber", "const double *knot_optics"]
    types = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    # lbl_path_thermal_radiance's arguments with the knots behind level_table.
    old = declarations((ROOT / "include" / "lbl_amd_thermal_radiance.h").read_text())[
        "lbl_path_thermal_radiance"]
    assert old[9] == "const double *level_table"
    assert declared[long] == old[:10] + knots + old[10:]
    grey = abi.THERMAL_RADIANCE_PROTOTYPES["lbl_path_thermal_radiance"]
    assert abi.SCATTERER_RADIANCE_PROTOTYPES[long] == grey[:10] + types + grey[10:]
    # lbl_path_solar_radiance's with the grid and the knots behind level_table, in
    # lbl_path_two_stream_spectral's order.
    old = declarations((ROOT / "include" / "lbl_amd_solar_radiance.h").read_text())[
        "lbl_path_solar_radiance"]
    assert old[8] == "const double *level_table"
    assert declared[short] == old[:9] + ["int32_t grid"] + knots + old[9:]
    flux = declarations((ROOT / "include" / "lbl_amd_scatterer.h").read_text())[
        "lbl_path_two_stream_spectral"]
    assert declared[short][:13] == flux[:13]
    grey = abi.SOLAR_RADIANCE_PROTOTYPES["lbl_path_solar_radiance"]
    assert abi.SCATTERER_RADIANCE_PROTOTYPES[short] == \
        grey[:9] + [ctypes.c_int32] + types + grey[9:]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    for name, parameters in declared.items():
        argtypes = abi.SCATTERER_RADIANCE_PROTOTYPES[name]
        assert len(argtypes) == len(parameters), name
        for argtype, parameter in zip(argtypes, parameters):
            abi_header.check_parameter(argtype, parameter, addresses=True)
        function = getattr(lib, name)
        assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
        for table in (abi.PROTOTYPES, abi.SCATTERER_PROTOTYPES, abi.THERMAL_RADIANCE_PROTOTYPES,
                      abi.SOLAR_RADIANCE_PROTOTYPES, abi.RESULT_TYPES):
            assert name not in table
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    for method in ("path_thermal_radiance_spectral", "path_solar_radiance_spectral"):
        assert callable(getattr(engine_module.Engine, method))


def test_header_kernels_and_docstrings_state_the_same_definition():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    design = (ROOT / "DESIGN.md").read_text()
    section = squeeze(design[design.index("## 30."):])
    header = squeeze(HEADER)
    long = (ROOT / "pylbl_amd" / "csrc" / "thermal_radiance.h").read_text()
    short = (ROOT / "pylbl_amd" / "csrc" / "solar_radiance.h").read_text()
    assert "lbl_amd_scatterer.h" in header
    for line in ("a = (3*(gp*mu))/2", "gc = h_c/w_c (0 where w_c == 0)", "1 - 2^-53",
                 "bit for bit", "scatterer_lane"):
        assert line in header and line in section, line
    for text in (Spectroscopy.compute_thermal_radiance_spectral.__doc__, ):
        text = squeeze(text)
        for line in ("j = the largest index with k_j <= nu, limited to 0 .. M-2",
                     "u = (nu - k_j)/(k_{j+1} - k_j), limited to [0, 1]",
                     "a = (3*(gp*mu))/2"):
            assert line in text, line
    assert "kSolarViewMaxAsymmetry = 1. - 0x1p-53;" in short
    assert rc.MAX_ASYMMETRY == np.nextafter(1., 0.)
    # The levels are not written again, and every column is placed by scatterer.h's one function.
    assert long.count("double thermal_view_cloudy(") == 1
    assert short.count("double solar_view_level(") == 1
    for text, kernel in ((long, "thermal_view_kernel"), (short, "solar_view_kernel")):
        assert re.search(r"template <bool kVector, bool kSpectral = false>\s*__global__ "
                         r"__launch_bounds__\(kPathThreads\) void %s\(" % kernel, text), kernel
    lane = (ROOT / "pylbl_amd" / "csrc" / "scatterer.h").read_text()
    assert lane.count("ScattererLane scatterer_lane(") == 1
    assert "scatterer_lane(a.scatterer, c.nu)" in long
    assert "two_stream_knots<kVector>(a, l)" in short
    # (No second search: the loop over the knots stands in scatterer.h alone.)
    assert "while (hi - lo > 1)" in lane
    assert "while (hi - lo > 1)" not in long and "while (hi - lo > 1)" not in short


# ---------------------------------------------------------------------------------------------
# The requests.
def call_of(method, **keywords):
    call = dict(layer_thickness=ONES, scatterer_wavenumber=KNOTS)
    if method == "compute_solar_radiance":
        call["solar_zenith_cosine"] = 0.5
    else:
        call["surface_temperature"] = 288.
    call.update(keywords)
    return call


def untouchable(monkeypatch):
    def touched(*arguments, **more):
        raise AssertionError("the GPU side was reached")
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", touched)
    monkeypatch.setattr(engine_module, "default_engine", lambda device=0: surface.Untouchable())


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("keywords, match", BAD)
def test_bad_scatterers_are_refused_before_the_gpu(monkeypatch, method, keywords, match):
    untouchable(monkeypatch)
    spec = make_spectroscopy(SHAPE)
    with pytest.raises(ValueError, match=match):
        getattr(spec, rc.SPECTRAL_METHOD[method])(**call_of(method, **keywords))


@pytest.mark.parametrize("method", METHODS)
def test_the_grey_calls_errors_still_come_and_in_their_order(monkeypatch, method):
    untouchable(monkeypatch)
    spec = make_spectroscopy(SHAPE)
    new = getattr(spec, rc.SPECTRAL_METHOD[method])
    good = spectral()
    bad_knots = dict(good, scatterer_wavenumber=[610., 600., 590.])
    # What the grey call checks before its scatterer wins over a bad table ...
    with pytest.raises(ValueError, match="surface must be one of"):
        new(**call_of(method, surface="middle", **bad_knots))
    with pytest.raises(ValueError, match="layer_thickness|layer thicknesses"):
        new(**call_of(method, **dict(bad_knots, layer_thickness=np.ones((3, 4)))))
    if method == "compute_thermal_radiance":
        with pytest.raises(ValueError, match="diffusivity must be"):
            new(**call_of(method, diffusivity=3., **bad_knots))
    else:
        with pytest.raises(ValueError, match="solar_zenith_cosine must lie"):
            new(**call_of(method, **dict(bad_knots, solar_zenith_cosine=1.5)))
    # ... and what it checks behind it loses to one.
    with pytest.raises(ValueError, match="strictly ascending"):
        new(**call_of(method, view_zenith_cosine=0., **bad_knots))
    with pytest.raises(ValueError, match="strictly ascending"):
        new(**call_of(method, range_policy="never", **bad_knots))
    # With a good table the view's own checks, the quantities, bands and instrument.
    for keywords, match in ((dict(view_zenith_cosine=0.), r"view_zenith_cosine must lie in \(0"),
                            (dict(view_zenith_cosine=1.01), "view_zenith_cosine must lie"),
                            (dict(view_zenith_cosine=[1., 1.]), "view_zenith_cosine"),
                            (dict(quantities=("upward_flux",)), "upward_flux"),
                            (dict(range_policy="never"), "range_policy"),
                            (dict(band_edges=[600.5]), "band")):
        with pytest.raises(ValueError, match=match):
            new(**call_of(method, **keywords, **good))
    if method == "compute_thermal_radiance":
        with pytest.raises(ValueError, match="only available on the grid"):
            new(**call_of(method, quantities=("brightness_temperature",),
                          band_edges=[600., 600.5], **good))
        with pytest.raises(TypeError, match="interface_temperature"):
            new(**call_of(method, interface_temperature=np.ones((3, 6)), **good))
    else:
        with pytest.raises(ValueError, match="relative_azimuth must be finite"):
            new(**call_of(method, relative_azimuth=np.nan, **good))
        with pytest.raises(ValueError, match="brightness_temperature"):
            new(**call_of(method, quantities=("brightness_temperature",), **good))
    spec.group = object()
    with pytest.raises(NotImplementedError, match=rc.SPECTRAL_METHOD[method] + " does"):
        new(**call_of(method, **good))


@pytest.mark.parametrize("method", METHODS)
def test_the_spectral_methods_take_the_grey_ones_arguments_and_the_knots(method):
    grey = inspect.signature(getattr(Spectroscopy, method)).parameters
    assert "scatterer_wavenumber" not in grey
    new = inspect.signature(getattr(Spectroscopy, rc.SPECTRAL_METHOD[method])).parameters
    assert list(new)[3:7] == ["scatterer_wavenumber", TAU, OMEGA, G]
    empty = inspect.Parameter.empty
    assert all(new[name].default is empty for name in list(new)[1:7])
    assert set(new) == set(grey) | {"scatterer_wavenumber"}
    for name in set(grey) - {TAU, OMEGA, G}:
        assert new[name].default == grey[name].default, name
    others = [name for name in new if name not in ("scatterer_wavenumber", TAU, OMEGA, G)]
    assert others == [name for name in grey if name not in (TAU, OMEGA, G)]


def test_requests_hold_the_knot_table_and_a_level_table_without_scatterer():
    from pylbl_amd import two_stream
    spec = make_spectroscopy(SHAPE)
    optics = spectral()
    thickness = np.arange(1., 16.).reshape(SHAPE)
    long = two_stream._thermal_radiance_request(
        spec, thickness, 288., 0.7, 1., None, "first", 1.66, optics[TAU], optics[OMEGA],
        optics[G], ("radiance",), None, None, "reference", scatterer_wavenumber=KNOTS,
        caller="compute_thermal_radiance_spectral")
    short = two_stream._solar_radiance_request(
        spec, thickness, 0.5, 0.7, 180., None, None, 1., "first", 0.2, None, True, None,
        optics[TAU], optics[OMEGA], optics[G], ("radiance",), None, None, "reference",
        scatterer_wavenumber=KNOTS, caller="compute_solar_radiance_spectral")
    expect = np.stack([optics[name].reshape(15, 3) for name in (TAU, OMEGA, G)], axis=2)
    for request in (long, short):
        assert np.array_equal(request.scatterer_knots, KNOTS)
        assert np.array_equal(request.scatterer_optics, expect)
        assert request.scatterer_optics.flags.c_contiguous
        assert np.array_equal(request.level_table[:, 0], thickness.ravel())
        assert np.all(request.mu == 0.7)
    assert np.all(long.level_table[:, 1:4] == 0.) and long.edge_temperature is None
    assert np.all(short.level_table[:, 2:] == 0.) and np.all(short.level_table[:, 1] > 0.)
    # Without the keyword the requests are what they were, and hold no table.
    grey = {name: value[..., 1] for name, value in optics.items()}
    plain = two_stream._thermal_radiance_request(
        spec, thickness, 288., 0.7, 1., None, "first", 1.66, grey[TAU], grey[OMEGA], grey[G],
        ("radiance",), None, None, "reference")
    assert plain.scatterer_knots is None and plain.scatterer_optics is None
    assert np.array_equal(plain.level_table[:, 2], (grey[OMEGA]*grey[TAU]).ravel())


# ---------------------------------------------------------------------------------------------
# The queue.
def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


def queue_of(spec, engine, limit_bytes, method, **keywords):
    spec.device_output_limit = (8 << 30) if limit_bytes is None else limit_bytes
    engine.begin()
    engine.knot_tables, engine.view_tables = [], []
    name = rc.SPECTRAL_METHOD[method] if "scatterer_wavenumber" in keywords else method
    result = getattr(spec, name)(**keywords)
    return list(engine.log), result


FLUX_ENTRY = {"compute_thermal_radiance": "path_thermal_two_stream",
              "compute_solar_radiance": "path_two_stream"}
VIEW_ENTRY = {"compute_thermal_radiance": "path_thermal_radiance",
              "compute_solar_radiance": "path_solar_radiance"}
FLUX_ROWS = {"compute_thermal_radiance": ("up_rows", "down_rows"),
             "compute_solar_radiance": ("up_rows", "direct_rows", "diffuse_rows")}
LEVEL_BLOCKS = {"compute_thermal_radiance": 5, "compute_solar_radiance": 6}


def queue_call(method, surface_end, **keywords):
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    call = dict(layer_thickness=thickness, surface=surface_end, view_zenith_cosine=[1., 0.4])
    if method == "compute_solar_radiance":
        call.update(solar_zenith_cosine=[0.5, 0.8], surface_albedo=[0.2, 0.4],
                    relative_azimuth=[0., 120.])
    else:
        call.update(surface_temperature=[288., 270.], surface_emissivity=[0.9, 1.])
    call.update(keywords)
    return call


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_the_spectral_methods_queue_the_two_spectral_entries_per_run_and_the_grey_ones_todays(
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
    flux, view = FLUX_ENTRY[method], VIEW_ENTRY[method]
    blocks = LEVEL_BLOCKS[method]
    # Per level the call's blocks of 164 values and the table's 24 bytes per knot.
    path_bytes = 3*(blocks*surface.ROW_BYTES + 24*m)
    with rc.recorded(tmp_path) as (spec, engine):
        for limit, runs in ((None, 1), (2*path_bytes, 1), (2*path_bytes - 1, 2),
                            (path_bytes, 2)):
            log, result = queue_of(spec, engine, limit, method, scatterer_wavenumber=knots,
                                   **queue_call(method, surface_end, **optics))
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            names = [line.split("(")[0] for line in log if line.startswith("path_")]
            # The flux entry, then the view entry, per run; nothing of the grey entries.
            assert names == [flux + "_spectral", view + "_spectral"]*runs
            fluxes = [line for line in log if line.startswith(flux + "_spectral(")]
            views = [line for line in log if line.startswith(view + "_spectral(")]
            from_last = surface_end == "first"
            begins = [int(argument(line, "level_begin")) for line in views]
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            shared = ("beta", "grid", "columns", "n_paths", "levels_per_path", "level_begin",
                      "level_table", "knot_wavenumber", "knot_optics", "from_last",
                      "asynchronous") + FLUX_ROWS[method]
            for one, other in zip(fluxes, views):
                for name in shared:
                    assert argument(one, name) == argument(other, name), name
                assert argument(other, "from_last") == str(from_last)
                assert argument(other, "asynchronous") == "True"
                assert "edge_temperature" not in one and "band_start" not in one
                held = {argument(other, name) for name in ("beta", "radiance_rows") +
                        FLUX_ROWS[method]} | {argument(one, "work")}
                assert len(held) == 3 + len(FLUX_ROWS[method])
            # Every run passes the knots and its own rows of the table to both entries, beside a
            # level table that holds no scatterer.
            rows = 6//runs
            for tables in (engine.knot_tables, engine.view_tables):
                assert [begin for begin, _, _ in tables] == begins
                for begin, k, rows_of_table in tables:
                    assert np.array_equal(k, knots)
                    assert np.array_equal(rows_of_table, table[begin:begin + rows])
            assert result["radiance"].shape == (2, 160)
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, path_bytes - 1, method, scatterer_wavenumber=knots,
                     **queue_call(method, surface_end, **optics))
        # Bands and an instrument's rules are the grey call's: the view writes a block of the
        # call and the output receives its means.
        log, result = queue_of(spec, engine, None, method, scatterer_wavenumber=knots,
                               band_edges=[20., 30., 60.],
                               **queue_call(method, surface_end, **optics))
        line, = [line for line in log if line.startswith(view + "_spectral(")]
        assert argument(line, "band_start") != "None"
        assert argument(line, "radiance_mean") != argument(line, "radiance_rows")
        assert result["radiance"].shape == (2, 2)
        # The grey calls queue the grey entries, here ...
        grey_logs = {}
        for limit in (None, 3*blocks*surface.ROW_BYTES):
            log, _ = queue_of(spec, engine, limit, method,
                              **queue_call(method, surface_end, **grey))
            assert not any("_spectral(" in line for line in log)
            assert not engine.knot_tables and not engine.view_tables
            assert [line.split("(")[0] for line in log if line.startswith("path_")] == \
                [flux, view]*(1 if limit is None else 2)
            grey_logs[limit] = log
    # ... and line by line what they queue on the recorders from before, which know nothing of
    # the new entries.
    before = {"compute_thermal_radiance": trc.RadianceRecorder,
              "compute_solar_radiance": src.SolarRadianceRecorder}[method]
    with rc.recorded(tmp_path, before) as (spec, engine):
        assert not hasattr(engine, view + "_spectral")
        for limit, expect in grey_logs.items():
            spec.device_output_limit = (8 << 30) if limit is None else limit
            engine.begin()
            getattr(spec, method)(**queue_call(method, surface_end, **grey))
            log, expect = ([line for line in lines if not line.startswith("load_grid(")]
                           for lines in (list(engine.log), expect))
            assert log == expect and sum(line.startswith(view + "(") for line in log) >= 1
