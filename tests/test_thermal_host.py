"""CPU-only checks of Spectroscopy.compute_thermal_flux: that the case tables of
tests/thermal_cases.py reach every branch of csrc/twostream_thermal.h they are named for, the
float64-vs-long-double scan of the numpy mirror over those tables that measures E_cpu (printed;
thermal_cases.E_CPU records it and the GPU tests take their bound from it), the mirror against what
two-stream theory demands of it, the mirror without scatterers against the plain recurrence of
compute_flux with one angle, the header of the entry (include/lbl_amd_thermal.h) against its
ctypes signature, the argument checks (all raised before anything touches the GPU) and what one
call queues on a stand-in engine."""
import ctypes
import inspect
import json
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths
from pylbl_amd import engine as engine_module
from tests import abi_header, sweep_cases as cases, thermal_cases as tc
from tests import surface_cases as surface
from tests.abi_header import parameters_of
from tests.test_linear_source_host import make_spectroscopy

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_thermal.h").read_text()
KERNELS = (ROOT / "pylbl_amd" / "csrc" / "twostream_thermal.h").read_text()
DESIGN = (ROOT / "DESIGN.md").read_text()
F64, LD = np.float64, np.longdouble
ONES = np.ones((3, 5))


# ---------------------------------------------------------------------------------------------
# The case tables reach the branches they are named for.
def test_case_tables_reach_every_branch():
    for place in tc.CLOUD_PLACES:
        inputs = tc.cloud(place)
        for from_last in (False, True):
            li = inputs.layer_inputs(from_last)
            branch, group = li["branch"], inputs.group
            order = inputs.order(from_last).T
            cloudy = inputs.cloudy[order]                       # [L, PATHS]
            assert np.all((branch == tc.CLEAR) == ~cloudy[:, :, None])
            # Where the clouds are.
            where = {"first": [0], "last": [8], "every": list(range(9))}[place]
            if from_last and place != "every":
                where = [8 - where[0]]
            assert [i for i in range(9) if cloudy[i].all()] == where
            # omega_c = 1 over beta = 0: k2 = 0 exactly, the conservative branch.
            pure = (inputs.omega_c[order] == 1.)[:, :, None] & (group == 0)[None, None, :]
            assert np.any(pure) and np.all(li["k2"][pure] == 0.) and np.all(li["w"][pure] == 1.)
            assert np.all(branch[pure] == tc.CONSERVATIVE_BRANCH)
            # Both sides of k2*(1 + t*t) = 1e-10, within a factor 30 of it.
            near = (inputs.omega_c[order] == 1.)[:, :, None] & (group == 1)[None, None, :]
            criterion = (li["k2"]*(1. + li["t"]*li["t"]))[near]
            assert np.any((criterion > tc.CONSERVATIVE/30.) & (criterion <= tc.CONSERVATIVE))
            assert np.any((criterion > tc.CONSERVATIVE) & (criterion < 30.*tc.CONSERVATIVE))
            assert {tc.CONSERVATIVE_BRANCH, tc.GENERAL} <= set(np.unique(branch[near]))
            # omega_c = 0.5 and 0.999999 take the general branch.
            assert set(np.unique(inputs.omega_c[inputs.cloudy])) <= {1., 0.5, 0.999999}
            assert np.all(branch[(inputs.omega_c[order] == 0.5)] == tc.GENERAL)
            # tau = 3000 in clear levels; x = 0 in clear levels without beta and tau_c.
            if place != "every":
                assert np.all(branch[:, :, group == 2][8 - where[0]] == tc.CLEAR)
                assert np.any(li["tau"][branch == tc.CLEAR] >= 3000.*(1. - 1e-15))
                identity = (branch == tc.CLEAR) & (li["tau"] == 0.)
                assert np.any(identity) and np.all(identity[:, :, group != 0] == 0)
        assert set(inputs.table[inputs.cloudy, 3]) == {0., 0.85} or place != "every"
        assert inputs.table[:, 4].min() == 180. and inputs.table[:, 4].max() == 320.
        assert inputs.nu[0] == 1. and inputs.nu[-1] == 3000.
    # E = 0: exp(-(k*t)) underflows under tau_c = 3000 in the general branch.
    every = tc.cloud("every")
    li = every.layer_inputs(False)
    general = li["branch"] == tc.GENERAL
    with np.errstate(under="ignore"):
        e = np.exp(-(np.sqrt(li["k2"][general])*li["t"][general]))
    assert np.any(e == 0.) and np.any(every.table[:, 1] == 3000.)
    assert set(every.table[:, 3]) == {0., 0.85}
    assert {x.diffusivity for x in tc.value_cases()} == {1., 1.66, 2.}

    # The shapes: every loop of path_levels for both kernels, both orders, lanes of 1 and 2, and
    # both uniform branches inside a batch and inside the remainder loop.
    classes = {cases.depth_class(n, tc.UP_AHEAD) for n in tc.DEPTHS}
    assert classes == {"below", "one batch", "batch and remainder", "batches",
                       "batches and remainder"}
    a, b = tc.UP_AHEAD, tc.DOWN_AHEAD
    assert set(tc.DEPTHS) == {1, a, a + 1, 2*a, 2*a + 1, b, b + 1, 2*b, 2*b + 1}
    assert "kThermalUpAhead = kPathAhead" in KERNELS and tc.UP_AHEAD == cases.PATH_AHEAD
    assert "kThermalDownAhead = %d;" % tc.DOWN_AHEAD in KERNELS
    assert "kThermalConservative = 1e-10" in KERNELS and tc.CONSERVATIVE == 1e-10
    for depth in tc.DEPTHS:
        shape = tc.shape_inputs(513, depth, 40 + depth)
        cloudy = shape.cloudy.reshape(cases.PATHS, depth)
        assert np.all(cloudy[:, 1:] != cloudy[:, :-1])
        if depth >= 2*a + 1:
            assert cloudy[:, :a].any() and (~cloudy[:, :a]).any()
            assert cloudy[:, 2*a:].any() and (~cloudy[:, 2*a:]).any()
    codes = np.unique(tc.shape_inputs(513, 9, 49).layer_inputs(True)["branch"])
    assert set(codes) == {tc.CLEAR, tc.CONSERVATIVE_BRANCH, tc.GENERAL}
    vector = {cases.layout_is_vector(name, columns)
              for name in cases.LAYOUTS for columns in cases.LAYOUT_COLUMNS}
    assert vector == {True, False}
    assert {w for columns in cases.LAYOUT_COLUMNS for w in cases.lane_widths(columns)} == {1, 2}
    assert set(tc.EMISSIVITY) == {1., 0.3, 0.} and len(set(tc.SURFACE_T)) == 3


def test_float64_mirror_stays_close_to_long_double():
    """E_cpu: the worst |float64 - long double|/scale over every case table, printed."""
    worst = 0.
    for inputs, from_last in tc.all_cases():
        error, finite = tc.worst_error(inputs, from_last)
        assert finite, inputs.name
        print("%-20s D=%.2f from_last=%-5s worst |difference|/scale %.3g" % (
            inputs.name, inputs.diffusivity, from_last, error))
        worst = max(worst, error)
    print("E_cpu = %.3g" % worst)
    assert worst <= tc.E_CPU <= tc.E_CPU_CAP == 1e-10
    assert tc.E_CPU <= 2.*worst, "thermal_cases.E_CPU no longer records the measured value"
    assert tc.FLUX_FLOOR == 1e-13


# ---------------------------------------------------------------------------------------------
# The mirror's own properties, in float64, with bounds in units of E_CPU*scale.
def test_every_flux_is_finite_and_inside_its_range():
    worst = 0.
    for inputs, from_last in tc.all_cases():
        got = tc.mirror(F64, inputs, from_last)
        scale = got["scale"]
        for name in tc.NAMES:
            size = scale if name.startswith("top_") else tc.per_level(inputs, scale)
            value = got[name]
            assert np.all(np.isfinite(value)) and np.all(value >= 0.), (inputs.name, name)
            over = (value.astype(LD) - size)[size > 0.]/size[size > 0.]
            worst = max(worst, float(np.max(over, initial=0.)))
            assert np.all(value[size == 0.] == 0.)
        assert np.all(got["top_down"] == 0.)
    print("worst (flux - scale)/scale = %.3g E_cpu" % (worst/tc.E_CPU))
    assert worst <= tc.RANGE_BOUND*tc.E_CPU


def clouds_below(rng, depth, count):
    """Random levels [depth, count, 5] at 250 K, two thirds of them clouds, over beta = 0."""
    tau_c = 10.**rng.uniform(-3., 1.5, size=(depth, count))
    omega_c = np.where(rng.random((depth, count)) < 0.67,
                       rng.choice([1., 0.999999, 0.5, 0.9], size=(depth, count)), 0.)
    g_c = rng.uniform(0., 0.85, size=(depth, count))
    return np.stack([np.ones_like(tau_c), tau_c, omega_c*tau_c, g_c, np.full_like(tau_c, 250.)],
                    axis=-1)


def test_an_isothermal_cavity_under_an_opaque_lid_is_black():
    """All levels and the surface at one temperature under a clear lid of tau = 3000: up = down =
    piB at every interface below the lid, whatever clouds lie between and whatever eps is."""
    rng = np.random.default_rng(3)
    depth, count = 8, 200
    table = clouds_below(rng, depth, count)
    table[0, :, 1:4] = (3000., 0., 0.)
    nu = rng.uniform(1., 3000., size=count)
    worst = 0.
    for d in (1.66, 2.):
        for eps in (1., 0.3, 0.):
            got, inputs = tc.column(F64, table, d, np.zeros((depth, count)), nu, eps, 250.)
            assert np.all(inputs["branch"][0] == tc.CLEAR) and np.any(inputs["branch"] != tc.CLEAR)
            black = tc.pi_planck(LD, nu, 250.)
            for q in tc.QUANTITIES:
                error = np.abs(got[q][1:].astype(LD) - black)/black
                worst = max(worst, float(error.max()))
    print("worst |flux - piB|/piB under the lid = %.3g E_cpu" % (worst/tc.E_CPU))
    assert worst <= tc.LID_BOUND*tc.E_CPU


def test_two_halves_make_the_layer():
    """A level split into two halves of the same temperature leaves the fluxes at the outer
    interfaces unchanged: the solution of a homogeneous layer with its source is a semigroup in
    its depth."""
    rng = np.random.default_rng(5)
    depth, count = 5, 300
    table = clouds_below(rng, depth, count)
    table[..., 4] = rng.uniform(180., 320., size=(depth, count))
    table[..., 1:3] = np.minimum(table[..., 1:3], 20.)
    beta = 10.**rng.uniform(-4., 0., size=(depth, count))
    nu = rng.uniform(1., 3000., size=count)
    half = np.concatenate([table[:2], table[2:3], table[2:]], axis=0).copy()
    half[2:4, :, :3] = half[2:4, :, :3]/2.
    half_beta = np.concatenate([beta[:2], beta[2:3], beta[2:]], axis=0)
    worst = 0.
    for eps in (1., 0.3):
        whole, inputs = tc.column(F64, table, 1.66, beta, nu, eps, 300.)
        assert {tc.CLEAR, tc.GENERAL} <= set(np.unique(inputs["branch"][2]))
        split, _ = tc.column(F64, half, 1.66, half_beta, nu, eps, 300.)
        scale = tc.pi_planck(LD, nu, 320.)
        for q in tc.QUANTITIES:
            for i, j in ((0, 0), (2, 2), (3, 4), (5, 6)):
                error = np.abs(whole[q][i].astype(LD) - split[q][j])/scale
                worst = max(worst, float(error.max()))
    print("worst |whole - halves|/scale = %.3g E_cpu" % (worst/tc.E_CPU))
    assert worst <= tc.SPLIT_BOUND*tc.E_CPU


def test_general_branch_tends_to_the_conservative_one():
    """Both branches at the same layer differ like (1 - omega): the threshold is continuous."""
    rng = np.random.default_rng(7)
    count = 200
    tau = 10.**rng.uniform(-2., 1., size=count)
    g = rng.uniform(0., 0.85, size=count)
    nu = rng.uniform(100., 1500., size=count)
    worst = []
    for delta in (1e-6, 1e-8):
        results = []
        for omega in (1., 1. - delta):
            table = np.stack([np.ones(count), tau, omega*tau, g, np.full(count, 260.)],
                             axis=-1)[None]
            got, inputs = tc.column(LD, table, 1.66, np.zeros((1, count)), nu, 0.3, 300.)
            results.append((got, set(np.unique(inputs["branch"]))))
        assert results[0][1] == {tc.CONSERVATIVE_BRANCH} and results[1][1] == {tc.GENERAL}
        scale = tc.pi_planck(LD, nu, 300.)
        worst.append(max(float(np.max(np.abs(results[0][0][q] - results[1][0][q])/scale))
                         for q in tc.QUANTITIES))
    print("general - conservative at 1 - omega = 1e-6, 1e-8: %.3g, %.3g of scale" % tuple(worst))
    assert worst[0] <= 1e-3 and worst[1] <= 1.1e-2*worst[0]


def test_a_conservative_cloud_keeps_the_net_flux():
    """omega_c = 1 over beta = 0 absorbs and emits nothing: up - down is the same above and below
    the cloud."""
    rng = np.random.default_rng(9)
    depth, count = 5, 300
    table = clouds_below(rng, depth, count)
    table[..., 4] = rng.uniform(180., 320., size=(depth, count))
    tau_c = 10.**rng.uniform(-2., 1.5, size=count)
    table[2, :, 1], table[2, :, 2] = tau_c, tau_c
    beta = 10.**rng.uniform(-4., 0., size=(depth, count))
    beta[2] = 0.
    nu = rng.uniform(1., 3000., size=count)
    worst = 0.
    for eps in (1., 0.3, 0.):
        got, inputs = tc.column(F64, table, 1.66, beta, nu, eps, 300.)
        assert np.all(inputs["branch"][2] == tc.CONSERVATIVE_BRANCH)
        assert np.all(inputs["k2"][2] == 0.)
        net = got["up"].astype(LD) - got["down"]
        scale = tc.pi_planck(LD, nu, 320.)
        worst = max(worst, float(np.max(np.abs(net[2] - net[3])/scale)))
    print("worst |net above - net below|/scale = %.3g E_cpu" % (worst/tc.E_CPU))
    assert worst <= tc.NET_BOUND*tc.E_CPU


# ---------------------------------------------------------------------------------------------
# Without scatterers: compute_flux's recurrence with the one angle mu = 1/D, w = 1.
def plain_fluxes(kind, inputs, from_last):
    """{"up", "down", "top_up"} of the recurrence of lbl_path_flux (tests/sweep_cases.py) with
    one angle mu = 1/D and weight 1, laid out as mirror() lays them out."""
    n = inputs.levels_per_path
    mu = np.array([1./inputs.diffusivity])
    weight = np.array([1.])
    lengths = inputs.table[:, :1]/mu
    temperature = inputs.table[:, 4]
    down = cases.sweep_flux(kind, inputs.nu, inputs.beta, lengths, weight, temperature, n,
                            from_last)
    start, _ = cases.surface_start(kind, inputs.nu, inputs.surface_t, inputs.emissivity,
                                   down.total, down.total_mag)
    up = cases.sweep_flux(kind, inputs.nu, inputs.beta, lengths, weight, temperature, n,
                          not from_last, start)
    order = inputs.order(from_last)                             # [PATHS, L], space -> surface
    at_surface = kind(cases.FLUX_PI)*start
    below = np.zeros_like(up.flux)
    # The up sweep's flux after a level is at the interface above it: below the level before.
    below[order[:, :-1]] = up.flux[order[:, 1:]]
    below[order[:, -1]] = at_surface
    return {"down": down.flux, "up": below, "top_up": up.flux[order[:, 0]]}


@pytest.mark.parametrize("d", [1.66, 2.])
@pytest.mark.parametrize("from_last", [False, True])
def test_without_scatterers_it_is_the_flux_recurrence_with_one_angle(d, from_last):
    """Within 16*2^-53*(L + 1)*scale: x = D*(s*beta) and (s/mu)*beta differ by at most 4 ulp (mu
    = 1/D, the quotient, the two products), so exp(-x) by under 1.5*2^-53 absolute; about six more
    roundings where pi enters (pi*B*em against pi*(... + B*em)); at most 8*2^-53 per level and
    sweep, two sweeps."""
    worst = 0.
    for depth, seed in ((1, 1), (9, 2), (17, 3)):
        problem = cases.Problem(131, depth, seed=seed)
        zeros = np.zeros(problem.levels)
        table = np.stack([problem.thickness, zeros, zeros, zeros, problem.temperature], axis=1)
        inputs = tc.Inputs("clear", problem.nu, problem.beta, table, tc.SURFACE_T, tc.EMISSIVITY, d)
        got = tc.mirror(F64, inputs, from_last)
        expect = plain_fluxes(F64, inputs, from_last)
        bound = LD(16.*2.**-53*(depth + 1))
        for name, value in expect.items():
            scale = got["scale"] if name == "top_up" else tc.per_level(inputs, got["scale"])
            error = np.abs(got[name].astype(LD) - value.astype(LD))
            lit = scale > 0.
            worst = max(worst, float(np.max(error[lit]/(bound*scale[lit]))))
            assert np.all(error <= bound*scale), (depth, name)
    print("D = %g, from_last = %s: worst error / bound %.3g" % (d, from_last, worst))


# ---------------------------------------------------------------------------------------------
# The statements of the definition.
def test_header_docstring_design_and_kernel_state_the_same_formulas():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    section = DESIGN[DESIGN.index("## 23."):]
    for text in (HEADER, KERNELS, Spectroscopy.compute_thermal_flux.__doc__, section):
        text = squeeze(text)
        for formula in tc.FORMULAS:
            assert formula in text, formula
    # The layer is written once and both kernels call it; the clear branch is uniform.
    assert KERNELS.count("ThermalLayer thermal_layer(") == KERNELS.count(" thermal_layer(") == 1
    assert KERNELS.count("= thermal_layer<kLinear>(") == KERNELS.count("thermal_layer<") == 1
    assert KERNELS.count("faces.through(") == 2
    assert "kAhead = kLinear ? kThermalSourceUpAhead : kThermalUpAhead;" in KERNELS
    assert "path_levels<kAhead, kVector>" in KERNELS
    assert "path_levels<kThermalDownAhead, kVector>" in KERNELS
    assert "kThermalLevelWords = 5" in KERNELS
    signature = inspect.signature(Spectroscopy.compute_thermal_flux).parameters
    assert list(signature)[1:] == [
        "layer_thickness", "surface_temperature", "surface_emissivity", "emissivity_wavenumber",
        "surface", "diffusivity", "scatterer_optical_depth",
        "scatterer_single_scattering_albedo", "scatterer_asymmetry", "quantities", "band_edges",
        "remove_pedestal", "range_policy"]
    assert signature["diffusivity"].default == 1.66 == tc.DIFFUSIVITY == paths.DIFFUSIVITY
    assert signature["surface_emissivity"].default == 1. and signature["surface"].default == "first"
    assert signature["quantities"].default == ("upward_flux", "downward_flux")


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_thermal.h against abi.THERMAL_PROTOTYPES, whole, as
# tests/test_abi_host.py compares lbl_amd.h with abi.PROTOTYPES.
def declarations():
    """{function: [parameter, ...]} of the header, in its order, by abi_header's own pattern."""
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    found = {}
    for result, name, inside in re.findall(
            r"^(int|const char \*|void \*)\s*(lbl_\w+)\s*\(([^)]*)\)\s*;", code, re.M):
        assert result == "int" and name not in found, name
        found[name] = [re.sub(r"\s+", " ", p).strip() for p in inside.split(",")]
    assert set(re.findall(r"\b(lbl_\w+)\s*\(", code)) == set(found)
    return found


def test_header_declares_the_entry_and_ctypes_match():
    from pylbl_amd import abi
    declared = declarations()
    assert list(declared) == list(abi.THERMAL_PROTOTYPES) == ["lbl_path_thermal_two_stream"]
    sweep = declared["lbl_path_thermal_two_stream"]
    # The block, the grid handle and the run, as lbl_path_flux takes them.
    assert sweep[:9] == parameters_of("lbl_path_flux")[:9]
    assert sweep[:4] + sweep[5:9] == parameters_of("lbl_path_compute")[:8]
    outputs = ["double *%s" % name for name in engine_module.PATH_THERMAL_OUTPUTS]
    assert abi.PATH_THERMAL_OUTPUTS == (
        "up_rows", "down_rows", "top_up_rows", "top_down_rows", "up_mean", "down_mean",
        "top_up_mean", "top_down_mean")
    assert sweep[9:] == [
        "const double *level_table", "double diffusivity", "const double *surface_temperature",
        "const double *emissivity_rows", "const double *emissivity", "int32_t n_bands",
        "const int64_t *band_start", "double *work"] + outputs + ["int32_t flags"]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    for name, parameters in declared.items():
        argtypes = abi.THERMAL_PROTOTYPES[name]
        assert len(argtypes) == len(parameters), name
        for argtype, parameter in zip(argtypes, parameters):
            abi_header.check_parameter(argtype, parameter, addresses=True)
        function = getattr(lib, name)
        assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
        assert name not in abi.PROTOTYPES and name not in abi.TWO_STREAM_PROTOTYPES
        assert name not in abi.RESULT_TYPES
    # lbl_amd.h is as it was: the new header includes it and declares nothing of its own twice.
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    assert callable(engine_module.Engine.path_thermal_two_stream)


# ---------------------------------------------------------------------------------------------
# The requests.
KNOTS = np.array([590., 600., 610.])
CLOUD = dict(scatterer_optical_depth=ONES, scatterer_single_scattering_albedo=0.9*ONES,
             scatterer_asymmetry=0.8*ONES)
BAD = [
    (dict(layer_thickness=np.ones((3, 4))), "shape"),
    (dict(layer_thickness=-ONES), "finite and >= 0"),
    (dict(surface_temperature=0.), "finite and > 0"),
    (dict(surface_temperature=[288., np.nan, 288.]), "finite and > 0"),
    (dict(surface_temperature=np.full(5, 288.)), "shape"),
    (dict(surface_emissivity=1.2), r"\[0, 1\]"),
    (dict(surface_emissivity=[0.1, np.nan, 0.3]), r"\[0, 1\]"),
    (dict(surface_emissivity=np.ones(4)), "shape"),
    (dict(surface_emissivity=[0.1, 0.2], emissivity_wavenumber=KNOTS), "shape"),
    (dict(surface_emissivity=[0.1, 0.2, 1.3], emissivity_wavenumber=KNOTS), r"\[0, 1\]"),
    (dict(surface_emissivity=[0.1, 0.2, 0.3], emissivity_wavenumber=[3., 2., 1.]),
     "emissivity_wavenumber must be finite and strictly ascending"),
    (dict(surface="top"), "surface must be"),
    (dict(diffusivity=0.9), r"diffusivity must be one number in \[1, 2\]"),
    (dict(diffusivity=2.1), "diffusivity"),
    (dict(diffusivity=np.nan), "diffusivity"),
    (dict(diffusivity=[1.66, 1.66]), "diffusivity"),
    (dict(scatterer_optical_depth=ONES), "together or not at all"),
    (dict(scatterer_asymmetry=ONES*0.5, scatterer_optical_depth=ONES), "together or not at all"),
    (dict(CLOUD, scatterer_optical_depth=np.ones((3, 4))), "shape"),
    (dict(CLOUD, scatterer_optical_depth=-ONES), ">= 0"),
    (dict(CLOUD, scatterer_optical_depth=ONES*np.inf), "finite"),
    (dict(CLOUD, scatterer_single_scattering_albedo=1.01*ONES), r"\[0, 1\]"),
    (dict(CLOUD, scatterer_single_scattering_albedo=ONES*np.nan), "finite"),
    (dict(CLOUD, scatterer_asymmetry=ONES), r"\[0, 1\)"),
    (dict(CLOUD, scatterer_asymmetry=-0.1*ONES), r"\[0, 1\)"),
    (dict(quantities="direct_irradiance"), "quantities must be"),
    (dict(quantities=()), "quantities must be"),
    (dict(range_policy="other"), "range_policy"),
    (dict(band_edges=[600.5, 600.2]), "strictly increasing"),
]


def untouchable(monkeypatch):
    def touched(*arguments, **more):
        raise AssertionError("the GPU side was reached")
    monkeypatch.setattr(Spectroscopy, "_sweep_runs", touched)
    monkeypatch.setattr(engine_module, "default_engine", lambda device=0: surface.Untouchable())


@pytest.mark.parametrize("keywords, match", BAD)
def test_bad_arguments_are_refused_before_the_gpu(monkeypatch, keywords, match):
    untouchable(monkeypatch)
    spec = make_spectroscopy((3, 5))
    call = dict(layer_thickness=ONES, surface_temperature=288.)
    call.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_thermal_flux(**call)


def test_temperatures_and_heating_need_a_physical_atmosphere(monkeypatch):
    untouchable(monkeypatch)
    spec = make_spectroscopy((3, 5))
    spec.atmosphere.pressure = spec.atmosphere.pressure.copy()
    spec.atmosphere.pressure[1, 2] = 0.
    with pytest.raises(ValueError, match="heating rates need pressures"):
        spec.compute_thermal_flux(ONES, 288., quantities="heating_rate")
    spec.atmosphere.temperature = spec.atmosphere.temperature.copy()
    spec.atmosphere.temperature[0, 0] = 0.
    with pytest.raises(ValueError, match="temperatures"):
        spec.compute_thermal_flux(ONES, 288.)


def test_group_instrument_and_linear_source_are_not_offered():
    spec = make_spectroscopy((3, 5))
    spec.group = object()
    with pytest.raises(NotImplementedError):
        spec.compute_thermal_flux(ONES, 288.)
    offered = inspect.signature(Spectroscopy.compute_thermal_flux).parameters
    assert not {"instrument", "source", "interface_temperature", "angles", "group"} & set(offered)


def test_requests_hold_what_the_sweep_needs():
    spec = make_spectroscopy((3, 5))
    thickness = np.arange(1., 16.).reshape(3, 5)
    tau_c = np.linspace(0., 3., 15).reshape(3, 5)
    omega_c, g_c = np.full((3, 5), 0.7), np.linspace(0., 0.85, 15).reshape(3, 5)
    request = spec._thermal_flux_request(
        thickness, [288., 270., 300.], [1., 0.5, 0.], None, "last", 2., tau_c, omega_c, g_c,
        ("heating_rate", "upward_flux"), None, "reference")
    assert request.quantities == ("upward_flux", "heating_rate") and request.surface == "last"
    table = request.level_table
    assert table.shape == (15, 5) and table.flags.c_contiguous
    assert np.array_equal(table[:, 0], thickness.ravel())
    assert np.array_equal(table[:, 1], tau_c.ravel())
    assert np.array_equal(table[:, 2], (omega_c*tau_c).ravel())
    assert np.array_equal(table[:, 3], g_c.ravel())
    assert np.array_equal(table[:, 4], spec.atmosphere.temperature.ravel())
    assert request.diffusivity == 2. and request.emissivity_knots is None
    assert np.array_equal(request.surface_temperature, [288., 270., 300.])
    assert np.array_equal(request.surface_emissivity, [1., 0.5, 0.])
    request = spec._thermal_flux_request(
        thickness, 288., [[0.1, 0.2, 0.3]]*3, KNOTS, "first", 1.66, None, None, None,
        "downward_flux", [600., 600.5], "skip")
    assert np.array_equal(request.emissivity_knots, KNOTS)
    assert request.surface_emissivity.shape == (3, 3) and request.starts is not None
    assert np.all(request.level_table[:, 1:4] == 0.)
    assert np.array_equal(request.surface_temperature, [288.]*3)
    from pylbl_amd import spectroscopy
    assert paths.THERMAL_FLUX_QUANTITIES == spectroscopy.FLUX_QUANTITIES


# ---------------------------------------------------------------------------------------------
# The queue.
def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


def queue_of(spec, engine, limit_rows, **keywords):
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*surface.ROW_BYTES
    engine.begin()
    result = spec.compute_thermal_flux(**keywords)
    return list(engine.log), result


@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_one_call_computes_beta_once_per_run_of_whole_paths(tmp_path, monkeypatch, surface_end):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    quantities = paths.THERMAL_FLUX_QUANTITIES
    with tc.recorded(tmp_path) as (spec, engine):
        # 3 blocks per level and one per flux on the grid: 5 rows a level, 15 a path of three
        # levels.
        for limit, runs in ((None, 1), (30, 1), (29, 2), (15, 2)):
            log, result = queue_of(
                spec, engine, limit, layer_thickness=thickness, surface_temperature=[288., 270.],
                surface=surface_end, surface_emissivity=[[0.2, 0.4], [0.1, 0.3]],
                emissivity_wavenumber=[10., 70.], diffusivity=2., quantities=quantities)
            # Two lines gases: two compute calls per run, each level in exactly one run.
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            sweeps = [line for line in log if line.startswith("path_thermal_two_stream(")]
            assert len(sweeps) == runs
            begins = [int(argument(line, "level_begin")) for line in sweeps]
            from_last = surface_end == "first"
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            assert all(begin % 3 == 0 for begin in begins)
            assert {argument(line, "from_last") for line in sweeps} == {str(from_last)}
            assert {argument(line, "diffusivity") for line in sweeps} == {"2.0"}
            # The emissivity rows are filled once, before the first sweep.
            names = [line.split("(")[0] for line in log if line.startswith(
                ("surface_emissivity", "path_thermal_two_stream"))]
            assert names == ["surface_emissivity"] + ["path_thermal_two_stream"]*runs
            rows = next(line for line in log if line.startswith("surface_emissivity"))
            assert {argument(line, "emissivity_rows") for line in sweeps} == \
                {argument(rows, "rows")}
            assert {argument(line, "emissivity") for line in sweeps} == {"None"}
            for line in sweeps:
                blocks = {argument(line, name) for name in
                          ("beta", "work", "up_rows", "down_rows", "top_up_rows", "top_down_rows")}
                assert len(blocks) == 6 and "up_mean" not in line
            for q in ("upward_flux", "downward_flux"):
                assert result[q].shape == (2, 4, 160)
            assert result["heating_rate"].shape == (2, 3, 160)
        # One path does not fit: refused like compute_solar_flux.
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, 14, layer_thickness=thickness, surface_temperature=288.,
                     quantities=quantities)
        # Bands: the sweeps write blocks of the call, the outputs receive their means; a scalar
        # emissivity makes no rows.
        log, result = queue_of(spec, engine, None, layer_thickness=thickness,
                               surface_temperature=288., surface=surface_end,
                               surface_emissivity=0.3, band_edges=[20., 30., 60.],
                               quantities="upward_flux")
        sweep, = [line for line in log if line.startswith("path_thermal_two_stream(")]
        assert argument(sweep, "band_start") != "None" and "emissivity_rows=None" in sweep
        assert not any(line.startswith("surface_emissivity") for line in log)
        assert argument(sweep, "up_mean") != argument(sweep, "up_rows")
        assert "top_up_mean" in sweep and "down_rows" not in sweep
        assert result["upward_flux"].shape == (2, 4, 2)
        assert np.array_equal(result["band_points"], [40, 120])


def test_existing_calls_queue_what_they_queued(tmp_path):
    """compute_radiance's recorded queues are unchanged, and neither it nor compute_solar_flux
    reaches the new entry."""
    golden = json.loads((ROOT / "tests" / "golden" / "radiance_default_queue.json").read_text())
    got = surface.default_queues(tmp_path)
    assert set(golden) == set(got)
    for name, log in golden.items():
        assert got[name] == log, name
    with tc.recorded(tmp_path) as (spec, engine):
        engine.begin()
        spec.compute_solar_flux(np.ones(surface.SHAPE), 0.5)
        spec.compute_radiance(np.ones(surface.SHAPE), boundary_temperature=288.)
        assert any(line.startswith("path_two_stream") for line in engine.log)
        assert not any(line.startswith("path_thermal_two_stream") for line in engine.log)
