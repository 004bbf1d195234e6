"""CPU-only checks of Spectroscopy.compute_thermal_radiance: the float64-vs-long-double scan of the
numpy mirror of tests/thermal_radiance_cases.py over its case tables that measures E_cpu (printed;
thermal_radiance_cases.E_CPU records it and the GPU tests take their bound from it), that the
tables reach every branch of csrc/thermal_radiance.h, the mirror against what the transfer equation
demands of it (each bound beside what was measured), the mirror without scatterers against
compute_radiance's recurrence bit for bit, the statements of the definition, the header of the
entry (include/lbl_amd_thermal_radiance.h) against its ctypes signature, the argument checks (all
raised before anything touches the GPU) and what one call queues on a stand-in engine."""
import contextlib
import ctypes
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy, paths
from pylbl_amd import engine as engine_module
from tests import abi_header, sweep_cases as cases, thermal_cases as tc
from tests import surface_cases as surface
from tests import thermal_radiance_cases as rc
from tests.abi_header import parameters_of
from tests.test_linear_source_host import make_spectroscopy

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_thermal_radiance.h").read_text()
KERNELS = (ROOT / "pylbl_amd" / "csrc" / "thermal_radiance.h").read_text()
DESIGN = (ROOT / "DESIGN.md").read_text()
F64, LD = np.float64, np.longdouble
ONES = np.ones((3, 5))


# ---------------------------------------------------------------------------------------------
# E_cpu, and the branches the tables reach.
def test_float64_mirror_stays_close_to_long_double():
    """E_cpu: the worst |float64 - long double|/scale over every case table, printed."""
    worst = 0.
    for inputs, mu, from_last in rc.all_cases():
        error, finite = rc.worst_error(inputs, mu, from_last)
        assert finite, inputs.name
        print("%-20s D=%.2f from_last=%-5s worst |difference|/scale %.3g" % (
            inputs.name, inputs.diffusivity, from_last, error))
        worst = max(worst, error)
    print("E_cpu = %.3g" % worst)
    assert worst <= rc.E_CPU <= rc.E_CPU_CAP == 1e-10 == tc.E_CPU_CAP
    assert rc.E_CPU <= 2.*worst, "thermal_radiance_cases.E_CPU no longer records the measured value"
    assert rc.FLOOR == 1e-13 == tc.FLUX_FLOOR


def test_case_tables_reach_every_branch():
    codes, signs, weights = set(), set(), set()
    for inputs, mu in rc.value_cases():
        li = inputs.layer_inputs(False)
        branch = li["branch"]
        codes |= set(np.unique(branch))
        positive, series, y = rc.decisions(li, np.asarray(mu)[None, :, None])
        general = branch == tc.GENERAL
        signs |= set(np.sign(y[general]))
        if inputs.name == "pole":
            # y = 0 exactly where beta = 0 in path 0; 1 +- 1e-9 beside it in paths 1 and 2.
            still = general[:, 0, :] & (inputs.group == 0)[None, :]
            assert np.any(still) and np.all(y[:, 0, :][still] == 0.)
            assert inputs.k*inputs.mu[0] == 1.
            assert abs(inputs.k*inputs.mu[1] - 1. - 1e-9) < 1e-15
            assert abs(inputs.k*inputs.mu[2] - 1. + 1e-9) < 1e-15
            beside = y[:, 1:, :][:, :, inputs.group == 0]
            assert np.all(beside[:, 0] < 0.) and np.all(beside[:, 1] > 0.)
        if inputs.name == "deep":
            # k*t = 1000 and 1700 under a small t/mu: E = 0, and the one-sided h is 0*inf.
            _, _, k, _ = rc.scalars(F64, li)
            kt = (k*li["t"])[general]
            assert np.any(np.abs(kt - 1000.) < 1.) and np.any(kt > 1700.)
            with np.errstate(all="ignore"):
                one_sided = np.exp(-kt)*rc.phi(F64, 1.)*(-np.expm1(-y[general])/y[general])
            assert np.any(np.isnan(one_sided)) and np.any(y[general] < -800.)
        weights |= set(np.unique(series[branch == tc.CONSERVATIVE_BRANCH]))
    # Both branches of linear_weight under the conservative branch.
    assert weights == {False, True}
    assert codes == {tc.CLEAR, tc.CONSERVATIVE_BRANCH, tc.GENERAL} and signs == {-1., 0., 1.}
    assert rc.MU == (1., 0.6, 0.05)
    assert "kThermalViewAhead = %d;" % rc.VIEW_AHEAD in KERNELS
    assert "kLinearSeriesBelow = 1./16." in (ROOT / "pylbl_amd" / "csrc" / "radiance.h").read_text()
    # Every loop of path_levels with the rows in flight of the kernel.
    a = rc.VIEW_AHEAD
    assert {1, a, a + 1, 2*a, 2*a + 1} <= set(tc.DEPTHS)


# ---------------------------------------------------------------------------------------------
# The mirror's own properties.
def gauss_panels(t, pieces=48, points=24):
    """Nodes and weights on [0, t] in long double: Gauss-Legendre on panels that halve towards
    both ends, for integrands with a boundary layer at either face."""
    x, w = np.polynomial.legendre.leggauss(points)
    x, w = x.astype(LD), w.astype(LD)
    half = [LD(0.5)**j for j in range(1, pieces)]
    cuts = sorted(set([LD(0.), LD(1.)] + half + [LD(1.) - h for h in half]))
    nodes, weights = [], []
    for lo, hi in zip(cuts, cuts[1:]):
        nodes.append((lo + hi)/2 + (hi - lo)/2*x)
        weights.append((hi - lo)/2*w)
    return np.concatenate(nodes)*LD(t), np.concatenate(weights)*LD(t)


def quadrature(t, mu, a, f_up, f_down):
    """int_0^t [f+(tau)(1 + a) + f-(tau)(1 - a)] exp(-tau/mu) dtau/mu in long double."""
    tau, weight = gauss_panels(t)
    one = LD(1.)
    integrand = (f_up(tau)*(one + a) + f_down(tau)*(one - a))*np.exp(-tau/mu)/mu
    return np.sum(integrand*weight)


def test_closed_forms_match_quadrature_of_the_source():
    """C of both cloudy branches against Gauss-Legendre quadrature of J's bracket within a level,
    in long double, relative to |u1| + |d0|: k*mu = 1 exactly and 1 +- 1e-9, k*t = 1000 with t/mu
    = 20, and random levels."""
    rng = np.random.default_rng(11)
    worst = 0.
    general = [(1.25, 0.8, 3.), (1.25, 0.8*(1. + 1e-9), 3.), (1.25, 0.8*(1. - 1e-9), 3.),
               (50., 1., 20.), (2., 0.5, 1e-3), (1.9, 1., 40.)]
    general += [(rng.uniform(0.05, 2.), rng.uniform(0.05, 1.), 10.**rng.uniform(-3., 1.5))
                for _ in range(40)]
    assert general[0][0]*general[0][1] == 1. and general[3][0]*general[3][2] == 1000.
    for k, mu, t in general:
        k, mu, t = LD(k), LD(mu), LD(t)
        gamma, a = LD(rng.uniform(0., 0.99)), LD(rng.uniform(0., 0.7))
        u1, d0 = LD(rng.uniform(-1., 1.)), LD(rng.uniform(-1., 1.))
        c, p, q, _ = rc.general_c(LD, k, gamma, t, mu, a, u1, d0)
        expect = quadrature(
            t, mu, a, lambda tau: p*np.exp(-k*(t - tau)) + gamma*q*np.exp(-k*tau),
            lambda tau: gamma*p*np.exp(-k*(t - tau)) + q*np.exp(-k*tau))
        assert np.isfinite(c)
        worst = max(worst, float(abs(c - expect)/(abs(u1) + abs(d0))))
    for _ in range(40):
        g1, mu, t = LD(rng.uniform(0.2, 2.)), LD(rng.uniform(0.05, 1.)), LD(10.**rng.uniform(-4., 2.))
        a, u1, d0 = LD(rng.uniform(0., 0.7)), LD(rng.uniform(-1., 1.)), LD(rng.uniform(-1., 1.))
        c, n = rc.conservative_c(LD, g1, t, mu, a, u1, d0)
        expect = quadrature(t, mu, a, lambda tau: u1 - g1*n*(t - tau), lambda tau: d0 + g1*n*tau)
        worst = max(worst, float(abs(c - expect)/(abs(u1) + abs(d0))))
    print("worst |C - quadrature|/(|u1| + |d0|) = %.3g" % worst)
    assert worst <= rc.QUADRATURE_BOUND


def test_the_internal_solution_reproduces_the_flux_it_did_not_use():
    """f+ at a level's space-side face, P*E + Gamma*Q (conservative: u1 - x*N), is up[i] - piB:
    the level's solution was fixed by up[i+1] and down[i] alone.  In long double on long-double
    fluxes, relative to pi*scale.  In the general branch what is left is rounding; in the
    conservative one it is what the branch itself leaves out, which its criterion k2*(1 + t*t) <=
    1e-10 bounds: the two-stream layer there is the k = 0 one."""
    worst = {tc.GENERAL: 0., tc.CONSERVATIVE_BRANCH: 0.}
    for inputs in (tc.cloud("every"), rc.pole(), tc.shape_inputs(67, 5, 9)):
        for from_last in (False, True):
            fluxes = tc.mirror(LD, inputs, from_last)
            order = inputs.order(from_last)
            li = inputs.layer_inputs(from_last)
            g1, g2, k, _ = rc.scalars(LD, li)
            size = LD(cases.FLUX_PI)*rc.scale(inputs)
            for i in range(inputs.levels_per_path):
                pib = tc.pi_planck(LD, inputs.nu[None, :], inputs.table[order[:, i], 4][:, None])
                u1 = fluxes["up"][order[:, i]] - pib
                top = fluxes["up"][order[:, i - 1]] if i > 0 else fluxes["top_up"]
                d0 = (fluxes["down"][order[:, i - 1]] if i > 0 else LD(0.)) - pib
                t = li["t"][i].astype(LD)
                _, p, q, e = rc.general_c(LD, k[i], g2[i]/(g1[i] + k[i]), t, LD(1.), LD(0.), u1, d0)
                _, n = rc.conservative_c(LD, g1[i], t, LD(1.), LD(0.), u1, d0)
                with np.errstate(all="ignore"):
                    got = np.where(li["branch"][i] == tc.GENERAL,
                                   p*e + (g2[i]/(g1[i] + k[i]))*q, u1 - (g1[i]*t)*n)
                for code in worst:
                    cloudy = (li["branch"][i] == code) & (size > 0.)
                    if np.any(cloudy):
                        error = np.abs(got - (top - pib))[cloudy]/size[cloudy]
                        worst[code] = max(worst[code], float(error.max()))
    print("worst |f+(0) - (up[i] - piB)|/(pi*scale): general %.3g, conservative %.3g" % (
        worst[tc.GENERAL], worst[tc.CONSERVATIVE_BRANCH]))
    assert 0. < worst[tc.GENERAL] <= rc.TOP_BOUND
    assert 0. < worst[tc.CONSERVATIVE_BRANCH] <= rc.TOP_BOUND_CONSERVATIVE <= tc.CONSERVATIVE


def single_column(kind, table, d, beta, nu, eps, surface_t, mu):
    """The radiance of independent columns [count] through levels [L, count, 5] in the order space
    -> surface, on thermal_cases.column's float64 fluxes."""
    fluxes, li = tc.column(F64, table, d, beta, nu, eps, surface_t)
    depth = table.shape[0]
    one, pi = kind(1.), kind(cases.FLUX_PI)
    eps = kind(eps)
    rad = eps*cases.planck(kind, nu, surface_t) + (one - eps)*(fluxes["down"][depth].astype(kind)/pi)
    for i in range(depth - 1, -1, -1):
        here = {name: (value[i] if isinstance(value, np.ndarray) and value.ndim == 2 else value)
                for name, value in li.items()}
        b = cases.planck(kind, nu, table[i, :, 4])
        down0 = fluxes["down"][i] if i > 0 else np.zeros_like(fluxes["down"][0])
        rad = rc.level(kind, here, mu, b, fluxes["up"][i + 1], down0, rad)
    return rad, li


def test_two_halves_make_the_level():
    """A level split into two halves of the same temperature leaves the radiance unchanged."""
    rng = np.random.default_rng(5)
    depth, count = 5, 300
    table = np.zeros((depth, count, 5))
    table[..., 0] = 1.
    table[..., 1] = np.minimum(10.**rng.uniform(-3., 1.5, size=(depth, count)), 20.)
    omega = np.where(rng.random((depth, count)) < 0.67,
                     rng.choice([1., 0.999999, 0.5, 0.9], size=(depth, count)), 0.)
    table[..., 2] = omega*table[..., 1]
    table[..., 3] = rng.uniform(0., 0.85, size=(depth, count))
    table[..., 4] = rng.uniform(180., 320., size=(depth, count))
    beta = 10.**rng.uniform(-4., 0., size=(depth, count))
    nu = rng.uniform(1., 3000., size=count)
    half = np.concatenate([table[:2], table[2:3], table[2:]], axis=0).copy()
    half[2:4, :, :3] = half[2:4, :, :3]/2.
    half_beta = np.concatenate([beta[:2], beta[2:3], beta[2:]], axis=0)
    scale = cases.planck(LD, nu, 320.)
    worst = 0.
    for eps in (1., 0.3):
        for mu in (1., 0.6, 0.05):
            whole, li = single_column(F64, table, 1.66, beta, nu, eps, 300., mu)
            assert {tc.CLEAR, tc.GENERAL} <= set(np.unique(li["branch"][2]))
            split, _ = single_column(F64, half, 1.66, half_beta, nu, eps, 300., mu)
            worst = max(worst, float(np.max(np.abs(whole.astype(LD) - split)/scale)))
    print("worst |whole - halves|/scale = %.3g E_cpu" % (worst/rc.E_CPU))
    assert worst <= rc.SPLIT_BOUND*rc.E_CPU


def test_every_radiance_is_finite_and_inside_its_range():
    worst = 0.
    for inputs, mu, from_last in rc.all_cases():
        got = rc.mirror(F64, inputs, mu, from_last)
        value, size = got["radiance"], got["scale"]
        assert np.all(np.isfinite(value)) and np.all(value >= 0.), inputs.name
        assert np.all(np.isfinite(got["brightness_temperature"]))
        over = (value.astype(LD) - size)[size > 0.]/size[size > 0.]
        worst = max(worst, float(np.max(over, initial=0.)))
        assert np.all(value[size == 0.] == 0.)
    print("worst (radiance - scale)/scale = %.3g E_cpu" % (worst/rc.E_CPU))
    assert worst <= rc.RANGE_BOUND*rc.E_CPU


def test_general_branch_meets_the_conservative_one():
    """Both branches at the same level differ like (1 - omega): the threshold is continuous."""
    rng = np.random.default_rng(7)
    count = 200
    tau = 10.**rng.uniform(-2., 1., size=count)
    g = rng.uniform(0., 0.85, size=count)
    nu = rng.uniform(100., 1500., size=count)
    scale = cases.planck(LD, nu, 300.)
    worst = []
    for delta in (1e-6, 1e-8):
        results = []
        for omega in (1., 1. - delta):
            table = np.stack([np.ones(count), tau, omega*tau, g, np.full(count, 260.)],
                             axis=-1)[None]
            rad, li = single_column(LD, table, 1.66, np.zeros((1, count)), nu, 0.3, 300., 0.6)
            results.append((rad, set(np.unique(li["branch"]))))
        assert results[0][1] == {tc.CONSERVATIVE_BRANCH} and results[1][1] == {tc.GENERAL}
        worst.append(float(np.max(np.abs(results[0][0] - results[1][0])/scale)))
    print("general - conservative at 1 - omega = 1e-6, 1e-8: %.3g, %.3g of scale" % tuple(worst))
    assert worst[0] <= rc.THRESHOLD_BOUND and worst[1] <= 1.1e-2*worst[0]


@pytest.mark.parametrize("from_last", [False, True])
def test_without_scatterers_it_is_compute_radiance_bit_for_bit(from_last):
    """No scatterers, eps = 1 and mu = 1: the float64 mirror has the bits of lbl_path_radiance's
    recurrence from B(T_s), swept surface -> space."""
    for depth, seed in ((1, 1), (9, 2), (17, 3)):
        problem = cases.Problem(131, depth, seed=seed)
        zeros = np.zeros(problem.levels)
        table = np.stack([problem.thickness, zeros, zeros, zeros, problem.temperature], axis=1)
        inputs = tc.Inputs("clear", problem.nu, problem.beta, table, tc.SURFACE_T, np.ones(3))
        got = rc.mirror(F64, inputs, np.ones(3), from_last)["radiance"]
        # The surface lies behind level 0 with from_last: the view sweeps towards the last level.
        start = cases.boundary_start(F64, problem.nu, inputs.surface_t, np.ones(3))
        expect, _ = cases.sweep_radiance(F64, problem.nu, problem.beta, problem.thickness,
                                         problem.temperature, depth, not from_last, start)
        last = inputs.order(from_last)[:, 0]
        assert np.array_equal(got.view(np.uint64), expect[last].view(np.uint64)), depth


# ---------------------------------------------------------------------------------------------
# The statements of the definition.
def test_header_docstring_design_and_kernel_state_the_same_formulas():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    section = DESIGN[DESIGN.index("## 27."):]
    for text in (HEADER, KERNELS, Spectroscopy.compute_thermal_radiance.__doc__, section):
        text = squeeze(text)
        for formula in rc.FORMULAS:
            assert formula in text, formula
    assert "path_levels<kThermalViewAhead, kVector>" in KERNELS
    signature = inspect.signature(Spectroscopy.compute_thermal_radiance).parameters
    assert list(signature)[1:] == [
        "layer_thickness", "surface_temperature", "view_zenith_cosine", "surface_emissivity",
        "emissivity_wavenumber", "surface", "diffusivity", "scatterer_optical_depth",
        "scatterer_single_scattering_albedo", "scatterer_asymmetry", "quantities", "band_edges",
        "instrument", "remove_pedestal", "range_policy"]
    assert signature["view_zenith_cosine"].default == 1.
    assert signature["diffusivity"].default == 1.66 == paths.DIFFUSIVITY
    assert signature["quantities"].default == ("radiance",)
    # The existing kernels are as they were: the new header only includes them.
    assert '#include "twostream_thermal.h"' in KERNELS


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_thermal_radiance.h against abi.THERMAL_RADIANCE_PROTOTYPES, whole.
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
    assert list(declared) == list(abi.THERMAL_RADIANCE_PROTOTYPES) == ["lbl_path_thermal_radiance"]
    sweep = declared["lbl_path_thermal_radiance"]
    # The block, the grid handle and the run, as lbl_path_flux takes them.
    assert sweep[:9] == parameters_of("lbl_path_flux")[:9]
    assert sweep[9:] == [
        "const double *level_table", "double diffusivity", "const double *view_cosine",
        "const double *surface_temperature", "const double *emissivity_rows",
        "const double *emissivity", "const double *up_rows", "const double *down_rows",
        "int32_t n_bands", "const int64_t *band_start", "double *radiance_rows",
        "double *brightness_rows", "double *radiance_mean", "int32_t flags"]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    for name, parameters in declared.items():
        argtypes = abi.THERMAL_RADIANCE_PROTOTYPES[name]
        assert len(argtypes) == len(parameters), name
        for argtype, parameter in zip(argtypes, parameters):
            abi_header.check_parameter(argtype, parameter, addresses=True)
        function = getattr(lib, name)
        assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
        for table in (abi.PROTOTYPES, abi.TWO_STREAM_PROTOTYPES, abi.THERMAL_PROTOTYPES,
                      abi.THERMAL_SOURCE_PROTOTYPES, abi.KDIST_PROTOTYPES,
                      abi.SCATTERER_PROTOTYPES, abi.RESULT_TYPES):
            assert name not in table
    # lbl_amd.h is as it was: the new header includes it and declares nothing of its own twice.
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    assert callable(engine_module.Engine.path_thermal_radiance)


# ---------------------------------------------------------------------------------------------
# The requests.
KNOTS = np.array([590., 600., 610.])
CLOUD = dict(scatterer_optical_depth=ONES, scatterer_single_scattering_albedo=0.9*ONES,
             scatterer_asymmetry=0.8*ONES)
BAD = [
    (dict(layer_thickness=np.ones((3, 4))), "shape"),
    (dict(layer_thickness=-ONES), "finite and >= 0"),
    (dict(surface_temperature=0.), "finite and > 0"),
    (dict(surface_temperature=np.full(5, 288.)), "shape"),
    (dict(view_zenith_cosine=0.), r"view_zenith_cosine must lie in \(0, 1\]"),
    (dict(view_zenith_cosine=1.01), "view_zenith_cosine"),
    (dict(view_zenith_cosine=[0.5, np.nan, 1.]), "view_zenith_cosine"),
    (dict(view_zenith_cosine=[0.5, -0.5, 1.]), "view_zenith_cosine"),
    (dict(view_zenith_cosine=np.ones(4)), "shape"),
    (dict(surface_emissivity=1.2), r"\[0, 1\]"),
    (dict(surface_emissivity=[0.1, 0.2], emissivity_wavenumber=KNOTS), "shape"),
    (dict(surface_emissivity=[0.1, 0.2, 0.3], emissivity_wavenumber=[3., 2., 1.]),
     "emissivity_wavenumber must be finite and strictly ascending"),
    (dict(surface="top"), "surface must be"),
    (dict(diffusivity=0.9), r"diffusivity must be one number in \[1, 2\]"),
    (dict(diffusivity=np.nan), "diffusivity"),
    (dict(scatterer_optical_depth=ONES), "together or not at all"),
    (dict(CLOUD, scatterer_optical_depth=-ONES), ">= 0"),
    (dict(CLOUD, scatterer_single_scattering_albedo=1.01*ONES), r"\[0, 1\]"),
    (dict(CLOUD, scatterer_asymmetry=ONES), r"\[0, 1\)"),
    (dict(quantities="upward_flux"), "quantities must be"),
    (dict(quantities=()), "quantities must be"),
    (dict(quantities=("radiance", "brightness_temperature"), band_edges=[600., 600.5]),
     "brightness_temperature is only available on the grid"),
    (dict(range_policy="other"), "range_policy"),
    (dict(band_edges=[600.5, 600.2]), "strictly increasing"),
    (dict(instrument="iasi"), "instrument must be an Instrument"),
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
        spec.compute_thermal_radiance(**call)


def test_bands_and_instrument_exclude_each_other_and_group_is_not_offered(monkeypatch):
    untouchable(monkeypatch)
    from pylbl_amd.instrument import Instrument
    spec = make_spectroscopy((3, 5))
    instrument = Instrument.gaussian(np.array([600.2, 600.4]), 0.1)
    with pytest.raises(ValueError, match="band_edges or instrument, not both"):
        spec.compute_thermal_radiance(ONES, 288., band_edges=[600., 600.5], instrument=instrument)
    spec.group = object()
    with pytest.raises(NotImplementedError):
        spec.compute_thermal_radiance(ONES, 288.)


def test_requests_hold_what_the_sweep_needs():
    spec = make_spectroscopy((3, 5))
    thickness = np.arange(1., 16.).reshape(3, 5)
    tau_c = np.linspace(0., 3., 15).reshape(3, 5)
    omega_c, g_c = np.full((3, 5), 0.7), np.linspace(0., 0.85, 15).reshape(3, 5)
    request = spec._thermal_radiance_request(
        thickness, [288., 270., 300.], [1., 0.5, 0.05], [1., 0.5, 0.], None, "last", 2., tau_c,
        omega_c, g_c, ("brightness_temperature", "radiance"), None, None, "reference")
    assert request.quantities == ("radiance", "brightness_temperature")
    assert request.surface == "last" and request.instrument is None and request.starts is None
    flux = spec._thermal_flux_request(
        thickness, [288., 270., 300.], [1., 0.5, 0.], None, "last", 2., tau_c, omega_c, g_c,
        ("upward_flux", "downward_flux"), None, "reference")
    assert np.array_equal(request.level_table, flux.level_table)
    assert request.diffusivity == 2. and np.array_equal(request.mu, [1., 0.5, 0.05])
    assert np.array_equal(request.surface_temperature, [288., 270., 300.])
    assert np.array_equal(request.surface_emissivity, [1., 0.5, 0.])
    assert request.edge_temperature is None and request.scatterer_knots is None
    request = spec._thermal_radiance_request(
        thickness, 288., 0.6, [[0.1, 0.2, 0.3]]*3, KNOTS, "first", 1.66, None, None, None,
        "radiance", [600., 600.5], None, "skip")
    assert np.array_equal(request.emissivity_knots, KNOTS) and request.starts is not None
    assert np.array_equal(request.mu, [0.6]*3) and np.all(request.level_table[:, 1:4] == 0.)


# ---------------------------------------------------------------------------------------------
# The queue.
@contextlib.contextmanager
def recorded(directory):
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = rc.RadianceRecorder
    try:
        with surface.recorded(directory) as pair:
            yield pair
    finally:
        surface.SurfaceRecorder = before


def argument(line, name):
    return re.search(r"\b%s=([^,)]+)" % name, line).group(1)


def queue_of(spec, engine, limit_rows, **keywords):
    spec.device_output_limit = (8 << 30) if limit_rows is None else limit_rows*surface.ROW_BYTES
    engine.begin()
    result = spec.compute_thermal_radiance(**keywords)
    return list(engine.log), result


@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_one_call_computes_beta_once_per_run_of_whole_paths(tmp_path, monkeypatch, surface_end):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    both = ("radiance", "brightness_temperature")
    with recorded(tmp_path) as (spec, engine):
        # 5 blocks per level: 15 rows a path of three levels.
        for limit, runs in ((None, 1), (30, 1), (29, 2), (15, 2)):
            log, result = queue_of(
                spec, engine, limit, layer_thickness=thickness, surface_temperature=[288., 270.],
                view_zenith_cosine=[1., 0.4], surface=surface_end,
                surface_emissivity=[[0.2, 0.4], [0.1, 0.3]], emissivity_wavenumber=[10., 70.],
                diffusivity=2., quantities=both)
            # Two lines gases: two compute calls per run, each level in exactly one run.
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            names = [line.split("(")[0] for line in log if line.startswith(
                ("surface_emissivity", "path_thermal"))]
            assert names == ["surface_emissivity"] + \
                ["path_thermal_two_stream", "path_thermal_radiance"]*runs
            fluxes = [line for line in log if line.startswith("path_thermal_two_stream(")]
            views = [line for line in log if line.startswith("path_thermal_radiance(")]
            from_last = surface_end == "first"
            begins = [int(argument(line, "level_begin")) for line in views]
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            assert all(begin % 3 == 0 for begin in begins)
            for flux, view in zip(fluxes, views):
                for name in ("beta", "level_begin", "up_rows", "down_rows", "from_last",
                             "diffusivity", "emissivity_rows", "emissivity", "asynchronous"):
                    assert argument(flux, name) == argument(view, name), name
                assert argument(view, "from_last") == str(from_last)
                assert argument(view, "asynchronous") == "True"
                assert "top_up_rows" not in flux and "up_mean" not in flux
                blocks = {argument(view, name) for name in
                          ("beta", "up_rows", "down_rows", "radiance_rows", "brightness_rows")}
                blocks.add(argument(flux, "work"))
                assert len(blocks) == 6 and argument(view, "band_start") == "None"
            for q in both:
                assert result[q].shape == (2, 160)
        # One path does not fit.
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, 14, layer_thickness=thickness, surface_temperature=288.)
        # Bands: the sweep writes a block of the call, the output receives its means.
        log, result = queue_of(spec, engine, None, layer_thickness=thickness,
                               surface_temperature=288., surface=surface_end,
                               surface_emissivity=0.3, band_edges=[20., 30., 60.])
        view, = [line for line in log if line.startswith("path_thermal_radiance(")]
        assert argument(view, "band_start") != "None" and "emissivity_rows=None" in view
        assert argument(view, "radiance_mean") != argument(view, "radiance_rows")
        assert "brightness_rows" not in view
        assert not any(line.startswith("surface_emissivity") for line in log)
        assert result["radiance"].shape == (2, 2)
        assert np.array_equal(result["band_points"], [40, 120])


def test_existing_calls_do_not_reach_the_new_entry(tmp_path):
    with recorded(tmp_path) as (spec, engine):
        engine.begin()
        spec.compute_thermal_flux(np.ones(surface.SHAPE), 288.)
        spec.compute_radiance(np.ones(surface.SHAPE), boundary_temperature=288.)
        assert any(line.startswith("path_thermal_two_stream") for line in engine.log)
        assert not any(line.startswith("path_thermal_radiance") for line in engine.log)
