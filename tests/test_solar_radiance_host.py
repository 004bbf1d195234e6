"""CPU-only checks of Spectroscopy.compute_solar_radiance: the float64-vs-long-double scan of the
numpy mirror of tests/solar_radiance_cases.py over its case tables that measures E_cpu (printed;
solar_radiance_cases.E_CPU records it and the GPU tests take their bound from it), that the tables
reach every branch of csrc/solar_radiance.h, the mirror against what the transfer equation and the
two-stream equations demand of it (each bound beside what was measured), the statements of the
definition, the header of the entry (include/lbl_amd_solar_radiance.h) against its ctypes
signature, the argument checks (all raised before anything touches the GPU) and what one call
queues on a stand-in engine."""
import contextlib
import ctypes
import inspect
from pathlib import Path
import re

import numpy as np
import pytest

from pylbl_amd import Spectroscopy
from pylbl_amd import engine as engine_module
from tests import abi_header, sweep_cases as cases, two_stream_cases as ts
from tests import solar_radiance_cases as sc
from tests import surface_cases as surface
from tests import thermal_radiance_cases as rc
from tests import two_stream_ode_cases as ode
from tests.abi_header import parameters_of
from tests.test_linear_source_host import make_spectroscopy
from tests.test_thermal_radiance_host import gauss_panels

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd_solar_radiance.h").read_text()
KERNELS = (ROOT / "pylbl_amd" / "csrc" / "solar_radiance.h").read_text()
DESIGN = (ROOT / "DESIGN.md").read_text()
F64, LD = np.float64, np.longdouble
ONES = np.ones((3, 5))
GRID_POINTS = 100            # make_spectroscopy's grid
PI = LD(cases.FLUX_PI)


# ---------------------------------------------------------------------------------------------
# E_cpu, and the branches the tables reach.
def test_float64_mirror_stays_close_to_long_double():
    """E_cpu: the worst |float64 - long double|/scale over every case table, printed."""
    worst = 0.
    for inputs, mu, phi, from_last in sc.all_cases():
        cos_theta = sc.scattering_cosine(mu, inputs.mu0, phi)
        error, finite = sc.worst_error(inputs, mu, cos_theta, from_last)
        assert finite, inputs.name
        print("%-20s from_last=%-5s worst |difference|/scale %.3g" % (
            inputs.name, from_last, error))
        worst = max(worst, error)
    print("E_cpu = %.3g" % worst)
    assert worst <= sc.E_CPU <= sc.E_CPU_CAP == 1e-10 == ts.E_CPU_CAP
    assert sc.E_CPU <= 2.*worst, "solar_radiance_cases.E_CPU no longer records the measured value"
    assert sc.FLOOR == 1e-13 == ts.FLUX_FLOOR


def test_case_tables_reach_every_branch():
    codes, signs, weights = set(), set(), set()
    for inputs, mu, _ in sc.value_cases():
        li = sc.problem_inputs(inputs, False)
        branch = li["branch"]
        codes |= set(np.unique(branch))
        mu = np.asarray(mu)[None, :, None]
        positive, series = sc.decisions(li, mu)
        k = sc.scalars(F64, li)["k"]
        with np.errstate(all="ignore"):
            y = ((1. - k*mu)*li["t"])/mu
        general = (branch == ts.GENERAL) | (branch == ts.GUARDED)
        signs |= set(np.sign(y[general]))
        if inputs.name == "pole":
            still = general[:, 0, :] & (inputs.group == 0)[None, :]
            assert np.any(still) and np.all(y[:, 0, :][still] == 0.)
            assert inputs.k*inputs.mu[0] == 1.
            assert abs(inputs.k*inputs.mu[1] - 1. - 1e-9) < 1e-15
            assert abs(inputs.k*inputs.mu[2] - 1. + 1e-9) < 1e-15
        if inputs.name == "deep":
            kt = (k*li["t"])[general]
            assert np.any(np.abs(kt - 1000.) < 5.) and np.any(kt > 1700.)
        if inputs.name == "conservative cloud":
            assert set(np.unique(branch)) == {ts.CONSERVATIVE_BRANCH}
        weights |= set(np.unique(series[branch == ts.CONSERVATIVE_BRANCH]))
    assert weights == {False, True}
    assert codes == {ts.IDENTITY, ts.CONSERVATIVE_BRANCH, ts.GENERAL, ts.GUARDED,
                     sc.NO_SCATTERING}
    assert signs == {-1., 0., 1.}
    assert sc.MU == (1., 0.6, 0.05) and sc.MU0 == (1., 0.5, 0.1) and sc.PHI == (0., 90., 180.)
    pairs = {(m, m0) for mu, _ in sc.views() for m, m0 in zip(mu, sc.MU0)}
    assert len(pairs) == 9
    assert "kSolarViewAhead = %d;" % sc.VIEW_AHEAD in KERNELS
    # One row in flight: every depth takes the same loop of path_levels; the flux entry that
    # makes the rows on the GPU keeps kPathAhead in flight.
    assert {1, sc.VIEW_AHEAD + 1, ts.UP_AHEAD + 1} <= set(sc.DEPTHS)


# ---------------------------------------------------------------------------------------------
# Single levels [count] with fluxes of any size at their faces.
def random_levels(seed=31):
    """(table [count, 5], mu0, beta, sigma, mu, phi, names): levels one by one -- the pole k*mu = 1
    exactly and 1 +- 1e-9, k*t = 1000, conservative clouds thin and thick, Rayleigh levels,
    levels inside the guard, and random ones."""
    rng = np.random.default_rng(seed)
    rows, mu0, beta, sigma, mu = [], [], [], [], []

    def add(row, sun, b, s, view):
        rows.append(row), mu0.append(sun), beta.append(b), sigma.append(s), mu.append(view)
    # The pole: omega_c = 0.5, g_c = 0.25 without gas has one k for every tau_c.
    li = sc.view_inputs(np.array([1., 0., 2., 1., 0.25]), 0.7, 0., 0.)
    k = float(sc.scalars(F64, li)["k"])
    exact = rc.exact_reciprocal(k)
    assert exact is not None and k*exact == 1.
    for tau_c in (0.05, 2., 24.):
        for view in (exact, exact*(1. + 1e-9), exact*(1. - 1e-9)):
            add([1., 0., tau_c, 0.5*tau_c, 0.125*tau_c], 0.7, 0., 0., view)
    # k*t = 1000 under t/mu = 506 and 10120.
    for view in (1., 0.05):
        add([1., 0., 508., 10.16, 0.], 0.5, 0., 0., view)
    # Conservative clouds and Rayleigh levels.
    for tau_c in (1e-7, 1e-3, 0.4, 30.):
        add([1., 0., tau_c, tau_c, 0.8*tau_c], 0.3, 0., 0., 0.6)
        add([1., tau_c, 0., 0., 0.], 0.9, 0., 1., 0.05)
    # Inside the guard: two_stream_cases.resonance()'s levels.
    for d in ts.RESONANCE_D:
        k2 = ((1. + d)/0.8)**2
        u = (-3. + np.sqrt(9. + 4.*k2))/2.
        add([1., 0., 1., 1., 0.], 0.8, u/(1. - u), 0., 0.6)
    for _ in range(60):
        tau_c = 10.**rng.uniform(-3., 1.5)
        omega_c, g_c = rng.choice([1., rng.uniform(0., 1.)]), rng.uniform(0., 0.9)
        add([1., 10.**rng.uniform(-3., 0.5), tau_c, omega_c*tau_c, omega_c*tau_c*g_c],
            rng.uniform(0.05, 1.), 10.**rng.uniform(-4., 0.5), rng.choice([0., 1.]),
            rng.uniform(0.05, 1.))
    count = len(rows)
    return (np.array(rows), np.array(mu0), np.array(beta), np.array(sigma), np.array(mu),
            rng.uniform(0., 360., size=count), rng)


def test_closed_form_matches_quadrature_of_the_source():
    """The level's closed form against Gauss-Legendre quadrature of J(tau') exp(-tau'/mu)/mu on
    panels halving towards both faces, in long double, relative to (S_i + |up[i+1]| +
    |diffuse[i]|)/pi: both branches, the pole, k*t = 1000 and the guard."""
    table, mu0, beta, sigma, mu, phi, rng = random_levels()
    count = mu.size
    li = sc.view_inputs(table, mu0, beta, sigma)
    assert {ts.CONSERVATIVE_BRANCH, ts.GENERAL, ts.GUARDED} <= set(np.unique(li["branch"]))
    cos_theta = sc.scattering_cosine(mu, mu0, phi)
    up1, direct0, diffuse0 = (rng.uniform(0., 1., size=count) for _ in range(3))
    closed = sc.level(LD, li, mu, cos_theta, up1, direct0, diffuse0, np.zeros(count, dtype=LD))
    v = sc.solution(LD, li, up1, direct0, diffuse0)
    nodes, weights = gauss_panels(1.)
    t = li["t"].astype(LD)
    depth = nodes[:, None]*t[None, :]
    with np.errstate(all="ignore"):
        j = sc.source(LD, li, v, mu, cos_theta, depth)
        mu_ld = mu.astype(LD)
        expect = np.sum(j*np.exp(-depth/mu_ld)/mu_ld*(weights[:, None]*t[None, :]), axis=0)
    assert np.all(np.isfinite(closed)) and np.all(np.isfinite(expect))
    size = (direct0 + up1 + diffuse0).astype(LD)/PI
    error = np.abs(closed - expect)/size
    print("worst |closed form - quadrature|/scale = %.3g (level %d)" % (
        float(error.max()), int(np.argmax(error))))
    assert float(error.max()) <= sc.QUADRATURE_BOUND


def element_classes(li):
    branch = li["branch"]
    return {"general": branch == ts.GENERAL, "conservative": branch == ts.CONSERVATIVE_BRANCH,
            "guarded": branch == ts.GUARDED}


def guard_bound(li):
    """The header's 0.12*(1e-4 - |1 - k*mu0|), of F0, per element."""
    return sc.GUARD_SLOPE*(ts.RESONANCE - np.abs(1. - li["x"]))


def test_the_internal_solution_reproduces_the_fluxes_it_did_not_use():
    """F+(0) is up[i] and F-(t) is diffuse[i+1]: the level's solution was fixed by up[i+1],
    diffuse[i] and direct[i] alone, so this checks Z+-.  In long double on long-double fluxes,
    relative to F0: rounding in the general branch, the criterion in the conservative one, the
    header's bound inside the guard."""
    worst = dict.fromkeys(("general", "conservative", "guarded"), 0.)
    tables = [sc.under_sun(ts.cloud(), sc.MU0), sc.under_sun(ts.rayleigh_only(), sc.MU0),
              ts.resonance(), sc.conservative_cloud(), sc.pole(),
              sc.under_sun(ts.shape_inputs(67, 5, 9), sc.MU0)]
    for inputs in tables:
        for from_last in (False, True):
            fluxes = ts.mirror(LD, inputs, from_last)
            order = inputs.sun_order(from_last)
            li = sc.problem_inputs(inputs, from_last)
            f0 = inputs.f0().astype(LD)
            lit = f0 > 0.
            for i in range(inputs.levels_per_path):
                here = {name: value[i] for name, value in li.items()}
                direct0 = fluxes["direct"][order[:, i - 1]] if i > 0 else f0
                diffuse0 = fluxes["diffuse"][order[:, i - 1]] if i > 0 else np.zeros_like(f0)
                top = fluxes["up"][order[:, i - 1]] if i > 0 else fluxes["top_up"]
                v = sc.solution(LD, here, 0., 0., 0.)
                # solution() reads float64 rows; here the rows are long double: the same lines.
                with np.errstate(all="ignore"):
                    ws = v["w"]*direct0
                    v["zp"] = (ws*(v["g3"] - v["a2"]*v["m"]))/v["x"]
                    v["zm"] = -((ws*(v["g4"] + v["a1"]*v["m"]))/v["x"])
                    v["u1"] = fluxes["up"][order[:, i]] - v["zp"]*v["dm"]
                    v["d0"] = diffuse0 - v["zm"]
                    ge = v["gamma"]*v["e"]
                    v["p"] = (v["u1"] - ge*v["d0"])/(LD(1.) - ge*ge)
                    v["q"] = (v["d0"] - ge*v["u1"])/(LD(1.) - ge*ge)
                    v["n"] = (v["u1"] - v["d0"])/(LD(1.) + v["g1"]*v["t"])
                    plus, _ = sc.fields(LD, here, v, LD(0.))
                    _, minus = sc.fields(LD, here, v, v["t"])
                    error = np.maximum(np.abs(plus - top),
                                       np.abs(minus - fluxes["diffuse"][order[:, i]]))
                for name, where in element_classes(here).items():
                    where = where & lit
                    if not np.any(where):
                        continue
                    relative = (error/np.where(lit, f0, 1.))[where]
                    if name == "guarded":
                        assert np.all(relative <= guard_bound(here)[where] + sc.TOP_BOUND)
                    worst[name] = max(worst[name], float(relative.max()))
    print("worst |F+(0) - up[i]|, |F-(t) - diffuse[i+1]| of F0: general %.3g, conservative %.3g, "
          "guarded %.3g" % (worst["general"], worst["conservative"], worst["guarded"]))
    assert 0. < worst["general"] <= sc.TOP_BOUND
    assert 0. < worst["conservative"] <= sc.TOP_BOUND_CONSERVATIVE <= ts.CONSERVATIVE
    assert 0. < worst["guarded"]


def test_closed_form_fluxes_match_the_equations_inside_a_layer():
    """F+-(tau') at a few tau' inside one layer over a Lambertian surface, from
    two_stream_ode_cases' solver (the layer cut in two at tau', the interface between them) against
    the closed forms fed the solver's own fluxes at the layer's faces.  Of F0 = 1."""
    table, mu0, beta, sigma, _, _, rng = random_levels(seed=32)
    count = mu0.size
    li = sc.view_inputs(table, mu0, beta, sigma)
    albedo = rng.uniform(0., 1., size=count)
    worst = dict.fromkeys(("general", "conservative", "guarded"), 0.)
    for fraction in (0.25, 0.5, 0.9):
        t = li["t"]
        upper = fraction*t
        halves = []
        for part in (upper, t - upper):
            halves.append({"t": part, "w": li["w"], "gp": li["gp"], "mu0": li["mu0"],
                           "tau": li["tau"]})
        stacked = {name: np.stack([h[name] for h in halves]) for name in halves[0]}
        reference = ode.solar_column(ode.solar_layer(stacked), albedo, np.ones(count))
        v = sc.solution(LD, li, 0., 0., 0.)
        v["zp"] = (v["w"]*(v["g3"] - v["a2"]*v["m"]))/v["x"]
        v["zm"] = -((v["w"]*(v["g4"] + v["a1"]*v["m"]))/v["x"])
        v["u1"] = reference["up"][2] - v["zp"]*v["dm"]
        v["d0"] = -v["zm"]
        ge = v["gamma"]*v["e"]
        v["p"] = (v["u1"] - ge*v["d0"])/(LD(1.) - ge*ge)
        v["q"] = (v["d0"] - ge*v["u1"])/(LD(1.) - ge*ge)
        v["n"] = (v["u1"] - v["d0"])/(LD(1.) + v["g1"]*v["t"])
        with np.errstate(all="ignore"):
            plus, minus = sc.fields(LD, li, v, upper.astype(LD))
        error = np.maximum(np.abs(plus - reference["up"][1]),
                           np.abs(minus - reference["diffuse"][1]))
        for name, where in element_classes(li).items():
            assert np.any(where), name
            if name == "guarded":
                assert np.all(error[where] <= guard_bound(li)[where] + sc.ODE_BOUND)
            worst[name] = max(worst[name], float(error[where].max()))
    print("worst |closed form - equations| inside a layer, of F0: general %.3g, conservative "
          "%.3g, guarded %.3g" % (worst["general"], worst["conservative"], worst["guarded"]))
    assert 0. < worst["general"] <= sc.ODE_BOUND
    assert 0. < worst["conservative"] <= sc.ODE_BOUND_CONSERVATIVE <= ts.CONSERVATIVE
    assert 0. < worst["guarded"] <= ode.GUARD_ERROR


def random_columns(rng, depth, count):
    table = np.zeros((depth, count, 5))
    table[..., 0] = 1.
    table[..., 1] = np.where(rng.random((depth, count)) < 0.5,
                             10.**rng.uniform(-3., 0.3, size=(depth, count)), 0.)
    table[..., 2] = np.minimum(10.**rng.uniform(-3., 1.5, size=(depth, count)), 20.)
    omega = np.where(rng.random((depth, count)) < 0.67,
                     rng.choice([1., 0.999999, 0.5, 0.9], size=(depth, count)), 0.)
    table[..., 3] = omega*table[..., 2]
    table[..., 4] = table[..., 3]*rng.uniform(0., 0.85, size=(depth, count))
    beta = np.where(rng.random((depth, count)) < 0.8,
                    10.**rng.uniform(-4., 0., size=(depth, count)), 0.)
    return table, beta


def test_two_halves_make_the_level():
    """A level split into two halves leaves the radiance unchanged."""
    rng = np.random.default_rng(5)
    depth, count = 5, 300
    table, beta = random_columns(rng, depth, count)
    sigma = rng.choice([0., 1.], size=count)
    half = np.concatenate([table[:2], table[2:3], table[2:]], axis=0).copy()
    half[2:4] = half[2:4]/2.
    half_beta = np.concatenate([beta[:2], beta[2:3], beta[2:]], axis=0)
    f0 = np.ones(count)
    worst = 0.
    for albedo in (0., 0.3):
        for mu, mu0, phi in zip(sc.MU, sc.MU0, sc.PHI):
            cos_theta = sc.scattering_cosine(mu, mu0, phi)
            whole, peak, li = sc.single_column(LD, table, mu0, beta, sigma, albedo, f0, mu,
                                               cos_theta)
            assert {ts.CONSERVATIVE_BRANCH, ts.GENERAL} <= set(np.unique(li["branch"][2]))
            split, _, _ = sc.single_column(LD, half, mu0, half_beta, sigma, albedo, f0, mu,
                                           cos_theta)
            size = np.maximum(peak, f0.astype(LD)/PI)
            worst = max(worst, float(np.max(np.abs(whole - split)/size)))
    print("worst |whole - halves|/scale = %.3g" % worst)
    assert worst <= sc.SPLIT_BOUND


def test_every_radiance_is_finite_and_not_negative():
    for inputs, mu, phi, from_last in sc.all_cases():
        cos_theta = sc.scattering_cosine(mu, inputs.mu0, phi)
        for kind in (F64, LD):
            got = sc.mirror(kind, inputs, mu, cos_theta, from_last)
            assert np.all(np.isfinite(got["radiance"])), inputs.name
            assert np.all(got["radiance"] >= 0.), inputs.name
            assert np.all(got["radiance"][inputs.f0() == 0.] == 0.)


def test_without_scattering_only_the_reflected_beam_remains():
    """No Rayleigh row and no scatterer: I = (A*F0/pi)*exp(-sum tau/mu0)*exp(-sum tau/mu), to a few
    roundings per level of A*F0/pi."""
    worst = 0.
    for depth, seed in ((1, 1), (9, 2), (17, 3)):
        problem = cases.Problem(131, depth, seed=seed)
        zeros = np.zeros(problem.levels)
        table = np.stack([problem.thickness, zeros, zeros, zeros, zeros], axis=1)
        inputs = ts.Inputs("clear", problem.beta, table, sc.MU0, np.linspace(0.2, 1., 131),
                           np.zeros(131), (1., 0.3, 0.05))
        for from_last in (False, True):
            mu = np.array(sc.MU)
            got = sc.mirror(F64, inputs, mu, sc.scattering_cosine(mu, inputs.mu0, sc.PHI),
                            from_last)["radiance"]
            tau = (table[:, 0, None].astype(LD)*problem.beta.astype(LD)).reshape(
                cases.PATHS, depth, -1).sum(axis=1)
            size = inputs.albedo[:, None].astype(LD)*inputs.f0().astype(LD)/PI
            expect = size*np.exp(-tau/inputs.mu0[:, None].astype(LD)) * \
                np.exp(-tau/mu[:, None].astype(LD))
            error = float(np.max(np.abs(got.astype(LD) - expect)/size))
            worst = max(worst, error/(depth*2.**-53))
    print("worst error without scattering: %.3g roundings per level" % worst)
    assert worst <= sc.NO_SCATTERING_ROUNDINGS


def test_a_thin_rayleigh_level_scatters_once():
    """One thin Rayleigh level over a black surface: I -> (omega*PR/(4 pi mu))*(F0/mu0)*t as t ->
    0, the definition's Pmix/(4 pi) against the irradiance F0/mu0 across the beam; what is left is
    of the order t*(1/mu + 1/mu0)."""
    for mu, mu0, phi in ((1., 0.5, 0.), (0.6, 1., 90.), (0.3, 0.4, 180.)):
        cos_theta = sc.scattering_cosine(mu, mu0, phi)
        pr = 0.75*(1. + float(cos_theta)**2)
        previous = None
        for t in (1e-2, 1e-4, 1e-6, 1e-8):
            for omega in (1., 0.5):
                table = np.array([[[1., t*omega, 0., 0., 0.]]])
                beta = np.array([[t*(1. - omega)]])
                got, _, _ = sc.single_column(LD, table, mu0, beta, np.ones(1), 0., np.ones(1), mu,
                                             cos_theta)
                expect = (omega*pr/(4.*np.pi*mu))*(1./mu0)*t
                ratio = float(got[0])/expect
                assert abs(ratio - 1.) <= 2.*t*(1./mu + 1./mu0), (mu, mu0, t, omega, ratio)
            if previous is not None:
                assert abs(ratio - 1.) < previous
            previous = abs(ratio - 1.)


def test_general_branch_meets_the_conservative_one():
    """Both branches at the same level differ like (1 - omega): the threshold is continuous."""
    rng = np.random.default_rng(7)
    count = 200
    tau = 10.**rng.uniform(-2., 1., size=count)
    g = rng.uniform(0., 0.85, size=count)
    worst = []
    for delta in (1e-6, 1e-8):
        results = []
        for omega in (1., 1. - delta):
            table = np.stack([np.ones(count), np.zeros(count), tau, omega*tau, (omega*tau)*g],
                             axis=-1)[None]
            rad, peak, li = sc.single_column(LD, table, 0.5, np.zeros((1, count)),
                                             np.zeros(count), 0.3, np.ones(count), 0.6,
                                             sc.scattering_cosine(0.6, 0.5, 90.))
            results.append((rad, set(np.unique(li["branch"])), np.maximum(peak, 1./PI)))
        assert results[0][1] == {ts.CONSERVATIVE_BRANCH} and results[1][1] == {ts.GENERAL}
        worst.append(float(np.max(np.abs(results[0][0] - results[1][0])/results[0][2])))
    print("general - conservative at 1 - omega = 1e-6, 1e-8: %.3g, %.3g of scale" % tuple(worst))
    assert worst[0] <= sc.THRESHOLD_BOUND and worst[1] <= 1.1e-2*worst[0]


def test_azimuth_and_its_mirror_image_agree_bit_for_bit():
    rng = np.random.default_rng(3)
    mu, mu0 = rng.uniform(0.01, 1., size=500), rng.uniform(0.01, 1., size=500)
    phi = rng.uniform(-720., 720., size=500)
    phi[:4] = (0., 90., 180., 360.)
    one, other = sc.scattering_cosine(mu, mu0, phi), sc.scattering_cosine(mu, mu0, -phi)
    assert np.array_equal(one.view(np.uint64), other.view(np.uint64))
    assert np.all(np.abs(one) <= 1.)
    assert sc.scattering_cosine(1., 1., 77.) == -1.
    assert abs(sc.scattering_cosine(0.5, 0.5, 180.) + 1.) < 4e-16
    assert abs(sc.scattering_cosine(0.5, 0.5, 0.) - 0.5) < 4e-16
    spec = make_spectroscopy((3, 5))
    requests = [spec._solar_radiance_request(
        ONES, [1., 0.5, 0.1], [0.3, 0.6, 1.], sign*np.array([10., 90., 135.]), None, None, 1.,
        "first", 0.2, None, True, None, None, None, None, "radiance", None, None, "reference")
        for sign in (1., -1.)]
    assert np.array_equal(requests[0].cos_theta.view(np.uint64),
                          requests[1].cos_theta.view(np.uint64))
    assert np.array_equal(requests[0].cos_theta, sc.scattering_cosine(
        [0.3, 0.6, 1.], [1., 0.5, 0.1], [10., 90., 135.]))


# ---------------------------------------------------------------------------------------------
# The statements of the definition.
def test_header_docstring_design_and_kernel_state_the_same_formulas():
    def squeeze(text):
        return re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)", "\n", text))
    section = DESIGN[DESIGN.index("## 29."):]
    for text in (HEADER, KERNELS, Spectroscopy.compute_solar_radiance.__doc__, section):
        text = squeeze(text)
        for formula in sc.FORMULAS:
            assert re.sub(r"\s+", " ", formula) in text, formula
        assert "uses m for the beam" in text or "moved cosine m for the beam" in text
    assert "path_levels<kSolarViewAhead, kVector>" in KERNELS
    signature = inspect.signature(Spectroscopy.compute_solar_radiance).parameters
    assert list(signature)[1:] == [
        "layer_thickness", "solar_zenith_cosine", "view_zenith_cosine", "relative_azimuth",
        "solar_irradiance", "solar_wavenumber", "distance_factor", "surface", "surface_albedo",
        "albedo_wavenumber", "rayleigh", "rayleigh_cross_section", "scatterer_optical_depth",
        "scatterer_single_scattering_albedo", "scatterer_asymmetry", "quantities", "band_edges",
        "instrument", "remove_pedestal", "range_policy"]
    assert signature["view_zenith_cosine"].default == 1.
    assert signature["relative_azimuth"].default == 180.
    assert signature["quantities"].default == ("radiance",)
    flux = inspect.signature(Spectroscopy.compute_solar_flux).parameters
    for name in flux:
        if name not in ("self", "quantities"):
            assert signature[name].default == flux[name].default, name
    # The existing kernels are as they were: the new header only includes them.
    assert '#include "twostream.h"' in KERNELS and "two_stream_layer(" not in KERNELS
    readme = (ROOT / "README.md").read_text()
    assert "Against a multi-stream code, radiances are good to several per cent; the single " \
           "scattering is exact." in re.sub(r"\s+", " ", readme)


# ---------------------------------------------------------------------------------------------
# The C ABI: include/lbl_amd_solar_radiance.h against abi.SOLAR_RADIANCE_PROTOTYPES, whole.
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
    assert list(declared) == list(abi.SOLAR_RADIANCE_PROTOTYPES) == ["lbl_path_solar_radiance"]
    sweep = declared["lbl_path_solar_radiance"]
    two_stream = (ROOT / "include" / "lbl_amd_twostream.h").read_text()
    inside = re.search(r"int lbl_path_two_stream\(([^)]*)\)", two_stream).group(1)
    flux = [re.sub(r"\s+", " ", p).strip() for p in inside.split(",")]
    # The block, the run and the level table, as lbl_path_two_stream takes them.
    assert sweep[:10] == flux[:10]
    assert sweep[10:] == [
        "const double *view_cosine", "const double *scattering_cosine", "const double *solar_row",
        "const double *rayleigh_row", "const double *albedo_rows", "const double *albedo",
        "const double *up_rows", "const double *direct_rows", "const double *diffuse_rows",
        "int32_t n_bands", "const int64_t *band_start", "double *radiance_rows",
        "double *radiance_mean", "int32_t flags"]
    assert sweep[12:16] == flux[10:14] and sweep[19:21] == flux[14:16]
    import __graft_entry__
    __graft_entry__.build()
    lib = abi.library()
    for name, parameters in declared.items():
        argtypes = abi.SOLAR_RADIANCE_PROTOTYPES[name]
        assert len(argtypes) == len(parameters), name
        for argtype, parameter in zip(argtypes, parameters):
            abi_header.check_parameter(argtype, parameter, addresses=True)
        function = getattr(lib, name)
        assert list(function.argtypes) == list(argtypes) and function.restype is ctypes.c_int32
        for table in (abi.PROTOTYPES, abi.TWO_STREAM_PROTOTYPES, abi.THERMAL_PROTOTYPES,
                      abi.THERMAL_SOURCE_PROTOTYPES, abi.KDIST_PROTOTYPES,
                      abi.SCATTERER_PROTOTYPES, abi.THERMAL_RADIANCE_PROTOTYPES,
                      abi.RESULT_TYPES):
            assert name not in table
    # lbl_amd.h is as it was: the new header includes it and declares nothing of its own twice.
    assert '#include "lbl_amd.h"' in HEADER
    assert not set(declared) & set(abi_header.DECLARATIONS)
    assert parameters_of("lbl_path_compute")[:4] == sweep[:4]
    assert callable(engine_module.Engine.path_solar_radiance)


# ---------------------------------------------------------------------------------------------
# The requests.
KNOTS = np.array([590., 600., 610.])
CLOUD = dict(scatterer_optical_depth=ONES, scatterer_single_scattering_albedo=0.9*ONES,
             scatterer_asymmetry=0.8*ONES)
BAD = [
    (dict(layer_thickness=np.ones((3, 4))), "shape"),
    (dict(layer_thickness=-ONES), "finite and >= 0"),
    (dict(solar_zenith_cosine=0.), r"solar_zenith_cosine must lie in \(0, 1\]"),
    (dict(solar_zenith_cosine=[1., np.nan, 1.]), r"\(0, 1\]"),
    (dict(solar_zenith_cosine=np.ones(5)), "shape"),
    (dict(view_zenith_cosine=0.), r"view_zenith_cosine must lie in \(0, 1\]"),
    (dict(view_zenith_cosine=1.01), "view_zenith_cosine"),
    (dict(view_zenith_cosine=[0.5, np.nan, 1.]), "view_zenith_cosine"),
    (dict(view_zenith_cosine=[0.5, -0.5, 1.]), "view_zenith_cosine"),
    (dict(view_zenith_cosine=np.ones(4)), "shape"),
    (dict(relative_azimuth=np.inf), "relative_azimuth must be finite"),
    (dict(relative_azimuth=[0., np.nan, 10.]), "relative_azimuth must be finite"),
    (dict(relative_azimuth=np.zeros(4)), "shape"),
    (dict(distance_factor=0.), "distance_factor"),
    (dict(solar_wavenumber=KNOTS), "needs solar_irradiance"),
    (dict(solar_irradiance=-np.ones(GRID_POINTS)), "finite and >= 0"),
    (dict(surface="top"), "surface must be"),
    (dict(surface_albedo=1.2), r"\[0, 1\]"),
    (dict(surface_albedo=[0.1, 0.2], albedo_wavenumber=KNOTS), "shape"),
    (dict(surface_albedo=[0.1, 0.2, 0.3], albedo_wavenumber=[3., 2., 1.]),
     "albedo_wavenumber must be finite and strictly ascending"),
    (dict(rayleigh="yes"), "rayleigh must be"),
    (dict(rayleigh_cross_section=np.ones(GRID_POINTS - 1)), "one value per grid point"),
    (dict(rayleigh_cross_section=-np.ones(GRID_POINTS)), "finite and >= 0"),
    (dict(rayleigh=False, rayleigh_cross_section=np.ones(GRID_POINTS)), "only used with"),
    (dict(scatterer_optical_depth=ONES), "together or not at all"),
    (dict(CLOUD, scatterer_optical_depth=-ONES), ">= 0"),
    (dict(CLOUD, scatterer_single_scattering_albedo=1.01*ONES), r"\[0, 1\]"),
    (dict(CLOUD, scatterer_asymmetry=ONES), r"\[0, 1\)"),
    (dict(quantities="upward_flux"), "quantities must be"),
    (dict(quantities="brightness_temperature"), "quantities must be"),
    (dict(quantities=()), "quantities must be"),
    (dict(range_policy="other"), "range_policy"),
    (dict(band_edges=[600.5, 600.2]), "strictly increasing"),
    (dict(instrument="tropomi"), "instrument must be an Instrument"),
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
    call = dict(layer_thickness=ONES, solar_zenith_cosine=0.5)
    call.update(keywords)
    with pytest.raises(ValueError, match=match):
        spec.compute_solar_radiance(**call)


def test_bands_and_instrument_exclude_each_other_and_group_is_not_offered(monkeypatch):
    untouchable(monkeypatch)
    from pylbl_amd.instrument import Instrument
    spec = make_spectroscopy((3, 5))
    instrument = Instrument.gaussian(np.array([600.2, 600.4]), 0.1)
    with pytest.raises(ValueError, match="band_edges or instrument, not both"):
        spec.compute_solar_radiance(ONES, 0.5, band_edges=[600., 600.5], instrument=instrument)
    spec.atmosphere.pressure = spec.atmosphere.pressure.copy()
    spec.atmosphere.pressure[1, 2] = 0.
    with pytest.raises(ValueError, match="Rayleigh scattering needs pressures"):
        spec.compute_solar_radiance(ONES, 0.5)
    spec.group = object()
    with pytest.raises(NotImplementedError):
        spec.compute_solar_radiance(ONES, 0.5, rayleigh=False)


def test_requests_hold_what_the_sweep_needs():
    spec = make_spectroscopy((3, 5))
    thickness = np.arange(1., 16.).reshape(3, 5)
    tau_c = np.linspace(0., 3., 15).reshape(3, 5)
    omega_c, g_c = np.full((3, 5), 0.7), np.linspace(0., 0.85, 15).reshape(3, 5)
    sigma = np.full(GRID_POINTS, 1e-31)
    request = spec._solar_radiance_request(
        thickness, [1., 0.5, 0.1], [1., 0.5, 0.05], [0., 90., 180.], None, None, 1.02, "last",
        [1., 0.5, 0.], None, True, sigma, tau_c, omega_c, g_c, ("radiance",), None, None,
        "reference")
    assert request.quantities == ("radiance",)
    assert request.surface == "last" and request.instrument is None and request.starts is None
    flux = spec._solar_flux_request(
        thickness, [1., 0.5, 0.1], None, None, 1.02, "last", [1., 0.5, 0.], None, True, sigma,
        tau_c, omega_c, g_c, ("upward_flux", "downward_flux"), None, "reference")
    assert np.array_equal(request.level_table, flux.level_table)
    for name in ("mu0", "albedo", "scale", "rayleigh", "rayleigh_values"):
        assert np.array_equal(getattr(request, name), getattr(flux, name)), name
    assert np.array_equal(request.mu, [1., 0.5, 0.05]) and request.scatterer_knots is None
    assert np.array_equal(request.cos_theta, sc.scattering_cosine(
        [1., 0.5, 0.05], [1., 0.5, 0.1], [0., 90., 180.]))
    assert np.all(np.abs(request.cos_theta) <= 1.) and request.cos_theta[0] == -1.
    request = spec._solar_radiance_request(
        thickness, 0.5, 0.6, 180., None, None, 1., "first", [[0.1, 0.2, 0.3]]*3, KNOTS, False,
        None, None, None, None, "radiance", [600., 600.5], None, "skip")
    assert np.array_equal(request.albedo_knots, KNOTS) and request.starts is not None
    assert np.array_equal(request.mu, [0.6]*3) and np.all(request.level_table[:, 1:] == 0.)


# ---------------------------------------------------------------------------------------------
# The queue.
@contextlib.contextmanager
def recorded(directory):
    before = surface.SurfaceRecorder
    surface.SurfaceRecorder = sc.SolarRadianceRecorder
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
    result = spec.compute_solar_radiance(**keywords)
    return list(engine.log), result


@pytest.mark.parametrize("surface_end", ["first", "last"])
def test_one_call_computes_beta_once_per_run_of_whole_paths(tmp_path, monkeypatch, surface_end):
    from pylbl_amd import spectroscopy
    monkeypatch.setattr(spectroscopy, "_XARRAY", [None])
    thickness = np.linspace(50., 300., 6).reshape(surface.SHAPE)
    with recorded(tmp_path) as (spec, engine):
        # 6 blocks per level: 18 rows a path of three levels.
        for limit, runs in ((None, 1), (36, 1), (35, 2), (18, 2)):
            log, result = queue_of(
                spec, engine, limit, layer_thickness=thickness, solar_zenith_cosine=[0.5, 0.8],
                view_zenith_cosine=[1., 0.4], relative_azimuth=[0., 120.], surface=surface_end,
                surface_albedo=[[0.2, 0.4], [0.1, 0.3]], albedo_wavenumber=[10., 70.])
            # Two lines gases: two compute calls per run, each level in exactly one run.
            assert sum(line.startswith("compute(") for line in log) == 2*runs
            names = [line.split("(")[0] for line in log if line.startswith(
                ("solar_spectrum", "rayleigh_row", "surface_emissivity", "path_"))]
            assert names == ["solar_spectrum", "rayleigh_row", "surface_emissivity"] + \
                ["path_two_stream", "path_solar_radiance"]*runs
            fluxes = [line for line in log if line.startswith("path_two_stream(")]
            views = [line for line in log if line.startswith("path_solar_radiance(")]
            from_last = surface_end == "first"
            begins = [int(argument(line, "level_begin")) for line in views]
            assert begins == sorted(begins, reverse=from_last) and len(set(begins)) == runs
            assert all(begin % 3 == 0 for begin in begins)
            fill = next(line for line in log if line.startswith("rayleigh_row"))
            for flux, view in zip(fluxes, views):
                for name in ("beta", "level_begin", "level_table", "solar_zenith_cosine",
                             "solar_row", "up_rows", "direct_rows", "diffuse_rows", "from_last",
                             "rayleigh_row", "albedo_rows", "albedo", "asynchronous"):
                    assert argument(flux, name) == argument(view, name), name
                assert argument(view, "rayleigh_row") == argument(fill, "row")
                assert argument(view, "from_last") == str(from_last)
                assert argument(view, "asynchronous") == "True"
                # The flux entry writes the three row blocks only.
                assert "down_rows" not in flux and "top_up_rows" not in flux
                assert "up_mean" not in flux and "band_start" not in flux
                blocks = {argument(view, name) for name in
                          ("beta", "up_rows", "direct_rows", "diffuse_rows", "radiance_rows",
                           "solar_row", "rayleigh_row", "albedo_rows")}
                blocks.add(argument(flux, "work"))
                assert len(blocks) == 9 and argument(view, "band_start") == "None"
            assert result["radiance"].shape == (2, 160)
        # One path does not fit.
        with pytest.raises(ValueError, match="does not hold one path"):
            queue_of(spec, engine, 17, layer_thickness=thickness, solar_zenith_cosine=0.5)
        # Bands: the sweep writes a block of the call, the output receives its means; without
        # Rayleigh scattering no sigma row is made.
        log, result = queue_of(spec, engine, None, layer_thickness=thickness,
                               solar_zenith_cosine=0.5, surface=surface_end, rayleigh=False,
                               surface_albedo=0.3, band_edges=[20., 30., 60.])
        view, = [line for line in log if line.startswith("path_solar_radiance(")]
        assert argument(view, "band_start") != "None" and "albedo_rows=None" in view
        assert "rayleigh_row=None" in view
        assert argument(view, "radiance_mean") != argument(view, "radiance_rows")
        assert not any(line.startswith(("surface_emissivity", "rayleigh_row")) for line in log)
        assert result["radiance"].shape == (2, 2)
        assert np.array_equal(result["band_points"], [40, 120])


def test_existing_calls_do_not_reach_the_new_entry(tmp_path):
    with recorded(tmp_path) as (spec, engine):
        engine.begin()
        spec.compute_solar_flux(np.ones(surface.SHAPE), 0.5)
        spec.compute_solar(np.ones(surface.SHAPE), 0.5)
        assert any(line.startswith("path_two_stream") for line in engine.log)
        assert not any(line.startswith("path_solar_radiance") for line in engine.log)
